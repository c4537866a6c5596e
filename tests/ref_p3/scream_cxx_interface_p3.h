// empty on purpose: the reference's Microphysics.h includes this header of SCREAM's; its non-P3_CXX path needs nothing from it
#pragma once
