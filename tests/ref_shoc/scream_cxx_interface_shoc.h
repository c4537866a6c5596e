// physics/sgs/shoc/SGS.h includes a header of this name whether SHOC_CXX is defined or not; it belongs to SCREAM's C++ interface,
// which the harness does not use (the Fortran-call path is taken).  Empty on purpose.  TEST INFRASTRUCTURE ONLY.
#pragma once
