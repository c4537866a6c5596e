#pragma once
// Serial stand-in: NetCDF I/O is not used by the pinned paths.
