// statistics_emu.cpp -- HOST EMULATION of the statistics modules' arithmetic (pam_amd/csrc/statistics_device.h, compiled with g++
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror the kernels
// of modules_kernels.hip: one walk per (level, member) in ascending column order; one update per element.
#include "../../pam_amd/csrc/statistics_device.h"

using namespace pama::stats;

extern "C" {

// in: (nz, ncol, nens) contiguous; out: (nz, nens)
void emu_horizontal_average(int nz, int ncol, int nens, const double *in, double *out) {
  for (int k = 0; k < nz; k++)
    for (int e = 0; e < nens; e++)
      out[(long long)k * nens + e] = havg_walk<long long>(in + ((long long)k * ncol * nens + e), (long long)nens, ncol);
}

void emu_time_average_accumulate(long long n, const double *var, double *tavg, double factor) {
  for (long long i = 0; i < n; i++) tavg[i] = tavg_add(tavg[i], var[i], factor);
}

}
