// grayrad_emu.cpp -- HOST EMULATION of the grey radiation kernel (pam_amd/csrc/grayrad_device.h: column<IDX>; compiled with g++
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loop mirrors grayrad_kernel
// of modules_kernels.hip: one "thread" per (column, member), t = (j nx + i) nens + e, the narrow instance or (wide) the one with 64-bit
// element offsets.
#include "../../pam_amd/csrc/grayrad_device.h"

using namespace pama::grayrad;

extern "C" {

void emu_radiation_gray(int nens, int nx, int ny, int nz, double *temp, const double *rho_d, const double *rho_v, int num_liquid,
                        const double *const *liquid, int num_ice, const double *const *ice, const double *zint, const double *sfc_temp,
                        double k_d, double k_v, double k_l, double k_i, double sigma, double cp_d, double lw_down_top, double dt, double *heating,
                        double *olr, double *down_sfc, double *up_sfc, int wide) {
  const long long level = (long long)nx * ny * nens;
  Fields F;
  F.rho_d = rho_d; F.rho_v = rho_v;
  for (int i = 0; i < MAX_SPECIES; i++) {
    F.liquid[i] = i < num_liquid ? liquid[i] : nullptr;
    F.ice[i] = i < num_ice ? ice[i] : nullptr;
  }
  const Params P{k_d, k_v, k_l, k_i, sigma, cp_d, lw_down_top, dt, num_liquid, num_ice};
  for (long long t = 0; t < level; t++) {
    const int e = (int)(t % nens);
    if (wide) column<long long>(temp, F, zint + e, sfc_temp, t, level, (long long)nens, nz, P, heating, olr, down_sfc, up_sfc);
    else column<unsigned>(temp, F, zint + e, sfc_temp, (unsigned)t, (unsigned)level, (unsigned)nens, nz, P, heating, olr, down_sfc, up_sfc);
  }
}

}
