// grayrad_sw_emu.cpp -- HOST EMULATION of the grey shortwave kernel (pam_amd/csrc/grayrad_sw_device.h: column<IDX>; compiled with g++
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loop mirrors
// grayrad_sw_kernel of modules_kernels.hip: one "thread" per (column, member), t = (j nx + i) nens + e, the narrow instance or (wide) the
// one with 64-bit element offsets.
#include "../../pam_amd/csrc/grayrad_sw_device.h"

using namespace pama::grayrad_sw;

extern "C" {

void emu_radiation_gray_sw(int nens, int nx, int ny, int nz, double *temp, const double *rho_d, const double *rho_v, int num_liquid,
                           const double *const *liquid, int num_ice, const double *const *ice, const double *zint, const double *coszen,
                           const double *sfc_albedo, double solar_constant, double a_d, double a_v, double a_l, double a_i, double s_l, double s_i,
                           double albedo, double cp_d, double dt, double *heating, double *down_sfc, double *up_sfc, double *up_top, int wide) {
  const long long level = (long long)nx * ny * nens;
  Fields F;
  F.rho_d = rho_d; F.rho_v = rho_v;
  for (int i = 0; i < pama::grayrad::MAX_SPECIES; i++) {
    F.liquid[i] = i < num_liquid ? liquid[i] : nullptr;
    F.ice[i] = i < num_ice ? ice[i] : nullptr;
  }
  const Params P{a_d, a_v, a_l, a_i, s_l, s_i, solar_constant, albedo, cp_d, dt, num_liquid, num_ice};
  for (long long t = 0; t < level; t++) {
    const int e = (int)(t % nens);
    if (wide) column<long long>(temp, F, zint + e, coszen[e], sfc_albedo, t, level, (long long)nens, nz, P, heating, down_sfc, up_sfc, up_top);
    else column<unsigned>(temp, F, zint + e, coszen[e], sfc_albedo, (unsigned)t, (unsigned)level, (unsigned)nens, nz, P, heating, down_sfc, up_sfc, up_top);
  }
}

}
