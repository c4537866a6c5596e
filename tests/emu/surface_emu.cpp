// surface_emu.cpp -- HOST EMULATION of the surface-flux kernel (pam_amd/csrc/surface_device.h: column<SLAB>; compiled with g++
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loop mirrors
// surface_fluxes_kernel of modules_kernels.hip: one "thread" per (row, column, member), t = (j nx + i) nens + e, and the entry point's
// choice of the instance and of gc.
#include "../../pam_amd/csrc/surface_device.h"

using namespace pama::surface;

extern "C" {

void emu_surface_fluxes(int nens, int nx, int ny, int nz, const double *temp, const double *rho_d, const double *rho_v, const double *uvel,
                        const double *vvel, const double *zmid, const double *cn, const double *cstar, double *sfc_temp, const double *lw_down,
                        const double *lw_up, const double *sw_down, const double *sw_up, double gust, double wetness, double grav, double cp_d,
                        double R_v, double latvap, double slab_heat_capacity, double dt, double *sfc_shf, double *sfc_lhf) {
  (void)nz;
  const long long level = (long long)nx * ny * nens;
  const Params P{gust, wetness, grav, pama::sgs::ratio(grav, cp_d), cp_d, R_v, latvap, slab_heat_capacity, dt};
  const bool slab = slab_heat_capacity > 0 && dt != 0;
  for (long long t = 0; t < level; t++) {
    const int e = (int)(t % nens);
    const double *ld = lw_down ? lw_down + t : nullptr, *lu = lw_up ? lw_up + t : nullptr;
    const double *sd = sw_down ? sw_down + t : nullptr, *su = sw_up ? sw_up + t : nullptr;
    if (slab)
      column<true>(temp + t, rho_d + t, rho_v + t, uvel + t, vvel + t, zmid + e, cn + e, cstar + e, sfc_temp + t, ld, lu, sd, su, P, sfc_shf + t,
                   sfc_lhf + t);
    else
      column<false>(temp + t, rho_d + t, rho_v + t, uvel + t, vvel + t, zmid + e, cn + e, cstar + e, sfc_temp + t, ld, lu, sd, su, P, sfc_shf + t,
                    sfc_lhf + t);
  }
}

}
