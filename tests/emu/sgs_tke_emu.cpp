// sgs_tke_emu.cpp -- HOST EMULATION of the two coefficient kernels of the prognostic-TKE closure (pam_amd/csrc/sgs_device.h:
// coef_column_t<false, true> and coef_column_t<true, true> around tke_step; compiled with g++ -ffp-contract=off).
// TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror sgs_tke_coef_kernel and
// sgs_tke_coef_moist_kernel of modules_kernels.hip as sgs_moist_emu.cpp mirrors the Smagorinsky ones: one "thread" per (column, member),
// t = (j nx + i) nens + e; tke is updated in place.
#include <cmath>

#include "../../pam_amd/csrc/sgs_device.h"

using namespace pama::sgs;

extern "C" {

// ce, ce1, ce2 as every C++ wrapper forms them
void emu_sgs_tke_constants(double cs, double ck, double *out) {
  out[0] = tke_ce(cs, ck);
  out[1] = tke_ce1(out[0]);
  out[2] = tke_ce2(out[0]);
}

// f[6]: uvel, vvel, wvel, temp, rho_d, rho_v; cloud[num_cloud], precip[num_precip]: (nz, ny, nx, nens) each; moist == 0: the dry kernel
void emu_sgs_tke_coefficients(int moist, int nens, int nx, int ny, int nz, const double *const *f, double *tke, int num_cloud,
                              const double *const *cloud, int num_precip, const double *const *precip, const double *zint, const double *zmid,
                              double dx, double dy, double dt, double grav, double cp_d, double R_d, double R_v, double threshold, double ck,
                              double ce1, double ce2, double seed, double *tk, double *tkh) {
  const long long level = (long long)nx * ny * nens;
  const CoefParams P{twice(dx), twice(dy), grav, lapse(grav, cp_d), 0.0, 0.0};
  const TkeParams Q{dt, ck, ce1, ce2, seed};
  const MoistParams none{};
  const MoistParams M{R_d, R_v, cp_d, moist ? ratio(R_d, R_v) : 0.0, threshold, num_cloud, num_precip};
  for (long long t = 0; t < level; t++) {
    const long long c = t / nens;
    const int e = (int)(t - c * nens), j = (int)(c / nx), i = (int)(c - (long long)j * nx);
    if (moist)
      coef_column_t<true, true>(f, cloud, precip, M, zint + e, zmid + e, level, nens, nx, ny, nz, j, i, e, P, tk, tkh, &Q, tke);
    else
      coef_column_t<false, true>(f, nullptr, nullptr, none, zint + e, zmid + e, level, nens, nx, ny, nz, j, i, e, P, tk, tkh, &Q, tke);
  }
}

// one cell
void emu_sgs_tke_step(double tke, double rho, double def2, double n2, double delta, double dt, double ck, double ce1, double ce2, double seed,
                      double *out) {
  const TkeParams Q{dt, ck, ce1, ce2, seed};
  tke_step(tke, rho, def2, n2, delta, Q, out[0], out[1], out[2]);
}

}
