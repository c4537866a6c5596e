// sgs_moist_emu.cpp -- HOST EMULATION of the moist coefficient kernel and of the solve with surface fluxes of heat and vapour
// (pam_amd/csrc/sgs_device.h: coef_column_t<true>, solve_class_t<true>, exp_c; compiled with g++ -ffp-contract=off).
// TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror sgs_coef_moist_kernel and
// sgs_solve_flux_kernel of modules_kernels.hip as sgs_emu.cpp mirrors the dry ones: one "thread" per (column, member), t = (j nx + i) nens
// + e; c' in an array laid out like the kernel's LDS (poisoned first) or in a workspace of one field.
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../pam_amd/csrc/sgs_device.h"

using namespace pama::sgs;

extern "C" {

void emu_sgs_exp_c(const double *x, double *y, long long n) {
  for (long long q = 0; q < n; q++) y[q] = exp_c(x[q]);
}

// f[6]: uvel, vvel, wvel, temp, rho_d, rho_v; cloud[num_cloud], precip[num_precip]: (nz, ny, nx, nens) each
void emu_sgs_coefficients_moist(int nens, int nx, int ny, int nz, const double *const *f, int num_cloud, const double *const *cloud, int num_precip,
                                const double *const *precip, const double *zint, const double *zmid, double dx, double dy, double grav, double cp_d,
                                double R_d, double R_v, double threshold, double cs, double prandtl, double *tk, double *tkh) {
  const long long level = (long long)nx * ny * nens;
  const CoefParams P{twice(dx), twice(dy), grav, lapse(grav, cp_d), cs, prandtl};
  const MoistParams M{R_d, R_v, cp_d, ratio(R_d, R_v), threshold, num_cloud, num_precip};
  for (long long t = 0; t < level; t++) {
    const long long c = t / nens;
    const int e = (int)(t - c * nens), j = (int)(c / nx), i = (int)(c - (long long)j * nx);
    coef_column_t<true>(f, cloud, precip, M, zint + e, zmid + e, level, nens, nx, ny, nz, j, i, e, P, tk, tkh);
  }
}

// path 1: c' in "LDS" of `lanes` threads per workgroup; path 2: c' in a workspace (nz, ny, nx, nens).  trsfc[num_tracers]: sfc_lhf at the
// vapour's index, NULL elsewhere, as the entry point builds it
void emu_sgs_diffuse_fluxes(int nens, int nx, int ny, int nz, double *uvel, double *vvel, double *wvel, double *temp, int num_tracers,
                            double *const *tracers, const double *rho_d, const double *rho_v, const double *tk, const double *tkh,
                            const double *zint, const double *zmid, const double *sfc_u, const double *sfc_v, double dt, double grav, double cp_d,
                            const double *shf, const double *const *trsfc, double latvap, int path, int lanes) {
  const long long level = (long long)nx * ny * nens;
  const double gc = lapse(grav, cp_d);
  double *mom[3] = {uvel, vvel, wvel};
  const double *sfc[3] = {sfc_u, sfc_v, nullptr};
  double *heat[1] = {temp};
  const double *hsfc[1] = {shf};
  std::vector<double> lds((size_t)nz * lanes), ws(path == 2 ? (size_t)nz * level : 0, std::nan(""));
  for (long long t0 = 0; t0 < level; t0 += lanes) {
    for (size_t q = 0; q < lds.size(); q++) lds[q] = std::nan("");
    for (int lane = 0; lane < lanes && t0 + lane < level; lane++) {
      const long long t = t0 + lane;
      const int e = (int)(t % nens);
      double *cp = path == 2 ? ws.data() + t : lds.data() + lane;
      const long long cs = path == 2 ? level : (long long)lanes;
      solve_class_t<true>(C_MOMENTUM, mom, 3, sfc, t, rho_d, rho_v, tk, zint + e, zmid + e, level, (long long)nens, nz, dt, gc, cp, cs, 0.0);
      solve_class_t<true>(C_HEAT, heat, 1, hsfc, t, rho_d, rho_v, tkh, zint + e, zmid + e, level, (long long)nens, nz, dt, gc, cp, cs, cp_d);
      if (num_tracers > 0)
        solve_class_t<true>(C_TRACER, tracers, num_tracers, trsfc, t, rho_d, rho_v, tkh, zint + e, zmid + e, level, (long long)nens, nz, dt, gc, cp,
                            cs, latvap);
    }
  }
}

// the same bodies at strides of the caller's choice, one (column, member): the 64-bit offsets.  Every pointer is the array's element 0
void emu_sgs_flux_solve_at(int cls, double *const *f, int nf, const double *const *sfc, long long off, const double *rd, const double *rv,
                           const double *K, const double *zint, const double *zmid, long long level, long long zs, int nz, double dt, double gc,
                           double *cp, long long cs, double scale) {
  solve_class_t<true>(cls, f, nf, sfc, off, rd, rv, K, zint, zmid, level, zs, nz, dt, gc, cp, cs, scale);
}

void emu_sgs_moist_coef_at(const double *const *f, int num_cloud, const double *const *cloud, int num_precip, const double *const *precip,
                           const double *zint, const double *zmid, long long level, int nens, int nx, int ny, int nz, int j, int i, int e, double dx,
                           double dy, double grav, double cp_d, double R_d, double R_v, double threshold, double cs, double prandtl, double *tk,
                           double *tkh) {
  const CoefParams P{twice(dx), twice(dy), grav, lapse(grav, cp_d), cs, prandtl};
  const MoistParams M{R_d, R_v, cp_d, ratio(R_d, R_v), threshold, num_cloud, num_precip};
  coef_column_t<true>(f, cloud, precip, M, zint, zmid, level, nens, nx, ny, nz, j, i, e, P, tk, tkh);
}

}
