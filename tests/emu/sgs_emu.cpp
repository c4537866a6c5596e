// sgs_emu.cpp -- HOST EMULATION of the Smagorinsky SGS kernels (pam_amd/csrc/sgs_device.h, compiled with g++ -ffp-contract=off).
// TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror the kernels of modules_kernels.hip:
// one "thread" per (column, member), t = (j nx + i) nens + e; the solve works IN PLACE on the fields, the momentum class, then the heat
// class, then the tracer table, with c' either in an array laid out like the kernel's LDS (nz rows of `lanes` doubles per workgroup,
// poisoned first, so a c' read before it was formed shows) or in a workspace of one field (poisoned likewise).
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../pam_amd/csrc/sgs_device.h"

using namespace pama::sgs;

extern "C" {

// f[6]: uvel, vvel, wvel, temp, rho_d, rho_v, (nz, ny, nx, nens) each
void emu_sgs_coefficients(int nens, int nx, int ny, int nz, const double *const *f, const double *zint, const double *zmid, double dx, double dy,
                          double grav, double cp_d, double cs, double prandtl, double *tk, double *tkh) {
  const long long level = (long long)nx * ny * nens;
  const CoefParams P{twice(dx), twice(dy), grav, lapse(grav, cp_d), cs, prandtl};
  for (long long t = 0; t < level; t++) {
    const long long c = t / nens;
    const int e = (int)(t - c * nens), j = (int)(c / nx), i = (int)(c - (long long)j * nx);
    coef_column(f, zint + e, zmid + e, level, nens, nx, ny, nz, j, i, e, P, tk, tkh);
  }
}

// path 1: c' in "LDS" of `lanes` threads per workgroup; path 2: c' in a workspace (nz, ny, nx, nens)
void emu_sgs_diffuse(int nens, int nx, int ny, int nz, double *uvel, double *vvel, double *wvel, double *temp, int num_tracers,
                     double *const *tracers, const double *rho_d, const double *rho_v, const double *tk, const double *tkh, const double *zint,
                     const double *zmid, const double *sfc_u, const double *sfc_v, double dt, double grav, double cp_d, int path, int lanes) {
  const long long level = (long long)nx * ny * nens;
  const double gc = lapse(grav, cp_d);
  double *mom[3] = {uvel, vvel, wvel};
  const double *sfc[3] = {sfc_u, sfc_v, nullptr};
  double *heat[1] = {temp};
  std::vector<double> lds((size_t)nz * lanes), ws(path == 2 ? (size_t)nz * level : 0, std::nan(""));
  for (long long t0 = 0; t0 < level; t0 += lanes) {
    for (size_t q = 0; q < lds.size(); q++) lds[q] = std::nan("");
    for (int lane = 0; lane < lanes && t0 + lane < level; lane++) {
      const long long t = t0 + lane;
      const int e = (int)(t % nens);
      double *cp = path == 2 ? ws.data() + t : lds.data() + lane;
      const long long cs = path == 2 ? level : (long long)lanes;
      solve_class(C_MOMENTUM, mom, 3, sfc, t, rho_d, rho_v, tk, zint + e, zmid + e, level, (long long)nens, nz, dt, gc, cp, cs);
      solve_class(C_HEAT, heat, 1, nullptr, t, rho_d, rho_v, tkh, zint + e, zmid + e, level, (long long)nens, nz, dt, gc, cp, cs);
      if (num_tracers > 0)
        solve_class(C_TRACER, tracers, num_tracers, nullptr, t, rho_d, rho_v, tkh, zint + e, zmid + e, level, (long long)nens, nz, dt, gc, cp, cs);
    }
  }
}

// the same bodies at strides of the caller's choice, one (column, member): the 64-bit offsets.  Every pointer is the array's element 0;
// `level` is the distance between two levels of a field and `off` the flat index inside a level, either of which may exceed 2^31
void emu_sgs_solve_at(int cls, double *const *f, int nf, const double *const *sfc, long long off, const double *rd, const double *rv,
                      const double *K, const double *zint, const double *zmid, long long level, long long zs, int nz, double dt, double gc,
                      double *cp, long long cs) {
  solve_class(cls, f, nf, sfc, off, rd, rv, K, zint, zmid, level, zs, nz, dt, gc, cp, cs);
}

void emu_sgs_coef_at(const double *const *f, const double *zint, const double *zmid, long long level, int nens, int nx, int ny, int nz, int j, int i,
                     int e, double dx, double dy, double grav, double cp_d, double cs, double prandtl, double *tk, double *tkh) {
  const CoefParams P{twice(dx), twice(dy), grav, lapse(grav, cp_d), cs, prandtl};
  coef_column(f, zint, zmid, level, nens, nx, ny, nz, j, i, e, P, tk, tkh);
}

}
