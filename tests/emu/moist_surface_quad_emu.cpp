// moist_surface_quad_emu.cpp -- the REFERENCE of surface friction's arithmetic (pam_core/modules/surface_friction.h: z0_est :16-31,
// diag_ustar :44-63, z0 per member :96-103, the flux per cell :147-166) in binary128 (__float128, 113 bits), for
// tests/moist_surface_cases.py.  TEST INFRASTRUCTURE ONLY.  It is no emulation of the
// device bodies and calls none of them: the formulas are written out again from the reference's text, every constant the double the
// code holds (PI = 3.14159) taken as an exact number, every double input taken as an exact number.  The file carries the _emu suffix so
// that the one build helper of the tests builds it and watches its dependencies (tools/native_build.py: emu_library, libs = quadmath,
// pthread).
//
// Why 113 bits: np.longdouble carries 64, and the eight iterations of diag_ustar amplify its roundings as they amplify a double's, which
// leaves 5e-3 of a unit (2^-53 of the cell's scale) at the worst of a few hundred cells; the results here are good to 1e-30 and are
// handed back rounded to long double (at most 2^-11 = 4.9e-4 of a unit).
#include <quadmath.h>
#include <thread>
#include <vector>

#include "../../pam_amd/csrc/moist_surface_device.h"      // for the static_assert below alone

typedef __float128 Q;

namespace {
const Q VONK = 0.4, EPS = 1.0e-10, AM = 4.8, BM = 19.3, PI = 3.14159;      // the doubles of surface_friction.h:8-12, exactly
// "the doubles the code holds": a constant changed in the device header has to be changed here by hand, or this does not compile
static_assert(pama::moist::SF_VONK == 0.4 && pama::moist::SF_EPS == 1.0e-10 && pama::moist::SF_AM == 4.8 && pama::moist::SF_BM == 19.3 &&
                  pama::moist::SF_PI == 3.14159,
              "the constants of the reference are not those of moist_surface_device.h");

Q diag_ustar(Q z, Q bflx, Q wnd, Q z0) {                                    // :44-63
  const Q c1 = PI / 2 - 3 * logq((Q)2);
  const Q lnz = logq(z / z0);
  Q ustar = wnd * (VONK / lnz);
  if (bflx != 0) {
    for (int it = 0; it < 8; it++) {
      Q zeta = z * (-bflx * VONK / (ustar * ustar * ustar + EPS));
      if (zeta > 1) zeta = 1;
      if (zeta > 0) {
        ustar = VONK * wnd / (lnz + AM * zeta);
      } else {
        const Q x = sqrtq(sqrtq(1 - BM * zeta));
        const Q psi1 = 2 * logq(1 + x) + logq(1 + x * x) - 2 * atanq(x) + c1;
        ustar = wnd * VONK / (lnz - psi1);
      }
    }
  }
  return ustar;
}

void cells(long long i0, long long i1, const double *u, const double *v, const double *um, const double *vm, const double *rm,
           const double *zm0, const double *bflx, const double *z0, const double *r0, const double *r1, const double *r2,
           const double *dz, long double *fu, long double *fv, double *unit_u, double *unit_v) {
  const Q U = 0x1p-53;
  for (long long i = i0; i < i1; i++) {
    const Q uu = u[i], vv = v[i];
    Q wnd = sqrtq(uu * uu + vv * vv);                                       // :147-166
    if (wnd < 1) wnd = 1;
    const Q ustar = diag_ustar(zm0[i], bflx[i], wnd, z0[i]);
    const Q tau00 = (Q)rm[i] * ustar * ustar;
    const Q rho_sfc = 2 * (((Q)r0[i] + r1[i]) / 2) - ((Q)r1[i] + r2[i]) / 2;
    const Q k = tau00 / wnd * rho_sfc / dz[i];
    const Q s = fabsq(k);
    fu[i] = (long double)(-(uu - um[i]) * k);
    fv[i] = (long double)(-(vv - vm[i]) * k);
    unit_u[i] = (double)(U * (fabsq(uu) + fabsq((Q)um[i])) * s);
    unit_v[i] = (double)(U * (fabsq(vv) + fabsq((Q)vm[i])) * s);
  }
}
}  // namespace

extern "C" {

// every input an array of n doubles; fu, fv: n long doubles; unit_u, unit_v: n doubles.  The cells are dealt to `threads` host threads.
void quad_surface_friction_cells(long long n, int threads, const double *u, const double *v, const double *um, const double *vm,
                                 const double *rm, const double *zm0, const double *bflx, const double *z0, const double *r0,
                                 const double *r1, const double *r2, const double *dz, long double *fu, long double *fv, double *unit_u,
                                 double *unit_v) {
  if (threads < 1) threads = 1;
  if (n < 4096) threads = 1;
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++) {
    const long long i0 = n * t / threads, i1 = n * (t + 1) / threads;
    pool.emplace_back(cells, i0, i1, u, v, um, vm, rm, zm0, bflx, z0, r0, r1, r2, dz, fu, fv, unit_u, unit_v);
  }
  for (auto &th : pool) th.join();
}

// surface_friction_init per member (surface_friction.h:16-31 z0_est, :96-103): raw is z0 before the clamps, z0 after them
// ([1e-5, 1], the doubles 0.00001 and 1.0), both rounded once to long double.  rho_mean: the float64 slot-order mean, an exact input.
void quad_surface_friction_z0(int n, const double *zmid0, const double *bflx, const double *gu, const double *gv, const double *tau,
                              const double *rho_mean, long double *raw, long double *z0) {
  const Q c1 = PI / 2 - 3 * logq((Q)2);
  for (int i = 0; i < n; i++) {
    const Q z = zmid0[i], b = bflx[i], u = gu[i], v = gv[i];
    Q wnd = sqrtq(u * u + v * v);
    if (wnd < 1) wnd = 1;
    const Q ustar = sqrtq((Q)tau[i] / (Q)rho_mean[i]);
    Q zeta = z * (-b * VONK / (ustar * ustar * ustar + EPS));
    if (zeta > 1) zeta = 1;
    Q psi1;
    if (zeta >= 0) {
      psi1 = -AM * zeta;
    } else {
      const Q x = sqrtq(sqrtq(1 - BM * zeta));
      psi1 = 2 * logq(1 + x) + logq(1 + x * x) - 2 * atanq(x) + c1;
    }
    Q lnz = VONK * wnd / (ustar + EPS) + psi1;
    if (lnz < 0) lnz = 0;
    const Q r = z * expq(-lnz);
    Q c = r;
    if (c > 1) c = 1;
    if (c < (Q)0.00001) c = (Q)0.00001;
    raw[i] = (long double)r;
    z0[i] = (long double)c;
  }
}

}
