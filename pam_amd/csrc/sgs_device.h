// sgs_device.h -- the arithmetic of the native Smagorinsky-Lilly SGS closure (a first-order column scheme: eddy coefficients from the
// resolved deformation and the dry stability, then an implicit vertical diffusion of the winds, temp and every tracer), as device
// functions that are plain inline C++ outside hipcc: the HIP kernels in modules_kernels.hip call them, and tests/emu/sgs_emu.cpp compiles
// the same bodies with g++ (-ffp-contract=off).  The method is not part of the reference tree; the yardstick is the numpy restatement of
// the contract in tests/sgs_ref.py, held bit for bit (include/pam_amd_modules.h).
// Fields are (nz, ny, nx, nens), members fastest; inside a level a (column, member) has the flat index t = (j nx + i) nens + e, and every
// element offset is 64 bits wide.  zint (nz+1, nens) and zmid (nz, nens) are per member.
// Contraction into fma is switched off inside each body, so the device and the host give the same bits.
// The moist branch (coef_column_t<true>: condensate loading, a saturated N2 where cloud stands, with an exponential of its own, exp_c)
// and the surface fluxes of heat and vapour (solve_class_t<true>) are further instances of the same two bodies; the instances the dry
// entry points use (coef_column, solve_class) are the <false> ones.  tests/emu/sgs_moist_emu.cpp compiles the new ones under g++ and
// tests/sgs_moist_ref.py restates them.
// The prognostic-TKE (1.5-order) closure is one more instance of the coefficient walk (coef_column_t<MOIST, true>): tke_step() stands in
// eddy()'s place, the thread reads and writes its own cell of the tracer tke (rho e) level by level, and rho of level k rides along with
// the centre values.  The instances above are what they were (TKE defaults to false and its two arguments to nullptr).
// tests/emu/sgs_tke_emu.cpp compiles the new ones under g++ and tests/sgs_tke_ref.py restates them.
#pragma once

#include <cmath>

#include "msa_device.h"      // PAMA_D, PAMA_NO_CONTRACT

namespace pama {
namespace sgs {

constexpr int MAX_TRACERS = 64;          // tracers per call
constexpr int NREG = 4;                  // fields of a class whose running values a thread keeps in registers
constexpr int AHEAD = 4;                 // levels whose loads are requested before the first of them is used
enum { C_MOMENTUM, C_HEAT, C_TRACER };   // the three classes of rows

struct CoefParams {
  double two_dx, two_dy, grav, gc, cs, prandtl;      // gc = grav / cp_d
};

// host functions, once per call
inline double twice(double d) {
  PAMA_NO_CONTRACT
  return 2.0 * d;
}
inline double lapse(double grav, double cp_d) {
  PAMA_NO_CONTRACT
  return grav / cp_d;
}

PAMA_D double centred(double hi, double lo, double span) {
  PAMA_NO_CONTRACT
  const double d = hi - lo;
  return d / span;
}

// Tv = temp (1 + 0.608 rho_v / rho), rho = rho_d + rho_v
PAMA_D double virtual_temp(double temp, double rho_d, double rho_v) {
  PAMA_NO_CONTRACT
  const double rho = rho_d + rho_v;
  const double q = rho_v / rho;
  const double t = 0.608 * q;
  const double f = 1.0 + t;
  return temp * f;
}

// Def2 = 2 (ux^2 + vy^2 + wz^2) + (uy + vx)^2 + (uz + wx)^2 + (vz + wy)^2, left to right; without y the y derivatives are absent
PAMA_D double deformation(bool with_y, double ux, double uy, double uz, double vx, double vy, double vz, double wx, double wy, double wz) {
  PAMA_NO_CONTRACT
  double a = ux * ux;
  if (with_y) a = a + vy * vy;
  a = a + wz * wz;
  double d = 2.0 * a;
  double s = with_y ? uy + vx : vx;
  d = d + s * s;
  s = uz + wx;
  d = d + s * s;
  s = with_y ? vz + wy : vz;
  d = d + s * s;
  return d;
}

// N2 = grav / Tv_k * (dTv/dz + grav / cp_d): the unsaturated frequency
PAMA_D double stability(double grav, double gc, double tv, double dtvdz) {
  PAMA_NO_CONTRACT
  const double a = grav / tv;
  const double b = dtvdz + gc;
  return a * b;
}

// tk = (cs dz)^2 sqrt(max(Def2 - N2 / prandtl, 0)), a NaN argument staying a NaN; tkh = tk / prandtl
PAMA_D void eddy(double def2, double n2, double dz, double cs, double prandtl, double &tk, double &tkh) {
  PAMA_NO_CONTRACT
  const double l = cs * dz;
  const double l2 = l * l;
  const double arg = def2 - n2 / prandtl;
  const double m = arg < 0.0 ? 0.0 : arg;
  tk = l2 * std::sqrt(m);
  tkh = tk / prandtl;
}

// ---- the prognostic-TKE (1.5-order) closure: one cell's step of e = tke / rho and the coefficients it gives
struct TkeParams {
  double dt, ck, ce1, ce2, seed;
};

// host, once per class: ce = ck^3 / cs^4, so that the neutral fixed point is Smagorinsky's tk = (cs delta)^2 sqrt(Def2); ce1 and ce2 are
// Deardorff's split of the dissipation constant (0.19 + 0.51 l / delta, which is 0.7 at l = delta)
inline double tke_ce(double cs, double ck) {
  PAMA_NO_CONTRACT
  return ((ck * ck) * ck) / ((cs * cs) * (cs * cs));
}
inline double tke_ce1(double ce) {
  PAMA_NO_CONTRACT
  return (ce / 0.7) * 0.19;
}
inline double tke_ce2(double ce) {
  PAMA_NO_CONTRACT
  return (ce / 0.7) * 0.51;
}

// e0 = max(tke / rho, 0); l = delta where N2 <= 0, else 0.76 sqrt(e0 / N2) held inside [0.1 delta, delta]; pri = 1 + 2 l / delta;
// e1 = max(e0 + dt (ks Def2 - ks pri N2), 0) with ks = ck l sqrt(e0) + seed; e2 = e1 / (1 + dt (ce1 + ce2 l / delta) sqrt(e0) / l): the
// dissipation linearised about the TKE at entry; tk = ck l sqrt(e2), tkh = pri tk.  tke keeps its bits where e2 == tke / rho.  Every
// comparison is written so that a NaN takes the else arm and goes on through the arithmetic
PAMA_D void tke_step(double tke_in, double rho, double def2, double n2, double delta, const TkeParams &Q, double &tke_out, double &tk,
                     double &tkh) {
  PAMA_NO_CONTRACT
  const double x = tke_in / rho;
  const double e0 = x < 0.0 ? 0.0 : x;
  const double se = std::sqrt(e0);
  double l = delta;
  if (n2 > 0.0) {
    const double ls = (0.76 * se) / std::sqrt(n2);
    const double lo = 0.1 * delta;
    const double m = ls < lo ? lo : ls;
    l = m > delta ? delta : m;
  }
  const double r = l / delta;
  const double pri = 1.0 + 2.0 * r;
  const double ckl = Q.ck * l;
  const double ks = ckl * se + Q.seed;
  const double p = ks * def2;
  const double b = (ks * pri) * n2;
  const double s = p - b;
  double e1 = e0 + Q.dt * s;
  e1 = e1 < 0.0 ? 0.0 : e1;
  const double c = Q.ce1 + Q.ce2 * r;
  const double e2 = e1 / (1.0 + ((Q.dt * c) * se) / l);
  tke_out = e2 == x ? tke_in : rho * e2;
  tk = ckl * std::sqrt(e2);
  tkh = pri * tk;
}

// ---- the moist branch of the coefficients
constexpr int MAX_CLOUD = 4, MAX_PRECIP = 8;          // entries of the two tables of condensate densities

struct MoistParams {
  double R_d, R_v, cp_d, eps, threshold;              // eps = R_d / R_v, formed once; threshold: a mixing ratio
  int num_cloud, num_precip;
};

inline double ratio(double a, double b) {             // host, once per call
  PAMA_NO_CONTRACT
  return a / b;
}

// the exponential of the contract: n = floor(x log2(e) + 0.5); r = (x - n ln2_hi) - n ln2_lo; Horner of degree 13 with 1 / k!; ldexp.
// Within 1 ulp of a correctly rounded exp over the arguments the saturation pressure sees; NaN -> NaN, x < -700 -> 0, x > 700 -> +inf
PAMA_D double exp_c(double x) {
  PAMA_NO_CONTRACT
  if (x != x) return x;
  if (x < -700.0) return 0.0;
  if (x > 700.0) return HUGE_VAL;
  const double n = std::floor(x * 1.44269504088896338700 + 0.5);
  const double r = (x - n * 6.93147180369123816490e-01) - n * 1.90821492927058770002e-10;
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 1.0 / 2.0;
  p = p * r + 1.0;
  p = p * r + 1.0;
  return std::ldexp(p, (int)n);                        // |n| <= 1010: the result is a normal number, so the scaling is exact
}

// Lv(T) of liquid water, the reference's latent_heat_condensation, left to right as it is written there
PAMA_D double latent_heat(double temp) {
  PAMA_NO_CONTRACT
  const double tc = temp - 273.15;
  return (2500.8 - 2.36 * tc + 0.0016 * tc * tc - 0.00006 * tc * tc * tc) * 1000.0;
}

// qs = (es / (R_v temp)) / rho with es the reference's saturation_vapor_pressure over exp_c
PAMA_D double saturation_ratio(double temp, double rho, double R_v) {
  PAMA_NO_CONTRACT
  const double tc = temp - 273.15;
  const double x = (17.625 * tc) / (243.04 + tc);
  const double es = 610.94 * exp_c(x);
  const double a = es / (R_v * temp);
  return a / rho;
}

// what the stability needs of one cell.  Dry: trho = Tv only.  Moist: trho = temp ((1 + 0.608 qv) - ql), ql the loading of every
// condensate; qt = qv + ql; qs; sat = the cloud condensate exceeds threshold rho (strictly; never without a cloud table)
struct Thermo {
  double trho, temp, qs, qt;
  bool sat;
};

template <bool MOIST>
PAMA_D Thermo thermo(double temp, double rho_d, double rho_v, const double *const *cloud, const double *const *precip, long long o,
                     const MoistParams &M) {
  PAMA_NO_CONTRACT
  Thermo c;
  if constexpr (!MOIST) {
    c.trho = virtual_temp(temp, rho_d, rho_v);
    c.temp = 0.0; c.qs = 0.0; c.qt = 0.0; c.sat = false;
  } else {
    const double rho = rho_d + rho_v;
    const double qv = rho_v / rho;
    const double t = 0.608 * qv;
    double f = 1.0 + t;
    double cl = 0.0, load = 0.0;
    if (M.num_cloud > 0) cl = cloud[0][o];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 1; q < MAX_CLOUD; q++)
      if (q < M.num_cloud) cl = cl + cloud[q][o];
    load = M.num_cloud > 0 ? cl : (M.num_precip > 0 ? precip[0][o] : 0.0);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < MAX_PRECIP; q++)
      if (q < M.num_precip && (q > 0 || M.num_cloud > 0)) load = load + precip[q][o];
    c.qt = qv;
    if (M.num_cloud > 0 || M.num_precip > 0) {
      const double ql = load / rho;
      f = f - ql;
      c.qt = qv + ql;
    }
    c.trho = temp * f;
    c.temp = temp;
    c.sat = false;
    c.qs = 0.0;
    if (M.num_cloud > 0) {                             // without a cloud table no cell is saturated and qs is never used
      c.sat = cl > M.threshold * rho;
      c.qs = saturation_ratio(temp, rho, M.R_v);
    }
  }
  return c;
}

// the saturated frequency (Durran and Klemp 1982, eq. 36, in temperature form):
//   N2 = grav ((a1 / a2) ((dT/dz + gc) / T + (Lv / (cp_d T)) dqs/dz) - dqt/dz),
//   a1 = 1 + (Lv qs) / (R_d T), a2 = 1 + (((eps Lv) Lv) qs) / (((cp_d R_d) T) T)
PAMA_D double stability_saturated(double grav, double gc, const MoistParams &M, double temp, double qs, double dtdz, double dqsdz, double dqtdz) {
  PAMA_NO_CONTRACT
  const double lv = latent_heat(temp);
  const double a1 = 1.0 + (lv * qs) / (M.R_d * temp);
  const double a2 = 1.0 + (((M.eps * lv) * lv) * qs) / (((M.cp_d * M.R_d) * temp) * temp);
  const double b1 = (dtdz + gc) / temp;
  const double b2 = (lv / (M.cp_d * temp)) * dqsdz;
  const double b = b1 + b2;
  const double m = (a1 / a2) * b;
  return grav * (m - dqtdz);
}

PAMA_D double total_density(double rho_d, double rho_v) {
  PAMA_NO_CONTRACT
  return rho_d + rho_v;
}

PAMA_D int wrap_up(int i, int n) { return i + 1 == n ? 0 : i + 1; }
PAMA_D int wrap_down(int i, int n) { return i == 0 ? n - 1 : i - 1; }

// the eddy coefficients of one column (j, i) of member e, bottom to top.  f: uvel, vvel, wvel, temp, rho_d, rho_v, each pointing at
// element 0; zint, zmid point at (0, e).  The centre values of levels k-1, k, k+1 ride along in registers; the horizontal neighbours of
// level k are read from the fields.  tk and tkh overlap nothing that is read (the entry point refuses it)
// MOIST: cloud[M.num_cloud] and precip[M.num_precip] point at element 0 of the condensate densities, and a saturated level k takes
// stability_saturated; without it the two tables and M are never read
// TKE: the prognostic closure in place of eddy(): rho of level k rides along as well, tke (rho e, element 0) is read and written in the
// thread's own cell only, and Q holds the constants; P.cs and P.prandtl are not read.  Without it Q and tke are never read
template <bool MOIST, bool TKE = false>
PAMA_D void coef_column_t(const double *const *f, const double *const *cloud, const double *const *precip, const MoistParams &M, const double *zint,
                          const double *zmid, long long level, int nens, int nx, int ny, int nz, int j, int i, int e, const CoefParams &P,
                          double *__restrict__ tk, double *__restrict__ tkh, const TkeParams *Q = nullptr, double *__restrict__ tke = nullptr) {
  const bool with_y = ny > 1;
  const long long row = (long long)j * nx;
  const long long c0 = (row + i) * nens + e;
  const long long xp = (row + wrap_up(i, nx)) * nens + e, xm = (row + wrap_down(i, nx)) * nens + e;
  const long long yp = ((long long)wrap_up(j, ny) * nx + i) * nens + e, ym = ((long long)wrap_down(j, ny) * nx + i) * nens + e;
  const double *u = f[0], *v = f[1], *w = f[2], *T = f[3], *rd = f[4], *rv = f[5];
  double u_k = u[c0], v_k = v[c0], w_k = w[c0];
  Thermo a_k = thermo<MOIST>(T[c0], rd[c0], rv[c0], cloud, precip, c0, M);
  [[maybe_unused]] double rho_k = 0.0;
  if constexpr (TKE) rho_k = total_density(rd[c0], rv[c0]);
  double zm_k = zmid[0];
  double u_m = u_k, v_m = v_k, w_m = w_k, zm_m = zm_k;      // the one-sided difference at the ground
  Thermo a_m = a_k;
  double zi_k = zint[0];
  for (int k = 0; k < nz; k++) {
    const int ku = k + 1 < nz ? k + 1 : k;                               // the one-sided difference at the top
    const long long lu = (long long)ku * level + c0, lk = (long long)k * level;
    const double u_p = u[lu], v_p = v[lu], w_p = w[lu];
    const Thermo a_p = thermo<MOIST>(T[lu], rd[lu], rv[lu], cloud, precip, lu, M);
    [[maybe_unused]] double rho_p = 0.0, e_k = 0.0;
    if constexpr (TKE) {
      rho_p = total_density(rd[lu], rv[lu]);
      e_k = tke[lk + c0];
    }
    const double zm_p = zmid[(long long)ku * nens];
    const double zi_p = zint[(long long)(k + 1) * nens];
    const double span = zm_p - zm_m;
    const double uz = centred(u_p, u_m, span), vz = centred(v_p, v_m, span), wz = centred(w_p, w_m, span);
    const double ux = centred(u[lk + xp], u[lk + xm], P.two_dx), vx = centred(v[lk + xp], v[lk + xm], P.two_dx);
    const double wx = centred(w[lk + xp], w[lk + xm], P.two_dx);
    double uy = 0.0, vy = 0.0, wy = 0.0;
    if (with_y) {
      uy = centred(u[lk + yp], u[lk + ym], P.two_dy);
      vy = centred(v[lk + yp], v[lk + ym], P.two_dy);
      wy = centred(w[lk + yp], w[lk + ym], P.two_dy);
    }
    const double def2 = deformation(with_y, ux, uy, uz, vx, vy, vz, wx, wy, wz);
    double n2 = stability(P.grav, P.gc, a_k.trho, centred(a_p.trho, a_m.trho, span));
    if constexpr (MOIST) {
      if (a_k.sat)                                                         // level k alone decides, not its neighbours
        n2 = stability_saturated(P.grav, P.gc, M, a_k.temp, a_k.qs, centred(a_p.temp, a_m.temp, span), centred(a_p.qs, a_m.qs, span),
                                 centred(a_p.qt, a_m.qt, span));
    }
    double a, b;
    if constexpr (TKE) {
      double e_new;
      tke_step(e_k, rho_k, def2, n2, zi_p - zi_k, *Q, e_new, a, b);
      tke[lk + c0] = e_new;
      rho_k = rho_p;
    } else {
      eddy(def2, n2, zi_p - zi_k, P.cs, P.prandtl, a, b);
    }
    tk[lk + c0] = a;
    tkh[lk + c0] = b;
    u_m = u_k; v_m = v_k; w_m = w_k; a_m = a_k; zm_m = zm_k;
    u_k = u_p; v_k = v_p; w_k = w_p; a_k = a_p; zm_k = zm_p;
    zi_k = zi_p;
  }
}

// the dry instance, as pam_amd_sgs_smag_coefficients runs it
PAMA_D void coef_column(const double *const *f, const double *zint, const double *zmid, long long level, int nens, int nx, int ny, int nz, int j,
                        int i, int e, const CoefParams &P, double *__restrict__ tk, double *__restrict__ tkh) {
  const MoistParams none{};
  coef_column_t<false>(f, nullptr, nullptr, none, zint, zmid, level, nens, nx, ny, nz, j, i, e, P, tk, tkh);
}

// g at the face between levels k and k+1: dt rho_f K_f / dzf with rho_f and K_f the means of the two levels, left to right
PAMA_D double face_g(double dt, double rho_k, double rho_p, double K_k, double K_p, double dzf) {
  PAMA_NO_CONTRACT
  const double rf = 0.5 * (rho_k + rho_p);
  const double kf = 0.5 * (K_k + K_p);
  const double a = dt * rf;
  const double b = a * kf;
  return b / dzf;
}

// the flux as the row takes it: kinematic as given, or (FLUX) scaled by the class
template <bool FLUX>
PAMA_D double surface_term(int cls, double flux, double scale, double rho0) {
  PAMA_NO_CONTRACT
  if constexpr (FLUX) {
    if (cls == C_HEAT) return flux / (scale * rho0);
    if (cls == C_TRACER) return flux / scale;
  }
  return flux;
}

// backward Euler of one class over one (column, member): nf fields, IN PLACE, by the Thomas algorithm (ascending elimination, descending
// substitution, no pivoting).  Row k: -lower x(k-1) + diag x(k) - upper x(k+1) = r, lower(0) = upper(nz-1) = 0.0.
//   den = diag - lower c'(k-1); c'(k) = upper / den; d'(k) = (r + lower d'(k-1)) / den, c'(-1) = d'(-1) = 0.0;
//   x(nz-1) = d'(nz-1); x(k) = d'(k) + c'(k) x(k+1).
// d' lives in the field itself; c', common to the fields of the class, in cp (cp[k cs]: LDS or a device workspace).  f[t] and sfc[t]
// point at element 0 and get `off` (the flat index inside a level); rd, rv, K likewise; zint, zmid point at (0, e) with stride zs.
// rho is read one level ahead of the level being written and carried in registers, so a field of the table may be rho_v itself: every
// rho_v(k) is read before d'(k) takes its place.  The loads of AHEAD levels are requested before the first of them is used; the first
// NREG fields keep d'(k-1) and x(k+1) in registers, a longer table reads them back from the field
// FLUX: the surface flux of the heat class is a heat flux in W/m2, r += (dt (sfc / (scale rho(0)))) / dz(0) with scale = cp_d, and that
// of the tracer class a mass flux of latent heat, r += (dt (sfc / scale)) / dz(0) with scale = the latent heat; momentum is as without
template <bool FLUX>
PAMA_D void solve_class_t(int cls, double *const *f, int nf, const double *const *sfc, long long off, const double *rd, const double *rv,
                          const double *K, const double *zint, const double *zmid, long long level, long long zs, int nz, double dt, double gc,
                          double *cp, long long cs, double scale) {
  PAMA_NO_CONTRACT
  double prev[NREG];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int t = 0; t < NREG; t++) prev[t] = 0.0;
  rd += off; rv += off; K += off;
  double rho_m = 0.0, rho_k = rd[0] + rv[0], K_k = K[0], zi_k = zint[0], zm_k = zmid[0], g_m = 0.0, dzf_m = 0.0, cprev = 0.0;
  for (int k0 = 0; k0 < nz; k0 += AHEAD) {
    double a_rd[AHEAD], a_rv[AHEAD], a_K[AHEAD], a_zi[AHEAD], a_zm[AHEAD], a_f[AHEAD][NREG];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const int kk = k0 + b;
      const long long kc = kk < nz ? kk : nz - 1, kp = kk + 1 < nz ? kk + 1 : nz - 1, ki = kk + 1 < nz ? kk + 1 : nz;
      a_rd[b] = rd[kp * level]; a_rv[b] = rv[kp * level]; a_K[b] = K[kp * level];
      a_zm[b] = zmid[kp * zs]; a_zi[b] = zint[ki * zs];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int t = 0; t < NREG; t++)
        if (t < nf) a_f[b][t] = f[t][off + kc * level];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const int k = k0 + b;
      if (k >= nz) break;
      const bool first = k == 0, last = k == nz - 1;
      const long long o = off + (long long)k * level;
      const double rho_p = a_rd[b] + a_rv[b];
      const double dz = a_zi[b] - zi_k;
      const double dzf_p = last ? 0.0 : a_zm[b] - zm_k;
      const double g_p = last ? 0.0 : face_g(dt, rho_k, rho_p, K_k, a_K[b], dzf_p);
      const double rdz = rho_k * dz;
      const double gs = g_m + g_p;
      const double diag = 1.0 + gs / rdz;
      double lower, upper;
      if (cls == C_TRACER) {
        lower = first ? 0.0 : g_m / (rho_m * dz);
        upper = last ? 0.0 : g_p / (rho_p * dz);
      } else {
        lower = first ? 0.0 : g_m / rdz;
        upper = last ? 0.0 : g_p / rdz;
      }
      const double den = diag - lower * cprev;
      const double c = upper / den;
      if (!last) cp[(long long)k * cs] = c;
      double heat = 0.0;
      if (cls == C_HEAT) {
        const double hu = upper * dzf_p;
        const double hl = lower * dzf_m;
        heat = gc * (hu - hl);
      }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int t = 0; t < NREG; t++)
        if (t < nf) {
          double r = a_f[b][t];
          if (cls == C_HEAT) r = r + heat;
          if (first && sfc && sfc[t]) r = r + (dt * surface_term<FLUX>(cls, sfc[t][off], scale, rho_k)) / dz;
          const double d = (r + lower * prev[t]) / den;
          f[t][o] = d;
          prev[t] = d;
        }
      for (int t = NREG; t < nf; t++) {
        double r = f[t][o];
        if (cls == C_HEAT) r = r + heat;
        if (first && sfc && sfc[t]) r = r + (dt * surface_term<FLUX>(cls, sfc[t][off], scale, rho_k)) / dz;
        const double p = first ? 0.0 : f[t][o - level];
        f[t][o] = (r + lower * p) / den;
      }
      rho_m = rho_k; rho_k = rho_p; K_k = a_K[b]; zi_k = a_zi[b]; zm_k = a_zm[b]; g_m = g_p; dzf_m = dzf_p; cprev = c;
    }
  }
  // prev[t] is x(nz-1) = d'(nz-1) of the first NREG fields
  for (int k0 = nz - 2; k0 >= 0; k0 -= AHEAD) {
    double a_c[AHEAD], a_f[AHEAD][NREG];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const long long kc = k0 - b > 0 ? k0 - b : 0;
      a_c[b] = cp[kc * cs];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int t = 0; t < NREG; t++)
        if (t < nf) a_f[b][t] = f[t][off + kc * level];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const int k = k0 - b;
      if (k < 0) break;
      const long long o = off + (long long)k * level;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int t = 0; t < NREG; t++)
        if (t < nf) {
          const double x = a_f[b][t] + a_c[b] * prev[t];
          f[t][o] = x;
          prev[t] = x;
        }
      for (int t = NREG; t < nf; t++) f[t][o] = f[t][o] + a_c[b] * f[t][o + level];
    }
  }
}

// the instance without fluxes of heat and vapour, as pam_amd_sgs_smag_diffuse runs it
PAMA_D void solve_class(int cls, double *const *f, int nf, const double *const *sfc, long long off, const double *rd, const double *rv,
                        const double *K, const double *zint, const double *zmid, long long level, long long zs, int nz, double dt, double gc,
                        double *cp, long long cs) {
  solve_class_t<false>(cls, f, nf, sfc, off, rd, rv, K, zint, zmid, level, zs, nz, dt, gc, cp, cs, 0.0);
}

}  // namespace sgs
}  // namespace pama
