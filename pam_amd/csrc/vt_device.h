// vt_device.h -- the arithmetic of CRM variance transport (Hannah and Pressel 2022; E3SM-MMF's use_MMF_VT, bulk form), as device
// functions that are plain inline C++ outside hipcc: the HIP kernels in modules_kernels.hip call them, and tests/emu/vt_emu.cpp compiles
// the same bodies with g++ (-ffp-contract=off).  The method is not part of the reference tree; the yardstick is the numpy restatement of
// the contract in tests/vt_ref.py, held bit for bit.
//   level statistics of a quantity x at (k,e), ONE pass, shifted by the level's first cell: c = x(k,0,e), d(i) = x(k,i,e) - c,
//   A = M(d), B = M(d d) (d d rounded, then times r rounded, then added), mean = c + A, var = B - A A (A A rounded, no fma), a negative
//   var becomes 0.0 and a NaN stays.  M is the level mean of msa_device.h: slot i % 16, ascending cells, ascending slots, from 0.0.
// Fields are (nz, ncol, nens), members fastest: `f[i]` points at (k, 0, e) of field i and `stride` is nens, always 64 bits wide.
// Contraction into fma is switched off inside each body, so the device and the host give the same bits.
#pragma once
#include <cmath>

#include "msa_device.h"      // mean_add, total_water, fold, plus, max0, min0, vapor_mode, vapor_new: used, not copied

namespace pama {
namespace vt {

namespace ms = pama::msa;
constexpr int NS = ms::NS;
enum { Q_T, Q_Q, Q_U, NQ };                              // the three transported quantities: temp, total water, uvel
enum { F_TEMP, F_VAPOR, F_CLOUD, F_ICE, F_U, NF };       // the field table; cloud and ice may be absent (null), uvel only with use_u

PAMA_D double minus(double a, double b) {
  PAMA_NO_CONTRACT
  return a - b;
}
PAMA_D double times(double a, double b) {
  PAMA_NO_CONTRACT
  return a * b;
}

// the shifts of one (level, member): the quantities at the level's first cell
PAMA_D void first_cell(const double *const *f, bool use_u, double (&c)[NQ]) {
  c[Q_T] = f[F_TEMP][0];
  c[Q_Q] = ms::total_water(f[F_VAPOR], f[F_CLOUD], f[F_ICE], 0);
  c[Q_U] = use_u ? f[F_U][0] : 0.0;
}

// one slot's share of A = M(d) (a[0..3)) and B = M(d d) (b[0..3)) of one (level, member); uvel is not read unless use_u
PAMA_D void stats_walk(const double *const *f, long long stride, int ncol, int slot, bool use_u, const double (&c)[NQ], double (&a)[NQ],
                       double (&b)[NQ]) {
  const double r = ms::r_ncol(ncol);
  for (int q = 0; q < NQ; q++) { a[q] = 0.0; b[q] = 0.0; }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
  for (int i = slot; i < ncol; i += NS) {
    const long long o = (long long)i * stride;
    const double dt = minus(f[F_TEMP][o], c[Q_T]);
    a[Q_T] = ms::mean_add(a[Q_T], dt, r);
    b[Q_T] = ms::mean_add(b[Q_T], times(dt, dt), r);
    const double dq = minus(ms::total_water(f[F_VAPOR], f[F_CLOUD], f[F_ICE], o), c[Q_Q]);
    a[Q_Q] = ms::mean_add(a[Q_Q], dq, r);
    b[Q_Q] = ms::mean_add(b[Q_Q], times(dq, dq), r);
    if (use_u) {
      const double du = minus(f[F_U][o], c[Q_U]);
      a[Q_U] = ms::mean_add(a[Q_U], du, r);
      b[Q_U] = ms::mean_add(b[Q_U], times(du, du), r);
    }
  }
}

// mean = c + A; var = B - A A, never negative; a NaN stays a NaN
PAMA_D void finish(double c, double A, double B, double &mean, double &var) {
  PAMA_NO_CONTRACT
  mean = c + A;
  const double aa = A * A;
  const double v = B - aa;
  var = v < 0 ? 0.0 : v;
}

// the factor by which the anomalies of one (level, member) are stretched: one division and one root
PAMA_D double scale(double var, double tend, double dt, double lim) {
  PAMA_NO_CONTRACT
  if (!(var > 0)) return 1.0;
  const double grown = dt * tend;
  const double ratio = 1.0 + grown / var;
  if (ratio != ratio) return 1.0;
  const double s = std::sqrt(ratio > 0 ? ratio : 0.0);
  const double lo = 1.0 - lim, hi = 1.0 + lim;
  return s < lo ? lo : (s > hi ? hi : s);
}

// the variance the CRM produced over the GCM step, as a tendency: one true division
PAMA_D double feedback(double var_now, double var_start, double gcm_dt) {
  PAMA_NO_CONTRACT
  return (var_now - var_start) / gcm_dt;
}

// g = s - 1; g (x - mean), the product rounded before it is added to anything
PAMA_D double gain(double s) { return minus(s, 1.0); }
PAMA_D double stretch(double g, double x, double mean) { return times(g, minus(x, mean)); }

// sweep 1 of apply: one slot's share of P = S(max(v', 0)) and N = S(min(v', 0)), v' = water_vapor + g_q (q - mean_q)
PAMA_D void vapor_walk(const double *const *f, long long stride, int ncol, int slot, double g_q, double mean_q, double (&pn)[2]) {
  PAMA_NO_CONTRACT
  pn[0] = 0.0; pn[1] = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
  for (int i = slot; i < ncol; i += NS) {
    const long long o = (long long)i * stride;
    const double v = ms::plus(f[F_VAPOR][o], stretch(g_q, ms::total_water(f[F_VAPOR], f[F_CLOUD], f[F_ICE], o), mean_q));
    pn[0] = pn[0] + ms::max0(v);
    pn[1] = pn[1] + ms::min0(v);
  }
}

// sweep 2 of apply: one slot's cells of one (level, member), each read and written once.  A quantity whose g is 0 keeps the bits of its
// fields (they are not read either); cloud and ice are read where g_q != 0 and never written
PAMA_D void apply_walk(double *temp, double *vapor, const double *cloud, const double *ice, double *uvel, long long stride, int ncol, int slot,
                       const double (&g)[NQ], const double (&mean)[NQ], bool use_u, int mode, double factor) {
  const bool do_t = g[Q_T] != 0, do_q = g[Q_Q] != 0, do_u = use_u && g[Q_U] != 0;
  if (!do_t && !do_q && !do_u) return;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
  for (int i = slot; i < ncol; i += NS) {
    const long long o = (long long)i * stride;
    if (do_q) vapor[o] = ms::vapor_new(vapor[o], stretch(g[Q_Q], ms::total_water(vapor, cloud, ice, o), mean[Q_Q]), mode, factor);
    if (do_t) temp[o] = ms::plus(temp[o], stretch(g[Q_T], temp[o], mean[Q_T]));
    if (do_u) uvel[o] = ms::plus(uvel[o], stretch(g[Q_U], uvel[o], mean[Q_U]));
  }
}

}  // namespace vt
}  // namespace pama
