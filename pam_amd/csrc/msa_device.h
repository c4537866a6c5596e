// msa_device.h -- the arithmetic of CRM mean-state acceleration (Jones, Bretherton and Pritchard 2015; E3SM-MMF's crm_accel_factor,
// crm_accel_uv), as device functions that are plain inline C++ outside hipcc: the HIP kernels in modules_kernels.hip call them, and
// tests/emu/msa_emu.cpp compiles the same bodies with g++ (-ffp-contract=off).  The method is not part of the reference tree; the yardstick is the numpy
// restatement of the contract in tests/msa_ref.py, held bit for bit.
//   level mean M(f)(k,e): cell c belongs to slot c % 16; a slot adds f(k,c,e) * r (r = 1/ncol, the product rounded first) over its
//   cells in ascending c from 0.0; the 16 slot sums are added in ascending slot order from 0.0 (an empty slot adds +0.0).
//   level sum  S(f)(k,e): the same without r.
// Fields are (nz, ncol, nens), members fastest: `p` points at (k, 0, e) and `stride` is nens, always 64 bits wide.
// Contraction into fma is switched off inside each body, so the device and the host give the same bits.
#pragma once

#ifndef PAMA_D      // as awfl_device.h has it
#if defined(__HIPCC__)
#define PAMA_D __device__ __forceinline__
#else
#define PAMA_D inline
#endif
#endif

#ifndef PAMA_NO_CONTRACT
#if defined(__clang__)
#define PAMA_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PAMA_NO_CONTRACT
#endif
#endif

namespace pama {
namespace msa {

constexpr int NS = 16;                                   // slots per (level, member)
enum { Q_T, Q_Q, Q_U, Q_V, NQ };                         // the four accelerated quantities: temp, total water, uvel, vvel
enum { F_TEMP, F_VAPOR, F_CLOUD, F_ICE, F_U, F_V, NF };  // the field table; cloud and ice may be absent (null)

PAMA_D double r_ncol(int ncol) { return 1.0 / (double)ncol; }

// one step of a slot's walk: acc + v * r, the product rounded before the add
PAMA_D double mean_add(double acc, double v, double r) {
  PAMA_NO_CONTRACT
  return acc + v * r;
}

// q = water_vapor + cloud + ice, left to right; an absent species is skipped (no + 0.0)
PAMA_D double total_water(const double *vapor, const double *cloud, const double *ice, long long o) {
  PAMA_NO_CONTRACT
  double q = vapor[o];
  if (cloud) q = q + cloud[o];
  if (ice) q = q + ice[o];
  return q;
}

// the 16 slot sums of one (level, member) in ascending slot order from 0.0: what slot_reduce does through LDS on the device
PAMA_D double fold(const double *part, long long step) {
  PAMA_NO_CONTRACT
  double a = 0.0;
  for (int sl = 0; sl < NS; sl++) a = a + part[(long long)sl * step];
  return a;
}

// one slot's share of the four level means of one (level, member); f[i] points at (k, 0, e) of field i
PAMA_D void mean_walk(const double *const *f, long long stride, int ncol, int slot, double (&acc)[NQ]) {
  const double r = r_ncol(ncol);
  acc[Q_T] = 0.0; acc[Q_Q] = 0.0; acc[Q_U] = 0.0; acc[Q_V] = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
  for (int c = slot; c < ncol; c += NS) {
    const long long o = (long long)c * stride;
    acc[Q_T] = mean_add(acc[Q_T], f[F_TEMP][o], r);
    acc[Q_Q] = mean_add(acc[Q_Q], total_water(f[F_VAPOR], f[F_CLOUD], f[F_ICE], o), r);
    acc[Q_U] = mean_add(acc[Q_U], f[F_U][o], r);
    acc[Q_V] = mean_add(acc[Q_V], f[F_V][o], r);
  }
}

// tendencies: the change of the level mean over the CRM step
PAMA_D double tendency(double mean, double save) {
  PAMA_NO_CONTRACT
  return mean - save;
}

// the acceleration ceases where |tend_T| <= max_ttend does NOT hold: a NaN or an infinite tendency ceases
PAMA_D bool ceases(double tend_t, double max_ttend) { return !((tend_t < 0 ? -tend_t : tend_t) <= max_ttend); }

// d_x = a * tend_x, once per (level, member)
PAMA_D double increment(double accel_factor, double tend) {
  PAMA_NO_CONTRACT
  return accel_factor * tend;
}

PAMA_D double plus(double v, double d) {
  PAMA_NO_CONTRACT
  return v + d;
}
PAMA_D double max0(double v) { return v > 0 ? v : 0.0; }   // a NaN gives 0.0
PAMA_D double min0(double v) { return v < 0 ? v : 0.0; }

// sweep 1 of apply: one slot's share of P = S(max(v', 0)) and N = S(min(v', 0)), v' = water_vapor + d_q
PAMA_D void vapor_walk(const double *vapor, long long stride, int ncol, int slot, double d_q, double (&pn)[2]) {
  PAMA_NO_CONTRACT
  pn[0] = 0.0; pn[1] = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 8
#endif
  for (int c = slot; c < ncol; c += NS) {
    const double v = plus(vapor[(long long)c * stride], d_q);
    pn[0] = pn[0] + max0(v);
    pn[1] = pn[1] + min0(v);
  }
}

// what the level of one member does with its vapour: 0 = no negative value, v' is kept; 1 = filled, max(v', 0) * factor with
// factor = 1 + N / P (a true division, once per (level, member)); 2 = P + N <= 0 (or not a number): the whole level becomes 0
enum { V_CLEAN, V_FILL, V_ZERO };
PAMA_D int vapor_mode(double P, double N, double &factor) {
  PAMA_NO_CONTRACT
  factor = 1.0;
  if (!(N < 0)) return V_CLEAN;
  if (P + N > 0) { factor = 1.0 + N / P; return V_FILL; }
  return V_ZERO;
}
PAMA_D double vapor_new(double v_old, double d_q, int mode, double factor) {
  PAMA_NO_CONTRACT
  const double v = plus(v_old, d_q);
  if (mode == V_CLEAN) return v;
  if (mode == V_FILL) return max0(v) * factor;
  return 0.0;
}

// sweep 2 of apply: one slot's cells of one (level, member).  uvel and vvel are not touched (not read either) unless accel_uv
PAMA_D void apply_walk(double *temp, double *vapor, double *uvel, double *vvel, long long stride, int ncol, int slot, double d_t, double d_q,
                       double d_u, double d_v, bool accel_uv, int mode, double factor) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
  for (int c = slot; c < ncol; c += NS) {
    const long long o = (long long)c * stride;
    vapor[o] = vapor_new(vapor[o], d_q, mode, factor);
    temp[o] = plus(temp[o], d_t);
    if (accel_uv) {
      uvel[o] = plus(uvel[o], d_u);
      vvel[o] = plus(vvel[o], d_v);
    }
  }
}

}  // namespace msa
}  // namespace pama
