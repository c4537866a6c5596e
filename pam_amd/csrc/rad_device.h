// rad_device.h -- the arithmetic of the CRM-to-GCM handoff (the radiation column aggregates of E3SM-MMF's crm_rad_* arrays and the CRM
// feedback tendencies of its crm_output), as device functions that are plain inline C++ outside hipcc: the HIP kernels in
// modules_kernels.hip call them, and tests/emu/rad_emu.cpp compiles the same bodies with g++ (-ffp-contract=off).  The methods are not
// part of the reference tree; the yardstick is the numpy restatement of the contract in tests/rad_ref.py, held bit for bit (DESIGN.md
// section 8).
//   per-cell values: d = rho_d + rho_v; qx = rho_x / d (IEEE divisions, d == 0 is not special); cld = cldfrac, or 1.0 / 0.0 by
//   rho_c + rho_i > 0 (an absent species skipped, a NaN gives 0.0).  An absent species is not computed at all.
//   group mean A(v)(k,jr,ir,e), r = 1 / (gx gy): the cell at local row jj, local column ii has g = jj gx + ii and belongs to slot g % 16;
//   a slot adds v * r (the product rounded first) over its cells in ascending g from 0.0; the 16 slot sums are added in ascending slot
//   order from 0.0 (an empty slot adds +0.0).  With the whole level as the group this is msa_device.h's level mean M.
// Fields are (nz, ny, nx, nens), members fastest: the pointers of a walk stand at the group's first cell of the walker's member, `stride`
// is nens and `rowstride` nx * nens, always 64 bits wide.  A walk never divides: it steps (jj, ii) by 16 cells with 16 / gx and 16 % gx.
// Contraction into fma is switched off inside each body, so the device and the host give the same bits.
#pragma once

#include "msa_device.h"      // NS, mean_add, fold: the slot order itself

namespace pama {
namespace rad {

constexpr int NS = msa::NS;
// the field table of a walk: the aggregate reads [F_TEMP, F_CLD], the feedback all but F_CLD; rho_c, rho_i, cldfrac may be absent (null)
enum { F_TEMP, F_RHOD, F_RHOV, F_RHOC, F_RHOI, F_CLD, F_U, F_V, NF };
enum { A_T, A_QV, A_QC, A_QI, A_CLD, NA };                // the aggregates: rad_temperature, rad_qv, rad_qc, rad_qi, rad_cld
enum { B_T, B_QV, B_QC, B_QI, B_U, B_V, NB };             // the feedback's quantities
enum { G_TEMP, G_RHOD, G_RHOV, G_RHOC, G_RHOI, G_U, G_V, NG };      // the feedback's gcm table

PAMA_D double r_cells(int gx, int gy) { return 1.0 / ((double)gx * (double)gy); }

PAMA_D double moist_density(double rho_d, double rho_v) {
  PAMA_NO_CONTRACT
  return rho_d + rho_v;
}
PAMA_D double mixing_ratio(double rho_x, double d) {
  PAMA_NO_CONTRACT
  return rho_x / d;
}
// without cldfrac: 1.0 where the condensate present is positive, 0.0 where it is not (a NaN, or no condensate at all)
PAMA_D double cloud_flag(bool has_c, double rho_c, bool has_i, double rho_i) {
  PAMA_NO_CONTRACT
  if (!has_c && !has_i) return 0.0;
  const double s = has_c ? (has_i ? rho_c + rho_i : rho_c) : rho_i;
  return s > 0 ? 1.0 : 0.0;
}

// the per-cell values of the two entry points; v[] of an absent species is left alone
struct Aggregate {
  static constexpr int NQ = NA;
  static PAMA_D void cell(const double *const *f, long long o, double (&v)[NA]) {
    const double d = moist_density(f[F_RHOD][o], f[F_RHOV][o]);
    const bool has_c = f[F_RHOC] != nullptr, has_i = f[F_RHOI] != nullptr;
    const double rho_c = has_c ? f[F_RHOC][o] : 0.0, rho_i = has_i ? f[F_RHOI][o] : 0.0;
    v[A_T] = f[F_TEMP][o];
    v[A_QV] = mixing_ratio(f[F_RHOV][o], d);
    if (has_c) v[A_QC] = mixing_ratio(rho_c, d);
    if (has_i) v[A_QI] = mixing_ratio(rho_i, d);
    v[A_CLD] = f[F_CLD] ? f[F_CLD][o] : cloud_flag(has_c, rho_c, has_i, rho_i);
  }
};
struct Feedback {
  static constexpr int NQ = NB;
  static PAMA_D void cell(const double *const *f, long long o, double (&v)[NB]) {
    const double d = moist_density(f[F_RHOD][o], f[F_RHOV][o]);
    v[B_T] = f[F_TEMP][o];
    v[B_QV] = mixing_ratio(f[F_RHOV][o], d);
    if (f[F_RHOC]) v[B_QC] = mixing_ratio(f[F_RHOC][o], d);
    if (f[F_RHOI]) v[B_QI] = mixing_ratio(f[F_RHOI][o], d);
    v[B_U] = f[F_U][o];
    v[B_V] = f[F_V][o];
  }
};

// where a walk stands inside its group, and how it moves on by one cell and by the 16 cells between two cells of one slot
struct Cursor {
  int jj, ii;
};
PAMA_D void advance(Cursor &c, int dj, int di, int gx) {
  c.jj += dj;
  c.ii += di;
  if (c.ii >= gx) { c.ii -= gx; c.jj++; }
}

// ONE slot's share of a group: the cells g = slot, slot + 16, ... < ncell in ascending order, c standing at cell `slot`.  UNROLL: cells
// whose loads are in flight together on the device (a long walk wants four, the short walks of a small group two)
template <class K, int UNROLL = 2>
PAMA_D void slot_walk(const double *const *f, long long stride, long long rowstride, int gx, int ncell, int slot, Cursor c, double r,
                      double (&acc)[K::NQ]) {
  const int dj = NS / gx, di = NS % gx;
#pragma unroll
  for (int q = 0; q < K::NQ; q++) acc[q] = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll UNROLL
#endif
  for (int g = slot; g < ncell; g += NS) {
    double v[K::NQ];
#pragma unroll
    for (int q = 0; q < K::NQ; q++) v[q] = 0.0;      // an absent species adds 0.0 * r to a sum nobody reads
    K::cell(f, (long long)c.jj * rowstride + (long long)c.ii * stride, v);
#pragma unroll
    for (int q = 0; q < K::NQ; q++) acc[q] = msa::mean_add(acc[q], v[q], r);
    advance(c, dj, di, gx);
  }
}

// slots [s0, s0 + ns) of a group by ONE walker, folded in ascending order onto tot (0.0 at s0 == 0): ns == 16 is the whole group mean
template <class K>
PAMA_D void slots_walk(const double *const *f, long long stride, long long rowstride, int gx, int ncell, int s0, int ns, double r,
                       double (&tot)[K::NQ]) {
  PAMA_NO_CONTRACT
  Cursor c{s0 / gx, s0 % gx};
  for (int s = s0; s < s0 + ns; s++) {
    double acc[K::NQ];
    slot_walk<K>(f, stride, rowstride, gx, ncell, s, c, r, acc);
#pragma unroll
    for (int q = 0; q < K::NQ; q++) tot[q] = tot[q] + acc[q];
    advance(c, 0, 1, gx);
  }
}

// rad_x = rad_x + A(x) * factor, the product rounded first
PAMA_D double accumulate(double old, double a, double factor) {
  PAMA_NO_CONTRACT
  return old + a * factor;
}

// the GCM's value of quantity q at one (level, member): g[i] is the value of gcm table entry i there (absent: anything)
PAMA_D double gcm_value(const double (&g)[NG], int q) {
  if (q == B_T) return g[G_TEMP];
  if (q == B_U) return g[G_U];
  if (q == B_V) return g[G_V];
  const double d = moist_density(g[G_RHOD], g[G_RHOV]);
  return mixing_ratio(q == B_QV ? g[G_RHOV] : q == B_QC ? g[G_RHOC] : g[G_RHOI], d);
}
PAMA_D double feedback_tendency(double mean, double gcm, double gcm_dt) {
  PAMA_NO_CONTRACT
  return (mean - gcm) / gcm_dt;
}

}  // namespace rad
}  // namespace pama
