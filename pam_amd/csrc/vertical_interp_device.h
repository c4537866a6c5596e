// vertical_interp_device.h -- the arithmetic of pam::VerticalInterp<ord> (pam_core/vertical_interp.h), orders 3 and 5: the HIP kernels
// in modules_kernels.hip call these bodies, and tests/emu/vertical_interp_emu.cpp compiles the same text with g++ (-ffp-contract=off).
//   ghost interfaces, normalised locations, the matrices   vertical_interp.h:159-169, :181-189, :215-272   (host, once per init)
//   compute_weno_coefs, TV, convexify, sample_val          vertical_interp.h:276-349, :353-373, :126-134   (per cell)
//   the boundary rules and the final average               vertical_interp.h:73-84, :95-111, :118
// The reference's operation order is kept everywhere (sums start from 0 and add their terms in index order, products are rounded
// before they are added); contraction into fma is switched off inside each body, so the device and the host give the same bits.
// Orders 7 and 9 are refused: the reference's sample_val drops a `* z` there (:139, :145).
// The matrices are inverted by the dycore's Gauss-Jordan (awfl_vertical.h: deviation D3, YAKL's matinv_ge is not in the tree).
#pragma once

#include "awfl_vertical.h"   // sten_to_coefs_variable_host, matinv_ge_host

#if defined(__HIPCC__)
#define PAMA_VI_HD __host__ __device__ __forceinline__
#else
#define PAMA_VI_HD inline
#endif

#ifndef PAMA_NO_CONTRACT
#if defined(__clang__)
#define PAMA_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PAMA_NO_CONTRACT
#endif
#endif

namespace pama {
namespace vinterp {

constexpr int BC_ZERO_GRADIENT = 0;   // vertical_interp.h:14-15
constexpr int BC_ZERO_VALUE = 1;
constexpr double EPS = 1.0e-20;       // :12

// sizes of one (level, member) table: recon_lo (hs+1,hs+1,hs+1) then recon_hi (ord,ord): 8 + 9 = 17 doubles (order 3), 27 + 25 = 52
template <int ORD>
struct Dims {
  static_assert(ORD == 3 || ORD == 5, "VerticalInterp: orders 3 and 5 only");
  static constexpr int hs = (ORD - 1) / 2;
  static constexpr int NLO = (hs + 1) * (hs + 1) * (hs + 1);
  static constexpr int NHI = ORD * ORD;
  static constexpr int NTAB = NLO + NHI;
};

// the constructor's ideal weights {1, .., 1, 1000}, convexified (:25-50, :276-280)
template <int ORD>
PAMA_VI_HD void ideal_weights(double (&idl)[Dims<ORD>::hs + 2]) {
  PAMA_NO_CONTRACT
  constexpr int hs = Dims<ORD>::hs;
  for (int i = 0; i < hs + 1; i++) idl[i] = 1.0;
  idl[hs + 1] = 1000.0;
  double sum = 0.0;
  for (int i = 0; i < hs + 2; i++) sum += idl[i];
  for (int i = 0; i < hs + 2; i++) idl[i] /= (sum + EPS);
}

// ---- init: host only -------------------------------------------------------------------------------------------------------------

// zint_ghost(kg) of :159-169; zint: one member's nz+1 interfaces, `stride` apart
inline double ghost_interface(const double *zint, long long stride, int nz, int hs, int kg) {
  PAMA_NO_CONTRACT
  if (kg < hs) {
    const double dz0 = zint[1 * stride] - zint[0];
    return zint[0] - (hs - kg) * dz0;
  } else if (kg < hs + nz + 1) {
    return zint[(long long)(kg - hs) * stride];
  } else {
    const double dztop = zint[(long long)nz * stride] - zint[(long long)(nz - 1) * stride];
    return zint[(long long)nz * stride] + dztop * (kg - hs - nz);
  }
}

// recon_lo (hs+1,hs+1,hs+1) and recon_hi (ord,ord) of level k (:181-209)
template <int ORD>
inline void level_tables(const double *zint, long long stride, int nz, int k, double *lo, double *hi) {
  PAMA_NO_CONTRACT
  constexpr int hs = Dims<ORD>::hs;
  double locs[ORD + 1];
  for (int kk = 0; kk < ORD + 1; kk++) locs[kk] = ghost_interface(zint, stride, nz, hs, k + kk);
  const double zmid = (locs[hs + 1] + locs[hs]) / 2;
  const double dzmid = locs[hs + 1] - locs[hs];
  for (int kk = 0; kk < ORD + 1; kk++) locs[kk] = (locs[kk] - zmid) / dzmid;
  sten_to_coefs_variable_host(ORD, locs, hi);
  for (int i = 0; i < hs + 1; i++) sten_to_coefs_variable_host(hs + 1, locs + i, lo + i * (hs + 1) * (hs + 1));
}

// a member's interfaces are usable: finite and strictly increasing (the reference would divide by zero or build singular matrices)
inline bool column_ok(const double *zint, long long stride, int nz) {
  for (int k = 0; k <= nz; k++) {
    const double z = zint[(long long)k * stride];
    if (!std::isfinite(z)) return false;
    if (k > 0 && !(z > zint[(long long)(k - 1) * stride])) return false;
  }
  return true;
}

// ---- cells_to_edges: host and device ---------------------------------------------------------------------------------------------

// TV of :353-373, the terms added left to right
PAMA_VI_HD double tv2(const double *a) {
  PAMA_NO_CONTRACT
  return 1.0 * (a[1] * a[1]);
}
PAMA_VI_HD double tv3(const double *a) {
  PAMA_NO_CONTRACT
  return 1.0 * (a[1] * a[1]) + 4.3333333333333333333333333333333333333 * (a[2] * a[2]);
}
PAMA_VI_HD double tv5(const double *a) {
  PAMA_NO_CONTRACT
  return 1.0 * (a[1] * a[1]) + 4.3333333333333333333333333333333333333 * (a[2] * a[2]) + 0.5 * a[1] * a[3] +
         39.112500000000000000000000000000000000 * (a[3] * a[3]) + 4.2 * a[2] * a[4] +
         625.83571428571428571428571428571428571 * (a[4] * a[4]);
}
template <int N>
PAMA_VI_HD double tv(const double *a) {
  static_assert(N == 2 || N == 3 || N == 5, "TV of 2, 3 or 5 coefficients");
  if constexpr (N == 2) return tv2(a);
  else if constexpr (N == 3) return tv3(a);
  else return tv5(a);
}

// sample_val (:126-134), Horner
template <int ORD>
PAMA_VI_HD double sample_val(const double (&c)[ORD], double z) {
  PAMA_NO_CONTRACT
  if constexpr (ORD == 3) return (c[2] * z + c[1]) * z + c[0];
  else return (((c[4] * z + c[3]) * z + c[2]) * z + c[1]) * z + c[0];
}

// compute_weno_coefs (:285-349) of one cell, then its two samples: `lower` at -0.5 (limits(1,k)), `upper` at +0.5 (limits(0,k+1)).
// u: the cell's stencil; lo, hi: its level's matrices, entry m at lo[m * stride] / hi[m * stride]; idl: ideal_weights().
template <int ORD, class STRIDE>
PAMA_VI_HD void cell_samples(const double (&u)[ORD], const double *lo, const double *hi, STRIDE stride,
                             const double (&idl)[Dims<ORD>::hs + 2], double &lower, double &upper) {
  PAMA_NO_CONTRACT
  constexpr int hs = Dims<ORD>::hs;
  double a_lo[hs + 1][hs + 1], a_hi[ORD];
  for (int i = 0; i < hs + 1; i++)
    for (int ii = 0; ii < hs + 1; ii++) {
      double tmp = 0;
      for (int s = 0; s < hs + 1; s++) tmp += lo[(STRIDE)((i * (hs + 1) + s) * (hs + 1) + ii) * stride] * u[i + s];
      a_lo[i][ii] = tmp;
    }
  for (int ii = 0; ii < ORD; ii++) {
    double tmp = 0;
    for (int s = 0; s < ORD; s++) tmp += hi[(STRIDE)(s * ORD + ii) * stride] * u[s];
    a_hi[ii] = tmp;
  }
  // the bridge polynomial
  for (int i = 0; i < hs + 1; i++)
    for (int ii = 0; ii < hs + 1; ii++) a_hi[ii] -= idl[i] * a_lo[i][ii];
  for (int ii = 0; ii < ORD; ii++) a_hi[ii] /= idl[hs + 1];
  double t[hs + 2], wts[hs + 2];
  for (int i = 0; i < hs + 1; i++) t[i] = tv<hs + 1>(a_lo[i]);
  t[hs + 1] = tv<ORD>(a_hi);
  for (int i = 0; i < hs + 2; i++) wts[i] = idl[i] / (t[i] * t[i] + EPS);
  double sum = 0.0;
  for (int i = 0; i < hs + 2; i++) sum += wts[i];
  for (int i = 0; i < hs + 2; i++) wts[i] /= (sum + EPS);
  double aw[ORD];
  for (int i = 0; i < ORD; i++) aw[i] = wts[hs + 1] * a_hi[i];
  for (int i = 0; i < hs + 1; i++)
    for (int ii = 0; ii < hs + 1; ii++) aw[ii] += wts[i] * a_lo[i][ii];
  lower = sample_val<ORD>(aw, -0.5);
  upper = sample_val<ORD>(aw, 0.5);
}

// stencil entry of a level outside the column (:73-84): zero, or the column's first / last cell -- `edge_cell`, which for the upper
// end is the window's previous entry (data(nz-1) itself or an earlier copy of it), so that no input is read twice
PAMA_VI_HD double ghost_value(int bc, double edge_cell) { return bc == BC_ZERO_GRADIENT ? edge_cell : 0.0; }

// :118 with the boundary rules of :95-111 applied to the two estimates
PAMA_VI_HD double edge_average(double from_below, double from_above) {
  PAMA_NO_CONTRACT
  return 0.5 * (from_below + from_above);
}
PAMA_VI_HD double bottom_edge(int bc_lower, double lower0) {
  return bc_lower == BC_ZERO_VALUE ? edge_average(0.0, 0.0) : edge_average(lower0, lower0);
}
PAMA_VI_HD double top_edge(int bc_upper, double upper_last) {
  return bc_upper == BC_ZERO_VALUE ? edge_average(0.0, 0.0) : edge_average(upper_last, upper_last);
}

// One column marched upwards with a rolling window of ORD values: every input is read once, every cell's polynomial is computed once
// and sampled at both of its edges.  data / edges: the column's level 0, levels `dstride` apart; tab_lo / tab_hi: level 0 of the
// column's matrices, entries `tstride` and levels `tlevel` apart.  The HIP kernels are this loop with the table staged and the loads
// issued ahead.
template <int ORD, class IDX>
PAMA_VI_HD void march_column(int nz, const double *data, IDX dstride, const double *tab_lo, const double *tab_hi, IDX tstride,
                             IDX tlevel_lo, IDX tlevel_hi, int bc_lower, int bc_upper, double *edges) {
  constexpr int hs = Dims<ORD>::hs;
  double idl[hs + 2];
  ideal_weights<ORD>(idl);
  double u[ORD];
  u[hs] = data[0];
  for (int kk = 0; kk < hs; kk++) u[kk] = ghost_value(bc_lower, u[hs]);
  for (int kk = hs + 1; kk < ORD; kk++) u[kk] = (kk - hs < nz) ? data[(IDX)(kk - hs) * dstride] : ghost_value(bc_upper, u[kk - 1]);
  double prev_upper = 0.0;
  for (int k = 0; k < nz; k++) {
    double lower, upper;
    cell_samples<ORD, IDX>(u, tab_lo + (IDX)k * tlevel_lo, tab_hi + (IDX)k * tlevel_hi, tstride, idl, lower, upper);
    edges[(IDX)k * dstride] = (k == 0) ? bottom_edge(bc_lower, lower) : edge_average(prev_upper, lower);
    prev_upper = upper;
    for (int kk = 0; kk < ORD - 1; kk++) u[kk] = u[kk + 1];
    u[ORD - 1] = (k + hs + 1 < nz) ? data[(IDX)(k + hs + 1) * dstride] : ghost_value(bc_upper, u[ORD - 2]);
  }
  edges[(IDX)nz * dstride] = top_edge(bc_upper, prev_upper);
}

}  // namespace vinterp
}  // namespace pama
