// hd_device.h -- the arithmetic of the horizontal hyperdiffusion (the scale-selective fourth-difference damping E3SM-MMF's CRM applies
// between the sponge layer and the physics), as device functions that are plain inline C++ outside hipcc: the HIP kernels in
// modules_kernels.hip call them, and tests/emu/hd_emu.cpp compiles the same bodies with g++ (-ffp-contract=off).  The method is not part
// of the reference tree; the yardstick is the numpy restatement of the contract in tests/hd_ref.py, held bit for bit.
//   one line along x, indices modulo nx: e1 = f[i-1] - f[i-2], e2 = f[i] - f[i-1], e3 = f[i+1] - f[i], e4 = f[i+2] - f[i+1],
//   D4x = (e4 - e1) - 3.0 (e3 - e2), every operation rounded, the product before the subtraction.  D4y likewise; D4 = D4x + D4y with
//   ny > 1, D4 = D4x with ny == 1 (no + 0.0).  f_new = f - c D4, c = dt / (16 tau), the product rounded first, every D4 from the field
//   as it was before the call.  A flagged field then gets the level fill of msa_device.h (P, N in its 16-slot order, vapor_mode).
// Fields are (nz, ny, nx, nens), members fastest; every element offset is 64 bits wide.
// Contraction into fma is switched off inside each body, so the device and the host give the same bits.
#pragma once

#include "msa_device.h"      // max0, min0, vapor_mode, fold, NS: used, not copied

namespace pama {
namespace hd {

namespace ms = pama::msa;
constexpr int NS = ms::NS;
constexpr int MAX_FIELDS = 64;           // fields per call
// the rows of one level a workgroup of the row-ring path holds in LDS: rows 0 and 1 (kept: they are overwritten long before rows
// ny-2 and ny-1 need them), rows ny-2 and ny-1 (read ahead: rows 0 and 1 need them), and a ring of RING rows in between
constexpr int RING = 6;
constexpr int RING_ROWS = RING + 4;

inline double coefficient(double dt, double tau) {      // a host function: once per call
  PAMA_NO_CONTRACT
  return dt / (16.0 * tau);
}

PAMA_D double diff(double hi, double lo) {
  PAMA_NO_CONTRACT
  return hi - lo;
}

// the fourth difference from the four first differences around a cell
PAMA_D double d4(double e1, double e2, double e3, double e4) {
  PAMA_NO_CONTRACT
  const double outer = e4 - e1;
  const double inner = e3 - e2;
  const double three = 3.0 * inner;
  return outer - three;
}

// the same from the five values f[i-2] .. f[i+2]
PAMA_D double d4_values(double m2, double m1, double v, double p1, double p2) {
  return d4(diff(m1, m2), diff(v, m1), diff(p1, v), diff(p2, p1));
}

PAMA_D double d4_sum(double d4x, double d4y) {
  PAMA_NO_CONTRACT
  return d4x + d4y;
}

PAMA_D double update(double f, double c, double D4) {
  PAMA_NO_CONTRACT
  const double p = c * D4;
  return f - p;
}

// ny == 1: one periodic line of nx >= 5 values, `stride` apart, IN PLACE.  The first two original values are kept and the last two
// are read ahead; every other value is read two cells ahead of the cell being written, so it is still the original.  Every first
// difference is computed once and handed on to the next cell.
PAMA_D void line_walk(double *p, long long stride, int nx, double c) {
  const double keep0 = p[0], keep1 = p[stride];
  const double last1 = p[(long long)(nx - 1) * stride];
  double v = keep0, ahead = keep1;                                       // f[i], f[i+1]
  double e1 = diff(last1, p[(long long)(nx - 2) * stride]);              // f[-1] - f[-2]
  double e2 = diff(v, last1);                                            // f[0] - f[-1]
  double e3 = diff(ahead, v);                                            // f[1] - f[0]
  for (int i0 = 0; i0 < nx; i0 += 4) {
    double far[4];                                                       // f[i+2] of four cells, all requested before the first write
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < 4; b++) {
      const int i2 = i0 + b + 2;
      far[b] = i2 < nx ? p[(long long)i2 * stride] : (i2 == nx ? keep0 : keep1);
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < 4; b++) {
      if (i0 + b >= nx) break;
      const double e4 = diff(far[b], ahead);
      p[(long long)(i0 + b) * stride] = update(v, c, d4(e1, e2, e3, e4));
      e1 = e2; e2 = e3; e3 = e4;
      v = ahead; ahead = far[b];
    }
  }
}

// where row r of a level lies in the row-ring path's LDS (in rows); ny >= 5, so the three kinds are disjoint
PAMA_D int ring_slot(int r, int ny) {
  if (r < 2) return r;
  if (r >= ny - 2) return 2 + (r - (ny - 2));
  return 4 + r % RING;
}
PAMA_D bool ring_row(int r, int ny) { return r >= 2 && r < ny - 2; }      // a row that passes through the ring
PAMA_D int wrap(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// one cell of a row from ORIGINAL rows: r0 is the cell's row, rm2 .. rp2 its neighbours in y (unused without `with_y`), each pointing
// at (row, x = 0, the member); xs is the distance between two x neighbours.  Used on LDS rows (row ring) and on the field itself
// (workspace path, where the result goes elsewhere)
PAMA_D double cell_new(const double *rm2, const double *rm1, const double *r0, const double *rp1, const double *rp2, long long xs, int i,
                       int nx, bool with_y, double c) {
  const long long o = (long long)i * xs;
  const double v = r0[o];
  double D4 = d4_values(r0[(long long)wrap(i - 2, nx) * xs], r0[(long long)wrap(i - 1, nx) * xs], v, r0[(long long)wrap(i + 1, nx) * xs],
                        r0[(long long)wrap(i + 2, nx) * xs]);
  if (with_y) D4 = d4_sum(D4, d4_values(rm2[o], rm1[o], v, rp1[o], rp2[o]));
  return update(v, c, D4);
}

// the same for cell (j, i) of a level laid out in place: lvl points at (row 0, x = 0, the member), the rows are rowstride apart.  With
// ny == 1 no row but the cell's own is ever formed
PAMA_D double cell_at(const double *lvl, long long xs, long long rowstride, int nx, int ny, int i, int j, double c) {
  const double *r0 = lvl + (long long)j * rowstride;
  if (ny == 1) return cell_new(r0, r0, r0, r0, r0, xs, i, nx, false, c);
  return cell_new(lvl + (long long)wrap(j - 2, ny) * rowstride, lvl + (long long)wrap(j - 1, ny) * rowstride, r0,
                  lvl + (long long)wrap(j + 1, ny) * rowstride, lvl + (long long)wrap(j + 2, ny) * rowstride, xs, i, nx, true, c);
}

// the fill, sweep 1: one slot's share of P = S(max(f, 0)) and N = S(min(f, 0)) of one (level, member); p points at (k, 0, e)
PAMA_D void fill_walk(const double *p, long long stride, int ncol, int slot, double (&pn)[2]) {
  PAMA_NO_CONTRACT
  pn[0] = 0.0; pn[1] = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 8
#endif
  for (int c = slot; c < ncol; c += NS) {
    const double v = p[(long long)c * stride];
    pn[0] = pn[0] + ms::max0(v);
    pn[1] = pn[1] + ms::min0(v);
  }
}

// the fill, sweep 2: a clean (level, member) is not written at all
PAMA_D double fill_new(double v, int mode, double factor) {
  PAMA_NO_CONTRACT
  if (mode == ms::V_FILL) return ms::max0(v) * factor;
  return 0.0;
}
PAMA_D void fill_apply_walk(double *p, long long stride, int ncol, int slot, int mode, double factor) {
  if (mode == ms::V_CLEAN) return;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
  for (int c = slot; c < ncol; c += NS) {
    const long long o = (long long)c * stride;
    p[o] = fill_new(p[o], mode, factor);
  }
}

}  // namespace hd
}  // namespace pama
