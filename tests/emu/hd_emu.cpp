// hd_emu.cpp -- HOST EMULATION of the hyperdiffusion kernels (pam_amd/csrc/hd_device.h, compiled with g++ -ffp-contract=off).
// TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror the kernels of modules_kernels.hip
// and work IN PLACE on the field, as they do: the line walker per (level, member); the row ring per (level, block of `me` members) with
// an array laid out like the kernel's LDS (hd::RING_ROWS rows of nx * me, slots from hd::ring_slot) that is filled with a poison value
// first, so a row read before it was loaded shows; the workspace path; and the fill on mean-state acceleration's block shape.
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../pam_amd/csrc/hd_device.h"

using namespace pama::hd;

extern "C" {

// field: (nz, 1, nx, nens)
void emu_hd_line(int nens, int nx, int nz, double *field, double c) {
  for (long long t = 0; t < (long long)nz * nens; t++) {
    const long long k = t / nens, e = t % nens;
    line_walk(field + k * nx * nens + e, (long long)nens, nx, c);
  }
}

// field: (nz, ny, nx, nens), ny >= 5; me: members per workgroup, a power of two
void emu_hd_ring(int nens, int nx, int ny, int nz, int me, double *field, double c) {
  if (me < 1 || (me & (me - 1)) != 0 || ny < 5) return;
  const int rowlen = nx * me;
  const long long rowstride = (long long)nx * nens;
  std::vector<double> lds((size_t)RING_ROWS * rowlen);
  for (int k = 0; k < nz; k++)
    for (int e0 = 0; e0 < nens; e0 += me) {
      const int mw = nens - e0 < me ? nens - e0 : me;
      double *f = field + (long long)k * ny * rowstride + e0;
      for (size_t i = 0; i < lds.size(); i++) lds[i] = std::nan("");
      auto load = [&](int r) {
        double *dst = lds.data() + (size_t)ring_slot(r, ny) * rowlen;
        for (int t = 0; t < rowlen; t++) {
          const int m = t % me, i = t / me;
          if (m < mw) dst[t] = f[(long long)r * rowstride + (long long)i * nens + m];
        }
      };
      // a ring row is requested from the field before the step's cells are written and put into the ring after them, as the kernel does it
      std::vector<double> pre((size_t)rowlen);
      auto fetch = [&](int r) {
        for (int t = 0; t < rowlen; t++) {
          const int m = t % me, i = t / me;
          if (m < mw) pre[t] = f[(long long)r * rowstride + (long long)i * nens + m];
        }
      };
      auto stash = [&](int r) {
        double *dst = lds.data() + (size_t)ring_slot(r, ny) * rowlen;
        for (int t = 0; t < rowlen; t++)
          if (t % me < mw) dst[t] = pre[t];
      };
      load(0); load(1); load(ny - 2); load(ny - 1);
      if (ring_row(2, ny)) load(2);
      for (int j = 0; j < ny; j++) {
        if (ring_row(j + 3, ny)) fetch(j + 3);
        const double *rm2 = lds.data() + (size_t)ring_slot(wrap(j - 2, ny), ny) * rowlen, *rm1 = lds.data() + (size_t)ring_slot(wrap(j - 1, ny), ny) * rowlen;
        const double *r0 = lds.data() + (size_t)ring_slot(j, ny) * rowlen;
        const double *rp1 = lds.data() + (size_t)ring_slot(wrap(j + 1, ny), ny) * rowlen, *rp2 = lds.data() + (size_t)ring_slot(wrap(j + 2, ny), ny) * rowlen;
        for (int t = 0; t < rowlen; t++) {
          const int m = t % me, i = t / me;
          if (m < mw) f[(long long)j * rowstride + (long long)i * nens + m] = cell_new(rm2 + m, rm1 + m, r0 + m, rp1 + m, rp2 + m, (long long)me, i, nx, true, c);
        }
        if (ring_row(j + 3, ny)) stash(j + 3);
      }
    }
}

// field: (nz, ny, nx, nens); ws: as large
void emu_hd_workspace(int nens, int nx, int ny, int nz, double *field, double *ws, double c) {
  const long long rowstride = (long long)nx * nens, total = (long long)nz * ny * rowstride;
  for (long long idx = 0; idx < total; idx++) {
    const long long cell = idx / nens, row = cell / nx;
    const int e = (int)(idx - cell * nens), i = (int)(cell - row * nx);
    const long long k = row / ny;
    const int j = (int)(row - k * ny);
    const double *lvl = field + k * ny * rowstride + e;
    ws[idx] = cell_at(lvl, (long long)nens, rowstride, nx, ny, i, j, c);
  }
  for (long long idx = 0; idx < total; idx++) field[idx] = ws[idx];
}

// field: (nz, ncol, nens); me: members per workgroup (1..64); written: (nz, nens), 1 where the fill pass wrote the level
void emu_hd_fill(int nens, int ncol, int nz, int me, double *field, int *written) {
  if (me < 1 || me > 64) return;
  std::vector<double> red((size_t)2 * NS * 64);
  for (int k = 0; k < nz; k++)
    for (int blk = 0; blk * me < nens; blk++) {
      for (int slot = 0; slot < NS; slot++)
        for (int m = 0; m < me; m++) {
          const int e = blk * me + m;
          double pn[2] = {0.0, 0.0};
          if (e < nens) fill_walk(field + (long long)k * ncol * nens + e, (long long)nens, ncol, slot, pn);
          red[((size_t)0 * NS + slot) * 64 + m] = pn[0];
          red[((size_t)1 * NS + slot) * 64 + m] = pn[1];
        }
      for (int slot = 0; slot < NS; slot++)
        for (int m = 0; m < me; m++) {
          const int e = blk * me + m;
          if (e >= nens) continue;
          const double P = ms::fold(&red[(size_t)0 * NS * 64 + m], 64), N = ms::fold(&red[(size_t)1 * NS * 64 + m], 64);
          double factor;
          const int mode = ms::vapor_mode(P, N, factor);
          written[(long long)k * nens + e] = mode != ms::V_CLEAN;
          fill_apply_walk(field + (long long)k * ncol * nens + e, (long long)nens, ncol, slot, mode, factor);
        }
    }
}

double emu_hd_coefficient(double dt, double tau) { return coefficient(dt, tau); }

// the same bodies at strides of the caller's choice, a handful of cells each: the 64-bit offsets.  base points at the first cell
void emu_hd_line_at(double *base, long long stride, int nx, double c) { line_walk(base, stride, nx, c); }

// -> f_new of cell (j, i) of a level whose x neighbours are xs apart and whose rows are rowstride apart
double emu_hd_cell_at(const double *base, long long xs, long long rowstride, int nx, int ny, int i, int j, double c) {
  return cell_at(base, xs, rowstride, nx, ny, i, j, c);
}

// the fill of one (level, member) whose ncol cells are stride apart; -> the mode
int emu_hd_fill_at(double *base, long long stride, int ncol) {
  double part[2][NS];
  for (int slot = 0; slot < NS; slot++) {
    double pn[2];
    fill_walk(base, stride, ncol, slot, pn);
    part[0][slot] = pn[0];
    part[1][slot] = pn[1];
  }
  double factor;
  const int mode = ms::vapor_mode(ms::fold(part[0], 1), ms::fold(part[1], 1), factor);
  for (int slot = 0; slot < NS; slot++) fill_apply_walk(base, stride, ncol, slot, mode, factor);
  return mode;
}

}
