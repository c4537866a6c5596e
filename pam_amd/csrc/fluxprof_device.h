// fluxprof_device.h -- the arithmetic of the CRM flux profiles (the convective mass fluxes by conditional sampling mcup, mcdn, mcuup, mcudn
// and the cloud fraction profile cld of SAM / E3SM-MMF's crm_output, the resolved vertical fluxes of heat, total water and horizontal
// momentum and the resolved turbulence kinetic energy; SAM and E3SM-MMF sum them with one atomicAdd per cell and quantity), as device
// functions that are plain inline C++ outside hipcc: the HIP kernel in modules_kernels.hip calls them, and tests/emu/fluxprof_emu.cpp
// compiles the same bodies with g++ (-ffp-contract=off).  The method is not part of the reference tree; the yardstick is the numpy
// restatement of the contract in tests/fluxprof_ref.py, held bit for bit.
//   per cell: rho = rho_d + rho_v; m = rho w; q = total_water / rho; cloudy where rho_c + rho_i > qc_threshold rho; up where w > 0.
//   sampled sums: M(m) over the cells of one class each (cloudy/up, cloudy/not up, clear/up, clear/not up) and M(1) over the cloudy cells.
//   shifted moments, vt_device.h's one-pass form: c_x = x at the level's first cell, d_x = x - c_x, A_x = M(d_x) for m, temp, q, uvel,
//   vvel, wvel; B_mx = M(d_m d_x) for temp, q, uvel, vvel; B_xx = M(d_x d_x) for uvel, vvel, wvel.
//   finish: flux_x = B_mx - A_m A_x; var_x = vt::finish; tke = 0.5 ((var_u + var_v) + var_w).
// M is the level mean of msa_device.h: slot c % 16, ascending cells, ascending slots, from 0.0.
// Fields are (nz, ncol, nens), members fastest: `f[i]` points at (k, 0, e) of field i and `stride` is nens, always 64 bits wide.
// Contraction into fma is switched off inside each body, so the device and the host give the same bits.
#pragma once

#include "vt_device.h"       // minus, times, finish; msa_device.h: NS, mean_add, total_water, r_ncol, plus: used, not copied

namespace pama {
namespace fluxprof {

namespace ms = pama::msa;
constexpr int NS = ms::NS;
enum { F_RHOD, F_VAPOR, F_CLOUD, F_ICE, F_TEMP, F_U, F_V, F_W, NF };                            // the field table; cloud and ice may be absent (null)
enum { O_MCUP, O_MCDN, O_MCUUP, O_MCUDN, O_CLD, O_FLUX_T, O_FLUX_Q, O_FLUX_U, O_FLUX_V, O_TKE, NO };   // the outputs
enum { X_M, X_T, X_Q, X_U, X_V, X_W, NX };                                                      // the shifted quantities of a cell
constexpr int NCLS = 4;                                                                         // the classes, in the order of the outputs
// the 18 sums of a slot: the four classes' M(m) and the cloudy cells' M(1); A_x of the six quantities; B_mx of temp, q, uvel, vvel; B_xx of
// uvel, vvel, wvel
enum { S_CLS = 0, S_CLD = NCLS, S_A = S_CLD + 1, S_BM = S_A + NX, S_BX = S_BM + 4, NSUM = S_BX + 3 };
// cells whose loads are in flight per lane in the kernel's walk, eight loads each.  tools/kernel_resources.py gives 94 / 124 VGPRs at 1 / 2
// without scratch and 128 VGPRs with 28 / 84 B of scratch per lane at 3 / 4 (the block is 1024 lanes: 128 VGPRs at the most); 2 is the
// most that compiles without scratch
constexpr int WALK_UNROLL = 2;

PAMA_D double ratio(double a, double b) {
  PAMA_NO_CONTRACT
  return a / b;
}

// cond > qc_threshold rho, the product rounded; a NaN on either side: not cloudy.  With both condensates absent nothing is formed
PAMA_D bool cloudy(const double *cloud, const double *ice, long long o, double qc_threshold, double rho) {
  PAMA_NO_CONTRACT
  if (!cloud && !ice) return false;
  const double cond = cloud ? (ice ? cloud[o] + ice[o] : cloud[o]) : ice[o];
  return cond > qc_threshold * rho;
}
// w > 0: a NaN, 0.0 and -0.0 are not up
PAMA_D bool up(double w) { return w > 0; }
// the class of a cell, in the order of the outputs mcup, mcdn, mcuup, mcudn
PAMA_D int cell_class(bool is_cloudy, bool is_up) { return is_cloudy ? (is_up ? O_MCUP : O_MCDN) : (is_up ? O_MCUUP : O_MCUDN); }

// the six quantities of the cell at offset o; -> rho
PAMA_D double cell_values(const double *const *f, long long o, double (&x)[NX]) {
  const double rho = ms::plus(f[F_RHOD][o], f[F_VAPOR][o]);
  x[X_W] = f[F_W][o];
  x[X_M] = vt::times(rho, x[X_W]);
  x[X_T] = f[F_TEMP][o];
  x[X_Q] = ratio(ms::total_water(f[F_VAPOR], f[F_CLOUD], f[F_ICE], o), rho);
  x[X_U] = f[F_U][o];
  x[X_V] = f[F_V][o];
  return rho;
}

// the shifts of one (level, member): the quantities at the level's first cell
PAMA_D void first_cell(const double *const *f, double (&c)[NX]) { (void)cell_values(f, 0, c); }

// one cell onto the 18 sums of its slot.  A cell adds m r to the sum of its own class only (selects, not an index into the registers)
PAMA_D void cell_add(const double (&x)[NX], bool is_cloudy, bool is_up, const double (&c)[NX], double r, double (&s)[NSUM]) {
  const int cls = cell_class(is_cloudy, is_up);
#pragma unroll
  for (int i = 0; i < NCLS; i++) s[S_CLS + i] = i == cls ? ms::mean_add(s[S_CLS + i], x[X_M], r) : s[S_CLS + i];
  s[S_CLD] = is_cloudy ? ms::mean_add(s[S_CLD], 1.0, r) : s[S_CLD];
  double d[NX];
#pragma unroll
  for (int i = 0; i < NX; i++) {
    d[i] = vt::minus(x[i], c[i]);
    s[S_A + i] = ms::mean_add(s[S_A + i], d[i], r);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) s[S_BM + i] = ms::mean_add(s[S_BM + i], vt::times(d[X_M], d[X_T + i]), r);
#pragma unroll
  for (int i = 0; i < 3; i++) s[S_BX + i] = ms::mean_add(s[S_BX + i], vt::times(d[X_U + i], d[X_U + i]), r);
}

// ONE slot's share of the 18 sums of one (level, member): the cells slot, slot + 16, ... < ncol in ascending order.  UNROLL: cells whose
// loads are in flight together on the device; the order of the arithmetic is the same whatever it is
template <int UNROLL>
PAMA_D void slot_walk(const double *const *f, long long stride, int ncol, int slot, double qc_threshold, const double (&c)[NX],
                      double (&s)[NSUM]) {
  const double r = ms::r_ncol(ncol);
#pragma unroll
  for (int i = 0; i < NSUM; i++) s[i] = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll UNROLL
#endif
  for (int i = slot; i < ncol; i += NS) {
    const long long o = (long long)i * stride;
    double x[NX];
    const double rho = cell_values(f, o, x);
    cell_add(x, cloudy(f[F_CLOUD], f[F_ICE], o, qc_threshold, rho), up(x[X_W]), c, r, s);
  }
}

// the ten values of one (level, member) from its 18 level sums
PAMA_D void finish(const double (&s)[NSUM], double (&val)[NO]) {
#pragma unroll
  for (int i = 0; i <= NCLS; i++) val[O_MCUP + i] = s[S_CLS + i];
#pragma unroll
  for (int i = 0; i < 4; i++) val[O_FLUX_T + i] = vt::minus(s[S_BM + i], vt::times(s[S_A + X_M], s[S_A + X_T + i]));
  double var[3], mean;
#pragma unroll
  for (int i = 0; i < 3; i++) vt::finish(0.0, s[S_A + X_U + i], s[S_BX + i], mean, var[i]);
  val[O_TKE] = vt::times(0.5, ms::plus(ms::plus(var[0], var[1]), var[2]));
}

// out_x = out_x + value * factor, the product rounded first
PAMA_D double accumulate(double old, double value, double factor) { return ms::plus(old, vt::times(value, factor)); }

}  // namespace fluxprof
}  // namespace pama
