// coldiag_device.h -- the arithmetic of the CRM column diagnostics (total, low, middle and high cloud cover, liquid and ice water path,
// precipitable water, surface precipitation: the per-step aggregation of E3SM-MMF's pam_statistics and, before it, the column scan of SAM's
// crm_module), as device functions that are plain inline C++ outside hipcc: the HIP kernels in modules_kernels.hip call them, and
// tests/emu/coldiag_emu.cpp compiles the same bodies with g++ (-ffp-contract=off).  The method is not part of the reference tree; the
// yardstick is the numpy restatement of the contract in tests/coldiag_ref.py, held bit for bit.
//   per column (j,i,e), top-down k = nz-1 .. 0: dz = zint(k+1,e) - zint(k,e); w_x = rho_x dz; pw, lwp, iwp add w_v, w_c, w_i from +0.0;
//   cw = w_c + w_i (an absent species skipped); cld = cldfrac, or rad::cloud_flag; p = plugins::compute_pressure; the level is low where
//   p >= p_low, high where p < p_high, middle otherwise (a NaN pressure: middle); the pairs (cwp_X, cf_X) of total and of the level's
//   class take cwp_X + cw and max(cf_X, cld) (a NaN cld is ignored); cldX = cwp_X > cwp_threshold ? cf_X : 0.0.
//   per member: out_x = out_x + M(x) * factor with M msa_device.h's 16-slot mean over the ny nx columns (rad_device.h's walk over one group
//   of ny nx cells in a row).
// Fields are (nz, ncol, nens), members fastest: inside a level a (column, member) has the flat index t = c nens + e, always 64 bits wide.
// Contraction into fma is switched off inside each body, so the device and the host give the same bits.
#pragma once

#include "plugins_device.h"  // compute_pressure
#include "rad_device.h"      // cloud_flag, slot_walk, slots_walk, accumulate; msa_device.h: NS, mean_add, fold

namespace pama {
namespace coldiag {

constexpr int NS = msa::NS;
enum { F_TEMP, F_RHOD, F_RHOV, F_RHOC, F_RHOI, F_CLD, NF };                                            // the field table of the scan
enum { O_CLDTOT, O_CLDLOW, O_CLDMED, O_CLDHGH, O_LWP, O_IWP, O_PW, O_PRECL, O_PRECI, NO };             // the outputs
constexpr int NW = O_PW + 1;                                                                          // the column values the scan writes
enum { C_TOT, C_LOW, C_MED, C_HGH, NC };                                                               // total and the pressure classes
// levels whose loads are in flight per lane in the scan kernel.  tools/kernel_resources.py gives 53 / 92 / 145 / 245 VGPRs at 1 / 2 / 4 / 8,
// none with scratch: 8 / 5 / 3 / 2 waves per SIMD.  Measured at the C2 grid the four are within the spread of two runs of one of them
// (0.02 ms of 0.5 ms: already at 1 a compute unit has 80 KB of loads in flight); 2 is the most that keeps five waves per SIMD
constexpr int SCAN_UNROLL = 2;

struct Params {
  double R_d, R_v, p_low, p_high, cwp_threshold;
};

// the running values of one column
struct Column {
  double cwp[NC], cf[NC], lwp, iwp, pw;
};
PAMA_D void column_start(Column &c) {
#pragma unroll
  for (int x = 0; x < NC; x++) { c.cwp[x] = 0.0; c.cf[x] = 0.0; }
  c.lwp = 0.0; c.iwp = 0.0; c.pw = 0.0;
}

PAMA_D double layer_depth(double z_top, double z_bottom) {
  PAMA_NO_CONTRACT
  return z_top - z_bottom;
}
PAMA_D double layer_path(double rho, double dz) {
  PAMA_NO_CONTRACT
  return rho * dz;
}
PAMA_D double path_add(double acc, double w) {
  PAMA_NO_CONTRACT
  return acc + w;
}
// a NaN pressure fails both comparisons: middle
PAMA_D int pressure_class(double p, double p_low, double p_high) { return p >= p_low ? C_LOW : (p < p_high ? C_HGH : C_MED); }
PAMA_D double cover(double cwp, double cf, double cwp_threshold) { return cwp > cwp_threshold ? cf : 0.0; }

// a field element is read once per call and never again: on the device the scan's loads are non-temporal (measured at the C2 grid in
// one run: 0.493 ms against 0.518 and 0.531 ms with plain loads); the value is the same
#if defined(__HIP_DEVICE_COMPILE__)
#define PAMA_CD_STREAM(p) __builtin_nontemporal_load(p)
#else
#define PAMA_CD_STREAM(p) (*(p))
#endif

// the values of one cell: what the scan holds in registers while the loads of the levels below it are in flight
struct Cell {
  double temp, rho_d, rho_v, rho_c, rho_i, cld, z_bottom;
};
PAMA_D void cell_load(const double *const *f, long long o, const double *zint, long long zo, Cell &v) {
  v.rho_v = PAMA_CD_STREAM(f[F_RHOV] + o);
  v.z_bottom = zint[zo];
  const bool has_c = f[F_RHOC] != nullptr, has_i = f[F_RHOI] != nullptr;
  v.rho_c = has_c ? PAMA_CD_STREAM(f[F_RHOC] + o) : 0.0;
  v.rho_i = has_i ? PAMA_CD_STREAM(f[F_RHOI] + o) : 0.0;
  if (has_c || has_i) {                             // without condensate there is no cloud cover: temp, rho_d and cldfrac are not read
    v.temp = PAMA_CD_STREAM(f[F_TEMP] + o);
    v.rho_d = PAMA_CD_STREAM(f[F_RHOD] + o);
    v.cld = f[F_CLD] ? PAMA_CD_STREAM(f[F_CLD] + o) : 0.0;
  } else {
    v.temp = 0.0; v.rho_d = 0.0; v.cld = 0.0;
  }
}

// one level of a column's walk; z_top is the interface above it
PAMA_D void level_update(Column &c, const Cell &v, double z_top, bool has_c, bool has_i, bool has_cld, const Params &P) {
  PAMA_NO_CONTRACT
  const double dz = layer_depth(z_top, v.z_bottom);
  c.pw = path_add(c.pw, layer_path(v.rho_v, dz));
  if (!has_c && !has_i) return;
  double w_c = 0.0, w_i = 0.0;
  if (has_c) { w_c = layer_path(v.rho_c, dz); c.lwp = path_add(c.lwp, w_c); }
  if (has_i) { w_i = layer_path(v.rho_i, dz); c.iwp = path_add(c.iwp, w_i); }
  const double cw = has_c ? (has_i ? w_c + w_i : w_c) : w_i;
  const double cld = has_cld ? v.cld : rad::cloud_flag(has_c, v.rho_c, has_i, v.rho_i);
  const int cls = pressure_class(plugins::compute_pressure(v.rho_d, v.rho_v, v.temp, P.R_d, P.R_v), P.p_low, P.p_high);
#pragma unroll
  for (int x = 0; x < NC; x++) {                    // selects, not an index into the registers
    const bool on = x == C_TOT || x == cls;
    c.cwp[x] = on ? path_add(c.cwp[x], cw) : c.cwp[x];
    c.cf[x] = (on && cld > c.cf[x]) ? cld : c.cf[x];
  }
}

// ONE column of ONE member, top-down; t: its flat index inside a level, level: the elements of a level (ncol nens).  UNROLL levels are
// loaded before the first of them is used, so that their (up to six) loads each are in flight together; the levels that are left over at
// the bottom go one by one.  The order of the arithmetic is the same whatever UNROLL is
template <int UNROLL>
PAMA_D void column_scan(const double *const *f, const double *zint, long long t, long long level, int nens, int e, int nz, const Params &P,
                        Column &c) {
  const bool has_c = f[F_RHOC] != nullptr, has_i = f[F_RHOI] != nullptr, has_cld = f[F_CLD] != nullptr;
  column_start(c);
  double z_top = zint[(long long)nz * nens + e];
  int k = nz - 1;
  for (; k >= UNROLL - 1; k -= UNROLL) {
    Cell v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) cell_load(f, (long long)(k - u) * level + t, zint, (long long)(k - u) * nens + e, v[u]);
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      level_update(c, v[u], z_top, has_c, has_i, has_cld, P);
      z_top = v[u].z_bottom;
    }
  }
  for (; k >= 0; k--) {
    Cell v;
    cell_load(f, (long long)k * level + t, zint, (long long)k * nens + e, v);
    level_update(c, v, z_top, has_c, has_i, has_cld, P);
    z_top = v.z_bottom;
  }
}

// the column's values where the scan's workspace has an array for them (ws[x] null: the output is absent)
PAMA_D void column_store(const Column &c, double *const *ws, long long t, const Params &P) {
#pragma unroll
  for (int x = 0; x < NC; x++)
    if (ws[O_CLDTOT + x]) ws[O_CLDTOT + x][t] = cover(c.cwp[x], c.cf[x], P.cwp_threshold);
  if (ws[O_LWP]) ws[O_LWP][t] = c.lwp;
  if (ws[O_IWP]) ws[O_IWP][t] = c.iwp;
  ws[O_PW][t] = c.pw;
}

// the mean's per-cell value for rad_device.h's walks: ONE column array (ncol, nens), as it is
struct Means {
  static constexpr int NQ = 1;
  static PAMA_D void cell(const double *const *f, long long o, double (&v)[1]) { v[0] = f[0][o]; }
};

PAMA_D double r_columns(int ncol) { return rad::r_cells(ncol, 1); }

}  // namespace coldiag
}  // namespace pama
