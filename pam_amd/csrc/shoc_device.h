// shoc_device.h -- the arithmetic of the SHOC coupling layer (physics/sgs/shoc/SGS.h): what PAM does around shoc_main, as functions the
// HIP kernels in modules_kernels.hip call and tests/emu/shoc_emu.cpp compiles with g++ (-ffp-contract=off).
//   pack_cell / pack_edge     SGS.h:326-411   coupler state -> SHOC inputs, vertical axis flipped
//   unpack_cell               SGS.h:718-756   SHOC outputs -> coupler state
//   offset                    the one place where a flat index into a SHOC array is made
//   standin_column            a TEST DOUBLE for shoc_main: no physics, see below
// The reference's order of operations is kept and contraction into fma is switched off inside each body; divisions are the IEEE ones.
// x^y goes through pow_pos_fast (awfl_device.h), which gives the same bits on the host and on the device.  SHOC itself (SCREAM's code)
// is not part of this library.
#pragma once
#include "../../include/pam_amd_modules.h"
#include "awfl_device.h"      // pow_pos_fast + its tables
#include "plugins_device.h"   // compute_pressure, PAMA_NO_CONTRACT

#if defined(__HIPCC__)
#define PAMA_SH_HD __host__ __device__ __forceinline__
#else
#define PAMA_SH_HD inline
#endif

namespace pama {
namespace shoc {

constexpr int MAX_QTRACERS = 7;   // P3: cloud_water_num, rain, rain_num, ice, ice_num, ice_rime, ice_rime_vol (SGS.h:243-249)

// the per-cell values pack_cell makes, in the order the kernels hand them to the SHOC arrays
enum CellValue { C_THV, C_ZT_GRID, C_PRES, C_PDEL, C_W_FIELD, C_INV_EXNER, C_HOST_DSE, C_TKE, C_THETAL, C_QW, C_U_WIND, C_V_WIND,
                 C_WTHV_SEC, C_TK, C_QL, C_CLDFRAC, C_TKH, C_EXNER, C_QTRACER0, C_MAX = C_QTRACER0 + MAX_QTRACERS };
// the per-cell values unpack_cell reads from the SHOC arrays
enum UnpackValue { U_QW, U_QL, U_THETAL, U_EXNER, U_U_WIND, U_V_WIND, U_TKE, U_WTHV_SEC, U_TK, U_TKH, U_CLDFRAC, U_QL2, U_QTRACER0,
                   U_MAX = U_QTRACER0 + MAX_QTRACERS };
// and what it writes to the coupler state
enum StateValue { S_TEMP, S_RHO_V, S_RHO_C, S_UVEL, S_VVEL, S_TKE, S_WTHV_SEC, S_TK, S_TKH, S_CLDFRAC, S_INV_QC_RELVAR, S_QTRACER0,
                  S_MAX = S_QTRACER0 + MAX_QTRACERS };

// R_d ... latvap: the SGS class's (SGS.h:60-80); pres_R_d, pres_R_v: the COUPLER's options R_d, R_v, which compute_pressure_array reads
// (pam_coupler.h:375-376; the microphysics sets them)
struct Consts { double p0, grav, R_d, cp_d, cv_d, latvap, pres_R_d, pres_R_v; };

// std::max / std::min of the reference with their argument order: a NaN in b gives a
PAMA_SH_HD double smax(double a, double b) { return a < b ? b : a; }
PAMA_SH_HD double smin(double a, double b) { return b < a ? b : a; }

// Flat index of (col, s[, comp]) in a SHOC array of nlev levels (nlevi for the interface arrays) and ncomp components; s is SHOC's level,
// 0 at the model top: s = nz-1-k for cells, nz-k for interfaces.
//   layout 0   the reference's Fortran-call layout (comp, lev, col), column fastest
//   layout 1   SCREAM's C++ layout (col, comp, lev), level fastest: hwind (col,2,lev), qtracers (col,tr,lev), wtracer_sfc (col,tr)
// IDX: the kernels' unsigned instances use it while every byte offset fits 32 bits.
template <class IDX>
PAMA_SH_HD IDX offset_t(int layout, IDX col, int s, IDX ncol, int nlev, int comp = 0, int ncomp = 1) {
  return layout == 0 ? ((IDX)comp * (IDX)nlev + (IDX)s) * ncol + col : (col * (IDX)ncomp + (IDX)comp) * (IDX)nlev + (IDX)s;
}
PAMA_SH_HD long long offset(int layout, long long col, int s, long long ncol, int nlev, int comp = 0, int ncomp = 1) {
  return offset_t<long long>(layout, col, s, ncol, nlev, comp, ncomp);
}

struct CellIn {
  double rho_d, rho_v, rho_c, uvel, vvel, wvel, temp, tke, wthv_sec, tk, tkh, cldfrac;
  double q[MAX_QTRACERS];
  double zmid, zint_k, zint_k1, zint_0;   // of the column's member: (k, iens), iens = col % nens
};

// SGS.h:353-396 for one cell.  v[C_*]: the SHOC inputs of level nz-1-k.  pmid is PamCoupler::compute_pressure_array (SGS.h:265): the coupler's
// options R_d, R_v, not the plug-in's; v[C_PDEL] / 2 is the half-layer weight the interface pressures use (SGS.h:403-408: the same expression).
PAMA_D void pack_cell(const CellIn &in, int ntr, const Consts &c, const PowTab *T, double *v) {
  PAMA_NO_CONTRACT
  const double rho_total = in.rho_d + in.rho_v;
  const double z = in.zmid;
  const double dz = in.zint_k1 - in.zint_k;
  const double t = in.temp;
  const double qv = smax(0.0, in.rho_v) / rho_total;
  const double ql = smax(0.0, in.rho_c) / rho_total;
  const double pmid = plugins::compute_pressure(in.rho_d, in.rho_v, t, c.pres_R_d, c.pres_R_v);
  const double exner = pow_pos_fast(pmid / c.p0, c.R_d / c.cp_d, T);
  const double theta = t / exner;
  const double f1 = 0.61 * qv;
  const double f2 = 1 + f1;
  const double theta_v = theta * (f2 - ql);
  const double rex = 1 / exner;
  const double lc = c.latvap / c.cp_d;
  const double g1 = rex * lc;
  const double theta_l = theta - g1 * ql;
  const double zt = z - in.zint_0;
  const double phis = in.zint_0 * c.grav;
  const double gr = c.grav * rho_total;
  const double e1 = c.cp_d * t;
  const double e2 = c.grav * zt;
  const double e3 = e1 + e2;
  v[C_QL] = ql;
  v[C_QW] = qv + ql;
  v[C_ZT_GRID] = zt;
  v[C_PRES] = pmid;
  v[C_PDEL] = gr * dz;
  v[C_THV] = theta_v;
  v[C_W_FIELD] = in.wvel;
  v[C_EXNER] = exner;
  v[C_INV_EXNER] = 1.0 / exner;
  v[C_HOST_DSE] = e3 + phis;
  v[C_THETAL] = theta_l;
  v[C_U_WIND] = in.uvel;
  v[C_V_WIND] = in.vvel;
  v[C_WTHV_SEC] = in.wthv_sec;
  v[C_TKE] = smax(0.004, in.tke / rho_total);
  v[C_TK] = in.tk;
  v[C_TKH] = in.tkh;
  v[C_CLDFRAC] = in.cldfrac;
#pragma unroll
  for (int tr = 0; tr < MAX_QTRACERS; tr++)
    if (tr < ntr) v[C_QTRACER0 + tr] = smax(0.0, in.q[tr] / rho_total);
}

// SGS.h:401-410: the pressure of interface k from the cells below (k-1) and above (k): p* their pmid, d* their pdel.  The three branches
// are the reference's; an argument of a cell that does not exist is not read.
PAMA_SH_HD double pack_edge(int k, int nz, double p_km1, double d_km1, double p_k, double d_k) {
  PAMA_NO_CONTRACT
  if (k == 0) return p_k + d_k / 2;
  if (k == nz) return p_km1 - d_km1 / 2;
  const double a = p_km1 - d_km1 / 2;
  const double b = a + p_k;
  const double s = b + d_k / 2;
  return 0.5 * s;
}

// SGS.h:718-756 for one cell.  in[U_*]: SHOC's arrays at level nz-1-k (in[U_EXNER]: what pack_cell stored); temp_old, rho_d: the coupler's.
PAMA_SH_HD void unpack_cell(const double *in, double temp_old, double rho_d, int ntr, const Consts &c, double *out) {
  PAMA_NO_CONTRACT
  const double qw = in[U_QW];
  const double ql = in[U_QL];
  const double qv = qw - ql;
  const double lc = c.latvap / c.cp_d;
  const double a = in[U_THETAL] * in[U_EXNER];
  const double b = lc * ql;
  const double temp_new = a + b;
  const double d = temp_new - temp_old;
  const double d1 = d * c.cv_d;
  out[S_TEMP] = temp_old + d1 / c.cp_d;
  const double n = qv * rho_d;
  const double rho_v = smax(0.0, n / (1 - qv));
  out[S_RHO_V] = rho_v;
  const double rho_total = rho_d + rho_v;
  out[S_RHO_C] = smax(0.0, ql * rho_total);
  out[S_UVEL] = in[U_U_WIND];
  out[S_VVEL] = in[U_V_WIND];
  out[S_TKE] = in[U_TKE] * rho_total;
  out[S_WTHV_SEC] = in[U_WTHV_SEC];
  out[S_TK] = in[U_TK];
  out[S_TKH] = in[U_TKH];
  out[S_CLDFRAC] = smax(0.0, smin(1.0, in[U_CLDFRAC]));
#pragma unroll
  for (int tr = 0; tr < MAX_QTRACERS; tr++)
    if (tr < ntr) out[S_QTRACER0 + tr] = smax(0.0, in[U_QTRACER0 + tr] * rho_total);
  const double rcm = ql;
  const double rcm2 = in[U_QL2];
  double r = 1;
  if (rcm != 0 && rcm2 != 0) {
    const double sq = rcm * rcm;
    r = smin(10.0, smax(0.001, sq / rcm2));
  }
  out[S_INV_QC_RELVAR] = r;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// standin_column: a TEST DOUBLE for shoc_main, NOT PHYSICS.  It exists so that the coupling layer can be tested without SCREAM: it is
// deterministic, works on one column without looking at any other (nor at the column's number), writes every output and in/out array,
//   * replaces every in/out profile by 0.25 x(s-1) + 0.5 x(s) + 0.25 x(s+1) (ends repeated), so a flipped or shifted level shows;
//   * folds a weighted sum of every pure input (the interface arrays, the surface fluxes, host_dx/dy, phis ... included) into pblh, ustar
//     and obklen, so a mis-wired or mis-transposed input shows;
//   * uses the incoming tk, wthv_sec and cldfrac of a level as switches that drive the outputs into every branch of unpack_cell:
//     tk < 0 negates qw and the tracers, wthv_sec < 0 zeroes ql, cldfrac picks ql2 = 0, ql^2 * 2048, ql^2 * 2 or ql^2 / 128, and
//     cldfrac leaves as 3 x - 1.
template <class IDX>
PAMA_SH_HD void standin_column(const pam_amd_shoc_args_t &A, IDX col) {
  PAMA_NO_CONTRACT
  const int L = A.layout, nlev = A.nlev, nlevi = A.nlevi, ntr = A.num_qtracers;
  const IDX ncol = (IDX)A.ncol;
#define PAMA_SH_AT(p, s) (p)[offset_t<IDX>(L, col, (s), ncol, nlev)]
#define PAMA_SH_ATI(p, s) (p)[offset_t<IDX>(L, col, (s), ncol, nlevi)]
  double acc = 0.0;
  acc = acc + A.host_dx[col] * 0.0009765625;
  acc = acc + A.host_dy[col] * 0.00048828125;
  acc = acc + A.wthl_sfc[col] * 3.0;
  acc = acc + A.wqw_sfc[col] * 5.0;
  acc = acc + A.uw_sfc[col] * 7.0;
  acc = acc + A.vw_sfc[col] * 11.0;
  acc = acc + A.phis[col] * 0.00390625;
  for (int tr = 0; tr < ntr; tr++) acc = acc + A.wtracer_sfc[offset_t<IDX>(L, col, 0, ncol, 1, tr, ntr)] * (13.0 + tr);
  for (int s = 0; s < nlev; s++) {
    const double w = 1.0 + s * 0.0625;
    double t = PAMA_SH_AT(A.thv, s) * 0.001;
    t = t + PAMA_SH_AT(A.zt_grid, s) * 0.0002;
    t = t + PAMA_SH_AT(A.pres, s) * 0.00003;
    t = t + PAMA_SH_AT(A.pdel, s) * 0.0004;
    t = t + PAMA_SH_AT(A.w_field, s) * 0.5;
    t = t + PAMA_SH_AT(A.inv_exner, s) * 0.7;
    acc = acc + w * t;
  }
  for (int s = 0; s < nlevi; s++) {
    const double w = 1.0 + s * 0.03125;
    double t = PAMA_SH_ATI(A.zi_grid, s) * 0.0003;
    t = t + PAMA_SH_ATI(A.presi, s) * 0.00002;
    acc = acc + w * t;
  }
  A.pblh[col] = acc;
  A.ustar[col] = acc * 0.5;
  A.obklen[col] = acc * -0.25;

  // the in/out profiles: 0 host_dse, 1 tke, 2 thetal, 3 qw, 4 u, 5 v, 6 wthv_sec, 7 tk, 8 ql, 9 cldfrac, 10.. qtracers
  constexpr int NIO = 10 + MAX_QTRACERS;
  double *io[NIO] = {A.host_dse, A.tke, A.thetal, A.qw, A.hwind, A.hwind, A.wthv_sec, A.tk, A.ql, A.cldfrac};
  int comp[NIO] = {0, 0, 0, 0, 0, 1, 0, 0, 0, 0}, ncomp[NIO] = {1, 1, 1, 1, 2, 2, 1, 1, 1, 1};
  for (int tr = 0; tr < MAX_QTRACERS; tr++) { io[10 + tr] = A.qtracers; comp[10 + tr] = tr; ncomp[10 + tr] = ntr; }
  const int nio = 10 + ntr;
  double prev[NIO], cur[NIO], next[NIO], m[NIO];
  for (int a = 0; a < nio; a++) prev[a] = cur[a] = io[a][offset_t<IDX>(L, col, 0, ncol, nlev, comp[a], ncomp[a])];
  for (int s = 0; s < nlev; s++) {
    for (int a = 0; a < nio; a++) {
      next[a] = s + 1 < nlev ? io[a][offset_t<IDX>(L, col, s + 1, ncol, nlev, comp[a], ncomp[a])] : cur[a];
      const double lo = 0.25 * prev[a];
      const double mid = 0.5 * cur[a];
      const double hi = 0.25 * next[a];
      const double lm = lo + mid;
      m[a] = lm + hi;
    }
    const bool flip = cur[7] < 0, dry = cur[6] < 0;
    const double cf = cur[9];
    const double qn = dry ? 0.0 : m[8];
    const double q2 = qn * qn;
    for (int a = 0; a < nio; a++) {
      double o = m[a];
      if (a == 3 || a >= 10) o = flip ? -m[a] : m[a];
      if (a == 8) o = qn;
      if (a == 9) o = 3.0 * m[a] - 1.0;
      io[a][offset_t<IDX>(L, col, s, ncol, nlev, comp[a], ncomp[a])] = o;
    }
    PAMA_SH_AT(A.ql2, s) = cf < 0.2 ? 0.0 : (cf < 0.4 ? q2 * 2048.0 : (cf < 0.7 ? q2 * 2.0 : q2 * 0.0078125));
    PAMA_SH_AT(A.mix, s) = PAMA_SH_AT(A.zt_grid, s) * 0.5;
    PAMA_SH_AT(A.isotropy, s) = PAMA_SH_AT(A.pres, s) * 0.0009765625;
    PAMA_SH_AT(A.w_sec, s) = PAMA_SH_AT(A.pdel, s) * 0.001;
    PAMA_SH_AT(A.wqls_sec, s) = PAMA_SH_AT(A.w_field, s) * 0.25;
    PAMA_SH_AT(A.brunt, s) = PAMA_SH_AT(A.inv_exner, s) * 0.01;
    PAMA_SH_AT(A.tkh, s) = m[7] * 2.0;
    for (int a = 0; a < nio; a++) { prev[a] = cur[a]; cur[a] = next[a]; }
  }
  double *edge_out[9] = {A.thl_sec, A.qw_sec, A.qwthl_sec, A.wthl_sec, A.wqw_sec, A.wtke_sec, A.uw_sec, A.vw_sec, A.w3};
  for (int s = 0; s < nlevi; s++) {
    const double z = PAMA_SH_ATI(A.zi_grid, s);
    const double p = PAMA_SH_ATI(A.presi, s) * 0.000244140625;
    for (int j = 0; j < 9; j++) PAMA_SH_ATI(edge_out[j], s) = z * (j + 1.0) + p;
  }
#undef PAMA_SH_AT
#undef PAMA_SH_ATI
}

}  // namespace shoc
}  // namespace pama
