// shoc_emu.cpp -- HOST EMULATION of the SHOC coupling layer's device bodies (pam_amd/csrc/shoc_device.h, compiled with g++
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops stand for the kernels of
// modules_kernels.hip: shoc_pack_kernel (a cell's values once, pmid and pdel of the cell below kept for the interface pressure),
// shoc_standin_kernel (one column per thread) and shoc_unpack_kernel.  `args` holds HOST pointers here.
#include "../../pam_amd/csrc/shoc_device.h"
#include "../../pam_amd/csrc/awfl_vertical.h"   // build_pow_tab

using namespace pama::shoc;

namespace {
const pama::PowTab *tab() {
  static pama::PowTab T;
  static bool built = false;
  if (!built) { pama::build_pow_tab(T); built = true; }
  return &T;
}
enum { ST_RHO_D, ST_RHO_V, ST_RHO_C, ST_UVEL, ST_VVEL, ST_WVEL, ST_TEMP, ST_TKE, ST_WTHV_SEC, ST_TK, ST_TKH, ST_CLDFRAC, ST_FLX_U, ST_FLX_V,
       ST_ZINT, ST_ZMID };
}  // namespace

extern "C" {

long long emu_shoc_offset(int layout, long long col, int s, long long ncol, int nlev, int comp, int ncomp, int wide) {
  if (wide) return offset(layout, col, s, ncol, nlev, comp, ncomp);
  return (long long)offset_t<unsigned>(layout, (unsigned)col, s, (unsigned)ncol, nlev, comp, ncomp);
}

// st: the 16 arrays of the enum above; q: num_qtracers tracer arrays; consts: p0, grav, R_d, cp_d, latvap, pres_R_d, pres_R_v
void emu_shoc_pack(const pam_amd_shoc_args_t *args, int nens, const double *const *st, const double *const *q, double dx, double dy,
                   const double *consts) {
  const pam_amd_shoc_args_t &A = *args;
  const int L = A.layout, nz = A.nlev, ntr = A.num_qtracers;
  const long long ncol = A.ncol;
  const Consts c = {consts[0], consts[1], consts[2], consts[3], 0.0, consts[4], consts[5], consts[6]};
  double *dst[C_MAX] = {};
  int comp[C_MAX] = {}, ncomp[C_MAX];
  for (int a = 0; a < C_MAX; a++) ncomp[a] = 1;
  dst[C_THV] = A.thv; dst[C_ZT_GRID] = A.zt_grid; dst[C_PRES] = A.pres; dst[C_PDEL] = A.pdel; dst[C_W_FIELD] = A.w_field;
  dst[C_INV_EXNER] = A.inv_exner; dst[C_HOST_DSE] = A.host_dse; dst[C_TKE] = A.tke; dst[C_THETAL] = A.thetal; dst[C_QW] = A.qw;
  dst[C_U_WIND] = A.hwind; dst[C_V_WIND] = A.hwind; dst[C_WTHV_SEC] = A.wthv_sec; dst[C_TK] = A.tk; dst[C_QL] = A.ql;
  dst[C_CLDFRAC] = A.cldfrac; dst[C_TKH] = A.tkh; dst[C_EXNER] = A.exner;
  ncomp[C_U_WIND] = ncomp[C_V_WIND] = 2;
  comp[C_V_WIND] = 1;
  for (int tr = 0; tr < ntr; tr++) { dst[C_QTRACER0 + tr] = A.qtracers; comp[C_QTRACER0 + tr] = tr; ncomp[C_QTRACER0 + tr] = ntr; }
  for (long long col = 0; col < ncol; col++) {
    const int e = (int)(col % nens);
    const double z0 = st[ST_ZINT][e];
    A.host_dx[col] = dx;
    A.host_dy[col] = dy;
    A.wthl_sfc[col] = 0;
    A.wqw_sfc[col] = 0;
    A.uw_sfc[col] = st[ST_FLX_U][col];
    A.vw_sfc[col] = st[ST_FLX_V][col];
    A.phis[col] = z0 * c.grav;
    for (int tr = 0; tr < ntr; tr++) A.wtracer_sfc[offset(L, col, 0, ncol, 1, tr, ntr)] = 0;
    double p_km1 = 0, d_km1 = 0;
    for (int k = 0; k <= nz; k++) {
      double v[C_MAX] = {};
      const double zk = st[ST_ZINT][(long long)k * nens + e];
      if (k < nz) {
        const long long o = (long long)k * ncol + col;
        CellIn in;
        in.rho_d = st[ST_RHO_D][o]; in.rho_v = st[ST_RHO_V][o]; in.rho_c = st[ST_RHO_C][o]; in.uvel = st[ST_UVEL][o]; in.vvel = st[ST_VVEL][o];
        in.wvel = st[ST_WVEL][o]; in.temp = st[ST_TEMP][o]; in.tke = st[ST_TKE][o]; in.wthv_sec = st[ST_WTHV_SEC][o]; in.tk = st[ST_TK][o];
        in.tkh = st[ST_TKH][o]; in.cldfrac = st[ST_CLDFRAC][o];
        for (int tr = 0; tr < MAX_QTRACERS; tr++) in.q[tr] = tr < ntr ? q[tr][o] : 0.0;
        in.zmid = st[ST_ZMID][(long long)k * nens + e];
        in.zint_k = zk;
        in.zint_k1 = st[ST_ZINT][(long long)(k + 1) * nens + e];
        in.zint_0 = z0;
        pack_cell(in, ntr, c, tab(), v);
        for (int a = 0; a < C_QTRACER0 + ntr; a++) dst[a][offset(L, col, nz - 1 - k, ncol, nz, comp[a], ncomp[a])] = v[a];
      }
      A.zi_grid[offset(L, col, nz - k, ncol, nz + 1)] = zk - z0;
      A.presi[offset(L, col, nz - k, ncol, nz + 1)] = pack_edge(k, nz, p_km1, d_km1, v[C_PRES], v[C_PDEL]);
      p_km1 = v[C_PRES];
      d_km1 = v[C_PDEL];
    }
  }
}

void emu_shoc_standin(const pam_amd_shoc_args_t *args, int wide) {
  for (long long col = 0; col < args->ncol; col++) {
    if (wide) standin_column<long long>(*args, col);
    else standin_column<unsigned>(*args, (unsigned)col);
  }
}

// out: temp, rho_v, rho_c, uvel, vvel, tke, wthv_sec, tk, tkh, cldfrac, inv_qc_relvar (S_* order); q: the tracers; consts: cp_d, cv_d, latvap
void emu_shoc_unpack(const pam_amd_shoc_args_t *args, const double *rho_d, double *const *out, double *const *q, const double *consts) {
  const pam_amd_shoc_args_t &A = *args;
  const int L = A.layout, nz = A.nlev, ntr = A.num_qtracers;
  const long long ncol = A.ncol;
  const Consts c = {0.0, 0.0, 0.0, consts[0], consts[1], consts[2], 0.0, 0.0};
  const double *src[U_MAX] = {};
  int comp[U_MAX] = {}, ncomp[U_MAX];
  for (int a = 0; a < U_MAX; a++) ncomp[a] = 1;
  src[U_QW] = A.qw; src[U_QL] = A.ql; src[U_THETAL] = A.thetal; src[U_EXNER] = A.exner; src[U_U_WIND] = A.hwind; src[U_V_WIND] = A.hwind;
  src[U_TKE] = A.tke; src[U_WTHV_SEC] = A.wthv_sec; src[U_TK] = A.tk; src[U_TKH] = A.tkh; src[U_CLDFRAC] = A.cldfrac; src[U_QL2] = A.ql2;
  ncomp[U_U_WIND] = ncomp[U_V_WIND] = 2;
  comp[U_V_WIND] = 1;
  for (int tr = 0; tr < ntr; tr++) { src[U_QTRACER0 + tr] = A.qtracers; comp[U_QTRACER0 + tr] = tr; ncomp[U_QTRACER0 + tr] = ntr; }
  for (int k = 0; k < nz; k++)
    for (long long col = 0; col < ncol; col++) {
      const long long o = (long long)k * ncol + col;
      double in[U_MAX] = {}, res[S_MAX] = {};
      for (int a = 0; a < U_QTRACER0 + ntr; a++) in[a] = src[a][offset(L, col, nz - 1 - k, ncol, nz, comp[a], ncomp[a])];
      unpack_cell(in, out[S_TEMP][o], rho_d[o], ntr, c, res);
      for (int a = 0; a < S_QTRACER0; a++) out[a][o] = res[a];
      for (int tr = 0; tr < ntr; tr++) q[tr][o] = res[S_QTRACER0 + tr];
    }
}

}
