// p3_emu.cpp -- HOST EMULATION of the P3 coupling layer's device bodies (pam_amd/csrc/p3_device.h, compiled with g++
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops stand for the kernels of
// modules_kernels.hip: p3_pack_kernel (a cell's values once), p3_standin_kernel (one column per thread) and p3_unpack_kernel.  `args`
// holds HOST pointers here.
#include "../../pam_amd/csrc/p3_device.h"
#include "../../pam_amd/csrc/awfl_vertical.h"   // build_pow_tab

using namespace pama::p3;

namespace {
const pama::PowTab *tab() {
  static pama::PowTab T;
  static bool built = false;
  if (!built) { pama::build_pow_tab(T); built = true; }
  return &T;
}
enum { ST_RHO_D, ST_RHO_V, ST_RHO_C, ST_TEMP, ST_NCCN, ST_NUCEAT, ST_NI_ACT, ST_Q_PREV, ST_T_PREV, ST_ZINT };
template <class IDX>
long long off(int layout, long long col, int k, long long ncol, int nz, int plane, int nplanes) {
  return (long long)offset_t<IDX>(layout, (IDX)col, k, (IDX)ncol, nz, plane, nplanes);
}
}  // namespace

extern "C" {

long long emu_p3_offset(int layout, long long col, int k, long long ncol, int nz, int plane, int nplanes, int wide) {
  return wide ? off<long long>(layout, col, k, ncol, nz, plane, nplanes) : off<unsigned>(layout, col, k, ncol, nz, plane, nplanes);
}

// st: the 10 arrays of the enum above (rho_v, rho_c, temp are in/out where adjust != 0); q: the seven tracers;
// consts: R_d, R_v, cp_d, cp_v, cp_l, p0, grav; iters (nz, ncol), may be NULL: the iterations of the adjustment per cell
void emu_p3_pack(const pam_amd_p3_args_t *args, int nens, double *const *st, const double *const *q, int adjust, int first_step,
                 const double *consts, int wide, int *iters) {
  const pam_amd_p3_args_t &A = *args;
  const int L = A.layout, nz = A.nlev;
  const long long ncol = A.ncol;
  const Consts c = {consts[0], consts[1], consts[2], consts[3], consts[4], consts[5], consts[6], 0.0};
  double *dst[C_MAX] = {};
  dst[C_QC] = A.qc; dst[C_NC] = A.nc; dst[C_QR] = A.qr; dst[C_NR] = A.nr; dst[C_TH_ATM] = A.th_atm; dst[C_QV] = A.qv; dst[C_QI] = A.qi;
  dst[C_QM] = A.qm; dst[C_NI] = A.ni; dst[C_BM] = A.bm; dst[C_PRES] = A.pres; dst[C_DZ] = A.dz; dst[C_NC_NUCEAT_TEND] = A.nc_nuceat_tend;
  dst[C_NCCN_PRESCRIBED] = A.nccn_prescribed; dst[C_NI_ACTIVATED] = A.ni_activated; dst[C_DPRES] = A.dpres; dst[C_INV_EXNER] = A.inv_exner;
  dst[C_Q_PREV] = A.q_prev; dst[C_T_PREV] = A.t_prev; dst[C_EXNER] = A.exner;
  double *one[4] = {A.cld_frac_l, A.cld_frac_i, A.cld_frac_r, A.inv_qc_relvar};
  auto at = [&](long long col, int k, int nzz, int plane, int nplanes) {
    return wide ? off<long long>(L, col, k, ncol, nzz, plane, nplanes) : off<unsigned>(L, col, k, ncol, nzz, plane, nplanes);
  };
  for (long long col = 0; col < ncol; col++) {
    const int e = (int)(col % nens);
    for (int r = 0; r < 3; r++) A.col_location[at(col, 0, 1, r, 3)] = 1;
    for (int k = 0; k < nz; k++) {
      const long long o = (long long)k * ncol + col;
      CellIn in;
      in.rho_d = st[ST_RHO_D][o]; in.rho_v = st[ST_RHO_V][o]; in.rho_c = st[ST_RHO_C][o]; in.temp = st[ST_TEMP][o];
      for (int tr = 0; tr < NTRACERS; tr++) in.q[tr] = q[tr][o];
      in.nccn_prescribed = st[ST_NCCN][o]; in.nc_nuceat_tend = st[ST_NUCEAT][o]; in.ni_activated = st[ST_NI_ACT][o];
      in.q_prev = st[ST_Q_PREV][o]; in.t_prev = st[ST_T_PREV][o];
      in.zint_k = st[ST_ZINT][(long long)k * nens + e];
      in.zint_k1 = st[ST_ZINT][(long long)(k + 1) * nens + e];
      double v[C_MAX] = {};
      const int it = adjust ? pack_cell<true>(in, first_step != 0, c, tab(), v) : pack_cell<false>(in, first_step != 0, c, tab(), v);
      if (iters) iters[o] = it;
      if (adjust && it > 0) { st[ST_RHO_V][o] = in.rho_v; st[ST_RHO_C][o] = in.rho_c; st[ST_TEMP][o] = in.temp; }
      for (int a = 0; a < C_MAX; a++) dst[a][at(col, k, nz, 0, 1)] = v[a];
      for (int a = 0; a < 4; a++) one[a][at(col, k, nz, 0, 1)] = 1;
    }
  }
}

void emu_p3_standin(const pam_amd_p3_args_t *args, int wide) {
  for (long long col = 0; col < args->ncol; col++) {
    if (wide) standin_column<long long>(*args, col);
    else standin_column<unsigned>(*args, (unsigned)col);
  }
}

// out: the S_* arrays in that order (temp in/out); surf: precip_liq_surf_out, precip_ice_surf_out; consts: cp_d, cv_d
void emu_p3_unpack(const pam_amd_p3_args_t *args, const double *rho_d, double *const *out, double *const *surf, const double *consts,
                   int wide) {
  const pam_amd_p3_args_t &A = *args;
  const int L = A.layout, nz = A.nlev;
  const long long ncol = A.ncol;
  const Consts c = {0.0, 0.0, consts[0], 0.0, 0.0, 0.0, 0.0, consts[1]};
  const double *src[U_MAX] = {};
  src[U_QC] = A.qc; src[U_NC] = A.nc; src[U_QR] = A.qr; src[U_NR] = A.nr; src[U_QI] = A.qi; src[U_NI] = A.ni; src[U_QM] = A.qm;
  src[U_BM] = A.bm; src[U_QV] = A.qv; src[U_TH_ATM] = A.th_atm; src[U_EXNER] = A.exner; src[U_LIQ_ICE] = A.liq_ice_exchange;
  src[U_VAP_LIQ] = A.vap_liq_exchange; src[U_VAP_ICE] = A.vap_ice_exchange;
  for (long long col = 0; col < ncol; col++) {
    surf[0][col] = A.precip_liq_surf[col];
    surf[1][col] = A.precip_ice_surf[col];
  }
  for (int k = 0; k < nz; k++)
    for (long long col = 0; col < ncol; col++) {
      const long long o = (long long)k * ncol + col;
      const long long w = wide ? off<long long>(L, col, k, ncol, nz, 0, 1) : off<unsigned>(L, col, k, ncol, nz, 0, 1);
      double in[U_MAX] = {}, res[S_MAX] = {};
      for (int a = 0; a < U_MAX; a++) in[a] = src[a][w];
      unpack_cell(in, out[S_TEMP][o], rho_d[o], c, res);
      for (int a = 0; a < S_MAX; a++) out[a][o] = res[a];
    }
}

}
