// esmt_emu.cpp -- HOST EMULATION of the scalar momentum transport kernels (pam_amd/csrc/esmt_device.h: set_cell, mean_walk, tendency,
// forward, thomas, inverse_update; compiled with g++ -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into
// libpam_amd_awfl.so).  The loops mirror the kernels of modules_kernels.hip: for the means a "workgroup" per (level, member) whose 16
// slots are folded in ascending order (msa::fold, what slot_reduce does through LDS); for the force the three launches in their order,
// a "thread" per (level, member, block of wavenumbers), per (wavenumber, member) and per (level, member, block of x cells), and the
// entry point's k1, s and s_nyq.  wide: the long long instances.  The arguments are those of the C ABI and are expected to have passed
// its checks.
#include "../../pam_amd/csrc/esmt_device.h"

using namespace pama::esmt;
namespace ms = pama::msa;

extern "C" {

void emu_esmt_set(int nens, int nx, int nz, const double *rho_d, const double *rho_v, const double *src_u, const double *src_v, double *eu,
                  double *ev) {
  const long long level = (long long)nx * nens, cells = level * nz;
  for (long long t = 0; t < cells; t++) {
    const long long row = (t / level) * nens + t % nens;
    eu[t] = set_cell(rho_d[t], rho_v[t], src_u[row]);
    ev[t] = set_cell(rho_d[t], rho_v[t], src_v[row]);
  }
}

void emu_esmt_diagnose(int nens, int nx, int nz, const double *rho_d, const double *rho_v, const double *eu, const double *ev, double *rho_mean,
                       double *u_mean, double *v_mean, const double *gcm_u, const double *gcm_v, double gcm_dt, int feedback, double *tend_u,
                       double *tend_v) {
  for (int k = 0; k < nz; k++)
    for (int e = 0; e < nens; e++) {
      const long long base = (long long)k * nx * nens + e, t = (long long)k * nens + e;
      double part[NM][ms::NS];
      for (int slot = 0; slot < ms::NS; slot++) {
        double acc[NM];
        mean_walk(rho_d + base, rho_v + base, eu + base, ev + base, (long long)nens, nx, slot, acc);
        for (int q = 0; q < NM; q++) part[q][slot] = acc[q];
      }
      const double mr = ms::fold(part[M_RHO], 1), mu = ms::fold(part[M_U], 1), mv = ms::fold(part[M_V], 1);
      rho_mean[t] = mr;
      u_mean[t] = mu;
      v_mean[t] = mv;
      if (gcm_u) tend_u[t] = tendency(mu, gcm_u[t], gcm_dt, feedback != 0);
      if (gcm_v) tend_v[t] = tendency(mv, gcm_v[t], gcm_dt, feedback != 0);
    }
}

void emu_esmt_pgf(int nens, int nx, int nz, double *eu, double *ev, const double *wvel, const double *rho_d, const double *rho_v,
                  const double *zmid, const double *dz, const double *rho_mean, const double *u_mean, const double *v_mean, const double *force_u,
                  const double *force_v, const double *C, const double *S, double dx, double dt, int kmax, double *workspace, int wide) {
  const bool solve = kmax > 0 && (u_mean || v_mean);
  if (!solve && !force_u && !force_v) return;
  Args A;
  A.eu = eu; A.ev = ev; A.ws = workspace; A.w = wvel; A.rd = rho_d; A.rv = rho_v; A.zmid = zmid; A.dz = dz;
  A.rho_mean = rho_mean; A.u_mean = u_mean; A.v_mean = v_mean; A.force_u = force_u; A.force_v = force_v; A.C = C; A.S = S;
  A.k1 = 6.283185307179586 / ((double)nx * dx);
  A.s = 2.0 / (double)nx;
  A.s_nyq = 1.0 / (double)nx;
  A.dt = dt; A.nx = nx; A.nz = nz; A.nens = nens; A.kmax = kmax;
  if (solve) {
    for (int mb = 0; mb < (kmax + MODES - 1) / MODES; mb++)
      for (int k = 0; k < nz; k++)
        for (int e = 0; e < nens; e++) wide ? forward<long long>(A, k, e, mb) : forward<unsigned>(A, k, e, mb);
    for (int m = 1; m <= kmax; m++)
      for (int e = 0; e < nens; e++) wide ? thomas<long long>(A, m, e) : thomas<unsigned>(A, m, e);
  }
  for (int xb = 0; xb < (nx + XB - 1) / XB; xb++)
    for (int k = 0; k < nz; k++)
      for (int e = 0; e < nens; e++) wide ? inverse_update<long long>(A, k, e, xb) : inverse_update<unsigned>(A, k, e, xb);
}

}
