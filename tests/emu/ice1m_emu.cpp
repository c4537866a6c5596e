// ice1m_emu.cpp -- HOST EMULATION of the one-moment ice microphysics kernel (pam_amd/csrc/ice1m_device.h: column<IDX>; compiled with g++
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loop mirrors ice1m_kernel
// of modules_kernels.hip: one "thread" per (column, member), t = (j nx + i) nens + e, and the entry point's choice of the instance.
// wide: the long long instance.  The arguments are those of the C ABI and are expected to have passed its checks.
#include "../../pam_amd/csrc/ice1m_device.h"

using namespace pama::ice1m;

extern "C" {

void emu_ice1m_time_step(int nens, int nx, int ny, int nz, double *rho_v, double *rho_c, double *rho_i, double *rho_r, double *rho_s,
                         const double *rho_dry, double *temp, double *precl, double *preci, const double *zint, double dt, double R_v,
                         double cp_d, int wide) {
  const long long level = (long long)nx * ny * nens;
  Args A;
  A.rv = rho_v; A.rc = rho_c; A.ri = rho_i; A.rr = rho_r; A.rs = rho_s; A.temp = temp; A.precl = precl; A.preci = preci;
  A.rd = rho_dry; A.zint = zint; A.dt = dt; A.R_v = R_v; A.cp_d = cp_d;
  for (long long t = 0; t < level; t++) {
    const int e = (int)(t % nens);
    if (!wide) column<unsigned>(A, (unsigned)t, (unsigned)level, (unsigned)nens, e, nz);
    else column<long long>(A, t, level, (long long)nens, e, nz);
  }
}

// the sub-cycle count of every (column, member), as the kernel's pre-pass forms it
void emu_ice1m_sub_cycles(int nens, int nx, int ny, int nz, const double *rho_v, const double *rho_i, const double *rho_r,
                          const double *rho_s, const double *rho_dry, const double *zint, double dt, int *nsub) {
  const long long level = (long long)nx * ny * nens;
  Args A{};
  A.rv = const_cast<double *>(rho_v); A.ri = const_cast<double *>(rho_i); A.rr = const_cast<double *>(rho_r);
  A.rs = const_cast<double *>(rho_s); A.rd = rho_dry; A.zint = zint; A.dt = dt;
  for (long long t = 0; t < level; t++)
    nsub[t] = count_sub_cycles<long long>(A, t, level, (long long)nens, (int)(t % nens), nz, rho_dry[t] + rho_v[t]);
}

}
