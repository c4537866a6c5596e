// lsforcing_emu.cpp -- HOST EMULATION of the large-scale forcing kernels (pam_amd/csrc/lsforcing_device.h: mean_walk, increment,
// make_args, column<IDX, SUBS>; compiled with g++ -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into
// libpam_amd_awfl.so).  The loops mirror ls_nudging_kernel and ls_forcing_kernel of modules_kernels.hip: for the nudging a "workgroup"
// per (level, member) whose 16 slots are folded in ascending order (msa::fold, what slot_reduce does through LDS); for the forcing one
// "thread" per (column, member), t = (j nx + i) nens + e, and the entry point's choice of the instance and of gc.  wide: the long long
// instances.  The arguments are those of the C ABI and are expected to have passed its checks.
#include "../../pam_amd/csrc/lsforcing_device.h"
#include "../../pam_amd/csrc/sgs_device.h"      // sgs::ratio, the entry point's gc

using namespace pama::lsforcing;
namespace ms = pama::msa;

extern "C" {

void emu_ls_nudging(int nens, int nx, int ny, int nz, const double *const *fields, const double *const *target, const double *const *rate,
                    double dt, double *const *inc) {
  const int ncol = nx * ny;
  const bool want[NX] = {target[X_T] != nullptr, target[X_Q] != nullptr, target[X_U] != nullptr, target[X_V] != nullptr};
  if (!want[X_T] && !want[X_Q] && !want[X_U] && !want[X_V]) return;
  for (int k = 0; k < nz; k++)
    for (int e = 0; e < nens; e++) {
      const long long base = (long long)k * ncol * nens + e, t = (long long)k * nens + e;
      const double *f[NFIELDS];
      for (int i = 0; i < NFIELDS; i++) f[i] = fields[i] ? fields[i] + base : nullptr;
      double part[NX][ms::NS];
      for (int slot = 0; slot < ms::NS; slot++) {
        double acc[NX];
        mean_walk(f, (long long)nens, ncol, slot, want, acc);
        for (int x = 0; x < NX; x++) part[x][slot] = acc[x];
      }
      for (int x = 0; x < NX; x++)
        if (want[x]) inc[x][t] = increment(dt, rate[x][t], target[x][t], ms::fold(part[x], 1));
    }
}

void emu_ls_forcing(int nens, int nx, int ny, int nz, double *uvel, double *vvel, double *temp, int num_tracers, double *const *tracers,
                    const unsigned char *positive, const double *rho_d, const double *rho_v, const double *zmid, const double *wsub,
                    const double *temp_tend, const double *qv_tend, const double *const *inc, const double *fcor, const double *ug,
                    const double *vg, double dt, double grav, double cp_d, int wide) {
  const long long level = (long long)nx * ny * nens;
  const Args A = make_args(uvel, vvel, temp, num_tracers, tracers, positive, rho_d, rho_v, zmid, wsub, temp_tend, qv_tend, inc, fcor, ug, vg, dt,
                           pama::sgs::ratio(grav, cp_d));
  for (long long t = 0; t < level; t++) {
    const int e = (int)(t % nens);
    if (wsub && !wide) column<unsigned, true>(A, (unsigned)t, (unsigned)level, (unsigned)nens, e, nz);
    else if (wsub) column<long long, true>(A, t, level, (long long)nens, e, nz);
    else if (!wide) column<unsigned, false>(A, (unsigned)t, (unsigned)level, (unsigned)nens, e, nz);
    else column<long long, false>(A, t, level, (long long)nens, e, nz);
  }
}

}
