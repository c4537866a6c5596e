// rad_emu.cpp -- HOST EMULATION of the CRM-to-GCM handoff kernels (pam_amd/csrc/rad_device.h, compiled with g++ -ffp-contract=off).
// TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror the kernels of modules_kernels.hip
// under three mappings of the 16 slots of a (group, member) to walkers; the bits must not depend on the mapping:
//   1  block slots: 16 walkers, one slot each; the slot sums go to an array laid out like the kernel's LDS (rows of 64 members, blocks of
//      `me` consecutive members) and are folded in ascending slot order               (rad_aggregate_block_kernel, crm_feedback_kernel)
//   2  thread slots: one walker takes the 16 slots one after the other                (rad_aggregate_thread_kernel)
//   3  four walkers of four slots each, every one folding onto what the one before it handed on
#include <cstddef>
#include <vector>

#include "../../pam_amd/csrc/rad_device.h"

using namespace pama::rad;

namespace {

// the group means of K's quantities for every member of group (jr, ir) of level k -> tot[q * nens + e]
template <class K>
void group_means(int nens, int nx, int ny, int gx, int gy, int k, int jr, int ir, const double *const *fields, int mapping, int me,
                 std::vector<double> &tot) {
  const long long stride = nens, rowstride = (long long)nx * nens;
  const double r = r_cells(gx, gy);
  const int ncell = gx * gy;
  auto origin = [&](int e, const double *(&f)[NF]) {
    const long long base = (((long long)k * ny + (long long)jr * gy) * nx + (long long)ir * gx) * nens + e;
    for (int i = 0; i < NF; i++) f[i] = fields[i] ? fields[i] + base : nullptr;
  };
  if (mapping == 1) {
    std::vector<double> red((size_t)K::NQ * NS * 64);
    for (int b = 0; b * me < nens; b++) {
      for (int slot = 0; slot < NS; slot++)
        for (int m = 0; m < me; m++) {
          const int e = b * me + m;
          double acc[K::NQ];
          for (int q = 0; q < K::NQ; q++) acc[q] = 0.0;
          if (e < nens) {
            const double *f[NF];
            origin(e, f);
            slot_walk<K>(f, stride, rowstride, gx, ncell, slot, Cursor{slot / gx, slot % gx}, r, acc);
          }
          for (int q = 0; q < K::NQ; q++) red[((size_t)q * NS + slot) * 64 + m] = acc[q];
        }
      for (int m = 0; m < me && b * me + m < nens; m++)
        for (int q = 0; q < K::NQ; q++) tot[(size_t)q * nens + b * me + m] = pama::msa::fold(&red[(size_t)q * NS * 64 + m], 64);
    }
    return;
  }
  const int walkers = mapping == 2 ? 1 : 4, each = NS / walkers;
  for (int e = 0; e < nens; e++) {
    const double *f[NF];
    origin(e, f);
    double t[K::NQ];
    for (int q = 0; q < K::NQ; q++) t[q] = 0.0;
    for (int w = 0; w < walkers; w++) slots_walk<K>(f, stride, rowstride, gx, ncell, w * each, each, r, t);
    for (int q = 0; q < K::NQ; q++) tot[(size_t)q * nens + e] = t[q];
  }
}

}  // namespace

extern "C" {

// fields[6]: temp, rho_d, rho_v, rho_c | null, rho_i | null, cldfrac | null; rad[5]: in/out, null where the species is
int emu_rad_aggregate(int nens, int nx, int ny, int nz, int rad_nx, int rad_ny, const double *const *fields, double *const *rad, double factor,
                      int mapping, int me) {
  if (mapping < 1 || mapping > 3 || me < 1 || me > 64) return -1;      // wider than a row of the kernel's LDS: not a mapping the kernel has
  const double *F[NF];
  for (int i = 0; i < NF; i++) F[i] = i < 6 ? fields[i] : nullptr;
  const int gx = nx / rad_nx, gy = ny / rad_ny;
  std::vector<double> tot((size_t)NA * nens);
  for (int k = 0; k < nz; k++)
    for (int jr = 0; jr < rad_ny; jr++)
      for (int ir = 0; ir < rad_nx; ir++) {
        group_means<Aggregate>(nens, nx, ny, gx, gy, k, jr, ir, F, mapping, me, tot);
        for (int e = 0; e < nens; e++) {
          const long long o = (((long long)k * rad_ny + jr) * rad_nx + ir) * nens + e;
          for (int q = 0; q < NA; q++)
            if (rad[q]) rad[q][o] = accumulate(rad[q][o], tot[(size_t)q * nens + e], factor);
        }
      }
  return 0;
}

// fields[7]: temp, rho_d, rho_v, rho_c | null, rho_i | null, uvel, vvel; gcm[7], mean[6], tend[6]: (nz, nens), null where the species is
int emu_crm_feedback(int nens, int nx, int ny, int nz, const double *const *fields, const double *const *gcm, double gcm_dt, double *const *mean,
                     double *const *tend, int mapping, int me) {
  if (mapping < 1 || mapping > 3 || me < 1 || me > 64) return -1;
  const double *F[NF];
  for (int i = 0; i < NF; i++) F[i] = nullptr;
  for (int i = 0; i < 5; i++) F[i] = fields[i];
  F[F_U] = fields[5];
  F[F_V] = fields[6];
  std::vector<double> tot((size_t)NB * nens);
  for (int k = 0; k < nz; k++) {
    group_means<Feedback>(nens, nx, ny, nx, ny, k, 0, 0, F, mapping, me, tot);
    for (int e = 0; e < nens; e++) {
      const long long t = (long long)k * nens + e;
      double g[NG];
      for (int i = 0; i < NG; i++) g[i] = gcm[i] ? gcm[i][t] : 0.0;
      for (int q = 0; q < NB; q++) {
        if (!mean[q]) continue;
        mean[q][t] = tot[(size_t)q * nens + e];
        tend[q][t] = feedback_tendency(tot[(size_t)q * nens + e], gcm_value(g, q), gcm_dt);
      }
    }
  }
  return 0;
}

}
