// msa_emu.cpp -- HOST EMULATION of the mean-state acceleration kernels (pam_amd/csrc/msa_device.h, compiled with g++
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror the kernels of
// modules_kernels.hip: a workgroup = (level, block of `me` consecutive members) x 16 slots; every (member, slot) thread walks its
// cells with the device body, the slot sums go to an array laid out like the kernel's LDS (rows of 64 members) and are folded in
// ascending slot order.  `me` is the kernel's min(nens, 64) or any other block width: the bits must not depend on it.
#include <cstddef>
#include <vector>

#include "../../pam_amd/csrc/msa_device.h"

using namespace pama::msa;

extern "C" {

// fields[6]: (nz, ncol, nens) or null (cloud, ice); save[4], out[4]: (nz, nens).  is_save: out = mean; otherwise out = mean - save
// and *cease |= 1 where a temperature tendency ceases
void emu_msa_mean(int nens, int ncol, int nz, int me, const double *const *fields, const double *const *save, double *const *out,
                  double max_ttend, int *cease, int is_save) {
  if (me < 1 || me > 64) return;      // wider than a row of the kernel's LDS: not a mapping the kernel has
  std::vector<double> red((size_t)NQ * NS * 64);
  for (int k = 0; k < nz; k++)
    for (int b = 0; b * me < nens; b++) {
      for (int slot = 0; slot < NS; slot++)
        for (int m = 0; m < me; m++) {
          const int e = b * me + m;
          double acc[NQ] = {0.0, 0.0, 0.0, 0.0};
          if (e < nens) {
            const long long base = (long long)k * ncol * nens + e;
            const double *f[NF];
            for (int i = 0; i < NF; i++) f[i] = fields[i] ? fields[i] + base : nullptr;
            mean_walk(f, (long long)nens, ncol, slot, acc);
          }
          for (int q = 0; q < NQ; q++) red[((size_t)q * NS + slot) * 64 + m] = acc[q];
        }
      for (int m = 0; m < me; m++) {
        const int e = b * me + m;
        if (e >= nens) continue;
        const long long t = (long long)k * nens + e;
        for (int q = 0; q < NQ; q++) {
          const double mean = fold(&red[(size_t)q * NS * 64 + m], 64);
          if (is_save) {
            out[q][t] = mean;
          } else {
            const double tend = tendency(mean, save[q][t]);
            out[q][t] = tend;
            if (q == Q_T && ceases(tend, max_ttend)) *cease |= 1;
          }
        }
      }
    }
}

void emu_msa_apply(int nens, int ncol, int nz, int me, double *temp, double *vapor, double *uvel, double *vvel, const double *const *tend,
                   double accel_factor, int accel_uv, const int *cease) {
  if (cease && *cease != 0) return;
  if (me < 1 || me > 64) return;
  std::vector<double> red((size_t)2 * NS * 64);
  for (int k = 0; k < nz; k++)
    for (int b = 0; b * me < nens; b++) {
      for (int slot = 0; slot < NS; slot++)
        for (int m = 0; m < me; m++) {
          const int e = b * me + m;
          double pn[2] = {0.0, 0.0};
          if (e < nens) {
            const long long t = (long long)k * nens + e;
            vapor_walk(vapor + ((long long)k * ncol * nens + e), (long long)nens, ncol, slot, increment(accel_factor, tend[Q_Q][t]), pn);
          }
          red[((size_t)0 * NS + slot) * 64 + m] = pn[0];
          red[((size_t)1 * NS + slot) * 64 + m] = pn[1];
        }
      for (int slot = 0; slot < NS; slot++)
        for (int m = 0; m < me; m++) {
          const int e = b * me + m;
          if (e >= nens) continue;
          const long long t = (long long)k * nens + e, base = (long long)k * ncol * nens + e;
          const double P = fold(&red[(size_t)0 * NS * 64 + m], 64), N = fold(&red[(size_t)1 * NS * 64 + m], 64);
          double factor;
          const int mode = vapor_mode(P, N, factor);
          const double d_u = accel_uv ? increment(accel_factor, tend[Q_U][t]) : 0.0, d_v = accel_uv ? increment(accel_factor, tend[Q_V][t]) : 0.0;
          apply_walk(temp + base, vapor + base, accel_uv ? uvel + base : nullptr, accel_uv ? vvel + base : nullptr, (long long)nens, ncol, slot,
                     increment(accel_factor, tend[Q_T][t]), increment(accel_factor, tend[Q_Q][t]), d_u, d_v, accel_uv != 0, mode, factor);
        }
    }
}

}
