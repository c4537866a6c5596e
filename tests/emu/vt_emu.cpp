// vt_emu.cpp -- HOST EMULATION of the variance transport kernels (pam_amd/csrc/vt_device.h, compiled with g++ -ffp-contract=off).
// TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror the kernels of modules_kernels.hip:
// a workgroup = (level, block of `me` consecutive members) x 16 slots; every (member, slot) thread walks its cells with the device
// body, the slot sums go to an array laid out like the kernel's LDS (rows of 64 members) and are folded in ascending slot order.  `me`
// is the kernel's min(nens, 64) or any other block width: the bits must not depend on it.
#include <cstddef>
#include <vector>

#include "../../pam_amd/csrc/vt_device.h"

using namespace pama::vt;

extern "C" {

// fields[5]: (nz, ncol, nens) or null (cloud, ice; uvel without use_u); in[3], mean[3], var[3], out[3]: (nz, nens).
// epi 0: mean and var; 1: also out = scale(var, in = tend, p = dt, lim); 2: also out = (var - in) / p, in = var_start, p = gcm_dt
void emu_vt_stats(int nens, int ncol, int nz, int me, const double *const *fields, int use_u, int epi, const double *const *in, double p,
                  double lim, double *const *mean, double *const *var, double *const *out) {
  if (me < 1 || me > 64) return;      // wider than a row of the kernel's LDS: not a mapping the kernel has
  std::vector<double> red((size_t)2 * NQ * NS * 64), first((size_t)NQ * 64);
  for (int k = 0; k < nz; k++)
    for (int blk = 0; blk * me < nens; blk++) {
      for (int slot = 0; slot < NS; slot++)
        for (int m = 0; m < me; m++) {
          const int e = blk * me + m;
          double c[NQ] = {0.0, 0.0, 0.0}, a[NQ] = {0.0, 0.0, 0.0}, b[NQ] = {0.0, 0.0, 0.0};
          if (e < nens) {
            const long long base = (long long)k * ncol * nens + e;
            const double *f[NF];
            for (int i = 0; i < NF; i++) f[i] = fields[i] ? fields[i] + base : nullptr;
            first_cell(f, use_u != 0, c);
            stats_walk(f, (long long)nens, ncol, slot, use_u != 0, c, a, b);
          }
          for (int q = 0; q < NQ; q++) {
            red[((size_t)q * NS + slot) * 64 + m] = a[q];
            red[((size_t)(NQ + q) * NS + slot) * 64 + m] = b[q];
            if (slot == 0) first[(size_t)q * 64 + m] = c[q];
          }
        }
      for (int m = 0; m < me; m++) {
        const int e = blk * me + m;
        if (e >= nens) continue;
        const long long t = (long long)k * nens + e;
        for (int q = 0; q < NQ; q++) {
          if (q == Q_U && !use_u) continue;
          const double A = ms::fold(&red[(size_t)q * NS * 64 + m], 64), B = ms::fold(&red[(size_t)(NQ + q) * NS * 64 + m], 64);
          double mn, v;
          finish(first[(size_t)q * 64 + m], A, B, mn, v);
          mean[q][t] = mn;
          var[q][t] = v;
          if (epi == 1) out[q][t] = scale(v, in[q][t], p, lim);
          if (epi == 2) out[q][t] = feedback(v, in[q][t], p);
        }
      }
    }
}

void emu_vt_apply(int nens, int ncol, int nz, int me, double *const *fields, int use_u, const double *const *mean, const double *const *scale_in) {
  if (me < 1 || me > 64) return;
  std::vector<double> red((size_t)2 * NS * 64);
  for (int k = 0; k < nz; k++)
    for (int blk = 0; blk * me < nens; blk++) {
      for (int slot = 0; slot < NS; slot++)
        for (int m = 0; m < me; m++) {
          const int e = blk * me + m;
          double pn[2] = {0.0, 0.0};
          if (e < nens) {
            const long long t = (long long)k * nens + e, base = (long long)k * ncol * nens + e;
            const double g_q = gain(scale_in[Q_Q][t]);
            const double *f[NF];
            for (int i = 0; i < NF; i++) f[i] = fields[i] ? fields[i] + base : nullptr;
            if (g_q != 0) vapor_walk(f, (long long)nens, ncol, slot, g_q, mean[Q_Q][t], pn);
          }
          red[((size_t)0 * NS + slot) * 64 + m] = pn[0];
          red[((size_t)1 * NS + slot) * 64 + m] = pn[1];
        }
      for (int slot = 0; slot < NS; slot++)
        for (int m = 0; m < me; m++) {
          const int e = blk * me + m;
          if (e >= nens) continue;
          const long long t = (long long)k * nens + e, base = (long long)k * ncol * nens + e;
          double g[NQ] = {0.0, 0.0, 0.0}, mn[NQ] = {0.0, 0.0, 0.0};
          for (int q = 0; q < NQ; q++) {
            if (q == Q_U && !use_u) continue;
            g[q] = gain(scale_in[q][t]);
            mn[q] = mean[q][t];
          }
          const double P = ms::fold(&red[(size_t)0 * NS * 64 + m], 64), N = ms::fold(&red[(size_t)1 * NS * 64 + m], 64);
          double factor;
          const int mode = ms::vapor_mode(P, N, factor);
          apply_walk(fields[F_TEMP] + base, fields[F_VAPOR] + base, fields[F_CLOUD] ? fields[F_CLOUD] + base : nullptr,
                     fields[F_ICE] ? fields[F_ICE] + base : nullptr, use_u ? fields[F_U] + base : nullptr, (long long)nens, ncol, slot, g, mn,
                     use_u != 0, mode, factor);
        }
    }
}

}
