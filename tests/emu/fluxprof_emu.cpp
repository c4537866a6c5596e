// fluxprof_emu.cpp -- HOST EMULATION of the CRM flux profiles kernel (pam_amd/csrc/fluxprof_device.h, compiled with g++
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror
// flux_profiles_kernel of modules_kernels.hip; the bits must not depend on which walkers hold the 16 slots of a member nor on their order:
//   mapping  0  the kernel's: 16 walkers per member, one slot each, in blocks of `me` consecutive members; the slot sums go, three at a
//               time, to an array laid out like the kernel's LDS (rows of 64 members) and are folded in ascending slot order
//            1  the same with the walkers of a block in descending order (slots and members)
//            2  one walker does the 16 slots of a member one after the other and folds each onto the total as it goes
#include <cstddef>
#include <vector>

#include "../../pam_amd/csrc/fluxprof_device.h"

using namespace pama::fluxprof;

extern "C" {

// fields[8], out[10] as pam_amd_flux_profiles has them, in host memory
int emu_flux_profiles(int nens, int nx, int ny, int nz, const double *const *fields, double qc_threshold, double *const *out, double factor,
                      int mapping, int me) {
  if (mapping < 0 || mapping > 2 || me < 1 || me > 64) return -1;
  const int ncol = nx * ny;
  std::vector<double> sums((size_t)NSUM * NS * 64), red((size_t)3 * NS * 64);
  for (int k = 0; k < nz; k++)
    for (int b = 0; b * me < nens; b++) {
      // the walks of a block: sums[(i * NS + slot) * 64 + m]
      for (int n = 0; n < NS * me; n++) {
        const int id = mapping == 1 ? NS * me - 1 - n : n, slot = id / me, m = id % me, e = b * me + m;
        double c[NX], s[NSUM];
        for (int i = 0; i < NSUM; i++) s[i] = 0.0;
        if (e < nens) {
          const double *f[NF];
          for (int i = 0; i < NF; i++) f[i] = fields[i] ? fields[i] + (long long)k * ncol * nens + e : nullptr;
          first_cell(f, c);
          if (mapping == 2) slot_walk<1>(f, (long long)nens, ncol, slot, qc_threshold, c, s);
          else slot_walk<WALK_UNROLL>(f, (long long)nens, ncol, slot, qc_threshold, c, s);
        }
        for (int i = 0; i < NSUM; i++) sums[((size_t)i * NS + slot) * 64 + m] = s[i];
      }
      for (int m = 0; m < me && b * me + m < nens; m++) {
        const int e = b * me + m;
        double s[NSUM];
        if (mapping == 2) {                          // one walker: slot after slot onto the total
          for (int i = 0; i < NSUM; i++) {
            double a = 0.0;
            for (int sl = 0; sl < NS; sl++) a = pama::msa::plus(a, sums[((size_t)i * NS + sl) * 64 + m]);
            s[i] = a;
          }
        } else {                                     // rounds of three through the LDS rows
          for (int g = 0; g < NSUM; g += 3) {
            for (int q = 0; q < 3; q++)
              for (int sl = 0; sl < NS; sl++) red[((size_t)q * NS + sl) * 64 + m] = sums[((size_t)(g + q) * NS + sl) * 64 + m];
            for (int q = 0; q < 3; q++) s[g + q] = pama::msa::fold(&red[(size_t)q * NS * 64 + m], 64);
          }
        }
        double val[NO];
        finish(s, val);
        const long long t = (long long)k * nens + e;
        for (int q = 0; q < NO; q++)
          if (out[q]) out[q][t] = accumulate(out[q][t], val[q], factor);
      }
    }
  return 0;
}

}
