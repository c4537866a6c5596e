// kessler_emu.cpp -- HOST EMULATION of the per-column bodies of the Kessler kernels (pam_amd/csrc/kessler_device.h, compiled with
// g++ -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror the
// kernels of modules_kernels.hip: kessler_limit_kernel (one column per thread, the minimum over the bit patterns) and the four
// instances of kessler_column_kernel<SINGLE, IDX>, which the C ABI picks by the sub-cycle count and the array size; here the caller
// picks, so that <false, IDX> can be run at rainsplit == 1 and <*, long long> at small sizes.
#include <string.h>

#include "../../pam_amd/csrc/kessler_device.h"
#include "../../pam_amd/csrc/awfl_vertical.h"   // build_pow_tab

using namespace pama::kessler;

namespace {
const pama::PowTab *tab() {
  static pama::PowTab T;
  static bool built = false;
  if (!built) { pama::build_pow_tab(T); built = true; }
  return &T;
}
}  // namespace

extern "C" {

// pam_amd_kessler_max_stable_dt: returns 0 and *dt_max, or -1 where the C ABI returns PAM_AMD_ESTATE (limit not positive).
// level_step: the levels are dealt to that many passes per column, as the kernel's gridDim.y deals them to workgroups.
int emu_kessler_max_stable_dt(int nens, int nx, int ny, int nz, const double *rho_r, const double *rho_dry, const double *zmid,
                              double dt, int level_step, double *dt_max) {
  const long long ncol = (long long)ny * nx * nens;
  unsigned long long bits = 0x7f7f7f7f7f7f7f7full;   // the slot's initial value (hipMemsetAsync 0x7f)
  for (int k0 = 0; k0 < level_step; k0++)
    for (long long col = 0; col < ncol; col++) {
      const unsigned long long b = kessler_limit_column(nz, ncol, nens, col, (unsigned)k0, (unsigned)level_step, rho_r, rho_dry, zmid,
                                                        dt, tab());
      if (b != ~0ull && b < bits) bits = b;
    }
  double v;
  memcpy(&v, &bits, 8);
  *dt_max = v;
  return v > 0 ? 0 : -1;
}

// pam_amd_kessler_time_step's column kernel with a given sub-cycle count.  single / wide choose the template instance:
// single != 0 requires rainsplit == 1; exner: nz * ncol doubles of scratch (unused by the single instances).
int emu_kessler_columns(int nens, int nx, int ny, int nz, double *rho_v, double *rho_c, double *rho_r, const double *rho_dry,
                        double *temp, double *precl, const double *zmid, double *exner, double dt, int rainsplit, double R_d,
                        double R_v, double cp_d, double p0, int single, int wide) {
  if (rainsplit < 1 || (single && rainsplit != 1)) return -1;
  const long long ncol = (long long)ny * nx * nens;
  for (long long col = 0; col < ncol; col++) {
#define COLUMN(SINGLE, IDX)                                                                                                     \
  kessler_column<SINGLE, IDX>(nz, ncol, nens, col, rho_v, rho_c, rho_r, rho_dry, temp, precl, zmid, exner, dt, rainsplit, R_d, R_v, \
                              cp_d, p0, tab())
    if (single && !wide) COLUMN(true, unsigned);
    else if (single) COLUMN(true, long long);
    else if (!wide) COLUMN(false, unsigned);
    else COLUMN(false, long long);
#undef COLUMN
  }
  return 0;
}

}
