// vertical_interp_emu.cpp -- HOST EMULATION of pam::VerticalInterp's arithmetic (pam_amd/csrc/vertical_interp_device.h, compiled with
// g++ -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror
// modules_kernels.hip: one table per (level, member), one upward march per (column, member).
#include "../../pam_amd/csrc/vertical_interp_device.h"

using namespace pama::vinterp;

namespace {
template <int ORD>
int tables(int nz, int nens, const double *zint, double *lo, double *hi) {
  constexpr int NLO = Dims<ORD>::NLO, NHI = Dims<ORD>::NHI;
  for (int e = 0; e < nens; e++) {
    if (!column_ok(zint + e, nens, nz)) return -1;
    for (int k = 0; k < nz; k++) {
      double l[NLO], h[NHI];
      level_tables<ORD>(zint + e, nens, nz, k, l, h);
      for (int m = 0; m < NLO; m++) lo[((long long)k * NLO + m) * nens + e] = l[m];
      for (int m = 0; m < NHI; m++) hi[((long long)k * NHI + m) * nens + e] = h[m];
    }
  }
  return 0;
}

// tnens: members of the table (nens, or 1 for a shared table)
template <int ORD>
void edges(int nz, int ncol, int nens, int tnens, const double *data, const double *lo, const double *hi, int bc_lower, int bc_upper,
           double *out) {
  const long long lev = (long long)ncol * nens;
  for (int c = 0; c < ncol; c++)
    for (int e = 0; e < nens; e++) {
      const long long o = (long long)c * nens + e, te = tnens == 1 ? 0 : e;
      march_column<ORD, long long>(nz, data + o, lev, lo + te, hi + te, (long long)tnens, (long long)Dims<ORD>::NLO * tnens,
                                   (long long)Dims<ORD>::NHI * tnens, bc_lower, bc_upper, out + o);
    }
}
}  // namespace

extern "C" {

// zint (nz+1,nens); lo (nz,NLO,nens), hi (nz,NHI,nens).  -1: bad order or a member's interfaces are not finite and increasing
int emu_vertical_interp_tables(int ord, int nz, int nens, const double *zint, double *lo, double *hi) {
  if (ord == 3) return tables<3>(nz, nens, zint, lo, hi);
  if (ord == 5) return tables<5>(nz, nens, zint, lo, hi);
  return -1;
}

// data (nz,ncol,nens) -> out (nz+1,ncol,nens); the tables hold tnens members
int emu_vertical_interp_cells_to_edges(int ord, int nz, int ncol, int nens, int tnens, const double *data, const double *lo,
                                       const double *hi, int bc_lower, int bc_upper, double *out) {
  if (ord == 3) edges<3>(nz, ncol, nens, tnens, data, lo, hi, bc_lower, bc_upper, out);
  else if (ord == 5) edges<5>(nz, ncol, nens, tnens, data, lo, hi, bc_lower, bc_upper, out);
  else return -1;
  return 0;
}

}
