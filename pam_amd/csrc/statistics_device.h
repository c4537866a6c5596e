// statistics_device.h -- the arithmetic of the CRM statistics modules, as __host__ __device__ functions: the HIP kernels in
// modules_kernels.hip call them, and tests/emu/statistics_emu.cpp compiles the same bodies with g++ (-ffp-contract=off).
//   horizontal_average                        pam_core/modules/horizontal_average.h:67-73
//   time_average_init / time_average_accumulate  pam_core/modules/time_average.h:32-34, :67-70
// The reference's order is kept: the horizontal average walks the columns serially in ascending order and rounds every product
// before it is added; contraction into fma is switched off inside each body, so the device and the host give the same bits.
#pragma once

#if defined(__HIPCC__)
#define PAMA_ST_HD __host__ __device__ __forceinline__
#else
#define PAMA_ST_HD inline
#endif

#ifndef PAMA_NO_CONTRACT
#if defined(__clang__)
#define PAMA_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PAMA_NO_CONTRACT
#endif
#endif

namespace pama {
namespace stats {

// horizontal_average.h:70 (r_ncol = 1._fp / ncol)
PAMA_ST_HD double havg_r_ncol(int ncol) { return 1.0 / (double)ncol; }

// one step of horizontal_average.h:71: havg += var * r_ncol, the product rounded before the add
PAMA_ST_HD double havg_add(double acc, double v, double r_ncol) {
  PAMA_NO_CONTRACT
  return acc + v * r_ncol;
}

// the whole walk of one (field, level, member): v_i = p[i * stride], i = 0 .. ncol-1 in ascending order
template <class IDX>
PAMA_ST_HD double havg_walk(const double *p, IDX stride, int ncol) {
  const double r = havg_r_ncol(ncol);
  double acc = 0.0;
  for (int i = 0; i < ncol; i++) acc = havg_add(acc, p[(IDX)i * stride], r);
  return acc;
}

// time_average.h:69: tavg += var * factor, the product rounded before the add
PAMA_ST_HD double tavg_add(double tavg, double v, double factor) {
  PAMA_NO_CONTRACT
  return tavg + v * factor;
}

}  // namespace stats
}  // namespace pama
