// plugins_device.h -- the arithmetic of the forced radiation plug-in and of PamCoupler::compute_pressure_array, as
// __host__ __device__ functions: the HIP kernels in modules_kernels.hip call them, and tests/emu/plugins_emu.cpp compiles the same
// bodies with g++ (-ffp-contract=off).
//   Radiation::timeStep ("forced")           physics/radiation/forced/radiation.h:40-44
//   PamCoupler::compute_pressure             pam_core/pam_coupler.h:389-391
// The reference's order is kept and contraction into fma is switched off inside each body, so the device and the host give the same
// bits.  The division is the IEEE one (no reciprocal, no fast-math).
#pragma once

#if defined(__HIPCC__)
#define PAMA_PL_HD __host__ __device__ __forceinline__
#else
#define PAMA_PL_HD inline
#endif

#ifndef PAMA_NO_CONTRACT
#if defined(__clang__)
#define PAMA_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PAMA_NO_CONTRACT
#endif
#endif

namespace pama {
namespace plugins {

// radiation.h:43: temperature += rad_enthalpy_tend / cp_d * dt, left to right: T_new = fl(T + fl(fl(q / cp_d) * dt))
PAMA_PL_HD double radiation_forced(double T, double q, double cp_d, double dt) {
  PAMA_NO_CONTRACT
  const double h = q / cp_d;
  const double d = h * dt;
  return T + d;
}

// pam_coupler.h:390: rho_d*R_d*T + rho_v*R_v*T, left to right: fl(fl(fl(rho_d*R_d)*T) + fl(fl(rho_v*R_v)*T))
PAMA_PL_HD double compute_pressure(double rho_d, double rho_v, double T, double R_d, double R_v) {
  PAMA_NO_CONTRACT
  const double a = rho_d * R_d;
  const double b = rho_v * R_v;
  const double pd = a * T;
  const double pv = b * T;
  return pd + pv;
}

// radiation.h:41-42: the rad cell of CRM cell (j, i): i / (crm_nx / rad_nx), j / (crm_ny / rad_ny)
PAMA_PL_HD int rad_index(int i, int crm_n, int rad_n) { return i / (crm_n / rad_n); }

}  // namespace plugins
}  // namespace pama
