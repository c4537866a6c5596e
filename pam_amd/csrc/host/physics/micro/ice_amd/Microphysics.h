// physics/micro/ice_amd/Microphysics.h -- the native `Microphysics` plug-in with ice (-DPAM_MICRO=ice_amd): a bulk one-moment scheme with
// five water species, the microphysics with ice that needs no external library (as kessler_amd is the warm scheme that needs none), with
// the duck-typed members of the reference's physics/micro/*/Microphysics.h.  The method is not part of the reference tree; the contract is
// this project's (include/pam_amd_modules.h at pam_amd_ice1m_time_step).  One call of libpam_amd_awfl.so per step;
// every column forms its own sedimentation sub-cycle count, so ensemble shards exchange nothing.  Option "micro" = "ice1m"; the constants
// are Kessler's.  The coefficients are untuned starting points.
#pragma once
#include <array>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

#ifndef PAM_MICRO_CLASS
#define PAM_MICRO_CLASS Microphysics      // a driver that holds several Microphysics classes names each of them before the include
#endif

class PAM_MICRO_CLASS {
  static void chk(int rc) { if (rc) endrun(pam_amd_awfl_last_error()); }

 public:
  int static constexpr num_tracers = 5;
  real R_d = 287., cp_d = 1003., cp_v = 1859., R_v = 461., p0 = 1.e5, grav = 9.81;   // Kessler's values
  int static constexpr ID_V = 0, ID_C = 1, ID_I = 2, ID_R = 3, ID_S = 4;

  PAM_MICRO_CLASS() {}
  PAM_MICRO_CLASS(PAM_MICRO_CLASS const &) = delete;

  static int constexpr get_num_tracers() { return 5; }
  static auto constexpr get_diffused_tracers_indices() { return std::array<int, 5>{ID_V, ID_C, ID_I, ID_R, ID_S}; }
  static auto constexpr get_num_diffused_tracers() { return (size_t)5; }

  void init(pam::PamCoupler &coupler) {
    coupler.add_tracer("water_vapor", "Water Vapor", true, true);
    coupler.add_tracer("cloud_liquid", "Cloud liquid", true, true);
    coupler.add_tracer("cloud_ice", "Cloud ice", true, true);
    coupler.add_tracer("precip_liquid", "precip_liquid", true, true);
    coupler.add_tracer("precip_ice", "precip_ice", true, true);
    auto &dm = coupler.get_data_manager_device_readwrite();
    const std::vector<int> dims = {coupler.get_ny(), coupler.get_nx(), coupler.get_nens()};
    dm.register_and_allocate<real>("precl", "liquid surface precipitation rate", dims, {"y", "x", "nens"});      // allocations are zero-filled
    dm.register_and_allocate<real>("preci", "frozen surface precipitation rate", dims, {"y", "x", "nens"});
    coupler.set_option<std::string>("micro", "ice1m");
    coupler.set_option<real>("R_d", R_d);
    coupler.set_option<real>("R_v", R_v);
    coupler.set_option<real>("cp_d", cp_d);
    coupler.set_option<real>("cp_v", cp_v);
    coupler.set_option<real>("grav", grav);
    coupler.set_option<real>("p0", p0);
  }

  void timeStep(pam::PamCoupler &coupler) {
    int nz = coupler.get_nz(), ny = coupler.get_ny(), nx = coupler.get_nx(), nens = coupler.get_nens();
    auto &dm = coupler.get_data_manager_device_readwrite();
    chk(pam_amd_ice1m_time_step(nens, nx, ny, nz, dm.get<real, 4>("water_vapor").data(), dm.get<real, 4>("cloud_liquid").data(),
                                dm.get<real, 4>("cloud_ice").data(), dm.get<real, 4>("precip_liquid").data(),
                                dm.get<real, 4>("precip_ice").data(), dm.get<real const, 4>("density_dry").data(),
                                dm.get<real, 4>("temp").data(), dm.get<real, 3>("precl").data(), dm.get<real, 3>("preci").data(),
                                dm.get<real const, 2>("vertical_interface_height").data(), coupler.get_option<real>("crm_dt"), R_v, cp_d,
                                nullptr));
  }

  // sum of (rho_v + rho_c + rho_i + rho_r + rho_s) dz over the domain: a host sum of a copy, for budgets and tests
  real compute_total_mass(pam::PamCoupler &coupler) {
    int nz = coupler.get_nz(), ny = coupler.get_ny(), nx = coupler.get_nx(), nens = coupler.get_nens();
    auto &dm = coupler.get_data_manager_device_readwrite();
    const size_t level = (size_t)ny * nx * nens, n = level * nz;
    std::vector<real> z((size_t)(nz + 1) * nens), f(n);
    if (hipDeviceSynchronize() != hipSuccess) endrun("device error");
    if (hipMemcpy(z.data(), dm.get<real const, 2>("vertical_interface_height").data(), z.size() * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess)
      endrun("memcpy");
    long double total = 0;
    for (const char *name : {"water_vapor", "cloud_liquid", "cloud_ice", "precip_liquid", "precip_ice"}) {
      if (hipMemcpy(f.data(), dm.get<real const, 4>(name).data(), n * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
      for (int k = 0; k < nz; k++)
        for (size_t c = 0; c < level; c++) {
          const int e = (int)(c % nens);
          total += (long double)f[(size_t)k * level + c] * (long double)(z[(size_t)(k + 1) * nens + e] - z[(size_t)k * nens + e]);
        }
    }
    return (real)total;
  }

  std::string micro_name() const { return "ice1m"; }
  void finalize(pam::PamCoupler &coupler) {}
};
