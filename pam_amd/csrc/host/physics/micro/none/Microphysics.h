// physics/micro/none/Microphysics.h -- the `Microphysics` plug-in without a process (-DPAM_MICRO=none): the members of the
// reference's physics/micro/none/Microphysics.h.  init registers the one tracer every dycore needs, "water_vapor", zeroes it on
// the device (pam_amd_time_average_zero, include/pam_amd_modules.h) and sets the constants.
#pragma once
#include <array>
#include <string>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

class Microphysics {
 public:
  // Microphysics.h:9-32: the constants of the reference's constructor (cv_v = R_v - cp_v there, kept)
  real R_d = 287., cp_d = 1003., cv_d = cp_d - R_d, gamma_d = cp_d / cv_d, kappa_d = R_d / cp_d;
  real R_v = 461., cp_v = 1859, cv_v = R_v - cp_v, p0 = 1.e5, grav = 9.81;

  Microphysics() {}

  static int constexpr get_num_tracers() { return 1; }
  static auto constexpr get_diffused_tracers_indices() { return std::array<int, 1>{0}; }
  static auto constexpr get_num_diffused_tracers() { return (size_t)1; }

  void init(pam::PamCoupler &coupler) {                                        // Microphysics.h:50-78
    coupler.add_tracer("water_vapor", "Water Vapor", true, true);              // positive, adds mass
    auto &dm = coupler.get_data_manager_device_readwrite();
    auto rho_v = dm.get_collapsed<real>("water_vapor");
    long long size = (long long)coupler.get_nz() * coupler.get_ny() * coupler.get_nx() * coupler.get_nens();
    double *ptr = rho_v.data();
    if (pam_amd_time_average_zero(1, &size, &ptr, nullptr)) endrun(pam_amd_awfl_last_error());
    coupler.set_option<std::string>("micro", "none");
    coupler.set_option<real>("R_d", R_d);
    coupler.set_option<real>("R_v", R_v);
    coupler.set_option<real>("cp_d", cp_d);
    coupler.set_option<real>("cp_v", cp_v);
    coupler.set_option<real>("grav", grav);
    coupler.set_option<real>("p0", p0);
  }

  void timeStep(pam::PamCoupler &coupler) {}
  std::string micro_name() const { return "none"; }
  void finalize(pam::PamCoupler &coupler) {}
};
