// modules/saturation_adjustment.h -- modules::saturation_adjustment(coupler) with the reference's signature
// (pam_core/modules/saturation_adjustment.h:116), forwarding to pam_amd_saturation_adjustment (include/pam_amd_modules.h).
// Entry names and options ("micro", "R_v", "cp_d", "cp_v") are the reference's; cp_l is its 4188.
#pragma once
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

inline void saturation_adjustment(pam::PamCoupler &coupler) {
  int nz = coupler.get_nz(), ny = coupler.get_ny(), nx = coupler.get_nx(), nens = coupler.get_nens();
  auto &dm = coupler.get_data_manager_device_readwrite();
  double *rho_d = dm.get<real, 4>("density_dry").data();
  double *temp = dm.get<real, 4>("temp").data();
  double *rho_v = dm.get<real, 4>("water_vapor").data();
  double *rho_c = nullptr;
  std::string micro_scheme = coupler.get_option<std::string>("micro");                         // :126-129
  if (micro_scheme == "kessler") rho_c = dm.get<real, 4>("cloud_liquid").data();
  else if (micro_scheme == "p3") rho_c = dm.get<real, 4>("cloud_water").data();
  else if (micro_scheme == "ice1m") rho_c = dm.get<real, 4>("cloud_liquid").data();      // the liquid of the native scheme with ice (cloud_ice is not adjusted here)
  else endrun("ERROR: saturation_adjustment.h only currently supports kessler and p3 microphysics");
  std::vector<double const *> massy;                                                              // :130-137
  for (auto &name : coupler.get_tracer_names()) {
    std::string desc;
    bool found, positive, adds_mass;
    coupler.get_tracer_info(name, desc, found, positive, adds_mass);
    if (adds_mass) massy.push_back(dm.get<real, 4>(name).data());
  }
  int rc = pam_amd_saturation_adjustment(nens, nx, ny, nz, rho_d, rho_v, rho_c, temp, (int)massy.size(), massy.data(),
                                         coupler.get_option<real>("R_v"), coupler.get_option<real>("cp_d"),
                                         coupler.get_option<real>("cp_v"), 4188.0, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
