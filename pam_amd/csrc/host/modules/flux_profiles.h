// modules/flux_profiles.h -- the vertical-transport profiles of the CRM over pam_amd_flux_profiles (include/pam_amd_modules.h): the
// convective mass fluxes by conditional sampling (SAM / E3SM-MMF's crm_output fields mcup, mcdn, mcuup, mcudn), the cloud fraction
// profile, the resolved vertical fluxes of heat, total water and horizontal momentum and the resolved turbulence kinetic energy, per level
// and member, averaged over the CRM columns and over the CRM steps of a GCM step.  The method is not part of the reference tree; the
// contract is this project's.  In a GCM step:
//   modules::flux_profiles_init(coupler)     first: registers "prof_mcup", "prof_mcdn", "prof_mcuup", "prof_mcudn", "prof_cld",
//                                            "prof_flux_t", "prof_flux_qt", "prof_flux_u", "prof_flux_v", "prof_tke" {nz,nens} on first
//                                            use -- only those whose inputs the microphysics has -- and zeroes them
//   modules::flux_profiles(coupler, weight)  after the last module of every CRM step: prof_x += value * (crm_dt / gcm_physics_dt *
//                                            weight), the convention of modules::time_average_accumulate, so modules::MsaClock's weight
//                                            composes
// Options: "crm_dt", "gcm_physics_dt"; "crm_prof_qc_threshold" (1e-5 kg/kg: a cell is cloudy where its condensate exceeds this mixing
// ratio), set by the init where it is unset; "micro" names the condensate: kessler: cloud_liquid, no ice; p3: cloud_water and ice; none
// (or absent): neither, and then no "prof_mcup", "prof_mcdn" and "prof_cld".
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

struct FluxProfiles_ {
  int nens, nz, ny, nx;
  std::string cloud, ice;
  std::vector<std::string> names;        // the ten entries in the order of the C ABI; "" where absent
};

inline FluxProfiles_ flux_profiles_sizes_(pam::PamCoupler &coupler) {
  FluxProfiles_ s{coupler.get_nens(), coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), "", "", {}};
  if (s.nens < 1 || s.nz < 1 || s.ny < 1 || s.nx < 1) endrun("ERROR: flux_profiles: the coupler state is not allocated");
  std::string micro_scheme = coupler.option_exists("micro") ? coupler.get_option<std::string>("micro") : std::string("none");
  if (micro_scheme == "kessler") s.cloud = "cloud_liquid";
  else if (micro_scheme == "p3") { s.cloud = "cloud_water"; s.ice = "ice"; }
  else if (micro_scheme == "ice1m") { s.cloud = "cloud_liquid"; s.ice = "cloud_ice"; }
  else if (micro_scheme != "none") endrun("ERROR: flux_profiles only knows the kessler, p3 and none microphysics");
  bool cloudy = !s.cloud.empty() || !s.ice.empty();
  s.names = {cloudy ? "prof_mcup" : "", cloudy ? "prof_mcdn" : "", "prof_mcuup", "prof_mcudn", cloudy ? "prof_cld" : "",
             "prof_flux_t", "prof_flux_qt", "prof_flux_u", "prof_flux_v", "prof_tke"};
  return s;
}

inline void flux_profiles_init(pam::PamCoupler &coupler) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  FluxProfiles_ s = flux_profiles_sizes_(coupler);
  if (!coupler.option_exists("crm_prof_qc_threshold")) coupler.set_option<real>("crm_prof_qc_threshold", 1.e-5);
  std::vector<int> shape = {s.nz, s.nens};
  for (auto &n : s.names)
    if (!n.empty() && dm.entry_exists(n) && dm.get_shape(n) != shape) endrun("ERROR: flux_profiles: " + n + " exists with a shape other than {nz,nens}");
  std::vector<double *> out;
  std::vector<long long> sizes;
  for (auto &n : s.names) {
    if (n.empty()) continue;
    if (!dm.entry_exists(n)) dm.register_and_allocate<real>(n, "CRM flux profile, averaged over the columns and the GCM step", shape, {"z", "nens"});
    out.push_back(dm.get<real, 2>(n).data());
    sizes.push_back((long long)s.nz * s.nens);
  }
  int rc = pam_amd_time_average_zero((int)out.size(), sizes.data(), out.data(), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

inline void flux_profiles(pam::PamCoupler &coupler, real weight = 1) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  FluxProfiles_ s = flux_profiles_sizes_(coupler);
  if (!dm.entry_exists("prof_tke")) endrun("ERROR: prof_tke does not exist: call flux_profiles_init first");
  auto crm_dt = coupler.get_option<real>("crm_dt");
  auto gcm_dt = coupler.get_option<real>("gcm_physics_dt");
  if (!(gcm_dt > 0)) endrun("ERROR: flux_profiles: gcm_physics_dt must be positive");
  real factor = crm_dt / gcm_dt * weight;
  if (!std::isfinite(factor)) endrun("ERROR: flux_profiles: crm_dt / gcm_physics_dt x weight is not finite");
  auto qc_threshold = coupler.get_option<real>("crm_prof_qc_threshold");
  if (!(qc_threshold >= 0) || !std::isfinite(qc_threshold)) endrun("ERROR: flux_profiles: crm_prof_qc_threshold must be finite and >= 0");
  std::vector<int> shape = {s.nz, s.nens};
  double *out[10];
  for (int i = 0; i < 10; i++) {
    out[i] = nullptr;
    if (s.names[i].empty()) continue;
    if (!dm.entry_exists(s.names[i])) endrun("ERROR: " + s.names[i] + " does not exist: call flux_profiles_init first");
    if (dm.get_shape(s.names[i]) != shape) endrun("ERROR: flux_profiles: " + s.names[i] + " is not {nz,nens}");
    out[i] = dm.get<real, 2>(s.names[i]).data();
  }
  const double *fields[8] = {dm.get<real const, 4>("density_dry").data(), dm.get<real const, 4>("water_vapor").data(),
                             s.cloud.empty() ? nullptr : dm.get<real const, 4>(s.cloud).data(),
                             s.ice.empty() ? nullptr : dm.get<real const, 4>(s.ice).data(),
                             dm.get<real const, 4>("temp").data(), dm.get<real const, 4>("uvel").data(),
                             dm.get<real const, 4>("vvel").data(), dm.get<real const, 4>("wvel").data()};
  int rc = pam_amd_flux_profiles(s.nens, s.nx, s.ny, s.nz, fields, qc_threshold, out, factor, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
