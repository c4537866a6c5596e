// modules/radiation_aggregate.h -- the inputs of the external radiation calculation whose result the forced Radiation plug-in applies, over
// pam_amd_radiation_aggregate (include/pam_amd_modules.h): temperature, the vapour, cloud-liquid and cloud-ice mixing ratios and the cloud
// fraction, averaged over the rad_ny x rad_nx groups of CRM columns and over the CRM steps of a GCM step (E3SM-MMF's crm_rad_* arrays).  The
// method is not part of the reference tree; the contract is this project's.  In a GCM step:
//   modules::rad_aggregate_init(coupler)       first: registers "rad_temperature", "rad_qv", "rad_qc", "rad_qi", "rad_cld"
//                                              {nz,rad_ny,rad_nx,nens} on first use and zeroes them
//   modules::rad_aggregate(coupler, weight)    after the last module of every CRM step: rad_x += A(x) * (crm_dt / gcm_physics_dt * weight),
//                                              the convention of modules::time_average_accumulate, so modules::MsaClock's weight composes
// Options: "rad_nx", "rad_ny" (int, >= 1, divisors of the CRM grid, as the Radiation plug-in reads them), "crm_dt", "gcm_physics_dt";
// "micro" names the condensate: kessler: cloud_liquid, no ice (no "rad_qi"); p3: cloud_water and ice; none (or absent): neither.
// "cldfrac" {nz,ny,nx,nens} is the cloud fraction where the DataManager has it (SHOC registers it); otherwise a cell counts as cloudy
// where its condensate is positive.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

struct RadAggregate_ {
  int nens, nz, ny, nx, rad_ny, rad_nx;
  std::string cloud, ice;
};

inline RadAggregate_ rad_aggregate_sizes_(pam::PamCoupler &coupler) {
  RadAggregate_ s{coupler.get_nens(), coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), 0, 0, "", ""};
  if (s.nens < 1 || s.nz < 1 || s.ny < 1 || s.nx < 1) endrun("ERROR: rad_aggregate: the coupler state is not allocated");
  if (!coupler.option_exists("rad_nx") || !coupler.option_exists("rad_ny")) endrun("ERROR: rad_aggregate: options rad_nx and rad_ny are not set");
  s.rad_nx = coupler.get_option<int>("rad_nx");
  s.rad_ny = coupler.get_option<int>("rad_ny");
  if (s.rad_nx < 1 || s.rad_ny < 1 || s.nx % s.rad_nx != 0 || s.ny % s.rad_ny != 0)
    endrun("ERROR: rad_aggregate: rad_nx and rad_ny must be >= 1 and divide crm_nx and crm_ny");
  std::string micro_scheme = coupler.option_exists("micro") ? coupler.get_option<std::string>("micro") : std::string("none");
  if (micro_scheme == "kessler") s.cloud = "cloud_liquid";
  else if (micro_scheme == "p3") { s.cloud = "cloud_water"; s.ice = "ice"; }
  else if (micro_scheme == "ice1m") { s.cloud = "cloud_liquid"; s.ice = "cloud_ice"; }
  else if (micro_scheme != "none") endrun("ERROR: rad_aggregate only knows the kessler, p3 and none microphysics");
  return s;
}

inline void rad_aggregate_init(pam::PamCoupler &coupler) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  RadAggregate_ s = rad_aggregate_sizes_(coupler);
  std::vector<int> shape = {s.nz, s.rad_ny, s.rad_nx, s.nens};
  std::vector<std::string> names = {"rad_temperature", "rad_qv", "rad_cld"};
  if (!s.cloud.empty()) names.push_back("rad_qc");
  if (!s.ice.empty()) names.push_back("rad_qi");
  for (auto &n : names)
    if (dm.entry_exists(n) && dm.get_shape(n) != shape) endrun("ERROR: rad_aggregate: " + n + " exists with a shape other than {nz,rad_ny,rad_nx,nens}");
  std::vector<double *> rad;
  std::vector<long long> sizes;
  for (auto &n : names) {
    if (!dm.entry_exists(n)) dm.register_and_allocate<real>(n, "radiation input on the rad column groups, averaged over the GCM step", shape, {"z", "rad_y", "rad_x", "nens"});
    rad.push_back(dm.get<real, 4>(n).data());
    sizes.push_back((long long)s.nz * s.rad_ny * s.rad_nx * s.nens);
  }
  int rc = pam_amd_time_average_zero((int)rad.size(), sizes.data(), rad.data(), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

inline void rad_aggregate(pam::PamCoupler &coupler, real weight = 1) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  RadAggregate_ s = rad_aggregate_sizes_(coupler);
  auto crm_dt = coupler.get_option<real>("crm_dt");
  auto gcm_dt = coupler.get_option<real>("gcm_physics_dt");
  if (!(gcm_dt > 0)) endrun("ERROR: rad_aggregate: gcm_physics_dt must be positive");
  real factor = crm_dt / gcm_dt * weight;
  if (!std::isfinite(factor)) endrun("ERROR: rad_aggregate: crm_dt / gcm_physics_dt x weight is not finite");
  std::vector<int> shape = {s.nz, s.rad_ny, s.rad_nx, s.nens}, cells = {s.nz, s.ny, s.nx, s.nens};
  const char *names[5] = {"rad_temperature", "rad_qv", "rad_qc", "rad_qi", "rad_cld"};
  double *rad[5];
  for (int i = 0; i < 5; i++) {
    rad[i] = nullptr;
    if ((i == 2 && s.cloud.empty()) || (i == 3 && s.ice.empty())) continue;
    if (!dm.entry_exists(names[i])) endrun(std::string("ERROR: ") + names[i] + " does not exist: call rad_aggregate_init first");
    if (dm.get_shape(names[i]) != shape) endrun(std::string("ERROR: rad_aggregate: ") + names[i] + " is not {nz,rad_ny,rad_nx,nens}");
    rad[i] = dm.get<real, 4>(names[i]).data();
  }
  bool has_cldfrac = dm.entry_exists("cldfrac");
  if (has_cldfrac && dm.get_shape("cldfrac") != cells) endrun("ERROR: rad_aggregate: cldfrac is not {nz,ny,nx,nens}");
  const double *fields[6] = {dm.get<real const, 4>("temp").data(), dm.get<real const, 4>("density_dry").data(),
                             dm.get<real const, 4>("water_vapor").data(),
                             s.cloud.empty() ? nullptr : dm.get<real const, 4>(s.cloud).data(),
                             s.ice.empty() ? nullptr : dm.get<real const, 4>(s.ice).data(),
                             has_cldfrac ? dm.get<real const, 4>("cldfrac").data() : nullptr};
  int rc = pam_amd_radiation_aggregate(s.nens, s.nx, s.ny, s.nz, s.rad_nx, s.rad_ny, fields, rad, factor, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
