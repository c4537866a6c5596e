// modules/time_average.h -- modules::time_average_init(coupler, var_names) and modules::time_average_accumulate(coupler, var_names)
// with the reference's signatures (pam_core/modules/time_average.h:8, :39), forwarding to pam_amd_time_average_zero /
// pam_amd_time_average_accumulate (include/pam_amd_modules.h).  "<var>_time_average" has the variable's own shape.  Deliberate
// deviations (the reference does not compile): the init reuses an output that exists already and zeroes it again
// (once per GCM step); the whole list is validated before anything is registered or written.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

inline long long time_average_size_(std::vector<int> const &shape) {
  long long n = 1;
  for (int d : shape) n *= d;
  return n;
}

inline void time_average_init(pam::PamCoupler &coupler, std::vector<std::string> var_names) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  int num_vars = var_names.size();
  std::vector<long long> sizes(num_vars);
  for (int i = 0; i < num_vars; i++) {
    auto var_name = var_names[i];
    auto tavg_name = var_name + std::string("_time_average");
    auto shape = dm.get_shape(var_name);
    if (dm.entry_exists(tavg_name) && dm.get_shape(tavg_name) != shape)
      endrun("ERROR: " + tavg_name + " exists with a shape other than " + var_name + "'s");
    sizes[i] = time_average_size_(shape);
  }
  if (num_vars == 0) return;
  std::vector<double *> tavg(num_vars);
  for (int i = 0; i < num_vars; i++) {
    auto var_name = var_names[i];
    auto tavg_name = var_name + std::string("_time_average");
    if (!dm.entry_exists(tavg_name)) dm.register_and_allocate<real>(tavg_name, "", dm.get_shape(var_name));
    tavg[i] = dm.get_collapsed<real>(tavg_name).data();
  }
  int rc = pam_amd_time_average_zero(num_vars, sizes.data(), tavg.data(), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

// weight: how many steps of model time this CRM step counts (modules::MsaClock under mean-state acceleration); it multiplies the
// factor.  The reference's two-argument form below is this one with weight 1, which leaves the factor as it is
inline void time_average_accumulate(pam::PamCoupler &coupler, std::vector<std::string> var_names, real weight) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  auto crm_dt = coupler.get_option<real>("crm_dt");
  auto gcm_dt = coupler.get_option<real>("gcm_physics_dt");
  if (!(gcm_dt > 0)) endrun("ERROR: time_average_accumulate: gcm_physics_dt must be positive");
  real factor = crm_dt / gcm_dt * weight;
  if (!std::isfinite(factor)) endrun("ERROR: time_average_accumulate: crm_dt / gcm_physics_dt x weight is not finite");
  int num_vars = var_names.size();
  std::vector<long long> sizes(num_vars);
  for (int i = 0; i < num_vars; i++) {
    auto var_name = var_names[i];
    auto tavg_name = var_name + std::string("_time_average");
    auto shape = dm.get_shape(var_name);
    if (!dm.entry_exists(tavg_name)) endrun("ERROR: " + tavg_name + " does not exist: call time_average_init first");
    if (dm.get_shape(tavg_name) != shape) endrun("ERROR: " + tavg_name + " has a shape other than " + var_name + "'s");
    sizes[i] = time_average_size_(shape);
  }
  if (num_vars == 0) return;
  std::vector<double const *> var(num_vars);
  std::vector<double *> tavg(num_vars);
  for (int i = 0; i < num_vars; i++) {
    var[i] = dm.get_collapsed<real const>(var_names[i]).data();
    tavg[i] = dm.get_collapsed<real>(var_names[i] + std::string("_time_average")).data();
  }
  int rc = pam_amd_time_average_accumulate(num_vars, sizes.data(), var.data(), tavg.data(), factor, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

inline void time_average_accumulate(pam::PamCoupler &coupler, std::vector<std::string> var_names) {
  time_average_accumulate(coupler, var_names, 1);
}

}  // namespace modules
