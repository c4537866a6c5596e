// modules/crm_feedback.h -- the CRM feedback tendencies a host model takes at the end of a GCM step, over pam_amd_crm_feedback
// (include/pam_amd_modules.h): (CRM level mean - GCM value) / gcm_physics_dt of temp, the vapour, cloud-liquid and cloud-ice mixing ratios,
// uvel and vvel -- the converse of modules::compute_gcm_forcing_tendencies, with its mixing ratios rho_x / (rho_d + rho_v)
// (gcm_forcing.h:108-110).  The method is not part of the reference tree; the contract is this project's.
//   modules::crm_feedback_init(coupler)      registers "crm_feedback_mean_{t,qv,qc,qi,u,v}" and "crm_feedback_tend_{t,qv,qc,qi,u,v}" {nz,nens}
//                                            on first use (qc, qi where the microphysics has the species)
//   modules::compute_crm_feedback(coupler)   fills them from the state and the "gcm_*" entries the coupler allocates
// Options: "gcm_physics_dt" (finite, > 0); "micro" names the condensate: kessler: cloud_liquid; p3: cloud_water and ice; none (or
// absent): neither.  The temperature tendency is in K/s; the dse form (cp_d x) is the host model's.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

struct CrmFeedback_ {
  std::string cloud, ice;
  bool has[6];      // t, qv, qc, qi, u, v
};

inline CrmFeedback_ crm_feedback_species_(pam::PamCoupler &coupler) {
  CrmFeedback_ s;
  std::string micro_scheme = coupler.option_exists("micro") ? coupler.get_option<std::string>("micro") : std::string("none");
  if (micro_scheme == "kessler") s.cloud = "cloud_liquid";
  else if (micro_scheme == "p3") { s.cloud = "cloud_water"; s.ice = "ice"; }
  else if (micro_scheme == "ice1m") { s.cloud = "cloud_liquid"; s.ice = "cloud_ice"; }
  else if (micro_scheme != "none") endrun("ERROR: crm_feedback only knows the kessler, p3 and none microphysics");
  for (int q = 0; q < 6; q++) s.has[q] = true;
  s.has[2] = !s.cloud.empty();
  s.has[3] = !s.ice.empty();
  return s;
}

inline void crm_feedback_init(pam::PamCoupler &coupler) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  int nz = coupler.get_nz(), nens = coupler.get_nens();
  if (nz < 1 || nens < 1) endrun("ERROR: crm_feedback: the coupler state is not allocated");
  CrmFeedback_ s = crm_feedback_species_(coupler);
  const char *q[6] = {"t", "qv", "qc", "qi", "u", "v"};
  for (int i = 0; i < 6; i++) {
    if (!s.has[i]) continue;
    for (auto what : {"crm_feedback_mean_", "crm_feedback_tend_"}) {
      std::string n = std::string(what) + q[i];
      if (dm.entry_exists(n)) {
        if (dm.get_shape(n) != std::vector<int>{nz, nens}) endrun("ERROR: crm_feedback: " + n + " exists with a shape other than {nz,nens}");
      } else {
        dm.register_and_allocate<real>(n, "CRM level mean, and its distance from the GCM's value over the GCM step", {nz, nens}, {"z", "nens"});
      }
    }
  }
}

inline void compute_crm_feedback(pam::PamCoupler &coupler) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  if (!dm.entry_exists("crm_feedback_tend_t")) endrun("ERROR: crm_feedback: call crm_feedback_init first");
  CrmFeedback_ s = crm_feedback_species_(coupler);
  auto gcm_dt = coupler.get_option<real>("gcm_physics_dt");
  if (!(gcm_dt > 0) || !std::isfinite(gcm_dt)) endrun("ERROR: crm_feedback: gcm_physics_dt must be finite and positive");
  const double *fields[7] = {dm.get<real const, 4>("temp").data(), dm.get<real const, 4>("density_dry").data(),
                             dm.get<real const, 4>("water_vapor").data(),
                             s.has[2] ? dm.get<real const, 4>(s.cloud).data() : nullptr,
                             s.has[3] ? dm.get<real const, 4>(s.ice).data() : nullptr,
                             dm.get<real const, 4>("uvel").data(), dm.get<real const, 4>("vvel").data()};
  const double *gcm[7] = {dm.get<real const, 2>("gcm_temp").data(), dm.get<real const, 2>("gcm_density_dry").data(),
                          dm.get<real const, 2>("gcm_water_vapor").data(),
                          s.has[2] ? dm.get<real const, 2>("gcm_cloud_water").data() : nullptr,
                          s.has[3] ? dm.get<real const, 2>("gcm_cloud_ice").data() : nullptr,
                          dm.get<real const, 2>("gcm_uvel").data(), dm.get<real const, 2>("gcm_vvel").data()};
  const char *q[6] = {"t", "qv", "qc", "qi", "u", "v"};
  double *mean[6], *tend[6];
  for (int i = 0; i < 6; i++) {
    mean[i] = tend[i] = nullptr;
    if (!s.has[i]) continue;
    if (!dm.entry_exists(std::string("crm_feedback_mean_") + q[i])) endrun("ERROR: crm_feedback: the microphysics changed since crm_feedback_init");
    mean[i] = dm.get<real, 2>(std::string("crm_feedback_mean_") + q[i]).data();
    tend[i] = dm.get<real, 2>(std::string("crm_feedback_tend_") + q[i]).data();
  }
  int rc = pam_amd_crm_feedback(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), fields, gcm, gcm_dt, mean, tend, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
