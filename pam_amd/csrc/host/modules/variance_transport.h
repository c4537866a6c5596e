// modules/variance_transport.h -- CRM variance transport (Hannah and Pressel 2022; E3SM-MMF's use_MMF_VT, bulk form) over
// pam_amd_vt_diagnose / pam_amd_vt_forcing / pam_amd_vt_apply / pam_amd_vt_feedback (include/pam_amd_modules.h).  The method is not part
// of the reference tree; the contract is this project's.  In a GCM step:
//   modules::vt_init(coupler)              first: registers the entries below on first use and fills "vt_var_start_*" with the variances
//                                          the CRM starts from; the GCM then sets "vt_tend_*" (units of x^2 per second)
//   per CRM step, after its last module:   modules::vt_apply_forcing(coupler [, dt]): the level statistics, the scale
//                                          sqrt(1 + dt tend / var) clamped to 1 +- crm_vt_scale_limit, and the anomalies of temp, total
//                                          water (through the vapour, its negative values filled from the level) and uvel stretched by it
//   modules::vt_compute_feedback(coupler)  last: "vt_feedback_*" = (var - var_start) / gcm_physics_dt
// Entries, {nz,nens} each, x = t, q and (with crm_vt_u) u: "vt_mean_x", "vt_var_x", "vt_var_start_x", "vt_scale_x", "vt_tend_x" (the GCM's
// input, zero-filled when registered), "vt_feedback_x".
// Options: "crm_vt_u" (bool, default false), "crm_vt_scale_limit" (real in (0,1), default 0.05), "crm_dt", "gcm_physics_dt"; "micro"
// names the condensate of the total water as in mean_state_acceleration.h.
#pragma once
#include <cmath>
#include <string>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

struct VtArrays_ {
  double *fields[5], *mean[3], *var[3], *var_start[3], *scale[3], *tend[3], *feedback[3];
  int use_u;
};

inline VtArrays_ vt_arrays_(pam::PamCoupler &coupler) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  if (!dm.entry_exists("vt_var_start_t")) endrun("ERROR: variance transport: call vt_init first");
  VtArrays_ A;
  A.use_u = coupler.get_option<bool>("crm_vt_u") ? 1 : 0;
  std::string micro_scheme = coupler.option_exists("micro") ? coupler.get_option<std::string>("micro") : std::string("none");
  std::string cloud, ice;
  if (micro_scheme == "kessler") cloud = "cloud_liquid";
  else if (micro_scheme == "p3") { cloud = "cloud_water"; ice = "ice"; }
  else if (micro_scheme == "ice1m") { cloud = "cloud_liquid"; ice = "cloud_ice"; }
  else if (micro_scheme != "none") endrun("ERROR: variance transport only knows the kessler, p3 and none microphysics");
  A.fields[0] = dm.get<real, 4>("temp").data();
  A.fields[1] = dm.get<real, 4>("water_vapor").data();
  A.fields[2] = cloud.empty() ? nullptr : (double *)dm.get<real const, 4>(cloud).data();
  A.fields[3] = ice.empty() ? nullptr : (double *)dm.get<real const, 4>(ice).data();
  A.fields[4] = A.use_u ? dm.get<real, 4>("uvel").data() : nullptr;
  const char *q[3] = {"t", "q", "u"};
  for (int i = 0; i < 3; i++) {
    const bool have = i < 2 || A.use_u;
    A.mean[i] = have ? dm.get<real, 2>(std::string("vt_mean_") + q[i]).data() : nullptr;
    A.var[i] = have ? dm.get<real, 2>(std::string("vt_var_") + q[i]).data() : nullptr;
    A.var_start[i] = have ? dm.get<real, 2>(std::string("vt_var_start_") + q[i]).data() : nullptr;
    A.scale[i] = have ? dm.get<real, 2>(std::string("vt_scale_") + q[i]).data() : nullptr;
    A.tend[i] = have ? dm.get<real, 2>(std::string("vt_tend_") + q[i]).data() : nullptr;
    A.feedback[i] = have ? dm.get<real, 2>(std::string("vt_feedback_") + q[i]).data() : nullptr;
  }
  return A;
}

inline void vt_init(pam::PamCoupler &coupler) {
  int nz = coupler.get_nz(), nens = coupler.get_nens();
  auto &dm = coupler.get_data_manager_device_readwrite();
  if (!coupler.option_exists("crm_vt_u")) coupler.set_option<bool>("crm_vt_u", false);
  if (!coupler.option_exists("crm_vt_scale_limit")) coupler.set_option<real>("crm_vt_scale_limit", 0.05);
  real lim = coupler.get_option<real>("crm_vt_scale_limit");
  if (!(lim > 0 && lim < 1)) endrun("ERROR: variance transport: crm_vt_scale_limit must lie in (0, 1)");
  if (!dm.entry_exists("vt_var_start_t")) {
    const char *q[3] = {"t", "q", "u"};
    for (int i = 0; i < (coupler.get_option<bool>("crm_vt_u") ? 3 : 2); i++) {
      std::string x = q[i];
      dm.register_and_allocate<real>("vt_mean_" + x, "level mean", {nz, nens}, {"z", "nens"});
      dm.register_and_allocate<real>("vt_var_" + x, "level variance", {nz, nens}, {"z", "nens"});
      dm.register_and_allocate<real>("vt_var_start_" + x, "level variance at the start of the GCM step", {nz, nens}, {"z", "nens"});
      dm.register_and_allocate<real>("vt_scale_" + x, "factor of the anomalies in the last CRM step", {nz, nens}, {"z", "nens"});
      dm.register_and_allocate<real>("vt_tend_" + x, "variance tendency from the GCM", {nz, nens}, {"z", "nens"});
      dm.register_and_allocate<real>("vt_feedback_" + x, "variance tendency of the CRM over the GCM step", {nz, nens}, {"z", "nens"});
      if (hipMemsetAsync(dm.get<real, 2>("vt_tend_" + x).data(), 0, (size_t)nz * nens * sizeof(real), 0) != hipSuccess)
        endrun("ERROR: variance transport: memset failed");
    }
  }
  VtArrays_ A = vt_arrays_(coupler);
  int rc = pam_amd_vt_diagnose(nens, coupler.get_nx(), coupler.get_ny(), nz, A.fields, A.use_u, A.mean, A.var_start, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

inline void vt_apply_forcing(pam::PamCoupler &coupler, real dt) {
  VtArrays_ A = vt_arrays_(coupler);
  int nens = coupler.get_nens(), nx = coupler.get_nx(), ny = coupler.get_ny(), nz = coupler.get_nz();
  int rc = pam_amd_vt_forcing(nens, nx, ny, nz, A.fields, A.use_u, A.tend, dt, coupler.get_option<real>("crm_vt_scale_limit"), A.mean, A.var,
                              A.scale, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
  rc = pam_amd_vt_apply(nens, nx, ny, nz, A.fields, A.use_u, A.mean, A.scale, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

inline void vt_apply_forcing(pam::PamCoupler &coupler) { vt_apply_forcing(coupler, coupler.get_option<real>("crm_dt")); }

inline void vt_compute_feedback(pam::PamCoupler &coupler) {
  VtArrays_ A = vt_arrays_(coupler);
  int rc = pam_amd_vt_feedback(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), A.fields, A.use_u, A.var_start,
                               coupler.get_option<real>("gcm_physics_dt"), A.mean, A.var, A.feedback, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
