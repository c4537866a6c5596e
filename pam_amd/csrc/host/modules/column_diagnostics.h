// modules/column_diagnostics.h -- the per-GCM-column diagnostics of the CRM over pam_amd_column_diagnostics (include/pam_amd_modules.h):
// total, low, middle and high cloud cover, liquid and ice water path, precipitable water and surface precipitation, averaged over the CRM
// columns and over the CRM steps of a GCM step (the per-step aggregation of E3SM-MMF's pam_statistics).  The method is not part of the
// reference tree; the contract is this project's.  In a GCM step:
//   modules::column_diagnostics_init(coupler)     first: registers "diag_cldtot", "diag_cldlow", "diag_cldmed", "diag_cldhgh", "diag_lwp",
//                                                 "diag_iwp", "diag_pw", "diag_precip_liq", "diag_precip_ice" {nens} on first use -- only
//                                                 those whose inputs the coupler has -- and zeroes them
//   modules::column_diagnostics(coupler, weight)  after the last module of every CRM step: diag_x += M(x) * (crm_dt / gcm_physics_dt *
//                                                 weight), the convention of modules::time_average_accumulate, so modules::MsaClock's
//                                                 weight composes
// Options: "R_d", "R_v", "crm_dt", "gcm_physics_dt"; "crm_diag_p_low" (70000 Pa), "crm_diag_p_high" (40000 Pa) and
// "crm_diag_cwp_threshold" (1e-3 kg/m2), set by the init where they are unset; "micro" names the condensate: kessler: cloud_liquid, no ice
// (no "diag_iwp"); p3: cloud_water and ice; none (or absent): neither, and then no cloud cover.  "cldfrac" {nz,ny,nx,nens} is the cloud
// fraction where the DataManager has it.  The liquid precipitation is "precl" (Kessler) or "precip_liq_surf_out" (P3), the ice
// precipitation "preci" (ice1m: cloud_liquid and cloud_ice) or "precip_ice_surf_out", each where the DataManager has it.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

struct ColumnDiagnostics_ {
  int nens, nz, ny, nx;
  std::string cloud, ice, precip_liq, precip_ice;
  std::vector<std::string> names;        // the nine entries in the order of the C ABI; "" where absent
};

inline ColumnDiagnostics_ column_diagnostics_sizes_(pam::PamCoupler &coupler) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  ColumnDiagnostics_ s{coupler.get_nens(), coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), "", "", "", "", {}};
  if (s.nens < 1 || s.nz < 1 || s.ny < 1 || s.nx < 1) endrun("ERROR: column_diagnostics: the coupler state is not allocated");
  std::string micro_scheme = coupler.option_exists("micro") ? coupler.get_option<std::string>("micro") : std::string("none");
  if (micro_scheme == "kessler") s.cloud = "cloud_liquid";
  else if (micro_scheme == "p3") { s.cloud = "cloud_water"; s.ice = "ice"; }
  else if (micro_scheme == "ice1m") { s.cloud = "cloud_liquid"; s.ice = "cloud_ice"; }
  else if (micro_scheme != "none") endrun("ERROR: column_diagnostics only knows the kessler, p3 and none microphysics");
  if (dm.entry_exists("precl")) s.precip_liq = "precl";
  else if (dm.entry_exists("precip_liq_surf_out")) s.precip_liq = "precip_liq_surf_out";
  if (dm.entry_exists("preci")) s.precip_ice = "preci";                                           // micro = ice1m
  else if (dm.entry_exists("precip_ice_surf_out")) s.precip_ice = "precip_ice_surf_out";
  std::vector<int> columns = {s.ny, s.nx, s.nens};
  for (auto &n : {s.precip_liq, s.precip_ice})
    if (!n.empty() && dm.get_shape(n) != columns) endrun("ERROR: column_diagnostics: " + n + " is not {ny,nx,nens}");
  bool cloudy = !s.cloud.empty() || !s.ice.empty();
  s.names = {cloudy ? "diag_cldtot" : "", cloudy ? "diag_cldlow" : "", cloudy ? "diag_cldmed" : "", cloudy ? "diag_cldhgh" : "",
             s.cloud.empty() ? "" : "diag_lwp", s.ice.empty() ? "" : "diag_iwp", "diag_pw",
             s.precip_liq.empty() ? "" : "diag_precip_liq", s.precip_ice.empty() ? "" : "diag_precip_ice"};
  return s;
}

inline void column_diagnostics_init(pam::PamCoupler &coupler) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  ColumnDiagnostics_ s = column_diagnostics_sizes_(coupler);
  if (!coupler.option_exists("crm_diag_p_low")) coupler.set_option<real>("crm_diag_p_low", 70000.);
  if (!coupler.option_exists("crm_diag_p_high")) coupler.set_option<real>("crm_diag_p_high", 40000.);
  if (!coupler.option_exists("crm_diag_cwp_threshold")) coupler.set_option<real>("crm_diag_cwp_threshold", 1.e-3);
  std::vector<int> shape = {s.nens};
  for (auto &n : s.names)
    if (!n.empty() && dm.entry_exists(n) && dm.get_shape(n) != shape) endrun("ERROR: column_diagnostics: " + n + " exists with a shape other than {nens}");
  std::vector<double *> out;
  std::vector<long long> sizes;
  for (auto &n : s.names) {
    if (n.empty()) continue;
    if (!dm.entry_exists(n)) dm.register_and_allocate<real>(n, "CRM column diagnostic, averaged over the columns and the GCM step", shape, {"nens"});
    out.push_back(dm.get<real, 1>(n).data());
    sizes.push_back((long long)s.nens);
  }
  int rc = pam_amd_time_average_zero((int)out.size(), sizes.data(), out.data(), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

inline void column_diagnostics(pam::PamCoupler &coupler, real weight = 1) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  ColumnDiagnostics_ s = column_diagnostics_sizes_(coupler);
  if (!dm.entry_exists("diag_pw")) endrun("ERROR: diag_pw does not exist: call column_diagnostics_init first");
  auto crm_dt = coupler.get_option<real>("crm_dt");
  auto gcm_dt = coupler.get_option<real>("gcm_physics_dt");
  if (!(gcm_dt > 0)) endrun("ERROR: column_diagnostics: gcm_physics_dt must be positive");
  real factor = crm_dt / gcm_dt * weight;
  if (!std::isfinite(factor)) endrun("ERROR: column_diagnostics: crm_dt / gcm_physics_dt x weight is not finite");
  std::vector<int> shape = {s.nens}, cells = {s.nz, s.ny, s.nx, s.nens};
  double *out[9];
  for (int i = 0; i < 9; i++) {
    out[i] = nullptr;
    if (s.names[i].empty()) continue;
    if (!dm.entry_exists(s.names[i])) endrun("ERROR: " + s.names[i] + " does not exist: call column_diagnostics_init first");
    if (dm.get_shape(s.names[i]) != shape) endrun("ERROR: column_diagnostics: " + s.names[i] + " is not {nens}");
    out[i] = dm.get<real, 1>(s.names[i]).data();
  }
  bool has_cldfrac = dm.entry_exists("cldfrac");
  if (has_cldfrac && dm.get_shape("cldfrac") != cells) endrun("ERROR: column_diagnostics: cldfrac is not {nz,ny,nx,nens}");
  const double *fields[6] = {dm.get<real const, 4>("temp").data(), dm.get<real const, 4>("density_dry").data(),
                             dm.get<real const, 4>("water_vapor").data(),
                             s.cloud.empty() ? nullptr : dm.get<real const, 4>(s.cloud).data(),
                             s.ice.empty() ? nullptr : dm.get<real const, 4>(s.ice).data(),
                             has_cldfrac ? dm.get<real const, 4>("cldfrac").data() : nullptr};
  const double *precip[2] = {s.precip_liq.empty() ? nullptr : dm.get<real const, 3>(s.precip_liq).data(),
                             s.precip_ice.empty() ? nullptr : dm.get<real const, 3>(s.precip_ice).data()};
  int rc = pam_amd_column_diagnostics(s.nens, s.nx, s.ny, s.nz, fields, dm.get<real const, 2>("vertical_interface_height").data(), precip,
                                      coupler.get_option<real>("R_d"), coupler.get_option<real>("R_v"),
                                      coupler.get_option<real>("crm_diag_p_low"), coupler.get_option<real>("crm_diag_p_high"),
                                      coupler.get_option<real>("crm_diag_cwp_threshold"), out, factor, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
