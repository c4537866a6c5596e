// modules/large_scale_forcing.h -- modules::ls_forcing_init(coupler, profiles) and modules::ls_forcing(coupler [, dt]): what a standalone
// CRM takes from outside its domain (SAM's forcing + subsidence + nudging + coriolis), forwarding to the C ABI (include/pam_amd_modules.h
// at pam_amd_ls_forcing).  Not part of the reference tree; shaped like modules/surface_fluxes.h.
//   modules::LsProfiles            HOST vectors, each empty (absent), nz values (every member alike) or nz*nens values (k, e), and fcor
//                                  empty, one value or nens values.  ug, vg and fcor come together; a target comes with its rate.
//   modules::ls_forcing_init       once, after the grid is set: registers what is given as DEVICE entries {nz,nens} "ls_wsub",
//                                  "ls_temp_tend", "ls_qv_tend", "ls_ug", "ls_vg", "ls_nudge_temp", "ls_nudge_qv", "ls_nudge_u",
//                                  "ls_nudge_v", "ls_nudge_rate_temp", "ls_nudge_rate_qv", "ls_nudge_rate_uv", "ls_fcor" {nens}, and
//                                  "ls_inc_temp/qv/u/v" {nz,nens} for every target.  What is not given is not registered, and its term
//                                  is absent.  From the host copies it sets the options "ls_courant_rate" = max |wsub| / min
//                                  (zmid(k+1) - zmid(k)) [1/s] and "ls_nudge_rate_max" [1/s]; a host model that overwrites an entry
//                                  between steps with values beyond them sets the two options again.
//   modules::ls_forcing            once per CRM step, after the sponge layer and before compute_surface_fluxes: pam_amd_ls_nudging where
//                                  a target is registered, then pam_amd_ls_forcing, in place on uvel, vvel, temp and every registered
//                                  tracer (the vapour is "water_vapor"); density_dry and wvel are never written.  Refuses dt
//                                  "ls_courant_rate" > 1 and dt "ls_nudge_rate_max" > 1 before anything is launched.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

struct LsProfiles {
  std::vector<real> wsub, temp_tend, qv_tend, ug, vg, nudge_temp, nudge_qv, nudge_u, nudge_v, nudge_rate_temp, nudge_rate_qv, nudge_rate_uv;
  std::vector<real> fcor;
};

inline void ls_forcing_init(pam::PamCoupler &coupler, LsProfiles const &p) {
  int nz = coupler.get_nz(), nens = coupler.get_nens();
  auto &dm = coupler.get_data_manager_device_readwrite();
  if (p.ug.empty() != p.vg.empty() || p.fcor.empty() != p.ug.empty()) endrun("ERROR: ls_forcing_init: ug, vg and fcor come together");
  struct Named { char const *name, *desc; std::vector<real> const *v; };
  const Named all[12] = {{"ls_wsub", "large-scale vertical velocity [m/s]", &p.wsub},
                         {"ls_temp_tend", "large-scale temperature tendency [K/s]", &p.temp_tend},
                         {"ls_qv_tend", "large-scale tendency of the vapour mixing ratio rho_v / rho [1/s]", &p.qv_tend},
                         {"ls_ug", "geostrophic wind, x [m/s]", &p.ug},
                         {"ls_vg", "geostrophic wind, y [m/s]", &p.vg},
                         {"ls_nudge_temp", "nudging target of the level-mean temperature [K]", &p.nudge_temp},
                         {"ls_nudge_qv", "nudging target of the level-mean rho_v / rho [1]", &p.nudge_qv},
                         {"ls_nudge_u", "nudging target of the level-mean uvel [m/s]", &p.nudge_u},
                         {"ls_nudge_v", "nudging target of the level-mean vvel [m/s]", &p.nudge_v},
                         {"ls_nudge_rate_temp", "nudging rate of temp [1/s]", &p.nudge_rate_temp},
                         {"ls_nudge_rate_qv", "nudging rate of rho_v / rho [1/s]", &p.nudge_rate_qv},
                         {"ls_nudge_rate_uv", "nudging rate of uvel and vvel [1/s]", &p.nudge_rate_uv}};
  if ((!p.nudge_temp.empty() && p.nudge_rate_temp.empty()) || (!p.nudge_qv.empty() && p.nudge_rate_qv.empty()) ||
      ((!p.nudge_u.empty() || !p.nudge_v.empty()) && p.nudge_rate_uv.empty()))
    endrun("ERROR: ls_forcing_init: a nudging target needs its rate");
  std::vector<real> wsub_host;
  real rate_max = 0;
  for (auto const &a : all) {
    if (a.v->empty()) continue;
    std::vector<real> h((size_t)nz * nens);
    if (a.v->size() == (size_t)nz) {
      for (int k = 0; k < nz; k++)
        for (int e = 0; e < nens; e++) h[(size_t)k * nens + e] = (*a.v)[k];
    } else if (a.v->size() == h.size()) {
      h = *a.v;
    } else {
      endrun(std::string("ERROR: ls_forcing_init: ") + a.name + " needs nz values or nz*nens values");
    }
    if (!dm.entry_exists(a.name)) dm.register_and_allocate<real>(a.name, a.desc, {nz, nens}, {"z", "nens"});
    if (hipMemcpy(dm.get<real, 2>(a.name).data(), h.data(), h.size() * sizeof(real), hipMemcpyHostToDevice) != hipSuccess) endrun("memcpy");
    if (std::string(a.name) == "ls_wsub") wsub_host = h;
    if (std::string(a.name).rfind("ls_nudge_rate_", 0) == 0) rate_max = std::max(rate_max, *std::max_element(h.begin(), h.end()));
  }
  if (!p.fcor.empty()) {
    if (p.fcor.size() != 1 && p.fcor.size() != (size_t)nens) endrun("ERROR: ls_forcing_init: fcor needs one value or nens values");
    std::vector<real> f(nens);
    for (int e = 0; e < nens; e++) f[e] = p.fcor[p.fcor.size() == 1 ? 0 : e];
    if (!dm.entry_exists("ls_fcor")) dm.register_and_allocate<real>("ls_fcor", "Coriolis parameter [1/s]", {nens}, {"nens"});
    if (hipMemcpy(dm.get<real, 1>("ls_fcor").data(), f.data(), f.size() * sizeof(real), hipMemcpyHostToDevice) != hipSuccess) endrun("memcpy");
  }
  char const *targets[4] = {"ls_nudge_temp", "ls_nudge_qv", "ls_nudge_u", "ls_nudge_v"};
  char const *incs[4] = {"ls_inc_temp", "ls_inc_qv", "ls_inc_u", "ls_inc_v"};
  for (int x = 0; x < 4; x++)
    if (dm.entry_exists(targets[x]) && !dm.entry_exists(incs[x]))
      dm.register_and_allocate<real>(incs[x], "nudging increment of the level mean", {nz, nens}, {"z", "nens"});
  real courant = 0;
  if (!wsub_host.empty() && nz > 1) {
    std::vector<real> zmid((size_t)nz * nens);
    if (hipMemcpy(zmid.data(), dm.get<real const, 2>("vertical_midpoint_height").data(), zmid.size() * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess)
      endrun("memcpy");
    for (int e = 0; e < nens; e++) {
      real wmax = 0, dzmin = zmid[(size_t)nens + e] - zmid[e];
      for (int k = 0; k < nz; k++) wmax = std::max(wmax, std::fabs(wsub_host[(size_t)k * nens + e]));
      for (int k = 0; k + 1 < nz; k++) dzmin = std::min(dzmin, zmid[(size_t)(k + 1) * nens + e] - zmid[(size_t)k * nens + e]);
      courant = std::max(courant, wmax / dzmin);
    }
  }
  coupler.set_option<real>("ls_courant_rate", courant);
  coupler.set_option<real>("ls_nudge_rate_max", rate_max);
}

inline void ls_forcing(pam::PamCoupler &coupler, real dt = -1) {
  if (!coupler.option_exists("ls_courant_rate")) endrun("ERROR: ls_forcing: call ls_forcing_init first");
  if (dt < 0) dt = coupler.get_option<real>("crm_dt");
  if (!(dt * coupler.get_option<real>("ls_courant_rate") <= 1.0))
    endrun("ERROR: ls_forcing: max |ls_wsub| dt exceeds the thinnest layer (dt x ls_courant_rate > 1)");
  if (!(dt * coupler.get_option<real>("ls_nudge_rate_max") <= 1.0))
    endrun("ERROR: ls_forcing: dt x nudging rate exceeds 1 (dt x ls_nudge_rate_max > 1)");
  auto &dm = coupler.get_data_manager_device_readwrite();
  auto profile = [&](char const *n) -> real const * { return dm.entry_exists(n) ? dm.get<real const, 2>(n).data() : nullptr; };
  int nens = coupler.get_nens(), nx = coupler.get_nx(), ny = coupler.get_ny(), nz = coupler.get_nz();
  std::vector<double *> tracers;
  std::vector<unsigned char> positive;
  for (auto &n : coupler.get_tracer_names()) {
    std::string desc;
    bool found = false, pos = false, adds_mass = false;
    coupler.get_tracer_info(n, desc, found, pos, adds_mass);
    tracers.push_back(dm.get<real, 4>(n).data());
    positive.push_back(found && pos ? 1 : 0);
  }
  real const *rho_d = dm.get<real const, 4>("density_dry").data(), *rho_v = dm.get<real const, 4>("water_vapor").data();
  char const *targets[4] = {"ls_nudge_temp", "ls_nudge_qv", "ls_nudge_u", "ls_nudge_v"};
  char const *rates[4] = {"ls_nudge_rate_temp", "ls_nudge_rate_qv", "ls_nudge_rate_uv", "ls_nudge_rate_uv"};
  char const *incs[4] = {"ls_inc_temp", "ls_inc_qv", "ls_inc_u", "ls_inc_v"};
  real const *target[4], *rate[4];
  real *inc[4];
  bool nudged = false;
  for (int x = 0; x < 4; x++) {
    target[x] = profile(targets[x]);
    rate[x] = target[x] ? profile(rates[x]) : nullptr;
    inc[x] = target[x] ? dm.get<real, 2>(incs[x]).data() : nullptr;
    nudged = nudged || target[x];
  }
  if (nudged) {
    real const *fields[5] = {dm.get<real const, 4>("temp").data(), rho_d, rho_v, dm.get<real const, 4>("uvel").data(),
                             dm.get<real const, 4>("vvel").data()};
    if (pam_amd_ls_nudging(nens, nx, ny, nz, fields, target, rate, dt, inc, nullptr)) endrun(pam_amd_awfl_last_error());
  }
  int rc = pam_amd_ls_forcing(nens, nx, ny, nz, dm.get<real, 4>("uvel").data(), dm.get<real, 4>("vvel").data(), dm.get<real, 4>("temp").data(),
                              (int)tracers.size(), tracers.empty() ? nullptr : tracers.data(), tracers.empty() ? nullptr : positive.data(), rho_d,
                              rho_v, profile("vertical_midpoint_height"), profile("ls_wsub"), profile("ls_temp_tend"), profile("ls_qv_tend"),
                              nudged ? inc : nullptr, dm.entry_exists("ls_fcor") ? dm.get<real const, 1>("ls_fcor").data() : nullptr,
                              profile("ls_ug"), profile("ls_vg"), dt, coupler.get_option<real>("grav"), coupler.get_option<real>("cp_d"), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
