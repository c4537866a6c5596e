// modules/surface_fluxes.h -- modules::surface_fluxes_init(coupler, sst, slab_depth) and modules::compute_surface_fluxes(coupler, dt):
// bulk surface fluxes over a slab ocean, forwarding to the C ABI (include/pam_amd_modules.h at pam_amd_surface_fluxes).  Not part of
// the reference tree; shaped like modules/surface_friction.h.
// The init registers "sfc_temp" {ny,nx,nens} where absent and fills it with sst, "sfc_shf" and "sfc_lhf" where absent under the names
// and descriptions of physics/sgs/smag_amd/SGS.h, and "sfc_cn" and "sfc_cstar" {nens}, which it forms on the host from row 0 of
// "vertical_midpoint_height" and the roughness height: the entry "z0" where modules::surface_friction_init has made one, else 1e-4 m.
// The options "sfc_slab_depth", "sfc_gust" (1 m/s) and "sfc_wetness" (0.98) are set only where absent.  The slab's heat capacity is
// 1000.0 * 4186.0 * sfc_slab_depth J/m2/K.  Momentum is not this scheme's: compute_surface_friction remains the source of sfc_mom_flx_u/v.
#pragma once
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

inline void surface_fluxes_init(pam::PamCoupler &coupler, real sst = 300.0, real slab_depth = 0.0) {
  auto ny = coupler.get_ny();
  auto nx = coupler.get_nx();
  auto nens = coupler.get_nens();
  auto &dm = coupler.get_data_manager_device_readwrite();
  if (!dm.entry_exists("sfc_temp")) {
    dm.register_and_allocate<real>("sfc_temp", "surface temperature [K]", {ny, nx, nens}, {"y", "x", "nens"});
    std::vector<real> h((size_t)ny * nx * nens, sst);
    if (hipMemcpy(dm.get<real, 3>("sfc_temp").data(), h.data(), h.size() * sizeof(real), hipMemcpyHostToDevice) != hipSuccess) endrun("memcpy");
  }
  if (!dm.entry_exists("sfc_shf")) dm.register_and_allocate<real>("sfc_shf", "input surface sensible heat flux [W/m2]", {ny, nx, nens}, {"y", "x", "nens"});
  if (!dm.entry_exists("sfc_lhf")) dm.register_and_allocate<real>("sfc_lhf", "input surface latent heat flux [W/m2]", {ny, nx, nens}, {"y", "x", "nens"});
  if (!dm.entry_exists("sfc_cn")) dm.register_and_allocate<real>("sfc_cn", "neutral surface transfer coefficient [1]", {nens}, {"nens"});
  if (!dm.entry_exists("sfc_cstar")) dm.register_and_allocate<real>("sfc_cstar", "unstable-branch coefficient of the surface transfer [1]", {nens}, {"nens"});
  std::vector<real> zmid0(nens), z0(nens, 1.0e-4), cn(nens), cstar(nens);
  if (hipMemcpy(zmid0.data(), dm.get<real const, 2>("vertical_midpoint_height").data(), nens * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess)
    endrun("memcpy");
  if (dm.entry_exists("z0") &&
      hipMemcpy(z0.data(), dm.get<real const, 1>("z0").data(), nens * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess)
    endrun("memcpy");
  for (int e = 0; e < nens; e++) {
    if (!(z0[e] > 0) || !(zmid0[e] > z0[e])) endrun("ERROR: surface_fluxes_init: the lowest level must lie above a positive roughness height");
    const real r = zmid0[e] / z0[e], k = 0.4 / std::log(r);
    cn[e] = k * k;
    cstar[e] = ((5.3 * 9.4) * cn[e]) * std::sqrt(r);
  }
  if (hipMemcpy(dm.get<real, 1>("sfc_cn").data(), cn.data(), nens * sizeof(real), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dm.get<real, 1>("sfc_cstar").data(), cstar.data(), nens * sizeof(real), hipMemcpyHostToDevice) != hipSuccess)
    endrun("memcpy");
  if (!coupler.option_exists("sfc_slab_depth")) coupler.set_option<real>("sfc_slab_depth", slab_depth);
  if (!coupler.option_exists("sfc_gust")) coupler.set_option<real>("sfc_gust", 1.0);
  if (!coupler.option_exists("sfc_wetness")) coupler.set_option<real>("sfc_wetness", 0.98);
}

inline void compute_surface_fluxes(pam::PamCoupler &coupler, real dt = -1) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  if (!dm.entry_exists("sfc_cn")) endrun("ERROR: compute_surface_fluxes: call surface_fluxes_init first");
  if (dt < 0) dt = coupler.get_option<real>("crm_dt");
  real const *lw_down = nullptr, *lw_up = nullptr, *sw_down = nullptr, *sw_up = nullptr;          // by pairs, where they exist
  if (dm.entry_exists("rad_lw_down_sfc") && dm.entry_exists("rad_lw_up_sfc")) {
    lw_down = dm.get<real const, 3>("rad_lw_down_sfc").data();
    lw_up = dm.get<real const, 3>("rad_lw_up_sfc").data();
  }
  if (dm.entry_exists("rad_sw_down_sfc") && dm.entry_exists("rad_sw_up_sfc")) {
    sw_down = dm.get<real const, 3>("rad_sw_down_sfc").data();
    sw_up = dm.get<real const, 3>("rad_sw_up_sfc").data();
  }
  real latvap = coupler.option_exists("latvap") ? coupler.get_option<real>("latvap") : 2501000.0;
  int rc = pam_amd_surface_fluxes(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), dm.get<real const, 4>("temp").data(),
                                  dm.get<real const, 4>("density_dry").data(), dm.get<real const, 4>("water_vapor").data(),
                                  dm.get<real const, 4>("uvel").data(), dm.get<real const, 4>("vvel").data(),
                                  dm.get<real const, 2>("vertical_midpoint_height").data(), dm.get<real const, 1>("sfc_cn").data(),
                                  dm.get<real const, 1>("sfc_cstar").data(), dm.get<real, 3>("sfc_temp").data(), lw_down, lw_up, sw_down, sw_up,
                                  coupler.get_option<real>("sfc_gust"), coupler.get_option<real>("sfc_wetness"), coupler.get_option<real>("grav"),
                                  coupler.get_option<real>("cp_d"), coupler.get_option<real>("R_v"), latvap,
                                  1000.0 * 4186.0 * coupler.get_option<real>("sfc_slab_depth"), dt, dm.get<real, 3>("sfc_shf").data(),
                                  dm.get<real, 3>("sfc_lhf").data(), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
