// modules/surface_friction.h -- modules::surface_friction_init(coupler, tau_in, bflx_in) and modules::compute_surface_friction(coupler)
// with the reference's signatures (pam_core/modules/surface_friction.h:66, :107), forwarding to the C ABI (include/pam_amd_modules.h).
// The init registers "z0" and "sfc_bflx" {nens} as the reference does (:75-76).  "sfc_mom_flx_u/v" {ny,nx,nens} belong to the SGS
// scheme in PAM (SHOC registers them, physics/sgs/shoc/SGS.h:119-120), and here to physics/sgs/smag_amd/SGS.h, which reads them as the
// lower boundary condition of uvel and vvel, and to physics/sgs/shoc_amd/SGS.h; the init registers them when they are absent (the SGS
// plug-in is `none`, or its init has not run yet).
#pragma once
#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

inline void surface_friction_init(pam::PamCoupler &coupler, realConst1d &tau_in, realConst1d &bflx_in) {
  auto nz = coupler.get_nz();
  auto ny = coupler.get_ny();
  auto nx = coupler.get_nx();
  auto nens = coupler.get_nens();
  if ((int)tau_in.size() != nens || (int)bflx_in.size() != nens) endrun("ERROR: surface_friction_init: tau and bflx need nens values");
  auto &dm = coupler.get_data_manager_device_readwrite();
  dm.register_and_allocate<real>("z0", "Momentum roughness height [m]", {nens}, {"nens"});
  dm.register_and_allocate<real>("sfc_bflx", "large-scale sfc buoyancy flux [K m/s]", {nens}, {"nens"});
  for (char const *n : {"sfc_mom_flx_u", "sfc_mom_flx_v"})
    if (!dm.entry_exists(n)) dm.register_and_allocate<real>(n, "surface momentum flux", {ny, nx, nens}, {"y", "x", "nens"});
  int rc = pam_amd_surface_friction_init(nens, nx, ny, nz, dm.get<real, 4>("density_dry").data(), dm.get<real, 4>("water_vapor").data(),
                                         dm.get<real, 2>("vertical_midpoint_height").data(), dm.get<real, 2>("gcm_uvel").data(),
                                         dm.get<real, 2>("gcm_vvel").data(), tau_in.data(), bflx_in.data(), dm.get<real, 1>("z0").data(),
                                         dm.get<real, 1>("sfc_bflx").data(), dm.get<real, 3>("sfc_mom_flx_u").data(),
                                         dm.get<real, 3>("sfc_mom_flx_v").data(), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

inline void compute_surface_friction(pam::PamCoupler &coupler) {
  auto nz = coupler.get_nz();
  auto ny = coupler.get_ny();
  auto nx = coupler.get_nx();
  auto nens = coupler.get_nens();
  auto &dm = coupler.get_data_manager_device_readwrite();
  int rc = pam_amd_surface_friction_compute(nens, nx, ny, nz, dm.get<real const, 4>("density_dry").data(),
                                            dm.get<real const, 4>("water_vapor").data(), dm.get<real const, 4>("uvel").data(),
                                            dm.get<real const, 4>("vvel").data(), dm.get<real const, 2>("vertical_midpoint_height").data(),
                                            dm.get<real const, 2>("vertical_interface_height").data(), dm.get<real, 1>("z0").data(),
                                            dm.get<real, 1>("sfc_bflx").data(), dm.get<real, 3>("sfc_mom_flx_u").data(),
                                            dm.get<real, 3>("sfc_mom_flx_v").data(), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
