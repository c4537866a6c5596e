// modules/hyperdiffusion.h -- the horizontal hyperdiffusion (the scale-selective fourth-difference damping of the 2 dx mode that
// E3SM-MMF's CRM applies between the sponge layer and the physics) over pam_amd_hyperdiffusion (include/pam_amd_modules.h).  The method
// is not part of the reference tree; the contract is this project's.
//   modules::hyperdiffusion_init(coupler, tau)   once: sets the option "crm_hyperdiff_timescale" (seconds; the 2 dx mode of one
//                                                direction decays by dt / tau per call, so tau >= crm_dt)
//   modules::hyperdiffusion(coupler [, dt])      once per CRM step, after the sponge layer and the surface friction and before SGS and
//                                                microphysics: temp, uvel, vvel, wvel and every registered tracer, in place; a tracer
//                                                registered as positive is handed on non-negative (the level fill of mean-state
//                                                acceleration).  density_dry is never touched.  dt defaults to the option "crm_dt".
#pragma once
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

inline void hyperdiffusion_init(pam::PamCoupler &coupler, real tau) {
  if (!(tau > 0)) endrun("ERROR: hyperdiffusion: crm_hyperdiff_timescale must be positive");
  coupler.set_option<real>("crm_hyperdiff_timescale", tau);
}

inline void hyperdiffusion(pam::PamCoupler &coupler, real dt) {
  if (!coupler.option_exists("crm_hyperdiff_timescale")) endrun("ERROR: hyperdiffusion: call hyperdiffusion_init first");
  auto &dm = coupler.get_data_manager_device_readwrite();
  std::vector<double *> f;
  std::vector<unsigned char> positive;
  for (char const *n : {"temp", "uvel", "vvel", "wvel"}) {
    f.push_back(dm.get<real, 4>(n).data());
    positive.push_back(0);
  }
  for (auto &n : coupler.get_tracer_names()) {
    std::string desc;
    bool found = false, pos = false, adds_mass = false;
    coupler.get_tracer_info(n, desc, found, pos, adds_mass);
    f.push_back(dm.get<real, 4>(n).data());
    positive.push_back(found && pos ? 1 : 0);
  }
  int rc = pam_amd_hyperdiffusion(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), (int)f.size(), f.data(),
                                  positive.data(), dt, coupler.get_option<real>("crm_hyperdiff_timescale"), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

inline void hyperdiffusion(pam::PamCoupler &coupler) { hyperdiffusion(coupler, coupler.get_option<real>("crm_dt")); }

}  // namespace modules
