// physics/radiation/forced_amd/radiation.h -- the C++ plug-in class PAM's drivers instantiate as `Radiation` (selected with
// -DPAM_RAD=forced_amd), same duck-typed members as the reference's physics/radiation/forced/radiation.h: the GCM's radiative
// heating, given on rad_ny x rad_nx groups of CRM columns, applied to the CRM temperature every CRM step.  Forwards to
// pam_amd_radiation_forced (include/pam_amd_modules.h).  Deliberate deviations: the sizes come from the
// coupler's getters, and options ncrms / crm_nz / crm_nx / crm_ny must agree with them where they exist (nothing in the reference
// tree sets them); rad_nx and rad_ny must divide the CRM grid; crm_dt must be finite and cp_d finite and positive.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

class Radiation {
  struct Sizes { int nens, nz, ny, nx, rad_ny, rad_nx; };

  static void agree(pam::PamCoupler const &coupler, char const *opt, int have) {
    if (coupler.option_exists(opt) && coupler.get_option<int>(opt) != have)
      endrun(std::string("ERROR: radiation: option ") + opt + " disagrees with the coupler's size");
  }

  static Sizes sizes(pam::PamCoupler const &coupler) {
    Sizes s{coupler.get_nens(), coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), 0, 0};
    if (s.nens < 1 || s.nz < 1 || s.ny < 1 || s.nx < 1) endrun("ERROR: radiation: the coupler state is not allocated");
    agree(coupler, "ncrms", s.nens);
    agree(coupler, "crm_nz", s.nz);
    agree(coupler, "crm_nx", s.nx);
    agree(coupler, "crm_ny", s.ny);
    s.rad_nx = coupler.get_option<int>("rad_nx");
    s.rad_ny = coupler.get_option<int>("rad_ny");
    if (s.rad_nx < 1 || s.rad_ny < 1 || s.nx % s.rad_nx != 0 || s.ny % s.rad_ny != 0)
      endrun("ERROR: radiation: rad_nx and rad_ny must be >= 1 and divide crm_nx and crm_ny");
    return s;
  }

 public:
  Radiation() {}
  std::string radiation_name() const { return "forced"; }

  void init(pam::PamCoupler &coupler) {                                        // radiation.h:16-25
    auto &dm = coupler.get_data_manager_device_readwrite();
    auto s = sizes(coupler);
    if (dm.entry_exists("rad_enthalpy_tend")) endrun("ERROR: Duplicate entry name rad_enthalpy_tend");
    coupler.set_option<std::string>("radiation", "forced");
    dm.register_and_allocate<real>("rad_enthalpy_tend", "radiation tendency from external calculation", {s.nz, s.rad_ny, s.rad_nx, s.nens},
                                   {"z", "rad_y", "rad_x", "nens"});
  }

  void timeStep(pam::PamCoupler &coupler) {                                    // radiation.h:27-45
    auto &dm = coupler.get_data_manager_device_readwrite();
    auto s = sizes(coupler);
    auto dt = coupler.get_option<real>("crm_dt");
    auto cp_d = coupler.get_option<real>("cp_d");
    if (!std::isfinite(dt)) endrun("ERROR: radiation: crm_dt must be finite");
    if (!std::isfinite(cp_d) || !(cp_d > 0)) endrun("ERROR: radiation: cp_d must be finite and positive");
    if (dm.get_shape("rad_enthalpy_tend") != std::vector<int>{s.nz, s.rad_ny, s.rad_nx, s.nens})
      endrun("ERROR: radiation: rad_enthalpy_tend is not (nz,rad_ny,rad_nx,nens)");
    int rc = pam_amd_radiation_forced(s.nens, s.nx, s.ny, s.nz, s.rad_nx, s.rad_ny, dm.get<real, 4>("temp").data(),
                                      dm.get<real const, 4>("rad_enthalpy_tend").data(), cp_d, dt, nullptr);
    if (rc) endrun(pam_amd_awfl_last_error());
  }

  void finalize(pam::PamCoupler &coupler) {}
};
