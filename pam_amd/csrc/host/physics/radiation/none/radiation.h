// physics/radiation/none/radiation.h -- the `Radiation` plug-in that does nothing (-DPAM_RAD=none): the members of the reference's
// physics/radiation/none/radiation.h.
#pragma once
#include <string>

#include "pam_coupler.h"

class Radiation {
 public:
  Radiation() {}
  std::string radiation_name() const { return "none"; }
  void init(pam::PamCoupler &coupler) { coupler.set_option<std::string>("radiation", "none"); }
  void timeStep(pam::PamCoupler &coupler) {}
  void finalize(pam::PamCoupler &coupler) {}
};
