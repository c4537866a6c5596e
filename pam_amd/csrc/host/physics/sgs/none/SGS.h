// physics/sgs/none/SGS.h -- the `SGS` plug-in that does nothing (-DPAM_SGS=none): the members of the reference's
// physics/sgs/none/SGS.h.
#pragma once
#include <string>

#include "pam_coupler.h"

class SGS {
 public:
  SGS() {}
  static int constexpr get_num_tracers() { return 0; }
  void init(pam::PamCoupler &coupler) { coupler.set_option<std::string>("sgs", "none"); }
  void timeStep(pam::PamCoupler &coupler) {}
  std::string sgs_name() const { return "none"; }
  void finalize(pam::PamCoupler &coupler) {}
};
