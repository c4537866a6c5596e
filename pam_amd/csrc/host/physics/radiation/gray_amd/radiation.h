// physics/radiation/gray_amd/radiation.h -- the native `Radiation` plug-in (-DPAM_RAD=gray_amd): a grey two-stream longwave scheme, the
// radiation that needs no external library (as kessler_amd is the microphysics and smag_amd the SGS closure that need none), with the
// duck-typed members of the reference's physics/radiation/*/radiation.h.  The method is not part of the reference tree; the contract is
// this project's (include/pam_amd_modules.h at pam_amd_radiation_gray).  Every rad_gray_every-th timeStep is one
// call of pam_amd_radiation_gray: it fills "rad_heating" (K/s), "rad_olr", "rad_lw_down_sfc" and "rad_lw_up_sfc" (W/m2) and applies the
// heating to temp; the steps between apply the stored "rad_heating" through pam_amd_radiation_forced with rad_nx = nx, rad_ny = ny
// and cp_d = 1.0, which is temp += rad_heating / 1.0 * crm_dt: exact, and no kernel of its own.  The cloud species come from option
// "micro": "kessler" gives "cloud_liquid" as liquid and no ice, "p3" gives "cloud_water" and "ice", "ice1m" gives "cloud_liquid" and "cloud_ice", "none" (or no option) neither.
// The surface radiates at "sfc_temp" (ny,nx,nens) where that entry exists, else at the lowest level's temp.
//   options read:  crm_dt, cp_d, micro, sigma (5.670374419e-8 where absent), rad_gray_k_d/k_v/k_l/k_i, rad_gray_lw_down_top, rad_gray_every
//   options set by init:  "radiation" = "gray"; rad_gray_k_d = 1e-4, rad_gray_k_v = 0.1, rad_gray_k_l = 85 (the GCSS DYCOMS-II value),
//                  rad_gray_k_i = 40 [m2/kg], rad_gray_lw_down_top = 0 [W/m2], rad_gray_every = 1, each only where absent.
// The default coefficients are a starting point: they are untuned.
// The sun: with option "rad_gray_shortwave" = true before init (false where absent) init also registers "rad_sw_heating" (K/s),
// "rad_sw_down_sfc", "rad_sw_up_sfc", "rad_sw_up_top" (W/m2) and "rad_coszen" (nens), the cosine of the solar zenith angle of every
// member, filled with rad_gray_sw_coszen; a host model overwrites "rad_coszen" between steps, and that is the diurnal cycle.  A
// recompute step is then the longwave call followed by one call of pam_amd_radiation_gray_sw (the surface reflects "sfc_albedo"
// (ny,nx,nens) where that entry exists, else rad_gray_sw_albedo), and a step between applies both stored heatings, two calls of
// pam_amd_radiation_forced.  Without the option the class makes exactly the calls described above.
//   options set by init where the sun is on, each only where absent:  rad_gray_sw_solar_constant = 1361 [W/m2], rad_gray_sw_coszen = 1,
//                  rad_gray_sw_albedo = 0.07, rad_gray_sw_a_d = 1e-6, rad_gray_sw_a_v = 2e-3, rad_gray_sw_a_l = 0.1, rad_gray_sw_a_i = 0.1
//                  (mass absorption), rad_gray_sw_s_l = 11, rad_gray_sw_s_i = 5 (mass backscatter: extinction x (1 - g) / 2) [m2/kg].
// These defaults too are untuned starting points.
#pragma once
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

#ifndef PAM_RAD_CLASS
#define PAM_RAD_CLASS Radiation      // a driver that holds several Radiation classes names each of them before the include
#endif

class PAM_RAD_CLASS {
  int calls = 0;                     // timeSteps since init: the fluxes are recomputed where calls % rad_gray_every == 0

  static void chk(int rc) { if (rc) endrun(pam_amd_awfl_last_error()); }
  static void dflt(pam::PamCoupler &coupler, char const *name, real v) {
    if (!coupler.option_exists(name)) coupler.set_option<real>(name, v);
  }

 public:
  PAM_RAD_CLASS() {}
  std::string radiation_name() const { return "gray"; }

  void init(pam::PamCoupler &coupler) {
    int nx = coupler.get_nx(), ny = coupler.get_ny(), nz = coupler.get_nz(), nens = coupler.get_nens();
    auto &dm = coupler.get_data_manager_device_readwrite();
    coupler.set_option<std::string>("radiation", "gray");
    dflt(coupler, "rad_gray_k_d", 1.0e-4);
    dflt(coupler, "rad_gray_k_v", 0.1);
    dflt(coupler, "rad_gray_k_l", 85.0);
    dflt(coupler, "rad_gray_k_i", 40.0);
    dflt(coupler, "rad_gray_lw_down_top", 0.0);
    if (!coupler.option_exists("rad_gray_every")) coupler.set_option<int>("rad_gray_every", 1);
    // allocations are zero-filled
    if (!dm.entry_exists("rad_heating")) dm.register_and_allocate<real>("rad_heating", "longwave heating rate [K/s]", {nz, ny, nx, nens}, {"z", "y", "x", "nens"});
    if (!dm.entry_exists("rad_olr")) dm.register_and_allocate<real>("rad_olr", "outgoing longwave radiation [W/m2]", {ny, nx, nens}, {"y", "x", "nens"});
    if (!dm.entry_exists("rad_lw_down_sfc")) dm.register_and_allocate<real>("rad_lw_down_sfc", "downward longwave flux at the surface [W/m2]", {ny, nx, nens}, {"y", "x", "nens"});
    if (!dm.entry_exists("rad_lw_up_sfc")) dm.register_and_allocate<real>("rad_lw_up_sfc", "upward longwave flux at the surface [W/m2]", {ny, nx, nens}, {"y", "x", "nens"});
    calls = 0;
    if (!coupler.option_exists("rad_gray_shortwave")) coupler.set_option<bool>("rad_gray_shortwave", false);
    if (!coupler.get_option<bool>("rad_gray_shortwave")) return;
    dflt(coupler, "rad_gray_sw_solar_constant", 1361.0);
    dflt(coupler, "rad_gray_sw_coszen", 1.0);
    dflt(coupler, "rad_gray_sw_albedo", 0.07);
    dflt(coupler, "rad_gray_sw_a_d", 1.0e-6);
    dflt(coupler, "rad_gray_sw_a_v", 2.0e-3);
    dflt(coupler, "rad_gray_sw_a_l", 0.1);
    dflt(coupler, "rad_gray_sw_a_i", 0.1);
    dflt(coupler, "rad_gray_sw_s_l", 11.0);
    dflt(coupler, "rad_gray_sw_s_i", 5.0);
    if (!dm.entry_exists("rad_sw_heating")) dm.register_and_allocate<real>("rad_sw_heating", "shortwave heating rate [K/s]", {nz, ny, nx, nens}, {"z", "y", "x", "nens"});
    if (!dm.entry_exists("rad_sw_down_sfc")) dm.register_and_allocate<real>("rad_sw_down_sfc", "downward shortwave flux at the surface [W/m2]", {ny, nx, nens}, {"y", "x", "nens"});
    if (!dm.entry_exists("rad_sw_up_sfc")) dm.register_and_allocate<real>("rad_sw_up_sfc", "upward shortwave flux at the surface [W/m2]", {ny, nx, nens}, {"y", "x", "nens"});
    if (!dm.entry_exists("rad_sw_up_top")) dm.register_and_allocate<real>("rad_sw_up_top", "upward shortwave flux at the model top [W/m2]", {ny, nx, nens}, {"y", "x", "nens"});
    if (!dm.entry_exists("rad_coszen")) {
      dm.register_and_allocate<real>("rad_coszen", "cosine of the solar zenith angle of every member", {nens}, {"nens"});
      std::vector<real> mu0(nens, coupler.get_option<real>("rad_gray_sw_coszen"));
      if (hipMemcpy(dm.get<real, 1>("rad_coszen").data(), mu0.data(), mu0.size() * sizeof(real), hipMemcpyHostToDevice) != hipSuccess)
        endrun("ERROR: radiation: could not fill rad_coszen");
    }
  }

  void timeStep(pam::PamCoupler &coupler) {
    int nx = coupler.get_nx(), ny = coupler.get_ny(), nz = coupler.get_nz(), nens = coupler.get_nens();
    real dt = coupler.get_option<real>("crm_dt"), cp_d = coupler.get_option<real>("cp_d");
    int every = coupler.get_option<int>("rad_gray_every");
    if (every < 1) endrun("ERROR: radiation: rad_gray_every must be >= 1");
    auto &dm = coupler.get_data_manager_device_readwrite();
    real *temp = dm.get<real, 4>("temp").data(), *heating = dm.get<real, 4>("rad_heating").data();
    bool sun = coupler.option_exists("rad_gray_shortwave") && coupler.get_option<bool>("rad_gray_shortwave");
    if (calls++ % every != 0) {        // between two flux computations: temp += rad_heating / 1.0 * crm_dt
      chk(pam_amd_radiation_forced(nens, nx, ny, nz, nx, ny, temp, heating, 1.0, dt, nullptr));
      if (sun) chk(pam_amd_radiation_forced(nens, nx, ny, nz, nx, ny, temp, dm.get<real const, 4>("rad_sw_heating").data(), 1.0, dt, nullptr));
      return;
    }
    std::string micro = coupler.option_exists("micro") ? coupler.get_option<std::string>("micro") : std::string("none");
    std::vector<double const *> liquid, ice;
    if (micro == "kessler") liquid.push_back(dm.get<real const, 4>("cloud_liquid").data());
    else if (micro == "p3") { liquid.push_back(dm.get<real const, 4>("cloud_water").data()); ice.push_back(dm.get<real const, 4>("ice").data()); }
    else if (micro == "ice1m") { liquid.push_back(dm.get<real const, 4>("cloud_liquid").data()); ice.push_back(dm.get<real const, 4>("cloud_ice").data()); }
    else if (micro != "none") endrun("ERROR: radiation: the gray scheme knows the species of micro = kessler, p3 and none, not of " + micro);
    real sigma = coupler.option_exists("sigma") ? coupler.get_option<real>("sigma") : 5.670374419e-8;
    real const *sfc_temp = dm.entry_exists("sfc_temp") ? dm.get<real const, 3>("sfc_temp").data() : nullptr;
    chk(pam_amd_radiation_gray(nens, nx, ny, nz, temp, dm.get<real const, 4>("density_dry").data(), dm.get<real const, 4>("water_vapor").data(),
                               (int)liquid.size(), liquid.data(), (int)ice.size(), ice.data(),
                               dm.get<real const, 2>("vertical_interface_height").data(), sfc_temp, coupler.get_option<real>("rad_gray_k_d"),
                               coupler.get_option<real>("rad_gray_k_v"), coupler.get_option<real>("rad_gray_k_l"),
                               coupler.get_option<real>("rad_gray_k_i"), sigma, cp_d, coupler.get_option<real>("rad_gray_lw_down_top"), dt, heating,
                               dm.get<real, 3>("rad_olr").data(), dm.get<real, 3>("rad_lw_down_sfc").data(),
                               dm.get<real, 3>("rad_lw_up_sfc").data(), nullptr));
    if (!sun) return;
    real const *sfc_albedo = dm.entry_exists("sfc_albedo") ? dm.get<real const, 3>("sfc_albedo").data() : nullptr;
    chk(pam_amd_radiation_gray_sw(nens, nx, ny, nz, temp, dm.get<real const, 4>("density_dry").data(), dm.get<real const, 4>("water_vapor").data(),
                                  (int)liquid.size(), liquid.data(), (int)ice.size(), ice.data(),
                                  dm.get<real const, 2>("vertical_interface_height").data(), dm.get<real const, 1>("rad_coszen").data(), sfc_albedo,
                                  coupler.get_option<real>("rad_gray_sw_solar_constant"), coupler.get_option<real>("rad_gray_sw_a_d"),
                                  coupler.get_option<real>("rad_gray_sw_a_v"), coupler.get_option<real>("rad_gray_sw_a_l"),
                                  coupler.get_option<real>("rad_gray_sw_a_i"), coupler.get_option<real>("rad_gray_sw_s_l"),
                                  coupler.get_option<real>("rad_gray_sw_s_i"), coupler.get_option<real>("rad_gray_sw_albedo"), cp_d, dt,
                                  dm.get<real, 4>("rad_sw_heating").data(), dm.get<real, 3>("rad_sw_down_sfc").data(),
                                  dm.get<real, 3>("rad_sw_up_sfc").data(), dm.get<real, 3>("rad_sw_up_top").data(), nullptr));
  }

  void finalize(pam::PamCoupler &coupler) {}
};
