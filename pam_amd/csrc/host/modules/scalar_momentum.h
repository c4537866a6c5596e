// modules/scalar_momentum.h -- explicit scalar momentum transport for 2-D CRMs (Tulich 2015; E3SM-MMF's use_MMF_ESMT): the large-scale
// u and v ride as two passive scalars that take the linearised pressure-gradient force every CRM step, forwarding to the C ABI
// (include/pam_amd_modules.h at pam_amd_esmt_pgf).  Not part of the reference tree; shaped like modules/large_scale_forcing.h.
//   modules::esmt_init(coupler [, kmax])   once, BEFORE the dycore is initialised (it takes its tracer table then): registers the
//                                  tracers "esmt_u" and "esmt_v" (not positive, adding no mass), the DEVICE entries {nz,nens}
//                                  "esmt_rho_mean", "esmt_u_mean", "esmt_v_mean", "esmt_u_forcing", "esmt_v_forcing", "esmt_u_tend",
//                                  "esmt_v_tend" (zeroed), the tables "esmt_cos" and "esmt_sin" {nx} formed on the host, and the
//                                  workspace "esmt_workspace" (6 kmax nz nens doubles); sets the option "esmt_kmax" (default nx / 2)
//   modules::esmt_set(coupler [, source])  both scalars = rho times a profile: "gcm" takes "gcm_uvel" / "gcm_vvel"; "crm" the level
//                                  means of uvel and vvel (pam_amd_msa_diagnose: the slot order every level mean of the project has)
//   modules::esmt_compute_forcing  once per GCM step: "esmt_x_forcing" = (gcm_x - M(esmt_x / rho)) / gcm_physics_dt
//   modules::esmt_pgf(coupler [, dt [, forcing]])  every CRM step, after the dycore and the sponge layer and before the SGS:
//                                  pam_amd_esmt_diagnose, then pam_amd_esmt_pgf in place on esmt_u and esmt_v
//   modules::esmt_compute_feedback at the end of a GCM step: "esmt_x_tend" = (M(esmt_x / rho) - gcm_x) / gcm_physics_dt
#pragma once
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

inline void esmt_init(pam::PamCoupler &coupler, int kmax = -1) {
  int nz = coupler.get_nz(), ny = coupler.get_ny(), nx = coupler.get_nx(), nens = coupler.get_nens();
  if (ny != 1) endrun("ERROR: esmt_init: explicit scalar momentum transport is for 2-D CRMs (ny == 1)");
  if (nx < 2 || nz < 2) endrun("ERROR: esmt_init: nx and nz must be >= 2");
  if (kmax == -1) kmax = nx / 2;
  if (kmax < 0 || kmax > nx / 2) endrun("ERROR: esmt_init: kmax must be in [0, nx / 2]");
  auto &dm = coupler.get_data_manager_device_readwrite();
  if (dm.entry_exists("esmt_cos")) endrun("ERROR: esmt_init: called twice");
  coupler.add_tracer("esmt_u", "large-scale u carried as a scalar [kg/m3 m/s]", false, false);
  coupler.add_tracer("esmt_v", "large-scale v carried as a scalar [kg/m3 m/s]", false, false);
  struct Named { char const *name, *desc; };
  const Named profiles[7] = {{"esmt_rho_mean", "level mean of the total density [kg/m3]"},
                             {"esmt_u_mean", "level mean of esmt_u / rho [m/s]"},
                             {"esmt_v_mean", "level mean of esmt_v / rho [m/s]"},
                             {"esmt_u_forcing", "GCM forcing of the scalar u [m/s2]"},
                             {"esmt_v_forcing", "GCM forcing of the scalar v [m/s2]"},
                             {"esmt_u_tend", "scalar momentum feedback, u [m/s2]"},
                             {"esmt_v_tend", "scalar momentum feedback, v [m/s2]"}};
  for (auto const &p : profiles) dm.register_and_allocate<real>(p.name, p.desc, {nz, nens}, {"z", "nens"});
  std::vector<real> cos_host(nx), sin_host(nx);
  if (pam_amd_esmt_tables(nx, cos_host.data(), sin_host.data())) endrun(pam_amd_awfl_last_error());
  dm.register_and_allocate<real>("esmt_cos", "table of the transform along x", {nx}, {"x"});
  dm.register_and_allocate<real>("esmt_sin", "table of the transform along x", {nx}, {"x"});
  if (hipMemcpy(dm.get<real, 1>("esmt_cos").data(), cos_host.data(), nx * sizeof(real), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dm.get<real, 1>("esmt_sin").data(), sin_host.data(), nx * sizeof(real), hipMemcpyHostToDevice) != hipSuccess)
    endrun("memcpy");
  long long words = pam_amd_esmt_workspace_doubles(nens, nz, kmax);
  dm.register_and_allocate<real>("esmt_workspace", "spectral coefficients and right-hand sides of the pressure solve",
                                 {(int)(words > 0 ? words : 1)});
  coupler.set_option<int>("esmt_kmax", kmax);
}

inline void esmt_set(pam::PamCoupler &coupler, std::string source = "gcm") {
  if (!coupler.option_exists("esmt_kmax")) endrun("ERROR: esmt_set: call esmt_init first");
  auto &dm = coupler.get_data_manager_device_readwrite();
  int nens = coupler.get_nens(), nx = coupler.get_nx(), ny = coupler.get_ny(), nz = coupler.get_nz();
  real const *src_u = nullptr, *src_v = nullptr;
  if (source == "gcm") {
    src_u = dm.get<real const, 2>("gcm_uvel").data();
    src_v = dm.get<real const, 2>("gcm_vvel").data();
  } else if (source == "crm") {
    real const *u = dm.get<real const, 4>("uvel").data(), *v = dm.get<real const, 4>("vvel").data();
    real const *fields[6] = {u, v, nullptr, nullptr, u, v};
    // the first two means of the table are not wanted: the tendencies of the feedback take them, and are written anew before use
    real *save[4] = {dm.get<real, 2>("esmt_u_tend").data(), dm.get<real, 2>("esmt_v_tend").data(), dm.get<real, 2>("esmt_u_mean").data(),
                     dm.get<real, 2>("esmt_v_mean").data()};
    if (pam_amd_msa_diagnose(nens, nx, ny, nz, fields, save, nullptr)) endrun(pam_amd_awfl_last_error());
    src_u = save[2];
    src_v = save[3];
  } else {
    endrun("ERROR: esmt_set: source must be \"gcm\" or \"crm\"");
  }
  if (pam_amd_esmt_set(nens, nx, ny, nz, dm.get<real const, 4>("density_dry").data(), dm.get<real const, 4>("water_vapor").data(), src_u, src_v,
                       dm.get<real, 4>("esmt_u").data(), dm.get<real, 4>("esmt_v").data(), nullptr))
    endrun(pam_amd_awfl_last_error());
}

namespace esmt_detail {
// the level means, and the tendencies against gcm_uvel / gcm_vvel where tend_u is given
inline void diagnose(pam::PamCoupler &coupler, char const *who, char const *tend_u, char const *tend_v, bool feedback) {
  if (!coupler.option_exists("esmt_kmax")) endrun(std::string("ERROR: ") + who + ": call esmt_init first");
  auto &dm = coupler.get_data_manager_device_readwrite();
  real const *gu = tend_u ? dm.get<real const, 2>("gcm_uvel").data() : nullptr, *gv = tend_u ? dm.get<real const, 2>("gcm_vvel").data() : nullptr;
  int rc = pam_amd_esmt_diagnose(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(),
                                 dm.get<real const, 4>("density_dry").data(), dm.get<real const, 4>("water_vapor").data(),
                                 dm.get<real const, 4>("esmt_u").data(), dm.get<real const, 4>("esmt_v").data(),
                                 dm.get<real, 2>("esmt_rho_mean").data(), dm.get<real, 2>("esmt_u_mean").data(),
                                 dm.get<real, 2>("esmt_v_mean").data(), gu, gv, tend_u ? coupler.get_option<real>("gcm_physics_dt") : 1.0,
                                 feedback ? 1 : 0, tend_u ? dm.get<real, 2>(tend_u).data() : nullptr,
                                 tend_u ? dm.get<real, 2>(tend_v).data() : nullptr, nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}
}  // namespace esmt_detail

inline void esmt_compute_forcing(pam::PamCoupler &coupler) {
  esmt_detail::diagnose(coupler, "esmt_compute_forcing", "esmt_u_forcing", "esmt_v_forcing", false);
}

inline void esmt_compute_feedback(pam::PamCoupler &coupler) {
  esmt_detail::diagnose(coupler, "esmt_compute_feedback", "esmt_u_tend", "esmt_v_tend", true);
}

inline void esmt_pgf(pam::PamCoupler &coupler, real dt = -1, bool forcing = true) {
  esmt_detail::diagnose(coupler, "esmt_pgf", nullptr, nullptr, false);
  if (dt < 0) dt = coupler.get_option<real>("crm_dt");
  auto &dm = coupler.get_data_manager_device_readwrite();
  int nens = coupler.get_nens(), nz = coupler.get_nz(), kmax = coupler.get_option<int>("esmt_kmax");
  auto profile = [&](char const *n) -> real const * { return dm.get<real const, 2>(n).data(); };
  int rc = pam_amd_esmt_pgf(nens, coupler.get_nx(), coupler.get_ny(), nz, dm.get<real, 4>("esmt_u").data(), dm.get<real, 4>("esmt_v").data(),
                            dm.get<real const, 4>("wvel").data(), dm.get<real const, 4>("density_dry").data(),
                            dm.get<real const, 4>("water_vapor").data(), profile("vertical_midpoint_height"), profile("vertical_cell_dz"),
                            profile("esmt_rho_mean"), profile("esmt_u_mean"), profile("esmt_v_mean"),
                            forcing ? profile("esmt_u_forcing") : nullptr, forcing ? profile("esmt_v_forcing") : nullptr,
                            dm.get<real const, 1>("esmt_cos").data(), dm.get<real const, 1>("esmt_sin").data(), coupler.get_dx(), dt, kmax,
                            dm.get<real, 1>("esmt_workspace").data(), pam_amd_esmt_workspace_doubles(nens, nz, kmax), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
