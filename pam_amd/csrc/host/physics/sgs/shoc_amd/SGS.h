// physics/sgs/shoc_amd/SGS.h -- the C++ plug-in class PAM's drivers instantiate as `SGS` (selected with -DPAM_SGS=shoc_amd,
// physics/sgs/CMakeLists.txt), same duck-typed members as the reference's physics/sgs/shoc/SGS.h.  It is the COUPLING LAYER of SHOC: what
// the reference does around shoc_main (SGS.h:254-411 and :718-756) runs as two fused launches of libpam_amd_awfl.so
// (pam_amd_shoc_pack / pam_amd_shoc_unpack, include/pam_amd_modules.h); SHOC itself is SCREAM's code and is handed in:
//
//     SGS sgs;
//     sgs.set_shoc_main(my_shoc_main, my_state);     // int my_shoc_main(const pam_amd_shoc_args_t *args, void *user)
//
// my_shoc_main receives the arguments of pam::shoc_main_cxx (SGS.h:487-537) under their names as DEVICE pointers, in `layout` 1 =
// SCREAM's C++ layout ((col, lev), level fastest; hwind (col,2,lev); qtracers (col,tr,lev)) or 0 = the Fortran-call layout ((lev, col),
// column fastest), works in place and returns 0.  args->stream carries the pack step; the unpack step follows on the same stream.
// The one addition to the reference's members is set_shoc_main; a timeStep without one is an error.
#pragma once
#include <string>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

class SGS {
  pam_amd_shoc_main_fn shoc_main = nullptr;
  void *shoc_user = nullptr;
  void *ws = nullptr;                // the workspace: one device allocation, made on the first step
  int ws_key[6] = {0, 0, 0, 0, -1, -1};

  static void chk(int rc) { if (rc) endrun(pam_amd_awfl_last_error()); }

  void free_workspace() {
    if (ws) (void)pam_amd_shoc_workspace_destroy(ws);
    ws = nullptr;
  }

 public:
  // SGS.h:30-52
  real R_d, cp_d, cv_d, gamma_d, kappa_d, R_v, cp_v, cv_v, p0;
  bool micro_kessler, micro_p3;
  real latvap, latice, karman;
  real grav, cp_l;
  real etime;
  int npbl;
  bool first_step;
  int layout = 1;                    // of the arrays shoc_main receives; set before the first timeStep

  int static constexpr ID_TKE = 0;   // Local index for Turbulent Kinetic Energy (m^2/s^2)

  SGS() {                            // SGS.h:60-80
    R_d           = 287.042;
    cp_d          = 1004.64;
    cv_d          = cp_d - R_d;
    gamma_d       = cp_d / cv_d;
    kappa_d       = R_d  / cp_d;
    R_v           = 461.505;
    cp_v          = 1859;
    cv_v          = R_v - cp_v;
    p0            = 1.e5;
    grav          = 9.80616;
    first_step    = true;
    cp_l          = 4218.;
    micro_kessler = false;
    micro_p3      = false;
    latvap        = 2501000.0;
    latice        = 333700.0;
    karman        = 0.4;
    npbl          = -1;
    etime         = 0;
  }
  SGS(SGS const &) = delete;
  ~SGS() { free_workspace(); }

  static int constexpr get_num_tracers() {
    return 1;
  }

  // SHOC's entry point and an opaque pointer passed back to it
  void set_shoc_main(pam_amd_shoc_main_fn fn, void *user = nullptr) {
    shoc_main = fn;
    shoc_user = user;
  }

  void init(pam::PamCoupler &coupler) {                                         // SGS.h:92-146
    int nx   = coupler.get_nx  ();
    int ny   = coupler.get_ny  ();
    int nz   = coupler.get_nz  ();
    int nens = coupler.get_nens();
    coupler.add_tracer("tke" , "Turbulent Kinetic Energy (m^2/s^2)"   , true     , false );
    auto &dm = coupler.get_data_manager_device_readwrite();
    // allocations are zero-filled: the reference's "sgs zero" and "surface momentum flux zero" kernels
    dm.register_and_allocate<real>( "wthv_sec"     , "Buoyancy flux [K m/s]"                , {nz,ny,nx,nens} , {"z","y","x","nens"} );
    dm.register_and_allocate<real>( "tk"           , "Eddy coefficient for momentum [m2/s]" , {nz,ny,nx,nens} , {"z","y","x","nens"} );
    dm.register_and_allocate<real>( "tkh"          , "Eddy coefficent for heat [m2/s]"      , {nz,ny,nx,nens} , {"z","y","x","nens"} );
    dm.register_and_allocate<real>( "cldfrac"      , "Cloud fraction [-]"                   , {nz,ny,nx,nens} , {"z","y","x","nens"} );
    dm.register_and_allocate<real>( "inv_qc_relvar", "Inverse relative cloud water variance", {nz,ny,nx,nens} , {"z","y","x","nens"} );
    dm.register_and_allocate<real>("sfc_shf", "input surface sensible heat flux"            , {ny,nx,nens}, {"y","x","nens"} );
    dm.register_and_allocate<real>("sfc_lhf", "input surface latent heat flux"              , {ny,nx,nens}, {"y","x","nens"} );
    dm.register_and_allocate<real>( "sfc_mom_flx_u", "Surface flux of U-momentum"           , {ny,nx,nens} , {"y","x","nens"} );
    dm.register_and_allocate<real>( "sfc_mom_flx_v", "Surface flux of V-momentum"           , {ny,nx,nens} , {"y","x","nens"} );
    size_t n4 = (size_t)nz * ny * nx * nens * sizeof(real);
    if (hipMemset(dm.get<real,4>("tke").data(), 0, n4) != hipSuccess) endrun("ERROR: SHOC: cannot zero tke");
    coupler.set_option<std::string>("sgs","shoc");
  }

  void timeStep( pam::PamCoupler &coupler ) {                                   // SGS.h:150-779
    // everything is checked before the first launch: a refused call leaves every field untouched
    if (!shoc_main)
      endrun("ERROR: SHOC: no shoc_main is registered; call set_shoc_main(fn, user) before timeStep (SHOC itself is not part of this library)");
    real dt = coupler.get_option<real>("crm_dt");
    // the pressure is compute_pressure_array's (SGS.h:265): the coupler's options R_d, R_v, which the microphysics sets
    real pres_R_d = coupler.get_option<real>("R_d"), pres_R_v = coupler.get_option<real>("R_v");
    int nz   = coupler.get_nz();
    int ny   = coupler.get_ny();
    int nx   = coupler.get_nx();
    int nens = coupler.get_nens();
    if (first_step) {
      // This check is here instead of init because it's not guaranteed the micro has called init before sgs
      if (! coupler.option_exists("micro")) {
        endrun("ERROR: SHOC requires coupler.set_option<std::string>(\"micro\",...) to be set");
      }
      std::string micro_scheme = coupler.get_option<std::string>("micro");
      if      (micro_scheme == "kessler") { micro_kessler = true; }
      else if (micro_scheme == "p3"     ) { micro_p3      = true; }
      else { endrun("ERROR: SHOC only meant to run with kessler or p3 microphysics"); }
    }
    auto &dm = coupler.get_data_manager_device_readwrite();
    // the cloud liquid tracer and the extra tracers SHOC diffuses, in the reference's order (SGS.h:238-250)
    char const *cloud = micro_kessler ? "cloud_liquid" : "cloud_water";
    char const *kessler_q[1] = {"precip_liquid"};
    char const *p3_q[7] = {"cloud_water_num", "rain", "rain_num", "ice", "ice_num", "ice_rime", "ice_rime_vol"};
    int num_qtracers = micro_kessler ? 1 : 7;
    char const *const *names = micro_kessler ? kessler_q : p3_q;
    real *q[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int tr = 0; tr < num_qtracers; tr++) q[tr] = dm.get<real,4>(names[tr]).data();
    real *rho_v = dm.get<real,4>("water_vapor").data(), *rho_c = dm.get<real,4>(cloud).data();
    real *uvel = dm.get<real,4>("uvel").data(), *vvel = dm.get<real,4>("vvel").data(), *temp = dm.get<real,4>("temp").data();
    real *tke = dm.get<real,4>("tke").data(), *wthv_sec = dm.get<real,4>("wthv_sec").data(), *tk = dm.get<real,4>("tk").data();
    real *tkh = dm.get<real,4>("tkh").data(), *cldfrac = dm.get<real,4>("cldfrac").data();
    real *inv_qc_relvar = dm.get<real,4>("inv_qc_relvar").data();
    real const *rho_d = dm.get<real const,4>("density_dry").data(), *wvel = dm.get<real const,4>("wvel").data();
    real const *flx_u = dm.get<real const,3>("sfc_mom_flx_u").data(), *flx_v = dm.get<real const,3>("sfc_mom_flx_v").data();
    real const *zint = dm.get<real const,2>("vertical_interface_height").data();
    real const *zmid = dm.get<real const,2>("vertical_midpoint_height" ).data();

    int key[6] = {nens, nx, ny, nz, num_qtracers, layout};
    bool same = ws != nullptr;
    for (int i = 0; i < 6; i++) same = same && key[i] == ws_key[i];
    if (!same) {
      free_workspace();
      chk(pam_amd_shoc_workspace_create(nens, nx, ny, nz, num_qtracers, layout, &ws));
      for (int i = 0; i < 6; i++) ws_key[i] = key[i];
    }
    // crm_dx, crm_dy (crm_dy = crm_dx when ny == 1, SGS.h:168-169) are formed from xlen, ylen inside
    chk(pam_amd_shoc_pack(ws, rho_d, rho_v, rho_c, uvel, vvel, wvel, temp, tke, q, wthv_sec, tk, tkh, cldfrac, flx_u, flx_v, zint, zmid,
                          coupler.get_xlen(), coupler.get_ylen(), pres_R_d, pres_R_v, R_d, cp_d, p0, grav, latvap, nullptr));
    pam_amd_shoc_args_t args;
    chk(pam_amd_shoc_workspace_args(ws, &args));
    args.dt = dt;
    args.nadv = 1;
    args.stream = nullptr;
    int rc = shoc_main(&args, shoc_user);
    if (rc) endrun("ERROR: SHOC: shoc_main returned " + std::to_string(rc));
    chk(pam_amd_shoc_unpack(ws, rho_d, rho_v, rho_c, uvel, vvel, temp, tke, q, wthv_sec, tk, tkh, cldfrac, inv_qc_relvar, cp_d, cv_d, latvap,
                            nullptr));
    first_step = false;
    etime += dt;
  }

  void finalize(pam::PamCoupler &coupler) {
    free_workspace();
  }

  std::string sgs_name() const {
    return "shoc";
  }
};
