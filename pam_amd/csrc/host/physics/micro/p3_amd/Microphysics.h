// physics/micro/p3_amd/Microphysics.h -- the C++ plug-in class PAM's drivers instantiate as `Microphysics` (selected with
// -DPAM_MICRO=p3_amd, physics/micro/CMakeLists.txt), same duck-typed members as the reference's physics/micro/p3/Microphysics.h.  It is the
// COUPLING LAYER of P3: what the reference does around p3_main (Microphysics.h:273-409 and :680-717, the saturation adjustment of
// :769-852 included) runs as two fused launches of libpam_amd_awfl.so (pam_amd_p3_pack / pam_amd_p3_unpack, include/pam_amd_modules.h) on
// one workspace allocated once; P3 itself is SCREAM's code and is handed in:
//
//     Microphysics micro;
//     micro.set_p3_main(my_p3_main, my_state);     // int my_p3_main(const pam_amd_p3_args_t *args, void *user)
//
// my_p3_main receives the arguments of pam::p3_main_cxx / p3_main_fortran under their names as DEVICE pointers, in `layout` 1 = SCREAM's
// C++ layout ((col, lev), level fastest, flipped) or 0 = the Fortran-call layout ((lev, col), column fastest, with `num_tend_out` planes of
// p3_tend_out), works in place and returns 0.  args->stream carries the pack step; the unpack step follows on the same stream.
// The P3 lookup tables and micro_p3_utils_init belong to whoever supplies p3_main: init() calls neither and does not read the option
// p3_lookup_data_path.  Not provided: the PAM_DEBUG mass check and the unused get_cloud_fraction.  The additions to the reference's
// members are set_p3_main, layout and num_tend_out; a timeStep without a p3_main is an error.
#pragma once
#include <array>
#include <string>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

class Microphysics {
  pam_amd_p3_main_fn p3_main = nullptr;
  void *p3_user = nullptr;
  void *ws = nullptr;                // the workspace: one device allocation, made on the first step
  int ws_key[6] = {0, 0, 0, 0, -1, -1};

  static void chk(int rc) { if (rc) endrun(pam_amd_awfl_last_error()); }

  void free_workspace() {
    if (ws) (void)pam_amd_p3_workspace_destroy(ws);
    ws = nullptr;
  }

 public:
  // Microphysics.h:41-58
  real R_d, cp_d, cv_d, gamma_d, kappa_d, R_v, cp_v, cv_v, p0;
  real grav, cp_l;
  bool sgs_shoc;
  bool first_step;
  real etime;
  int layout = 1;                    // of the arrays p3_main receives; set before the first timeStep
  int num_tend_out = -1;             // planes of p3_tend_out; -1: 49 in layout 0 (Microphysics.h:321), 0 in layout 1

  int static constexpr ID_C  = 0;  // Local index for Cloud Water Mass
  int static constexpr ID_NC = 1;  // Local index for Cloud Water Number
  int static constexpr ID_R  = 2;  // Local index for Rain Water Mass
  int static constexpr ID_NR = 3;  // Local index for Rain Water Number
  int static constexpr ID_I  = 4;  // Local index for Ice Mass
  int static constexpr ID_M  = 5;  // Local index for Ice Number
  int static constexpr ID_NI = 6;  // Local index for Ice-Rime Mass
  int static constexpr ID_BM = 7;  // Local index for Ice-Rime Volume
  int static constexpr ID_V  = 8;  // Local index for Water Vapor

  Microphysics() {                   // Microphysics.h:74-88
    R_d        = 287.042;
    cp_d       = 1004.64;
    cv_d       = cp_d - R_d;
    gamma_d    = cp_d / cv_d;
    kappa_d    = R_d  / cp_d;
    R_v        = 461.505;
    cp_v       = 1859;
    cv_v       = R_v - cp_v;
    p0         = 1.e5;
    grav       = 9.80616;
    first_step = true;
    cp_l       = 4188.0;
    sgs_shoc   = false;
    etime      = 0;
  }
  Microphysics(Microphysics const &) = delete;
  ~Microphysics() { free_workspace(); }

  static int constexpr get_num_tracers() {
    return 9;
  }

  static auto constexpr get_diffused_tracers_indices() {
    return std::array{ID_V, ID_C, ID_R, ID_I};
  }

  static auto constexpr get_num_diffused_tracers() {
    return std::size(get_diffused_tracers_indices());
  }

  // P3's entry point and an opaque pointer passed back to it
  void set_p3_main(pam_amd_p3_main_fn fn, void *user = nullptr) {
    p3_main = fn;
    p3_user = user;
  }

  void init(pam::PamCoupler &coupler) {                                         // Microphysics.h:108-210
    int nx   = coupler.get_nx  ();
    int ny   = coupler.get_ny  ();
    int nz   = coupler.get_nz  ();
    int nens = coupler.get_nens();
    //                 name                description            positive   adds mass
    coupler.add_tracer("cloud_water"     , "Cloud Water Mass"   , true     , true );
    coupler.add_tracer("cloud_water_num" , "Cloud Water Number" , true     , false);
    coupler.add_tracer("rain"            , "Rain Water Mass"    , true     , true );
    coupler.add_tracer("rain_num"        , "Rain Water Number"  , true     , false);
    coupler.add_tracer("ice"             , "Ice Mass"           , true     , true );
    coupler.add_tracer("ice_num"         , "Ice Number"         , true     , false);
    coupler.add_tracer("ice_rime"        , "Ice-Rime Mass"      , true     , false);
    coupler.add_tracer("ice_rime_vol"    , "Ice-Rime Volume"    , true     , false);
    coupler.add_tracer("water_vapor"     , "Water Vapor"        , true     , true );
    auto &dm = coupler.get_data_manager_device_readwrite();
    // allocations are zero-filled; the tracers are zeroed below: the reference's "micro zero" kernel
    dm.register_and_allocate<real>( "nccn_prescribed","prescribed cld nuclei concentration  [#/kg]",  {nz,ny,nx,nens},{"z","y","x","nens"});
    dm.register_and_allocate<real>( "nc_nuceat_tend", "activated cld nuclei number tendency [#/kg/s]",{nz,ny,nx,nens},{"z","y","x","nens"});
    dm.register_and_allocate<real>( "ni_activated",   "activated ice nuclei concentration   [#/kg]",  {nz,ny,nx,nens},{"z","y","x","nens"});
    dm.register_and_allocate<real>("q_prev","rho_v from prev step"       ,{nz,ny,nx,nens},{"z","y","x","nens"});
    dm.register_and_allocate<real>("t_prev" ,"Temperature from prev step",{nz,ny,nx,nens},{"z","y","x","nens"});
    dm.register_and_allocate<real>("precip_liq_surf_out","liq surface precipitation rate",{ny,nx,nens},{"y","x","nens"});
    dm.register_and_allocate<real>("precip_ice_surf_out","ice surface precipitation rate",{ny,nx,nens},{"y","x","nens"});
    dm.register_and_allocate<real>("liq_ice_exchange_out","p3 liq to ice phase change tendency",{nz,ny,nx,nens},{"z","y","x","nens"});
    dm.register_and_allocate<real>("vap_liq_exchange_out","p3 vap to liq phase change tendency",{nz,ny,nx,nens},{"z","y","x","nens"});
    dm.register_and_allocate<real>("vap_ice_exchange_out","p3 vap to ice phase change tendency",{nz,ny,nx,nens},{"z","y","x","nens"});
    size_t n4 = (size_t)nz * ny * nx * nens * sizeof(real);
    char const *zeroed[9] = {"cloud_water", "cloud_water_num", "rain", "rain_num", "ice", "ice_num", "ice_rime", "ice_rime_vol", "water_vapor"};
    for (auto name : zeroed)
      if (hipMemset(dm.get<real,4>(name).data(), 0, n4) != hipSuccess) endrun("ERROR: P3: cannot zero the tracers");
    real latvap = 2501000.0;
    real latice = 333700.0;
    coupler.set_option<std::string>("micro","p3");
    coupler.set_option<real>("latvap",latvap);
    coupler.set_option<real>("latice",latice);
    coupler.set_option<real>("R_d" ,R_d  );
    coupler.set_option<real>("R_v" ,R_v  );
    coupler.set_option<real>("cp_d",cp_d );
    coupler.set_option<real>("cp_v",cp_v );
    coupler.set_option<real>("grav",grav );
    coupler.set_option<real>("p0"  ,p0   );
    etime = 0;
  }

  void timeStep( pam::PamCoupler &coupler ) {                                   // Microphysics.h:214-741
    // everything is checked before the first launch: a refused call leaves every field untouched
    if (!p3_main)
      endrun("ERROR: P3: no p3_main is registered; call set_p3_main(fn, user) before timeStep (P3 itself is not part of this library)");
    real dt = coupler.get_option<real>("crm_dt");
    bool shoc = sgs_shoc;
    if (first_step) {
      if (coupler.get_option<std::string>("sgs") == "shoc") shoc = true;
    }
    int nz   = coupler.get_nz  ();
    int ny   = coupler.get_ny  ();
    int nx   = coupler.get_nx  ();
    int nens = coupler.get_nens();
    int nout = num_tend_out >= 0 ? num_tend_out : (layout == 0 ? 49 : 0);
    auto &dm = coupler.get_data_manager_device_readwrite();
    char const *names[7] = {"cloud_water_num", "rain", "rain_num", "ice", "ice_num", "ice_rime", "ice_rime_vol"};
    real *q[7];
    for (int tr = 0; tr < 7; tr++) q[tr] = dm.get<real,4>(names[tr]).data();
    real *rho_v = dm.get<real,4>("water_vapor").data(), *rho_c = dm.get<real,4>("cloud_water").data();
    real *temp = dm.get<real,4>("temp").data(), *q_prev = dm.get<real,4>("q_prev").data(), *t_prev = dm.get<real,4>("t_prev").data();
    real *liq_ice = dm.get<real,4>("liq_ice_exchange_out").data(), *vap_liq = dm.get<real,4>("vap_liq_exchange_out").data();
    real *vap_ice = dm.get<real,4>("vap_ice_exchange_out").data();
    real *p_liq = dm.get<real,3>("precip_liq_surf_out").data(), *p_ice = dm.get<real,3>("precip_ice_surf_out").data();
    real const *rho_d = dm.get<real const,4>("density_dry").data();
    real const *nccn = dm.get<real const,4>("nccn_prescribed").data(), *nuceat = dm.get<real const,4>("nc_nuceat_tend").data();
    real const *ni_act = dm.get<real const,4>("ni_activated").data();
    real const *zint = dm.get<real const,2>("vertical_interface_height").data();

    int key[6] = {nens, nx, ny, nz, layout, nout};
    bool same = ws != nullptr;
    for (int i = 0; i < 6; i++) same = same && key[i] == ws_key[i];
    if (!same) {
      free_workspace();
      chk(pam_amd_p3_workspace_create(nens, nx, ny, nz, layout, nout, &ws));
      for (int i = 0; i < 6; i++) ws_key[i] = key[i];
    }
    sgs_shoc = shoc;
    chk(pam_amd_p3_pack(ws, rho_d, rho_v, rho_c, temp, q, nccn, nuceat, ni_act, q_prev, t_prev, zint, sgs_shoc ? 0 : 1, first_step ? 1 : 0,
                        R_d, R_v, cp_d, cp_v, cp_l, p0, grav, nullptr));
    pam_amd_p3_args_t args;
    chk(pam_amd_p3_workspace_args(ws, &args));
    args.dt = dt;
    args.stream = nullptr;
    int rc = p3_main(&args, p3_user);
    if (rc) endrun("ERROR: P3: p3_main returned " + std::to_string(rc));
    chk(pam_amd_p3_unpack(ws, rho_d, rho_v, rho_c, q, temp, q_prev, t_prev, liq_ice, vap_liq, vap_ice, p_liq, p_ice, cp_d, cv_d, nullptr));
    first_step = false;
    etime += dt;
  }

  void finalize(pam::PamCoupler &coupler) {
    free_workspace();
  }

  std::string micro_name() const {
    return "p3";
  }
};
