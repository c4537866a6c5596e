// C entry points around the reference's own headers, compiled serially against the YAKL stand-in (oracle/ref/YAKL.h).
// TEST INFRASTRUCTURE ONLY: built by `make -C oracle` into oracle/_ref/libpam_ref.so when the reference tree is present,
// loaded by oracle/pam_ref.py.
//
// Each entry point builds a reference pam::PamCoupler (with its DataManager), registers the tracers in the caller's order,
// copies the caller's arrays in, calls the reference by name, and copies the arrays out.  Arrays use the coupler's layout:
// (nz,ny,nx,nens) with nens fastest, tracers (nt,nz,ny,nx,nens).  A failure inside the reference (endrun, yakl_throw)
// returns an error status instead of ending the process.
#define YAKL_STANDIN_DEFINE_GLOBALS
#include "YAKL.h"

#include "pam_coupler.h"
#include "Dycore.h"
#include "Microphysics.h"
#include "sponge_layer.h"
#include "gcm_forcing.h"
#include "broadcast_initial_gcm_column.h"
#include "saturation_adjustment.h"
#include "surface_friction.h"
#include "supercell_init.h"

#include <cstring>
#include <sstream>
#include <string>
#include <vector>

namespace pam {
std::mutex data_manager_mutex;
}

namespace {

struct RefDycore {
  pam::PamCoupler coupler;
  Dycore dycore;
  std::vector<std::string> names;
};

// one (nz,ny,nx,nens) field in or out of the coupler
void copy_in(pam::PamCoupler &c, char const *name, double const *src) {
  auto a = c.get_data_manager_device_readwrite().get<real, 4>(name);
  std::memcpy(a.data(), src, a.totElems() * sizeof(double));
}
void copy_out(pam::PamCoupler &c, char const *name, double *dst) {
  auto a = c.get_data_manager_device_readonly().get<real const, 4>(name);
  std::memcpy(dst, a.data(), a.totElems() * sizeof(double));
}

size_t cells(pam::PamCoupler const &c) { return size_t(c.get_nz()) * c.get_ny() * c.get_nx() * c.get_nens(); }

void fields_in(RefDycore &r, double const *rho_d, double const *u, double const *v, double const *w, double const *T,
               double const *tracers) {
  copy_in(r.coupler, "density_dry", rho_d);
  copy_in(r.coupler, "uvel", u);
  copy_in(r.coupler, "vvel", v);
  copy_in(r.coupler, "wvel", w);
  copy_in(r.coupler, "temp", T);
  size_t n = cells(r.coupler);
  for (size_t t = 0; t < r.names.size(); t++) copy_in(r.coupler, r.names[t].c_str(), tracers + t * n);
}

void fields_out(RefDycore &r, double *rho_d, double *u, double *v, double *w, double *T, double *tracers) {
  copy_out(r.coupler, "density_dry", rho_d);
  copy_out(r.coupler, "uvel", u);
  copy_out(r.coupler, "vvel", v);
  copy_out(r.coupler, "wvel", w);
  copy_out(r.coupler, "temp", T);
  size_t n = cells(r.coupler);
  for (size_t t = 0; t < r.names.size(); t++) copy_out(r.coupler, r.names[t].c_str(), tracers + t * n);
}

// std::cout sent nowhere for the lifetime of the object
struct QuietStdout {
  std::ostringstream sink;
  std::streambuf *old;
  QuietStdout() : old(std::cout.rdbuf(sink.rdbuf())) {}
  ~QuietStdout() { std::cout.rdbuf(old); }
};

std::vector<std::string> split_names(char const *names, int nt) {
  std::vector<std::string> out;
  std::string s(names ? names : "");
  size_t p = 0;
  while (int(out.size()) < nt) {
    size_t q = s.find('\n', p);
    out.push_back(s.substr(p, q == std::string::npos ? std::string::npos : q - p));
    if (q == std::string::npos) break;
    p = q + 1;
  }
  return out;
}

}  // namespace

extern "C" {

// ---- stand-in switches ----------------------------------------------------------------------------------------------
void pam_ref_set_alloc_fill(int zero) { yakl::set_alloc_fill(zero ? yakl::ALLOC_FILL_ZERO : yakl::ALLOC_FILL_NAN); }
void pam_ref_set_replay_label(char const *label) { yakl::set_replay_label(label); }
long pam_ref_replay_count() { return yakl::replay_count(); }
void pam_ref_reset_replay_count() { yakl::reset_replay_count(); }

// ---- AWFL Dycore ----------------------------------------------------------------------------------------------------
// names: nt tracer names separated by '\n'.  dz: (nz,nens).  consts: R_d, cp_d, R_v, cp_v, p0, grav, or NULL for the
// dycore's own defaults.  Dycore::init runs with EXTERNAL data (no standalone input file).
void *pam_ref_dycore_create(int nens, int nx, int ny, int nz, int nt, double xlen, double ylen, double const *dz,
                            char const *names, unsigned char const *positive, unsigned char const *adds_mass,
                            double const *consts) {
  RefDycore *r = nullptr;
  try {
    r = new RefDycore();
    r->names = split_names(names, nt);
    if (int(r->names.size()) != nt) throw std::string("tracer name count");
    auto &c = r->coupler;
    if (consts) {
      char const *keys[6] = {"R_d", "cp_d", "R_v", "cp_v", "p0", "grav"};
      for (int i = 0; i < 6; i++) c.set_option<real>(keys[i], consts[i]);
    }
    c.allocate_coupler_state(nz, ny, nx, nens);
    // the interface heights only feed vertical_cell_dz, which is then set to the caller's dz exactly
    real2d zint("zint", nz + 1, nens);
    for (int e = 0; e < nens; e++) {
      zint(0, e) = 0;
      for (int k = 0; k < nz; k++) zint(k + 1, e) = zint(k, e) + dz[k * nens + e];
    }
    c.set_grid(xlen, ylen, realConst2d(zint));
    auto dza = c.get_data_manager_device_readwrite().get<real, 2>("vertical_cell_dz");
    std::memcpy(dza.data(), dz, size_t(nz) * nens * sizeof(double));
    for (int t = 0; t < nt; t++) c.add_tracer(r->names[t], "", positive[t] != 0, adds_mass[t] != 0);
    // init's throw-away banded solve (D2) prints its result: kept off the caller's output
    QuietStdout quiet;
    r->dycore.init(c);
    return r;
  } catch (...) {
    delete r;
    return nullptr;
  }
}

void pam_ref_dycore_destroy(void *h) { delete static_cast<RefDycore *>(h); }

void pam_ref_dycore_set_grav_balance(void *h, int flag) {
  static_cast<RefDycore *>(h)->coupler.set_option<bool>("balance_hydrostasis_with_gravity", flag != 0);
}

double pam_ref_dycore_get_option(void *h, char const *key) {
  return static_cast<RefDycore *>(h)->coupler.get_option<real>(key);
}

// gcm: NULL, or gcm_density_dry, gcm_temp, gcm_water_vapor, gcm_cloud_water, gcm_cloud_ice, each (nz,nens)
int pam_ref_dycore_declare_hydrostatic(void *h, double const *rho_d, double const *u, double const *v, double const *w,
                                       double const *T, double const *tracers, double const *const *gcm) {
  auto &r = *static_cast<RefDycore *>(h);
  try {
    fields_in(r, rho_d, u, v, w, T, tracers);
    if (gcm) {
      char const *keys[5] = {"gcm_density_dry", "gcm_temp", "gcm_water_vapor", "gcm_cloud_water", "gcm_cloud_ice"};
      for (int i = 0; i < 5; i++) {
        auto a = r.coupler.get_data_manager_device_readwrite().get<real, 2>(keys[i]);
        std::memcpy(a.data(), gcm[i], a.totElems() * sizeof(double));
      }
    }
    r.dycore.declare_current_profile_as_hydrostatic(r.coupler, gcm != nullptr);
    return 0;
  } catch (...) {
    return -1;
  }
}

double pam_ref_dycore_compute_time_step(void *h, double const *rho_d, double const *u, double const *v, double const *w,
                                        double const *T, double const *tracers, double cfl) {
  auto &r = *static_cast<RefDycore *>(h);
  try {
    fields_in(r, rho_d, u, v, w, T, tracers);
    return r.dycore.compute_time_step(r.coupler, cfl);
  } catch (...) {
    return -1.0;
  }
}

// One Dycore::timeStep of crm_dt; fields updated in place.  Returns the sub-cycle count (-1 on failure) and the
// sub-cycle length in *dt_dyn, both from the reference's own compute_time_step.
int pam_ref_dycore_time_step(void *h, double *rho_d, double *u, double *v, double *w, double *T, double *tracers,
                             double crm_dt, double *dt_dyn) {
  auto &r = *static_cast<RefDycore *>(h);
  try {
    r.coupler.set_option<real>("crm_dt", crm_dt);
    fields_in(r, rho_d, u, v, w, T, tracers);
    real dt = r.dycore.compute_time_step(r.coupler);
    int ncycles = (int)std::ceil(crm_dt / dt);
    r.dycore.timeStep(r.coupler);
    fields_out(r, rho_d, u, v, w, T, tracers);
    if (dt_dyn) *dt_dyn = crm_dt / ncycles;
    return ncycles;
  } catch (...) {
    return -1;
  }
}

// Copy a real-valued DataManager entry (variable_gravity, hy_dens_cells, hy_pressure_cells, vert_sten_to_coefs,
// vert_weno_recon_lower, ...) into out[n].  Returns the entry's element count, or -1 if it is absent or n is too small.
long pam_ref_dycore_read(void *h, char const *name, double *out, long n) {
  auto &r = *static_cast<RefDycore *>(h);
  try {
    auto a = r.coupler.get_data_manager_device_readonly().get_collapsed<real const>(name);
    long m = long(a.totElems());
    if (m > n) return -1;
    std::memcpy(out, a.data(), size_t(m) * sizeof(double));
    return m;
  } catch (...) {
    return -1;
  }
}

// ---- coupler modules --------------------------------------------------------------------------------------------
// A reference PamCoupler of (nz,ny,nx,nens) with the grid zint (nz+1,nens) and the tracers in the caller's order; its
// DataManager entries are written and read by name, and a module of the reference is run on it by name.
struct RefCoupler {
  pam::PamCoupler coupler;
  Microphysics kessler;
};

void *pam_ref_coupler_create(int nens, int nx, int ny, int nz, int nt, double xlen, double ylen, double const *zint,
                             char const *names, unsigned char const *positive, unsigned char const *adds_mass) {
  RefCoupler *r = nullptr;
  try {
    r = new RefCoupler();
    auto &c = r->coupler;
    c.allocate_coupler_state(nz, ny, nx, nens);
    real2d zi("zint", nz + 1, nens);
    std::memcpy(zi.data(), zint, size_t(nz + 1) * nens * sizeof(double));
    c.set_grid(xlen, ylen, realConst2d(zi));
    auto nm = split_names(names, nt);
    if (int(nm.size()) != nt) throw std::string("tracer name count");
    for (int t = 0; t < nt; t++) c.add_tracer(nm[t], "", positive[t] != 0, adds_mass[t] != 0);
    return r;
  } catch (...) {
    delete r;
    return nullptr;
  }
}

void pam_ref_coupler_destroy(void *h) { delete static_cast<RefCoupler *>(h); }

void pam_ref_coupler_set_real(void *h, char const *key, double v) { static_cast<RefCoupler *>(h)->coupler.set_option<real>(key, v); }
void pam_ref_coupler_set_int(void *h, char const *key, int v) { static_cast<RefCoupler *>(h)->coupler.set_option<int>(key, v); }
void pam_ref_coupler_set_string(void *h, char const *key, char const *v) {
  static_cast<RefCoupler *>(h)->coupler.set_option<std::string>(key, std::string(v));
}

// register a real entry of the given dimensions (fresh memory: filled as the stand-in's allocation fill says)
int pam_ref_coupler_register(void *h, char const *name, int ndims, int const *dims) {
  try {
    std::vector<int> d(dims, dims + ndims);
    static_cast<RefCoupler *>(h)->coupler.get_data_manager_device_readwrite().register_and_allocate<real>(name, "", d);
    return 0;
  } catch (...) {
    return -1;
  }
}

// copy n values into / out of a real entry; returns the entry's element count, -1 if absent or of another size
long pam_ref_coupler_write(void *h, char const *name, double const *src, long n) {
  try {
    auto a = static_cast<RefCoupler *>(h)->coupler.get_data_manager_device_readwrite().get_collapsed<real>(name);
    if (long(a.totElems()) != n) return -1;
    std::memcpy(a.data(), src, size_t(n) * sizeof(double));
    return n;
  } catch (...) {
    return -1;
  }
}

long pam_ref_coupler_read(void *h, char const *name, double *dst, long n) {
  try {
    auto a = static_cast<RefCoupler *>(h)->coupler.get_data_manager_device_readonly().get_collapsed<real const>(name);
    if (long(a.totElems()) != n) return -1;
    std::memcpy(dst, a.data(), size_t(n) * sizeof(double));
    return n;
  } catch (...) {
    return -1;
  }
}

// Run one module of the reference on the coupler.  a, b: the per-member inputs of surface_friction_init (tau, bflx).
// kessler_init registers the Kessler tracers itself (call it on a coupler created without tracers).
int pam_ref_coupler_run(void *h, char const *module, double const *a, double const *b) {
  auto &r = *static_cast<RefCoupler *>(h);
  auto &c = r.coupler;
  std::string m(module);
  try {
    if (m == "sponge_layer") modules::sponge_layer(c);
    else if (m == "compute_gcm_forcing_tendencies") modules::compute_gcm_forcing_tendencies(c);
    else if (m == "apply_gcm_forcing_tendencies") modules::apply_gcm_forcing_tendencies(c);
    else if (m == "broadcast_initial_gcm_column") modules::broadcast_initial_gcm_column(c);
    else if (m == "broadcast_initial_gcm_column_dry_density") modules::broadcast_initial_gcm_column_dry_density(c);
    else if (m == "saturation_adjustment") modules::saturation_adjustment(c);
    else if (m == "surface_friction_init") {
      int nens = c.get_nens();
      realConst1d tau("tau", const_cast<double *>(a), nens), bflx("bflx", const_cast<double *>(b), nens);
      modules::surface_friction_init(c, tau, bflx);
    } else if (m == "compute_surface_friction") modules::compute_surface_friction(c);
    else if (m == "kessler_init") r.kessler.init(c);
    else if (m == "kessler_timeStep") r.kessler.timeStep(c);
    else return -2;
    return 0;
  } catch (...) {
    return -1;
  }
}

// the standalone driver's supercell column: zint (nz+1) -> rho_d, u, v, w, T, rho_v (nz each)
int pam_ref_supercell_init(int nz, double const *zint, double R_d, double R_v, double grav, double *rho_d, double *u, double *v,
                           double *w, double *T, double *rho_v) {
  try {
    realConst1d zi("zint", const_cast<double *>(zint), nz + 1);
    real1d cols[6] = {real1d("rho_d", rho_d, nz), real1d("u", u, nz), real1d("v", v, nz), real1d("w", w, nz), real1d("T", T, nz),
                      real1d("rho_v", rho_v, nz)};
    supercell_init(zi, cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], R_d, R_v, grav);
    return 0;
  } catch (...) {
    return -1;
  }
}

}  // extern "C"
