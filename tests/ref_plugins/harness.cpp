// C entry points around the reference's own physics/radiation/forced/radiation.h, physics/micro/none/Microphysics.h and
// PamCoupler::compute_pressure_array, compiled serially against the YAKL stand-in (oracle/ref/YAKL.h).  TEST INFRASTRUCTURE ONLY:
// tests/golden/make_ref_plugins_golden.py builds it in a temporary directory, calls it to write tests/golden/plugins_ref.npz and
// keeps nothing compiled.  Arrays use the coupler's layout, (nz,ny,nx,nens) with nens fastest.  Fresh allocations of the stand-in
// are filled with NaN bit patterns, so an element the reference never wrote shows.  A failure inside the reference (endrun,
// yakl_throw) returns -1.
#define YAKL_STANDIN_DEFINE_GLOBALS
#include "YAKL.h"

#include "pam_coupler.h"
#include "radiation.h"
#include "Microphysics.h"

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace pam {
std::mutex data_manager_mutex;
}

namespace {
void put(pam::PamCoupler &c, char const *name, double const *src) {
  auto a = c.get_data_manager_device_readwrite().get<real, 4>(name);
  std::memcpy(a.data(), src, a.totElems() * sizeof(double));
}
}  // namespace

extern "C" {

// Radiation::init + `calls` x Radiation::timeStep on a coupler whose size options are set as a GCM host would set them
int ref_radiation_forced(int nens, int nx, int ny, int nz, int rad_nx, int rad_ny, double *temp, double const *tend, double cp_d,
                         double crm_dt, int calls) {
  try {
    pam::PamCoupler c;
    c.allocate_coupler_state(nz, ny, nx, nens);
    c.set_option<int>("ncrms", nens);
    c.set_option<int>("crm_nz", nz);
    c.set_option<int>("crm_nx", nx);
    c.set_option<int>("crm_ny", ny);
    c.set_option<int>("rad_nx", rad_nx);
    c.set_option<int>("rad_ny", rad_ny);
    c.set_option<real>("crm_dt", crm_dt);
    c.set_option<real>("cp_d", cp_d);
    Radiation rad;
    rad.init(c);
    if (c.get_option<std::string>("radiation") != rad.radiation_name()) return -2;
    put(c, "temp", temp);
    put(c, "rad_enthalpy_tend", tend);
    for (int n = 0; n < calls; n++) rad.timeStep(c);
    auto t = c.get_data_manager_device_readonly().get<real const, 4>("temp");
    std::memcpy(temp, t.data(), t.totElems() * sizeof(double));
    rad.finalize(c);
    return 0;
  } catch (...) {
    return -1;
  }
}

int ref_compute_pressure(int nens, int nx, int ny, int nz, double const *rho_d, double const *rho_v, double const *temp, double R_d,
                         double R_v, double *pressure) {
  try {
    pam::PamCoupler c;
    c.allocate_coupler_state(nz, ny, nx, nens);
    c.add_tracer("water_vapor", "", true, true);
    c.set_option<real>("R_d", R_d);
    c.set_option<real>("R_v", R_v);
    put(c, "density_dry", rho_d);
    put(c, "water_vapor", rho_v);
    put(c, "temp", temp);
    auto p = c.compute_pressure_array();
    std::memcpy(pressure, p.data(), p.totElems() * sizeof(double));
    return 0;
  } catch (...) {
    return -1;
  }
}

// Microphysics::init of "none": consts[6] = options R_d, R_v, cp_d, cp_v, grav, p0; water_vapor = the tracer after init;
// info[4] = get_num_tracers(), coupler.get_num_tracers(), positive, adds_mass; name[16] = option "micro"
int ref_micro_none_init(int nens, int nx, int ny, int nz, double *consts, double *water_vapor, int *info, char *name) {
  try {
    pam::PamCoupler c;
    c.allocate_coupler_state(nz, ny, nx, nens);
    Microphysics micro;
    micro.init(c);
    char const *keys[6] = {"R_d", "R_v", "cp_d", "cp_v", "grav", "p0"};
    for (int i = 0; i < 6; i++) consts[i] = c.get_option<real>(keys[i]);
    auto v = c.get_data_manager_device_readonly().get<real const, 4>("water_vapor");
    std::memcpy(water_vapor, v.data(), v.totElems() * sizeof(double));
    std::string desc;
    bool found = false, positive = false, adds_mass = false;
    c.get_tracer_info("water_vapor", desc, found, positive, adds_mass);
    if (!found) return -2;
    info[0] = Microphysics::get_num_tracers();
    info[1] = c.get_num_tracers();
    info[2] = positive;
    info[3] = adds_mass;
    std::strncpy(name, c.get_option<std::string>("micro").c_str(), 15);
    name[15] = 0;
    if (micro.micro_name() != std::string(name)) return -3;
    return 0;
  } catch (...) {
    return -1;
  }
}

}  // extern "C"
