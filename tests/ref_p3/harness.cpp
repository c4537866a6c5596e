// C entry point around the reference's own physics/micro/p3/Microphysics.h, compiled serially against the YAKL stand-in (oracle/ref/YAKL.h)
// on its non-P3_CXX path: micro_p3_utils_init_fortran and p3_init_fortran do nothing, p3_main_fortran records the arrays and scalars it
// receives and runs the stand-in body of pam_amd/csrc/p3_device.h on them (layout 0: the Fortran-call layout).
// TEST INFRASTRUCTURE ONLY: tests/golden/make_ref_p3_golden.py builds it in a temporary directory, calls it to write
// tests/golden/p3_coupling_ref.npz and keeps nothing compiled.  A failure inside the reference (endrun, yakl_throw) returns -1.
// The reference's bisection ends on an unqualified `abs(cond2-cond1) <= tol` (:807, :844).  Its own builds see abs(double) there (the
// device headers declare it globally); a host translation unit that only has <cstdlib>'s ::abs(int) would truncate the bracket to 0 and
// stop after one iteration.  <stdlib.h> of the C++ library brings std::abs's overloads into the global namespace, as those builds have them.
#include <stdlib.h>
#include <cmath>
#define YAKL_STANDIN_DEFINE_GLOBALS
#include "YAKL.h"

#include "pam_coupler.h"
#include "Microphysics.h"

#include "../../pam_amd/csrc/p3_device.h"

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace pam {
std::mutex data_manager_mutex;
}

namespace {
double *g_received = nullptr;   // where p3_main_fortran records its input arrays, in the order below
double *g_scalars = nullptr;    // dt, it, its, ite, kts, kte, do_predict_nc, do_prescribed_CCN per call
int g_calls = 0;

void record(double *&at, double const *src, size_t n) {
  std::memcpy(at, src, n * sizeof(double));
  at += n;
}
void put(pam::PamCoupler &c, char const *name, double const *src) {
  auto a = c.get_data_manager_device_readwrite().get_collapsed<real>(name);
  std::memcpy(a.data(), src, a.totElems() * sizeof(double));
}
size_t take(pam::PamCoupler &c, char const *name, double *dst) {
  auto a = c.get_data_manager_device_readwrite().get_collapsed<real>(name);
  std::memcpy(dst, a.data(), a.totElems() * sizeof(double));
  return a.totElems();
}
}  // namespace

extern "C" void micro_p3_utils_init_fortran(real &, real &, real &, real &, real &, real &, real &, real &, real &, real &, real &, real &, int &,
                                            bool &) {}
extern "C" void p3_init_fortran(char const *, int &, char const *, int &) {}

// Recorded per call, each as the reference laid it out ((lev, col); col_location (3, col)): qc nc qr nr th_atm qv qi qm ni bm pres dz
// nc_nuceat_tend nccn_prescribed ni_activated inv_qc_relvar dpres inv_exner (the argument named exner) cld_frac_r cld_frac_l cld_frac_i
// q_prev t_prev col_location.
extern "C" void p3_main_fortran(double *qc, double *nc, double *qr, double *nr, double *th_atm, double *qv, double &dt, double *qi, double *qm,
                                double *ni, double *bm, double *pres, double *dz, double *nc_nuceat_tend, double *nccn_prescribed,
                                double *ni_activated, double *inv_qc_relvar, int &it, double *precip_liq_surf, double *precip_ice_surf, int &its,
                                int &ite, int &kts, int &kte, double *diag_eff_radius_qc, double *diag_eff_radius_qi, double *rho_qi,
                                bool &do_predict_nc, bool &do_prescribed_CCN, double *dpres, double *exner, double *qv2qi_depos_tend,
                                double *precip_total_tend, double *nevapr, double *qr_evap_tend, double *precip_liq_flux,
                                double *precip_ice_flux, double *cld_frac_r, double *cld_frac_l, double *cld_frac_i, double *p3_tend_out,
                                double *mu_c, double *lamc, double *liq_ice_exchange, double *vap_liq_exchange, double *vap_ice_exchange,
                                double *q_prev, double *t_prev, double *col_location, double *elapsed_s) {
  int ncol = ite - its + 1, nz = kte - kts + 1;
  size_t N = ncol, zn = (size_t)nz * N;
  double *at = g_received + (size_t)g_calls * (23 * zn + 3 * N);
  double *in[23] = {qc, nc, qr, nr, th_atm, qv, qi, qm, ni, bm, pres, dz, nc_nuceat_tend, nccn_prescribed, ni_activated, inv_qc_relvar, dpres,
                    exner, cld_frac_r, cld_frac_l, cld_frac_i, q_prev, t_prev};
  for (auto p : in) record(at, p, zn);
  record(at, col_location, 3 * N);
  double s[8] = {dt, (double)it, (double)its, (double)ite, (double)kts, (double)kte, (double)do_predict_nc, (double)do_prescribed_CCN};
  std::memcpy(g_scalars + 8 * g_calls, s, sizeof(s));
  g_calls++;
  // the stand-in body on these arrays: diag_eff_radius_qr and the layer's own exner are no arguments of the Fortran call
  std::vector<double> unused_qr(zn), unused_exner(zn);
  pam_amd_p3_args_t A;
  A.ncol = ncol; A.nlev = nz; A.dt = dt; A.it = it; A.its = its; A.ite = ite; A.kts = kts; A.kte = kte; A.do_predict_nc = do_predict_nc;
  A.do_prescribed_CCN = do_prescribed_CCN; A.layout = 0; A.num_tend_out = 49; A.stream = nullptr;
  A.qc = qc; A.nc = nc; A.qr = qr; A.nr = nr; A.th_atm = th_atm; A.qv = qv; A.qi = qi; A.qm = qm; A.ni = ni; A.bm = bm; A.pres = pres; A.dz = dz;
  A.nc_nuceat_tend = nc_nuceat_tend; A.nccn_prescribed = nccn_prescribed; A.ni_activated = ni_activated; A.inv_qc_relvar = inv_qc_relvar;
  A.precip_liq_surf = precip_liq_surf; A.precip_ice_surf = precip_ice_surf; A.diag_eff_radius_qc = diag_eff_radius_qc;
  A.diag_eff_radius_qi = diag_eff_radius_qi; A.diag_eff_radius_qr = unused_qr.data(); A.bulk_qi = rho_qi; A.precip_total_tend = precip_total_tend;
  A.nevapr = nevapr; A.qr_evap_tend = qr_evap_tend; A.dpres = dpres; A.inv_exner = exner; A.qv2qi_depos_tend = qv2qi_depos_tend;
  A.precip_liq_flux = precip_liq_flux; A.precip_ice_flux = precip_ice_flux; A.cld_frac_r = cld_frac_r; A.cld_frac_l = cld_frac_l;
  A.cld_frac_i = cld_frac_i; A.p3_tend_out = p3_tend_out; A.mu_c = mu_c; A.lamc = lamc; A.liq_ice_exchange = liq_ice_exchange;
  A.vap_liq_exchange = vap_liq_exchange; A.vap_ice_exchange = vap_ice_exchange; A.q_prev = q_prev; A.t_prev = t_prev;
  A.col_location = col_location; A.exner = unused_exner.data();
  for (long long col = 0; col < ncol; col++) pama::p3::standin_column<long long>(A, col);
  *elapsed_s = 0;
}

extern "C" {

// Microphysics::init and `nsteps` consecutive Microphysics::timeStep of the reference.  shoc: option sgs = "shoc" (no adjustment) or "none".
// names / arrays: num_in entries of the coupler to fill after init.  out_names: num_out entries read back after every step into `out`
// (step-major, in that order).  received / scalars: what p3_main_fortran was given per call (see above).
// info[20]: get_num_tracers(), calls of p3_main_fortran, then (positive, adds_mass) of the nine tracers in registration order.
// consts[11]: the constructor's R_d, cp_d, cv_d, gamma_d, kappa_d, R_v, cp_v, cv_v, p0, grav, cp_l; options[8]: latvap, latice, R_d, R_v,
// cp_d, cp_v, grav, p0 as init set them; etime[nsteps]; micro_option[16]: option "micro".
int ref_p3_time_steps(int nens, int nx, int ny, int nz, int shoc, double xlen, double ylen, double crm_dt, double const *zint, int num_in,
                      char const *const *names, double const *const *arrays, int nsteps, int num_out, char const *const *out_names,
                      double *out, double *received, double *scalars, int *info, double *consts, double *options, double *etime,
                      char *micro_option) {
  try {
    pam::PamCoupler c;
    c.allocate_coupler_state(nz, ny, nx, nens);
    c.set_option<real>("crm_dt", crm_dt);
    c.set_option<std::string>("sgs", shoc ? "shoc" : "none");
    real2d z("zint", nz + 1, nens);
    std::memcpy(z.data(), zint, (size_t)(nz + 1) * nens * sizeof(double));
    c.set_grid(xlen, ylen, realConst2d(z));
    Microphysics micro;
    double k0[11] = {micro.R_d, micro.cp_d, micro.cv_d, micro.gamma_d, micro.kappa_d, micro.R_v, micro.cp_v, micro.cv_v, micro.p0, micro.grav,
                     micro.cp_l};
    std::memcpy(consts, k0, sizeof(k0));
    micro.init(c);
    char const *opt[8] = {"latvap", "latice", "R_d", "R_v", "cp_d", "cp_v", "grav", "p0"};
    for (int i = 0; i < 8; i++) options[i] = c.get_option<real>(opt[i]);
    std::strncpy(micro_option, c.get_option<std::string>("micro").c_str(), 15);
    micro_option[15] = 0;
    if (micro.micro_name() != std::string(micro_option)) return -3;
    char const *tr[9] = {"cloud_water", "cloud_water_num", "rain", "rain_num", "ice", "ice_num", "ice_rime", "ice_rime_vol", "water_vapor"};
    auto tracer_names = c.get_tracer_names();
    if (tracer_names.size() != 9) return -4;
    for (int i = 0; i < 9; i++) {
      if (tracer_names[i] != tr[i]) return -4;
      std::string desc;
      bool found = false, positive = false, adds_mass = false;
      c.get_tracer_info(tr[i], desc, found, positive, adds_mass);
      if (!found) return -2;
      info[2 + 2 * i] = positive;
      info[3 + 2 * i] = adds_mass;
    }
    for (int i = 0; i < num_in; i++) put(c, names[i], arrays[i]);
    g_received = received;
    g_scalars = scalars;
    g_calls = 0;
    double *at = out;
    for (int s = 0; s < nsteps; s++) {
      micro.timeStep(c);
      for (int i = 0; i < num_out; i++) at += take(c, out_names[i], at);
      etime[s] = micro.etime;
    }
    info[0] = Microphysics::get_num_tracers();
    info[1] = g_calls;
    micro.finalize(c);
    return 0;
  } catch (std::exception const &e) {
    std::fprintf(stderr, "ref_p3_time_steps: %s\n", e.what());
    return -1;
  } catch (...) {
    return -1;
  }
}

}  // extern "C"
