// C entry point around the reference's own physics/sgs/shoc/SGS.h, compiled serially against the YAKL stand-in (oracle/ref/YAKL.h, with
// the reshape<2>({..}) of tests/ref_shoc/YAKL.h), on its non-SHOC_CXX path: shoc_init_fortran does nothing, shoc_main_fortran records
// the arrays it receives and runs the stand-in body of pam_amd/csrc/shoc_device.h on them (layout 0: the Fortran-call layout).
// TEST INFRASTRUCTURE ONLY: tests/golden/make_ref_shoc_golden.py builds it in a temporary directory, calls it to write
// tests/golden/shoc_coupling_ref.npz and keeps nothing compiled.  A failure inside the reference (endrun, yakl_throw) returns -1.
#define YAKL_STANDIN_DEFINE_GLOBALS
#include "YAKL.h"

#include "pam_coupler.h"
#include "MultipleFields.h"   // pam::MultiField: SGS.h uses it without including it
#include "SGS.h"

#include "../../pam_amd/csrc/shoc_device.h"

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace pam {
std::mutex data_manager_mutex;
}

namespace {
double *g_received = nullptr;   // where shoc_main_fortran records its input arrays, in the order below
int g_calls = 0;

void record(double *&at, double const *src, size_t n) {
  std::memcpy(at, src, n * sizeof(double));
  at += n;
}
void put(pam::PamCoupler &c, char const *name, double const *src) {
  auto a = c.get_data_manager_device_readwrite().get_collapsed<real>(name);
  std::memcpy(a.data(), src, a.totElems() * sizeof(double));
}
void take(pam::PamCoupler &c, char const *name, double *dst) {
  auto a = c.get_data_manager_device_readwrite().get_collapsed<real>(name);
  std::memcpy(dst, a.data(), a.totElems() * sizeof(double));
}
}  // namespace

extern "C" void shoc_init_fortran(int &, double &, double &, double &, double &, double &, double &, double &, double &, double *, int &,
                                  int &) {}

// Recorded, each as the reference laid it out: host_dx, host_dy, thv, zt_grid, zi_grid, pres, presi, pdel, wthl_sfc, wqw_sfc, uw_sfc,
// vw_sfc, wtracer_sfc, w_field, inv_exner (the argument named exner), phis, host_dse, tke, thetal, qw, u_wind, v_wind, qtracers, wthv_sec,
// tkh, tk, ql, cldfrac.
extern "C" void shoc_main_fortran(int &shcol, int &nlev, int &nlevi, double &dtime, int &nadv, real *host_dx, double *host_dy, double *thv,
                                  double *zt_grid, double *zi_grid, double *pres, double *presi, double *pdel, double *wthl_sfc,
                                  double *wqw_sfc, double *uw_sfc, double *vw_sfc, double *wtracer_sfc, int &num_qtracers, double *w_field,
                                  double *exner, double *phis, double *host_dse, double *tke, double *thetal, double *qw, double *u_wind,
                                  double *v_wind, double *qtracers, double *wthv_sec, double *tkh, double *tk, double *shoc_ql,
                                  double *shoc_cldfrac, double *pblh, double *shoc_mix, double *isotropy, double *w_sec, double *thl_sec,
                                  double *qw_sec, double *qwthl_sec, double *wthl_sec, double *wqw_sec, double *wtke_sec, double *uw_sec,
                                  double *vw_sec, double *w3, double *wqls_sec, double *brunt, double *shoc_ql2) {
  size_t N = shcol, zn = (size_t)nlev * N, zi = (size_t)nlevi * N, T = num_qtracers;
  double *at = g_received;
  record(at, host_dx, N); record(at, host_dy, N); record(at, thv, zn); record(at, zt_grid, zn); record(at, zi_grid, zi);
  record(at, pres, zn); record(at, presi, zi); record(at, pdel, zn); record(at, wthl_sfc, N); record(at, wqw_sfc, N);
  record(at, uw_sfc, N); record(at, vw_sfc, N); record(at, wtracer_sfc, T * N); record(at, w_field, zn); record(at, exner, zn);
  record(at, phis, N); record(at, host_dse, zn); record(at, tke, zn); record(at, thetal, zn); record(at, qw, zn);
  record(at, u_wind, zn); record(at, v_wind, zn); record(at, qtracers, T * zn); record(at, wthv_sec, zn); record(at, tkh, zn);
  record(at, tk, zn); record(at, shoc_ql, zn); record(at, shoc_cldfrac, zn);
  g_calls++;
  // the stand-in body on these arrays: u_wind and v_wind travel as one (2, lev, col) array; ustar, obklen and exner are no arguments of
  // the Fortran call
  std::vector<double> hwind(2 * zn), ustar(N), obklen(N), unused(zn);
  std::memcpy(hwind.data(), u_wind, zn * sizeof(double));
  std::memcpy(hwind.data() + zn, v_wind, zn * sizeof(double));
  pam_amd_shoc_args_t A;
  A.ncol = shcol; A.nlev = nlev; A.nlevi = nlevi; A.dt = dtime; A.nadv = nadv; A.num_qtracers = num_qtracers; A.layout = 0; A.stream = nullptr;
  A.host_dx = host_dx; A.host_dy = host_dy; A.thv = thv; A.zt_grid = zt_grid; A.zi_grid = zi_grid; A.pres = pres; A.presi = presi;
  A.pdel = pdel; A.wthl_sfc = wthl_sfc; A.wqw_sfc = wqw_sfc; A.uw_sfc = uw_sfc; A.vw_sfc = vw_sfc; A.wtracer_sfc = wtracer_sfc;
  A.w_field = w_field; A.inv_exner = exner; A.phis = phis; A.host_dse = host_dse; A.tke = tke; A.thetal = thetal; A.qw = qw;
  A.hwind = hwind.data(); A.qtracers = qtracers; A.wthv_sec = wthv_sec; A.tk = tk; A.ql = shoc_ql; A.cldfrac = shoc_cldfrac; A.pblh = pblh;
  A.ustar = ustar.data(); A.obklen = obklen.data(); A.mix = shoc_mix; A.isotropy = isotropy; A.w_sec = w_sec; A.thl_sec = thl_sec;
  A.qw_sec = qw_sec; A.qwthl_sec = qwthl_sec; A.wthl_sec = wthl_sec; A.wqw_sec = wqw_sec; A.wtke_sec = wtke_sec; A.uw_sec = uw_sec;
  A.vw_sec = vw_sec; A.w3 = w3; A.wqls_sec = wqls_sec; A.brunt = brunt; A.ql2 = shoc_ql2; A.tkh = tkh; A.exner = unused.data();
  for (long long col = 0; col < shcol; col++) pama::shoc::standin_column<long long>(A, col);
  std::memcpy(u_wind, hwind.data(), zn * sizeof(double));
  std::memcpy(v_wind, hwind.data() + zn, zn * sizeof(double));
}

extern "C" {

// One SGS::init + SGS::timeStep of the reference.  p3 = 0: option micro = kessler (tracers water_vapor, cloud_liquid, precip_liquid),
// 1: p3 (water_vapor, cloud_water and the seven of SGS.h:243-249).  names / arrays: num entries of the coupler to fill before the step
// and to read back after it ((nz,ny,nx,nens), the surface fluxes (ny,nx,nens)); zint (nz+1,nens); inv_qc_relvar: out; received: what
// shoc_main_fortran was given (see above); info[4]: get_num_tracers(), tke positive, tke adds_mass, calls of shoc_main_fortran;
// consts[16]: the constructor's R_d, cp_d, cv_d, gamma_d, kappa_d, R_v, cp_v, cv_v, p0, grav, cp_l, latvap, latice, karman, npbl, etime
// after the step; sgs_option[16]: option "sgs".  R_d, R_v: the coupler's options of those names.
int ref_shoc_time_step(int nens, int nx, int ny, int nz, int p3, double xlen, double ylen, double crm_dt, double R_d, double R_v, double const *zint,
                       int num,
                       char const *const *names, double *const *arrays, double *inv_qc_relvar, double *received, int *info, double *consts,
                       char *sgs_option) {
  try {
    pam::PamCoupler c;
    c.allocate_coupler_state(nz, ny, nx, nens);
    c.set_option<real>("crm_dt", crm_dt);
    c.set_option<real>("R_d", R_d);   // what a microphysics sets; compute_pressure_array reads them
    c.set_option<real>("R_v", R_v);
    real2d z("zint", nz + 1, nens);
    std::memcpy(z.data(), zint, (size_t)(nz + 1) * nens * sizeof(double));
    c.set_grid(xlen, ylen, realConst2d(z));
    c.add_tracer("water_vapor", "", true, true);
    if (p3) {
      char const *t[8] = {"cloud_water", "cloud_water_num", "rain", "rain_num", "ice", "ice_num", "ice_rime", "ice_rime_vol"};
      for (auto n : t) c.add_tracer(n, "", true, true);
      c.set_option<std::string>("micro", "p3");
    } else {
      c.add_tracer("cloud_liquid", "", true, true);
      c.add_tracer("precip_liquid", "", true, true);
      c.set_option<std::string>("micro", "kessler");
    }
    SGS sgs;
    double k0[16] = {sgs.R_d, sgs.cp_d, sgs.cv_d, sgs.gamma_d, sgs.kappa_d, sgs.R_v, sgs.cp_v, sgs.cv_v, sgs.p0, sgs.grav, sgs.cp_l, sgs.latvap,
                     sgs.latice, sgs.karman, (double)sgs.npbl, 0.0};
    sgs.init(c);
    for (int i = 0; i < num; i++) put(c, names[i], arrays[i]);
    g_received = received;
    g_calls = 0;
    sgs.timeStep(c);
    for (int i = 0; i < num; i++) take(c, names[i], arrays[i]);
    take(c, "inv_qc_relvar", inv_qc_relvar);
    std::string desc;
    bool found = false, positive = false, adds_mass = true;
    c.get_tracer_info("tke", desc, found, positive, adds_mass);
    if (!found) return -2;
    info[0] = SGS::get_num_tracers(); info[1] = positive; info[2] = adds_mass; info[3] = g_calls;
    k0[15] = sgs.etime;
    std::memcpy(consts, k0, sizeof(k0));
    std::strncpy(sgs_option, c.get_option<std::string>("sgs").c_str(), 15);
    sgs_option[15] = 0;
    if (sgs.sgs_name() != std::string(sgs_option)) return -3;
    sgs.finalize(c);
    return 0;
  } catch (std::exception const &e) {
    std::fprintf(stderr, "ref_shoc_time_step: %s\n", e.what());
    return -1;
  } catch (...) {
    return -1;
  }
}

}  // extern "C"
