// column_diag.cpp -- the C++ module modules/column_diagnostics.h driven from a file.  TEST INFRASTRUCTURE ONLY: tests/test_coldiag.py builds
// it with hipcc the way the examples' driver is built, tests/test_coldiag_gpu.py runs it.
//   column_diag IN OUT
// IN: six int32 (nz, ny, nx, nens, micro: 0 none | 1 kessler | 2 p3, steps), then float64 arrays: zint (nz+1,nens), then per step its weight
// (one value) and temp, density_dry, water_vapor, the cloud tracer, the ice tracer (nz,ny,nx,nens; those the microphysics has) and the
// liquid and the ice precipitation (ny,nx,nens; kessler: precl alone, p3: both, none: neither).  column_diagnostics_init runs twice, the
// second time after the entries were filled with 7: a GCM step starts from zero.  OUT: the nine diag_ entries (nens), those that exist, in
// the order of the C ABI.  stdout: "### entries" and their names.  A thrown message goes to stdout.
#include <cstdio>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "modules/column_diagnostics.h"

static void copy_in(real *dst, std::vector<double> const &src) {
  if (hipMemcpy(dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) endrun("copy failed");
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int h[6];
  if (std::fread(h, sizeof(int), 6, in) != 6) return 3;
  int nz = h[0], ny = h[1], nx = h[2], nens = h[3], micro = h[4], steps = h[5];
  size_t n4 = (size_t)nz * ny * nx * nens, n3 = (size_t)ny * nx * nens;
  auto take = [&](size_t n) { std::vector<double> v(n); if (std::fread(v.data(), sizeof(double), n, in) != n) endrun("short input"); return v; };
  int status = 0;
  try {
    pam::PamCoupler coupler;
    coupler.set_option<real>("crm_dt", 20.0);
    coupler.set_option<real>("gcm_physics_dt", 240.0);
    coupler.set_option<real>("R_d", 287.042);      // what a microphysics sets
    coupler.set_option<real>("R_v", 461.505);
    coupler.allocate_coupler_state(nz, ny, nx, nens);
    coupler.set_grid(16000.0, 12000.0, std::vector<real>(nz + 1, 0.0));
    std::vector<std::string> tracers = micro == 2 ? std::vector<std::string>{"water_vapor", "cloud_water", "ice"}
                                     : micro == 1 ? std::vector<std::string>{"water_vapor", "cloud_liquid", "precip_liquid"}
                                                  : std::vector<std::string>{"water_vapor"};
    for (auto const &t : tracers) coupler.add_tracer(t, "", true, true);
    coupler.set_option<std::string>("micro", micro == 2 ? "p3" : micro == 1 ? "kessler" : "none");
    auto &dm = coupler.get_data_manager_device_readwrite();
    std::vector<std::string> precip;
    if (micro == 1) precip = {"precl"};
    if (micro == 2) precip = {"precip_liq_surf_out", "precip_ice_surf_out"};
    for (auto const &n : precip) dm.register_and_allocate<real>(n, "surface precipitation rate", {ny, nx, nens}, {"y", "x", "nens"});
    copy_in(dm.get<real, 2>("vertical_interface_height").data(), take((size_t)(nz + 1) * nens));
    std::vector<std::string> names = {"temp", "density_dry", "water_vapor"};
    if (micro == 1) names.push_back("cloud_liquid");
    if (micro == 2) { names.push_back("cloud_water"); names.push_back("ice"); }
    const char *diag[9] = {"diag_cldtot", "diag_cldlow", "diag_cldmed", "diag_cldhgh", "diag_lwp", "diag_iwp", "diag_pw", "diag_precip_liq",
                           "diag_precip_ice"};
    modules::column_diagnostics_init(coupler);
    std::vector<double> sevens(nens, 7.0);
    for (const char *n : diag)
      if (dm.entry_exists(n)) copy_in(dm.get<real, 1>(n).data(), sevens);
    modules::column_diagnostics_init(coupler);
    for (int s = 0; s < steps; s++) {
      real weight = take(1)[0];
      for (auto const &name : names) copy_in(dm.get<real, 4>(name).data(), take(n4));
      for (auto const &name : precip) copy_in(dm.get<real, 3>(name).data(), take(n3));
      modules::column_diagnostics(coupler, weight);
    }
    if (hipDeviceSynchronize() != hipSuccess) endrun("synchronize failed");
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    std::printf("### entries");
    std::vector<double> host(nens);
    for (const char *n : diag) {
      if (!dm.entry_exists(n)) continue;
      std::printf(" %s", n);
      if (hipMemcpy(host.data(), dm.get<real const, 1>(n).data(), nens * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) endrun("copy failed");
      std::fwrite(host.data(), sizeof(double), nens, out);
    }
    std::printf("\n### options %g %g %g\n", (double)coupler.get_option<real>("crm_diag_p_low"), (double)coupler.get_option<real>("crm_diag_p_high"),
                (double)coupler.get_option<real>("crm_diag_cwp_threshold"));
    std::fclose(out);
  } catch (std::string const &msg) {
    std::printf("### failed %s\n", msg.c_str());
    status = 1;
  }
  std::fclose(in);
  pam_amd_modules_finalize();
  return status;
}
