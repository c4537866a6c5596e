// flux_profiles.cpp -- the C++ module modules/flux_profiles.h driven from a file.  TEST INFRASTRUCTURE ONLY: tests/test_fluxprof.py builds
// it with hipcc the way the examples' driver is built, tests/test_fluxprof_gpu.py runs it.
//   flux_profiles IN OUT
// IN: six int32 (nz, ny, nx, nens, micro: 0 none | 1 kessler | 2 p3, steps), then float64 arrays: per step its weight (one value) and
// density_dry, water_vapor, the cloud tracer, the ice tracer (those the microphysics has), temp, uvel, vvel, wvel (nz,ny,nx,nens).
// flux_profiles_init runs twice, the second time after the entries were filled with 7: a GCM step starts from zero.  OUT: the ten prof_
// entries (nz,nens), those that exist, in the order of the C ABI.  stdout: "### entries" and their names.  A thrown message goes to stdout.
#include <cstdio>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "modules/flux_profiles.h"

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
  size_t n4 = (size_t)nz * ny * nx * nens, n2 = (size_t)nz * nens;
  auto take = [&](size_t n) { std::vector<double> v(n); if (std::fread(v.data(), sizeof(double), n, in) != n) endrun("short input"); return v; };
  int status = 0;
  try {
    pam::PamCoupler coupler;
    coupler.set_option<real>("crm_dt", 20.0);
    coupler.set_option<real>("gcm_physics_dt", 240.0);
    coupler.allocate_coupler_state(nz, ny, nx, nens);
    coupler.set_grid(16000.0, 12000.0, std::vector<real>(nz + 1, 0.0));
    std::vector<std::string> tracers = micro == 2 ? std::vector<std::string>{"water_vapor", "cloud_water", "ice"}
                                     : micro == 1 ? std::vector<std::string>{"water_vapor", "cloud_liquid", "precip_liquid"}
                                                  : std::vector<std::string>{"water_vapor"};
    for (auto const &t : tracers) coupler.add_tracer(t, "", true, true);
    coupler.set_option<std::string>("micro", micro == 2 ? "p3" : micro == 1 ? "kessler" : "none");
    auto &dm = coupler.get_data_manager_device_readwrite();
    std::vector<std::string> names = {"density_dry", "water_vapor"};
    if (micro == 1) names.push_back("cloud_liquid");
    if (micro == 2) { names.push_back("cloud_water"); names.push_back("ice"); }
    for (const char *n : {"temp", "uvel", "vvel", "wvel"}) names.push_back(n);
    const char *prof[10] = {"prof_mcup", "prof_mcdn", "prof_mcuup", "prof_mcudn", "prof_cld", "prof_flux_t", "prof_flux_qt", "prof_flux_u",
                            "prof_flux_v", "prof_tke"};
    modules::flux_profiles_init(coupler);
    std::vector<double> sevens(n2, 7.0);
    for (const char *n : prof)
      if (dm.entry_exists(n)) copy_in(dm.get<real, 2>(n).data(), sevens);
    modules::flux_profiles_init(coupler);
    for (int s = 0; s < steps; s++) {
      real weight = take(1)[0];
      for (auto const &name : names) copy_in(dm.get<real, 4>(name).data(), take(n4));
      modules::flux_profiles(coupler, weight);
    }
    if (hipDeviceSynchronize() != hipSuccess) endrun("synchronize failed");
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    std::printf("### entries");
    std::vector<double> host(n2);
    for (const char *n : prof) {
      if (!dm.entry_exists(n)) continue;
      std::printf(" %s", n);
      if (hipMemcpy(host.data(), dm.get<real const, 2>(n).data(), n2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) endrun("copy failed");
      std::fwrite(host.data(), sizeof(double), n2, out);
    }
    std::printf("\n### options %g\n", (double)coupler.get_option<real>("crm_prof_qc_threshold"));
    std::fclose(out);
  } catch (std::string const &msg) {
    std::printf("### failed %s\n", msg.c_str());
    status = 1;
  }
  std::fclose(in);
  pam_amd_modules_finalize();
  return status;
}
