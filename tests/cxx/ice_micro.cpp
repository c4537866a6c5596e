// ice_micro.cpp -- the C++ plug-in class physics/micro/ice_amd/Microphysics.h driven from a file.  TEST INFRASTRUCTURE ONLY:
// tests/test_ice1m_gpu.py builds it with hipcc the way the examples' driver is built, and runs it.
//   ice_micro IN OUT
// IN: four int32 (nz, ny, nx, nens), then float64: dt (one value), zint (nz+1,nens), then density_dry, temp, water_vapor, cloud_liquid,
// cloud_ice, precip_liquid, precip_ice (nz,ny,nx,nens).  init, one timeStep.  OUT: the five species in the registration order, temp
// (nz,ny,nx,nens), precl, preci (ny,nx,nens), density_dry.  stdout: "### tracers" and their names, "### micro" and the option and the
// class's name, "### constants" R_d R_v cp_d cp_v grav p0, "### mass" before and after.  A thrown message goes to stdout.
#include <cstdio>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "physics/micro/ice_amd/Microphysics.h"

static void copy_in(real *dst, std::vector<double> const &src) {
  if (hipMemcpy(dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) endrun("copy failed");
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int h[4];
  if (std::fread(h, sizeof(int), 4, in) != 4) return 3;
  int nz = h[0], ny = h[1], nx = h[2], nens = h[3];
  size_t n4 = (size_t)nz * ny * nx * nens, n3 = (size_t)ny * nx * nens;
  auto take = [&](size_t n) { std::vector<double> v(n); if (std::fread(v.data(), sizeof(double), n, in) != n) endrun("short input"); return v; };
  int status = 0;
  try {
    pam::PamCoupler coupler;
    coupler.set_option<real>("crm_dt", take(1)[0]);
    coupler.allocate_coupler_state(nz, ny, nx, nens);
    coupler.set_grid(16000.0, 12000.0, std::vector<real>(nz + 1, 0.0));
    Microphysics micro;
    static_assert(Microphysics::num_tracers == 5 && Microphysics::get_num_tracers() == 5, "five tracers");
    micro.init(coupler);
    auto &dm = coupler.get_data_manager_device_readwrite();
    copy_in(dm.get<real, 2>("vertical_interface_height").data(), take((size_t)(nz + 1) * nens));
    for (const char *n : {"density_dry", "temp", "water_vapor", "cloud_liquid", "cloud_ice", "precip_liquid", "precip_ice"})
      copy_in(dm.get<real, 4>(n).data(), take(n4));
    std::printf("### tracers");
    for (auto const &n : coupler.get_tracer_names()) std::printf(" %s", n.c_str());
    std::printf("\n### micro %s %s\n", coupler.get_option<std::string>("micro").c_str(), micro.micro_name().c_str());
    std::printf("### constants %g %g %g %g %g %g\n", (double)coupler.get_option<real>("R_d"), (double)coupler.get_option<real>("R_v"),
                (double)coupler.get_option<real>("cp_d"), (double)coupler.get_option<real>("cp_v"), (double)coupler.get_option<real>("grav"),
                (double)coupler.get_option<real>("p0"));
    const double before = micro.compute_total_mass(coupler);
    coupler.run_module("micro", [&](pam::PamCoupler &c) { micro.timeStep(c); });
    if (hipDeviceSynchronize() != hipSuccess) endrun("synchronize failed");
    std::printf("### mass %.17g %.17g\n", before, (double)micro.compute_total_mass(coupler));
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    std::vector<double> host(n4);
    auto put = [&](const real *dev, size_t n) {
      if (hipMemcpy(host.data(), dev, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) endrun("copy failed");
      std::fwrite(host.data(), sizeof(double), n, out);
    };
    for (const char *n : {"water_vapor", "cloud_liquid", "cloud_ice", "precip_liquid", "precip_ice", "temp"}) put(dm.get<real const, 4>(n).data(), n4);
    for (const char *n : {"precl", "preci"}) put(dm.get<real const, 3>(n).data(), n3);
    put(dm.get<real const, 4>("density_dry").data(), n4);
    std::fclose(out);
    micro.finalize(coupler);
  } catch (std::string const &msg) {
    std::printf("### failed %s\n", msg.c_str());
    status = 1;
  }
  std::fclose(in);
  pam_amd_modules_finalize();
  return status;
}
