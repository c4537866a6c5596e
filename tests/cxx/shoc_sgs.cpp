// shoc_sgs.cpp -- the C++ plug-in class SGS of physics/sgs/shoc_amd/SGS.h driven from a file.  TEST INFRASTRUCTURE ONLY:
// tests/test_shoc_coupling_gpu.py builds it with hipcc the way the examples' driver is built.
//   shoc_sgs IN OUT MODE      MODE: run | no_shoc_main | no_micro | bad_micro
// IN: six int32 (nz, ny, nx, nens, p3 ? 1 : 0, layout), then float64 arrays: zint (nz+1,nens), zmid (nz,nens), sfc_mom_flx_u, sfc_mom_flx_v
// (ny,nx,nens), then (nz,ny,nx,nens): density_dry, water_vapor, the cloud tracer, uvel, vvel, wvel, temp, tke, wthv_sec, tk, tkh, cldfrac and
// the 1 or 7 extra tracers.  OUT: the same arrays after one timeStep, followed by inv_qc_relvar.  A thrown message goes to stdout.
#include <cstdio>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "physics/sgs/shoc_amd/SGS.h"

static void copy_in(real *dst, std::vector<double> const &src) {
  if (hipMemcpy(dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) endrun("copy failed");
}

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  std::string mode = argv[3];
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int h[6];
  if (std::fread(h, sizeof(int), 6, in) != 6) return 3;
  int nz = h[0], ny = h[1], nx = h[2], nens = h[3], p3 = h[4], layout = h[5];
  size_t n4 = (size_t)nz * ny * nx * nens, n3 = (size_t)ny * nx * nens;
  auto take = [&](size_t n) { std::vector<double> v(n); if (std::fread(v.data(), sizeof(double), n, in) != n) endrun("short input"); return v; };
  int status = 0;
  try {
    pam::PamCoupler coupler;
    coupler.set_option<real>("crm_dt", 2.0);
    coupler.set_option<real>("R_d", 287.0);      // what a microphysics sets; compute_pressure_array reads them
    coupler.set_option<real>("R_v", 461.0);
    coupler.allocate_coupler_state(nz, ny, nx, nens);
    coupler.set_grid(16000.0, 12000.0, std::vector<real>(nz + 1, 0.0));
    std::vector<std::string> tracers = p3 ? std::vector<std::string>{"water_vapor", "cloud_water", "cloud_water_num", "rain", "rain_num", "ice",
                                                                     "ice_num", "ice_rime", "ice_rime_vol"}
                                          : std::vector<std::string>{"water_vapor", "cloud_liquid", "precip_liquid"};
    for (auto const &t : tracers) coupler.add_tracer(t, "", true, true);
    if (mode == "bad_micro") coupler.set_option<std::string>("micro", "none");
    else if (mode != "no_micro") coupler.set_option<std::string>("micro", p3 ? "p3" : "kessler");
    SGS sgs;
    sgs.layout = layout;
    sgs.init(coupler);
    if (mode != "no_shoc_main") sgs.set_shoc_main(pam_amd_shoc_main_standin, nullptr);
    auto &dm = coupler.get_data_manager_device_readwrite();
    copy_in(dm.get<real, 2>("vertical_interface_height").data(), take((size_t)(nz + 1) * nens));
    copy_in(dm.get<real, 2>("vertical_midpoint_height").data(), take((size_t)nz * nens));
    copy_in(dm.get<real, 3>("sfc_mom_flx_u").data(), take(n3));
    copy_in(dm.get<real, 3>("sfc_mom_flx_v").data(), take(n3));
    std::vector<std::string> names = {"density_dry", "water_vapor", p3 ? "cloud_water" : "cloud_liquid", "uvel", "vvel", "wvel", "temp", "tke",
                                      "wthv_sec", "tk", "tkh", "cldfrac"};
    for (size_t t = 2; t < tracers.size(); t++) names.push_back(tracers[t]);
    for (auto const &name : names) copy_in(dm.get<real, 4>(name).data(), take(n4));
    bool static_ok = SGS::get_num_tracers() == 1 && sgs.sgs_name() == "shoc" && coupler.get_option<std::string>("sgs") == "shoc";
    try {
      sgs.timeStep(coupler);
    } catch (std::string const &msg) {
      std::printf("### threw %s\n", msg.c_str());
    }
    std::printf("### members %d etime %g first_step %d\n", (int)static_ok, (double)sgs.etime, (int)sgs.first_step);
    if (hipDeviceSynchronize() != hipSuccess) endrun("synchronize failed");
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    names.push_back("inv_qc_relvar");
    std::vector<double> host(n4);
    for (auto const &name : names) {
      if (hipMemcpy(host.data(), dm.get<real, 4>(name).data(), n4 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) endrun("copy failed");
      std::fwrite(host.data(), sizeof(double), n4, out);
    }
    std::fclose(out);
    sgs.finalize(coupler);
  } catch (std::string const &msg) {
    std::printf("### failed %s\n", msg.c_str());
    status = 1;
  }
  std::fclose(in);
  pam_amd_modules_finalize();
  return status;
}
