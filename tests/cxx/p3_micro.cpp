// p3_micro.cpp -- the C++ plug-in class Microphysics of physics/micro/p3_amd/Microphysics.h driven from a file.  TEST INFRASTRUCTURE ONLY:
// tests/test_p3_coupling_gpu.py builds it with hipcc the way the examples' driver is built.
//   p3_micro IN OUT MODE      MODE: run | no_p3_main | failing_p3_main | tend_out_layout1
// IN: seven int32 (nz, ny, nx, nens, shoc ? 1 : 0, layout, steps), then float64 arrays: zint (nz+1,nens), then (nz,ny,nx,nens): density_dry,
// water_vapor, cloud_water, temp, nccn_prescribed, nc_nuceat_tend, ni_activated, q_prev, t_prev and the seven tracers cloud_water_num ...
// ice_rime_vol.  OUT: the same 16 arrays after the steps, then liq/vap_liq/vap_ice_exchange_out, then precip_liq/ice_surf_out (ny,nx,nens).
// A thrown message goes to stdout.
#include <cstdio>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "physics/micro/p3_amd/Microphysics.h"

static void copy_in(real *dst, std::vector<double> const &src) {
  if (hipMemcpy(dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) endrun("copy failed");
}
static int failing_p3_main(const pam_amd_p3_args_t *, void *) { return 7; }

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  std::string mode = argv[3];
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int h[7];
  if (std::fread(h, sizeof(int), 7, in) != 7) return 3;
  int nz = h[0], ny = h[1], nx = h[2], nens = h[3], shoc = h[4], layout = h[5], steps = h[6];
  size_t n4 = (size_t)nz * ny * nx * nens, n3 = (size_t)ny * nx * nens;
  auto take = [&](size_t n) { std::vector<double> v(n); if (std::fread(v.data(), sizeof(double), n, in) != n) endrun("short input"); return v; };
  int status = 0;
  try {
    pam::PamCoupler coupler;
    coupler.set_option<real>("crm_dt", 2.0);
    coupler.set_option<std::string>("sgs", shoc ? "shoc" : "none");
    coupler.allocate_coupler_state(nz, ny, nx, nens);
    coupler.set_grid(16000.0, 12000.0, std::vector<real>(nz + 1, 0.0));
    Microphysics micro;
    micro.layout = layout;
    if (mode == "tend_out_layout1") micro.num_tend_out = 3;
    micro.init(coupler);
    if (mode == "failing_p3_main") micro.set_p3_main(failing_p3_main, nullptr);
    else if (mode != "no_p3_main") micro.set_p3_main(pam_amd_p3_main_standin, nullptr);
    auto &dm = coupler.get_data_manager_device_readwrite();
    copy_in(dm.get<real, 2>("vertical_interface_height").data(), take((size_t)(nz + 1) * nens));
    std::vector<std::string> names = {"density_dry", "water_vapor", "cloud_water", "temp", "nccn_prescribed", "nc_nuceat_tend", "ni_activated",
                                      "q_prev", "t_prev", "cloud_water_num", "rain", "rain_num", "ice", "ice_num", "ice_rime", "ice_rime_vol"};
    for (auto const &name : names) copy_in(dm.get<real, 4>(name).data(), take(n4));
    bool static_ok = Microphysics::get_num_tracers() == 9 && micro.micro_name() == "p3" && coupler.get_option<std::string>("micro") == "p3" &&
                     Microphysics::get_num_diffused_tracers() == 4 && coupler.get_option<real>("cp_v") == 1859 && micro.cv_v == micro.R_v - micro.cp_v;
    try {
      for (int s = 0; s < steps; s++) micro.timeStep(coupler);
    } catch (std::string const &msg) {
      std::printf("### threw %s\n", msg.c_str());
    }
    std::printf("### members %d etime %g first_step %d sgs_shoc %d\n", (int)static_ok, (double)micro.etime, (int)micro.first_step,
                (int)micro.sgs_shoc);
    if (hipDeviceSynchronize() != hipSuccess) endrun("synchronize failed");
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    names.push_back("liq_ice_exchange_out");
    names.push_back("vap_liq_exchange_out");
    names.push_back("vap_ice_exchange_out");
    std::vector<double> host(n4);
    for (auto const &name : names) {
      if (hipMemcpy(host.data(), dm.get<real, 4>(name).data(), n4 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) endrun("copy failed");
      std::fwrite(host.data(), sizeof(double), n4, out);
    }
    for (auto name : {"precip_liq_surf_out", "precip_ice_surf_out"}) {
      if (hipMemcpy(host.data(), dm.get<real, 3>(name).data(), n3 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) endrun("copy failed");
      std::fwrite(host.data(), sizeof(double), n3, out);
    }
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
