// ls_forcing.cpp -- the C++ module modules/large_scale_forcing.h driven from a file.  TEST INFRASTRUCTURE ONLY: tests/test_lsforcing.py
// builds it with hipcc the way the examples' driver is built and runs it without arguments, tests/test_lsforcing_gpu.py runs it on a case.
//   ls_forcing           no file: one call of each entry point with host arrays, which pass the checks; prints
//                        "### rc <nudging> <forcing>", PAM_AMD_ENOGPU twice where there is no device, and leaves with 0
//   ls_forcing IN OUT    IN: ten int32 (nz, ny, nx, nens, tracers, the vapour's place in the table, the positive flags as bits, the
//                        profiles given as bits in the order of modules::LsProfiles with fcor as bit 12, steps, 0), then float64: dt,
//                        zmid (nz,nens), the profiles that are given (nz,nens) and fcor (nens), then density_dry, uvel, vvel, temp and
//                        the tracers (nz,ny,nx,nens).  OUT: uvel, vvel, temp and the tracers after `steps` calls.  stdout: "### entries"
//                        and the ls_ entries that exist.  A thrown message goes to stdout.
#include <cstdio>
#include <string>
#include <vector>

#include "pam_coupler.h"
#include "modules/large_scale_forcing.h"

static void copy_in(real *dst, std::vector<double> const &src) {
  if (hipMemcpy(dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) endrun("copy failed");
}

static int without_a_file() {
  const int nens = 3, nx = 2, ny = 2, nz = 4, cells = nens * nx * ny * nz, rows = nz * nens;
  std::vector<std::vector<double>> f(8, std::vector<double>(cells, 1.0)), p(16, std::vector<double>(rows, 0.0));
  const double *fields[5] = {f[2].data(), f[3].data(), f[4].data(), f[0].data(), f[1].data()};
  const double *target[4] = {p[0].data(), p[1].data(), p[2].data(), p[3].data()}, *rate[4] = {p[4].data(), p[5].data(), p[6].data(), p[6].data()};
  double *inc[4] = {p[7].data(), p[8].data(), p[9].data(), p[10].data()};
  double *tracers[2] = {f[5].data(), f[4].data()};
  const unsigned char positive[2] = {1, 1};
  int a = pam_amd_ls_nudging(nens, nx, ny, nz, fields, target, rate, 10.0, inc, nullptr);
  int b = pam_amd_ls_forcing(nens, nx, ny, nz, f[0].data(), f[1].data(), f[2].data(), 2, tracers, positive, f[3].data(), f[4].data(), p[11].data(),
                             p[12].data(), p[13].data(), p[14].data(), inc, p[15].data(), p[5].data(), p[6].data(), 10.0, 9.80616, 1004.64, nullptr);
  std::printf("### rc %d %d\n", a, b);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 1) return without_a_file();
  if (argc != 3) return 2;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int h[10];
  if (std::fread(h, sizeof(int), 10, in) != 10) return 3;
  int nz = h[0], ny = h[1], nx = h[2], nens = h[3], ntr = h[4], vapour = h[5], flags = h[6], given = h[7], steps = h[8];
  size_t n4 = (size_t)nz * ny * nx * nens, n2 = (size_t)nz * nens;
  auto take = [&](size_t n) { std::vector<double> v(n); if (std::fread(v.data(), sizeof(double), n, in) != n) endrun("short input"); return v; };
  int status = 0;
  try {
    pam::PamCoupler coupler;
    real dt = take(1)[0];
    coupler.set_option<real>("crm_dt", dt);
    coupler.set_option<real>("grav", 9.80616);
    coupler.set_option<real>("cp_d", 1004.64);
    coupler.allocate_coupler_state(nz, ny, nx, nens);
    std::vector<real> zint(nz + 1);
    for (int k = 0; k <= nz; k++) zint[k] = 1000.0 * k;
    coupler.set_grid(16000.0, 12000.0, zint);
    std::vector<std::string> tracers;
    for (int i = 0; i < ntr; i++) {
      tracers.push_back(i == vapour ? std::string("water_vapor") : "tracer_" + std::to_string(i));
      coupler.add_tracer(tracers.back(), "", (flags >> i) & 1, true);
    }
    auto &dm = coupler.get_data_manager_device_readwrite();
    copy_in(dm.get<real, 2>("vertical_midpoint_height").data(), take(n2));
    modules::LsProfiles P;
    std::vector<real> *slots[12] = {&P.wsub, &P.temp_tend, &P.qv_tend, &P.ug, &P.vg, &P.nudge_temp, &P.nudge_qv, &P.nudge_u, &P.nudge_v,
                                    &P.nudge_rate_temp, &P.nudge_rate_qv, &P.nudge_rate_uv};
    for (int i = 0; i < 12; i++)
      if ((given >> i) & 1) *slots[i] = take(n2);
    if ((given >> 12) & 1) P.fcor = take(nens);
    modules::ls_forcing_init(coupler, P);
    std::vector<std::string> names = {"density_dry", "uvel", "vvel", "temp"};
    for (auto const &t : tracers) names.push_back(t);
    for (auto const &name : names) copy_in(dm.get<real, 4>(name).data(), take(n4));
    for (int s = 0; s < steps; s++) modules::ls_forcing(coupler);
    if (hipDeviceSynchronize() != hipSuccess) endrun("synchronize failed");
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    std::vector<double> host(n4);
    for (size_t i = 1; i < names.size(); i++) {
      if (hipMemcpy(host.data(), dm.get<real const, 4>(names[i]).data(), n4 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) endrun("copy failed");
      std::fwrite(host.data(), sizeof(double), n4, out);
    }
    std::fclose(out);
    std::printf("### entries");
    for (const char *n : {"ls_wsub", "ls_temp_tend", "ls_qv_tend", "ls_ug", "ls_vg", "ls_nudge_temp", "ls_nudge_qv", "ls_nudge_u", "ls_nudge_v",
                          "ls_nudge_rate_temp", "ls_nudge_rate_qv", "ls_nudge_rate_uv", "ls_fcor", "ls_inc_temp", "ls_inc_qv", "ls_inc_u", "ls_inc_v"})
      if (dm.entry_exists(n)) std::printf(" %s", n);
    std::printf("\n### options %.17g %.17g\n", (double)coupler.get_option<real>("ls_courant_rate"), (double)coupler.get_option<real>("ls_nudge_rate_max"));
  } catch (std::string const &msg) {
    std::printf("### failed %s\n", msg.c_str());
    status = 1;
  }
  std::fclose(in);
  pam_amd_modules_finalize();
  return status;
}
