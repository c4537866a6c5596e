// scalar_momentum.cpp -- the entry points behind modules/scalar_momentum.h called directly with host arrays, the way ls_forcing.cpp does
// without a file.  TEST INFRASTRUCTURE ONLY: tests/test_esmt.py builds it with hipcc the way the examples' driver is built and runs it.
//   "### refuse <what> <rc>"   one line per refusal of the contract: PAM_AMD_EINVAL (-1) before any device is asked for
//   "### nothing <rc> <rc>"    kmax == 0 without a force, and no mean without a force: PAM_AMD_OK, no launch, no device
//   "### rc <set> <diagnose> <pgf>"   three calls that pass every check: PAM_AMD_ENOGPU (-2) where there is no device.  (With a device the
//                              host arrays would be dereferenced by the kernels, so the calls are made only where there is none.)
//   "### untouched <0|1>"      every array still holds the pattern it was filled with
#include <cmath>
#include <cstdio>
#include <vector>

#include <hip/hip_runtime.h>

#include "pam_coupler.h"
#include "modules/scalar_momentum.h"

int main() {
  const int nens = 3, nx = 6, nz = 4, kmax = 3, cells = nens * nx * nz, rows = nz * nens;
  const long long words = pam_amd_esmt_workspace_doubles(nens, nz, kmax);
  std::vector<std::vector<double>> f(5, std::vector<double>(cells, 7.25)), p(11, std::vector<double>(rows, 7.25));
  std::vector<double> ct(nx, 7.25), st(nx, 7.25), work((size_t)words, 7.25);
  double *eu = f[0].data(), *ev = f[1].data(), *w = f[2].data(), *rd = f[3].data(), *rv = f[4].data();
  double *zmid = p[0].data(), *dz = p[1].data(), *rm = p[2].data(), *um = p[3].data(), *vm = p[4].data(), *fu = p[5].data(), *fv = p[6].data();
  double *gu = p[7].data(), *gv = p[8].data(), *tu = p[9].data(), *tv = p[10].data();
  auto pgf = [&](int ny_, int nz_, int nx_, int kmax_, double *eu_, double *um_, double dt_, double dx_, double *work_, long long words_) {
    return pam_amd_esmt_pgf(nens, nx_, ny_, nz_, eu_, ev, w, rd, rv, zmid, dz, rm, um_, vm, fu, fv, ct.data(), st.data(), dx_, dt_, kmax_, work_, words_,
                            nullptr);
  };
  std::printf("### refuse ny %d\n", pgf(2, nz, nx, kmax, eu, um, 10.0, 500.0, work.data(), words));
  std::printf("### refuse nz %d\n", pgf(1, 1, nx, kmax, eu, um, 10.0, 500.0, work.data(), words));
  std::printf("### refuse nx %d\n", pgf(1, nz, 1, 0, eu, um, 10.0, 500.0, work.data(), words));
  std::printf("### refuse kmax %d\n", pgf(1, nz, nx, nx / 2 + 1, eu, um, 10.0, 500.0, work.data(), words));
  std::printf("### refuse null %d\n", pgf(1, nz, nx, kmax, nullptr, um, 10.0, 500.0, work.data(), words));
  std::printf("### refuse force_without_mean %d\n", pgf(1, nz, nx, kmax, eu, nullptr, 10.0, 500.0, work.data(), words));
  std::printf("### refuse dt %d\n", pgf(1, nz, nx, kmax, eu, um, std::nan(""), 500.0, work.data(), words));
  std::printf("### refuse dx %d\n", pgf(1, nz, nx, kmax, eu, um, 10.0, 0.0, work.data(), words));
  std::printf("### refuse overlap %d\n", pgf(1, nz, nx, kmax, ev, um, 10.0, 500.0, work.data(), words));
  std::printf("### refuse workspace %d\n", pgf(1, nz, nx, kmax, eu, um, 10.0, 500.0, work.data(), words - 1));
  std::printf("### refuse diagnose_tend_without_gcm %d\n",
              pam_amd_esmt_diagnose(nens, nx, 1, nz, rd, rv, eu, ev, rm, um, vm, nullptr, gv, 1200.0, 0, tu, tv, nullptr));
  std::printf("### refuse set_ny %d\n", pam_amd_esmt_set(nens, nx, 3, nz, rd, rv, gu, gv, eu, ev, nullptr));
  int a = pam_amd_esmt_pgf(nens, nx, 1, nz, eu, ev, w, rd, rv, zmid, dz, rm, um, vm, nullptr, nullptr, ct.data(), st.data(), 500.0, 10.0, 0, nullptr, 0,
                           nullptr);
  int b = pam_amd_esmt_pgf(nens, nx, 1, nz, eu, ev, w, rd, rv, zmid, dz, rm, nullptr, nullptr, nullptr, nullptr, ct.data(), st.data(), 500.0, 10.0, kmax,
                           work.data(), words, nullptr);
  std::printf("### nothing %d %d\n", a, b);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    int s = pam_amd_esmt_set(nens, nx, 1, nz, rd, rv, gu, gv, eu, ev, nullptr);
    int d = pam_amd_esmt_diagnose(nens, nx, 1, nz, rd, rv, eu, ev, rm, um, vm, gu, gv, 1200.0, 1, tu, tv, nullptr);
    int g = pgf(1, nz, nx, kmax, eu, um, 10.0, 500.0, work.data(), words);
    std::printf("### rc %d %d %d\n", s, d, g);
  }
  bool same = true;
  for (auto const &v : f) for (double x : v) same = same && x == 7.25;
  for (auto const &v : p) for (double x : v) same = same && x == 7.25;
  for (double x : work) same = same && x == 7.25;
  std::printf("### untouched %d\n", same ? 1 : 0);
  return 0;
}
