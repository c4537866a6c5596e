// vtable_check.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_vertical_table_form.py builds and runs it on the host).
//
// Checks the stored vertical WENO table (awfl_device.h: VTable, make_vtable; awfl_vertical.h: build_vertical_tables) against the
// unfactored upper polynomial it replaces: on random stencils of every level (and member) of a grid, the factored blended TV, the even
// part e3 and the odd part o3 against the same quantities formed from h1..h4 of the level's DTable, and the whole polynomial
// (weno5_table) against the unfactored evaluation with the same tail.  Prints one line of key=value pairs.
//
// usage: vtable_check GRID_FILE NSAMPLES SEED      GRID_FILE: "nz nens" then the nz x nens cell thicknesses (level-major)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../pam_amd/csrc/awfl_device.h"
#include "../../pam_amd/csrc/awfl_vertical.h"

using namespace pama;

namespace {

struct Unfactored { double tvb, e3, o3, escale, oscale, left, right; };

// the upper polynomial from h1..h4, as weno5_table formed it before the factored table (explicit rounding points)
Unfactored unfactored(const DTable &t, const double u[5], const WenoConsts &wc) {
#pragma clang fp contract(off)
  constexpr double K13 = AWFL_TV5_A1A3 / AWFL_TV5_SQRT_A3A3, K24 = AWFL_TV5_A2A4 / AWFL_TV5_SQRT_A4A4;
  const double sq = std::sqrt(AWFL_TV3_A2A2);
  const double d[4] = {u[1] - u[0], u[2] - u[1], u[3] - u[2], u[4] - u[3]};
  double a1[3], a2[3], tv[3];
  for (int i = 0; i < 3; i++) {
    a1[i] = std::fma(t.lo1[i][1], d[i + 1], t.lo1[i][0] * d[i]);
    a2[i] = std::fma(t.lo2[i][1] * sq, d[i + 1], (t.lo2[i][0] * sq) * d[i]);
    tv[i] = std::fma(a1[i], a1[i], a2[i] * a2[i]);
  }
  double h[4], habs[4];
  for (int p = 0; p < 4; p++) {
    h[p] = std::fma(t.hi[p][0], d[0], std::fma(t.hi[p][1], d[1], std::fma(t.hi[p][2], d[2], t.hi[p][3] * d[3])));
    habs[p] = 0.0;
    for (int m = 0; m < 4; m++) habs[p] += std::fabs(t.hi[p][m] * d[m]);
  }
  const double t1 = std::fma(K13, h[2], h[0]), t2 = std::fma(K24, h[3], AWFL_TV5_A2A2 * h[1]);
  const double tv3 = std::fma(h[3], h[3], std::fma(h[2], h[2], std::fma(h[1], t2, h[0] * t1)));
  const double tv3s = std::fma(WENO_BLEND_LO / AWFL_WENO_SIGMA, (tv[0] + tv[1]) + tv[2], tv3);
  Unfactored r;
  r.tvb = AWFL_WENO_SIGMA * tv3s;
  r.e3 = std::fma(h[3], t.k4, h[1] * t.k2);
  r.o3 = std::fma(0.25 / AWFL_TV5_SQRT_A3A3, h[2], h[0]);
  r.escale = std::fabs(t.k4) * habs[3] + std::fabs(t.k2) * habs[1];
  r.oscale = 0.25 / AWFL_TV5_SQRT_A3A3 * habs[2] + habs[0];
  constexpr double EPS_TV = 1.0e-20, R3S = WENO_R3 * (AWFL_WENO_SIGMA * AWFL_WENO_SIGMA);
  const double d0 = std::fma(tv[0], tv[0], EPS_TV), d1 = std::fma(tv[1], tv[1] * WENO_R1, EPS_TV * WENO_R1);
  const double d2 = std::fma(tv[2], tv[2], EPS_TV), d3 = std::fma(tv3s, tv3s * R3S, EPS_TV * WENO_R3);
  weno5_tail(u[2], d0, d1, d2, d3, 1.0e-20 / weno_idl_c(0), a1, a2, r.e3, r.o3, t.k2 / sq, 0.5, wc, r.left, r.right);
  return r;
}

// the factored quantities from a stored table (VTable layout), formed as weno5_table forms them
void factored(const double *v, const double u[5], double &tvb, double &e3, double &o3) {
#pragma clang fp contract(off)
  const double d[4] = {u[1] - u[0], u[2] - u[1], u[3] - u[2], u[4] - u[3]};
  const double z0 = std::fma(v[12], d[0], std::fma(v[13], d[1], std::fma(v[14], d[2], v[15] * d[3])));
  const double z1 = std::fma(v[16], d[1], std::fma(v[17], d[2], v[18] * d[3]));
  const double z2 = std::fma(v[19], d[2], v[20] * d[3]);
  const double z3 = v[21] * d[3];
  tvb = std::fma(z0, z0, std::fma(z1, z1, std::fma(z2, z2, z3 * z3))) / std::sqrt(WENO_R3);
  e3 = std::fma(v[22], d[0], std::fma(v[23], d[1], std::fma(v[24], d[2], v[25] * d[3])));
  o3 = std::fma(v[26], d[0], std::fma(v[27], d[1], std::fma(v[28], d[2], v[29] * d[3])));
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: vtable_check GRID_FILE NSAMPLES SEED\n"); return 2; }
  FILE *f = std::fopen(argv[1], "r");
  int nz = 0, nens = 0;
  if (!f || std::fscanf(f, "%d %d", &nz, &nens) != 2 || nz < 1 || nens < 1) { std::fprintf(stderr, "bad grid file\n"); return 2; }
  std::vector<double> dz((size_t)nz * nens);
  for (double &x : dz)
    if (std::fscanf(f, "%lf", &x) != 1) { std::fprintf(stderr, "bad grid file\n"); return 2; }
  std::fclose(f);
  const int nsamples = std::atoi(argv[2]);
  std::mt19937_64 rng(std::strtoull(argv[3], nullptr, 10));
  std::normal_distribution<double> nd(0.0, 1.0);
  std::uniform_real_distribution<double> ud(-12.0, 6.0);

  const VerticalTables vt = build_vertical_tables(dz.data(), nz, nens);
  const WenoConsts wc = weno_consts();
  double err_tv = 0, err_e3 = 0, err_o3 = 0, err_lr = 0, min_piv = 1e300;
  long long n = 0;
  for (int k = 0; k < nz + 2; k++)
    for (int e = 0; e < (vt.per_ens ? nens : 1); e++) {
      double s2c[25], wrl[27], piv[4];
      const DTable t = level_dtable(dz.data() + e, nens, nz, k, s2c, wrl);
      (void)make_vtable(t, [](double x) { return std::sqrt(x); }, piv);
      for (int j = 0; j < 4; j++) min_piv = std::fmin(min_piv, piv[j]);
      const double *v = vt.per_ens ? nullptr : vt.table.data() + (size_t)k * VZ_STRIDE;
      double vloc[VZ_STRIDE];
      if (vt.per_ens) {
        for (int m = 0; m < VZ_STRIDE; m++) vloc[m] = vt.table[((size_t)k * VZ_STRIDE + m) * nens + e];
        v = vloc;
      }
      for (int s = 0; s < nsamples; s++) {
        double u[5];
        const double scale = std::exp2(ud(rng)), base = 300.0 * nd(rng);
        const int kind = s % 3;
        for (int m = 0; m < 5; m++) {
          const double x = m - 2.0;
          if (kind == 0) u[m] = base + scale * nd(rng);                                            // rough
          else if (kind == 1) u[m] = base + scale * (nd(rng) * x + 0.1 * nd(rng) * x * x) + 1e-6 * scale * nd(rng);   // smooth
          else u[m] = base + (m >= 2 + (s % 4) - 1 ? scale : 0.0);                                  // a step
        }
        const Unfactored o = unfactored(t, u, wc);
        double tvb, e3, o3, L, R;
        factored(v, u, tvb, e3, o3);
        if (o.tvb > 0) err_tv = std::fmax(err_tv, std::fabs(tvb - o.tvb) / o.tvb);
        if (o.escale > 0) err_e3 = std::fmax(err_e3, std::fabs(e3 - o.e3) / o.escale);
        if (o.oscale > 0) err_o3 = std::fmax(err_o3, std::fabs(o3 - o.o3) / o.oscale);
        weno5_table(u, v, 1, wc, L, R);
        double umax = 0;
        for (int m = 0; m < 5; m++) umax = std::fmax(umax, std::fabs(u[m]));
        err_lr = std::fmax(err_lr, std::fmax(std::fabs(L - o.left), std::fabs(R - o.right)) / umax);
        n++;
      }
    }
  std::printf("levels=%d per_ens=%d pivots_ok=%d min_pivot=%.6e samples=%lld err_tvb=%.3e err_e3=%.3e err_o3=%.3e err_lr=%.3e\n",
              nz + 2, vt.per_ens ? 1 : 0, vt.pivots_ok ? 1 : 0, min_piv, n, err_tv, err_e3, err_o3, err_lr);
  return 0;
}
