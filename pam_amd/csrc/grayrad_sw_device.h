// grayrad_sw_device.h -- the arithmetic of the native grey two-stream shortwave radiation scheme (one band, the sun's beam and the light
// it scatters back treated alike; the layers are combined by the adding method as Lacis and Hansen 1974 combine theirs),
// as device functions that are plain inline C++ outside hipcc: the HIP kernel in modules_kernels.hip calls them, and
// tests/emu/grayrad_sw_emu.cpp compiles the same bodies with g++ (-ffp-contract=off).  The method is not part of the reference tree; the
// yardstick is the numpy restatement of the contract in tests/grayrad_sw_ref.py, held bit for bit (include/pam_amd_modules.h at
// pam_amd_radiation_gray_sw).
// The layout, the tables of cloud species, IDX and the look-ahead are the longwave scheme's (grayrad_device.h), whose Fields, species_sum,
// difference and apply are used as they are.  coszen (nens) is per member, like zint.  Contraction into fma is switched off inside each
// body, so the device and the host give the same bits.  The exponential is the contract's own, pama::sgs::exp_c.
#pragma once

#include "grayrad_device.h"  // Fields, species_sum, difference, apply, MAX_SPECIES, AHEAD; sgs_device.h: exp_c, PAMA_D, PAMA_NO_CONTRACT

namespace pama {
namespace grayrad_sw {

using grayrad::AHEAD;
using grayrad::Fields;
using grayrad::apply;
using grayrad::difference;
using grayrad::species_sum;

struct Params {
  double a_d, a_v, a_l, a_i;             // mass absorption coefficients [m2/kg]
  double s_l, s_i;                       // mass backscatter coefficients of cloud liquid and cloud ice [m2/kg]: extinction x (1 - g) / 2
  double solar_constant, albedo, cp_d, dt;
  int num_liquid, num_ice;
};

// night is mu0 <= 0.0, so -0.0 is night and a NaN is day
PAMA_D bool night(double mu0) { return mu0 <= 0.0; }

// m = 1 / mu0: once per column
PAMA_D double slant(double mu0) {
  PAMA_NO_CONTRACT
  return 1.0 / mu0;
}

// reflectance R = r ta and transmittance T = tr ta of one cell, the same for both directions:
// ta = exp_c(-da), da = ((((a_d rho_d + a_v rho_v) + a_l L) + a_i I) dz) m;  tr = 1 / (1 + b), r = 1 - tr, b = ((s_l L + s_i I) dz) m
PAMA_D void layer(const Params &P, double m, double rho_d, double rho_v, double L, double I, double dz, double &R, double &T) {
  PAMA_NO_CONTRACT
  const double x = P.a_d * rho_d;
  const double y = P.a_v * rho_v;
  double a = x + y;
  a = a + P.a_l * L;
  a = a + P.a_i * I;
  const double da = (a * dz) * m;
  const double ta = sgs::exp_c(-da);
  const double u = P.s_l * L;
  const double v = P.s_i * I;
  const double s = u + v;
  const double b = (s * dz) * m;
  const double tr = 1.0 / (1.0 + b);
  const double r = 1.0 - tr;
  R = r * ta;
  T = tr * ta;
}

// q = 1 - Rb R: what the light bouncing between the cell and everything below it is divided by
PAMA_D double bounce(double Rb, double R) {
  PAMA_NO_CONTRACT
  return 1.0 - Rb * R;
}

// one step of the upward sweep: the reflectance of everything below the cell's upper interface, Rb' = R + ((T Rb) T) / q
PAMA_D double add_layer(double Rb, double R, double T, double q) {
  PAMA_NO_CONTRACT
  const double n = (T * Rb) * T;
  return R + n / q;
}

// one step of the downward sweep: Fd(k) = (T Fd(k+1)) / q
PAMA_D double pass_down(double Fd, double T, double q) {
  PAMA_NO_CONTRACT
  return (T * Fd) / q;
}

PAMA_D double product(double a, double b) {
  PAMA_NO_CONTRACT
  return a * b;
}

// heating = ((Fd(k+1) - Fd(k)) + (Fu(k) - Fu(k+1))) / ((cp_d (rho_d + rho_v)) dz)
PAMA_D double heating_rate(const Params &P, double fd_p, double fd_k, double fu_k, double fu_p, double rho_d, double rho_v, double dz) {
  PAMA_NO_CONTRACT
  const double dd = fd_p - fd_k;
  const double du = fu_k - fu_p;
  const double n = dd + du;
  const double rho = rho_d + rho_v;
  const double c = P.cp_d * rho;
  return n / (c * dz);
}

// both sweeps of one (column, member).  temp, heating and the fields of F point at element 0 and get off + k level; zint points at (0, e)
// with stride zs; mu0 is the member's coszen; sfc_albedo (NULL: P.albedo), down_sfc, up_sfc and up_top point at element 0 and get off.
// Night (mu0 <= 0): zeros in heating and in the three outputs, and nothing is read.  Day, upward, k = 0 .. nz-1: Rb(k), the reflectance
// of everything below the cell, is parked in heating(k), and Rb(k+1) = R + ((T Rb) T) / (1 - Rb R) from Rb(0) = the albedo.  Downward,
// k = nz-1 .. 0: R and T are formed again from the same inputs, Rb(k) is read back, Fd(k) = (T Fd(k+1)) / (1 - Rb(k) R) from Fd(nz) =
// solar_constant mu0, Fu(k) = Rb(k) Fd(k), heating(k) replaces Rb(k) and, where dt != 0, temp(k) takes it.
// The loads of AHEAD levels are requested before the first of them is used.  Nothing that is written overlaps anything that is read
// but temp and heating themselves (the entry point refuses it)
template <class IDX>
PAMA_D void column(double *temp, const Fields &F, const double *zint, double mu0, const double *sfc_albedo, IDX off, IDX level, IDX zs, int nz,
                   const Params &P, double *heating, double *down_sfc, double *up_sfc, double *up_top) {
  double *T = temp + off, *H = heating + off;
  if (night(mu0)) {
    for (int k = 0; k < nz; k++) H[(IDX)k * level] = 0.0;
    down_sfc[off] = 0.0; up_sfc[off] = 0.0; up_top[off] = 0.0;
    return;
  }
  const double *rd = F.rho_d + off, *rv = F.rho_v + off;
  // an absent species points at rho_d and is never read
  const double *l0 = P.num_liquid > 0 ? F.liquid[0] + off : rd, *l1 = P.num_liquid > 1 ? F.liquid[1] + off : rd;
  const double *i0 = P.num_ice > 0 ? F.ice[0] + off : rd, *i1 = P.num_ice > 1 ? F.ice[1] + off : rd;
  const double m = slant(mu0);

  double Rb = sfc_albedo ? sfc_albedo[off] : P.albedo, zi_k = zint[0];
  for (int k0 = 0; k0 < nz; k0 += AHEAD) {
    double a_rd[AHEAD], a_rv[AHEAD], a_L[AHEAD], a_I[AHEAD], a_zi[AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const IDX kc = (IDX)(k0 + b < nz ? k0 + b : nz - 1), o = kc * level;
      a_rd[b] = rd[o]; a_rv[b] = rv[o];
      a_L[b] = species_sum(P.num_liquid, P.num_liquid > 0 ? l0[o] : 0.0, P.num_liquid > 1 ? l1[o] : 0.0);
      a_I[b] = species_sum(P.num_ice, P.num_ice > 0 ? i0[o] : 0.0, P.num_ice > 1 ? i1[o] : 0.0);
      a_zi[b] = zint[(kc + (IDX)1) * zs];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const int k = k0 + b;
      if (k >= nz) break;
      double R, Tr;
      layer(P, m, a_rd[b], a_rv[b], a_L[b], a_I[b], difference(a_zi[b], zi_k), R, Tr);
      H[(IDX)k * level] = Rb;
      Rb = add_layer(Rb, R, Tr, bounce(Rb, R));
      zi_k = a_zi[b];
    }
  }

  double Fd = product(P.solar_constant, mu0), Fu = product(Rb, Fd), zi_p = zi_k;      // zi_k is zint(nz) now
  up_top[off] = Fu;
  for (int k0 = nz - 1; k0 >= 0; k0 -= AHEAD) {
    double a_rd[AHEAD], a_rv[AHEAD], a_L[AHEAD], a_I[AHEAD], a_T[AHEAD], a_zi[AHEAD], a_Rb[AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const IDX kc = (IDX)(k0 - b > 0 ? k0 - b : 0), o = kc * level;
      a_rd[b] = rd[o]; a_rv[b] = rv[o]; a_Rb[b] = H[o];
      a_T[b] = P.dt != 0.0 ? T[o] : 0.0;
      a_L[b] = species_sum(P.num_liquid, P.num_liquid > 0 ? l0[o] : 0.0, P.num_liquid > 1 ? l1[o] : 0.0);
      a_I[b] = species_sum(P.num_ice, P.num_ice > 0 ? i0[o] : 0.0, P.num_ice > 1 ? i1[o] : 0.0);
      a_zi[b] = zint[kc * zs];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const int k = k0 - b;
      if (k < 0) break;
      const double dz = difference(zi_p, a_zi[b]);
      double R, Tr;
      layer(P, m, a_rd[b], a_rv[b], a_L[b], a_I[b], dz, R, Tr);
      const double Fdk = pass_down(Fd, Tr, bounce(a_Rb[b], R));
      const double Fuk = product(a_Rb[b], Fdk);
      const double h = heating_rate(P, Fd, Fdk, Fuk, Fu, a_rd[b], a_rv[b], dz);
      H[(IDX)k * level] = h;
      if (P.dt != 0.0) T[(IDX)k * level] = apply(a_T[b], h, P.dt);
      Fd = Fdk;
      Fu = Fuk;
      zi_p = a_zi[b];
    }
  }
  down_sfc[off] = Fd;
  up_sfc[off] = Fu;
}

}  // namespace grayrad_sw
}  // namespace pama
