// grayrad_device.h -- the arithmetic of the native grey two-stream longwave radiation scheme (a Schwarzschild column scheme as idealised
// GCMs use it, Frierson et al. 2006, with the optical depth built from the water the CRM carries), as device functions that are plain
// inline C++ outside hipcc: the HIP kernel in modules_kernels.hip calls them, and tests/emu/grayrad_emu.cpp compiles the same bodies with
// g++ (-ffp-contract=off).  The method is not part of the reference tree; the yardstick is the numpy restatement of the contract in
// tests/grayrad_ref.py, held bit for bit (include/pam_amd_modules.h).
// Fields are (nz, ny, nx, nens), members fastest; inside a level a (column, member) has the flat index t = (j nx + i) nens + e.  zint
// (nz+1, nens) is per member.  IDX is the type of every element offset: unsigned while a field is below 2^29 doubles, long long beyond.
// Contraction into fma is switched off inside each body, so the device and the host give the same bits.  The exponential is the
// contract's own, pama::sgs::exp_c.
#pragma once

#include "sgs_device.h"      // exp_c, PAMA_D, PAMA_NO_CONTRACT

namespace pama {
namespace grayrad {

constexpr int MAX_SPECIES = 2;           // entries of the table of cloud-liquid densities, and of the table of cloud-ice densities
constexpr int AHEAD = 4;                 // levels whose loads are requested before the first of them is used

struct Params {
  double k_d, k_v, k_l, k_i;             // mass absorption coefficients [m2/kg], the diffusivity factor folded in
  double sigma, cp_d, lw_down_top, dt;
  int num_liquid, num_ice;
};

struct Fields {
  const double *rho_d, *rho_v, *liquid[MAX_SPECIES], *ice[MAX_SPECIES];
};

// the sum of a table at one cell: 0.0 of an empty one, else left to right
PAMA_D double species_sum(int n, double a, double b) {
  PAMA_NO_CONTRACT
  double s = 0.0;
  if (n > 0) s = a;
  if (n > 1) s = s + b;
  return s;
}

// t = exp_c(-dtau), dtau = (((k_d rho_d + k_v rho_v) + k_l L) + k_i I) dz; e = (sigma (T^2 T^2)) (1 - t)
PAMA_D void cell(const Params &P, double rho_d, double rho_v, double L, double I, double temp, double dz, double &t, double &e) {
  PAMA_NO_CONTRACT
  const double a = P.k_d * rho_d;
  const double b = P.k_v * rho_v;
  double c = a + b;
  c = c + P.k_l * L;
  c = c + P.k_i * I;
  const double dtau = c * dz;
  t = sgs::exp_c(-dtau);
  const double t2 = temp * temp;
  const double B = P.sigma * (t2 * t2);
  e = B * (1.0 - t);
}

// one step of either sweep: the flux that leaves the cell from the one that enters it
PAMA_D double attenuate(double flux, double t, double e) {
  PAMA_NO_CONTRACT
  return flux * t + e;
}

// what the upward sweep starts from
PAMA_D double surface_emission(double sigma, double ts) {
  PAMA_NO_CONTRACT
  const double t2 = ts * ts;
  return sigma * (t2 * t2);
}

PAMA_D double difference(double a, double b) {
  PAMA_NO_CONTRACT
  return a - b;
}

// heating = (parked + (U[k] - U[k+1])) / ((cp_d (rho_d + rho_v)) dz), parked = D[k+1] - D[k]
PAMA_D double heating_rate(const Params &P, double parked, double u_k, double u_p, double rho_d, double rho_v, double dz) {
  PAMA_NO_CONTRACT
  const double du = u_k - u_p;
  const double n = parked + du;
  const double rho = rho_d + rho_v;
  const double c = P.cp_d * rho;
  return n / (c * dz);
}

PAMA_D double apply(double temp, double heating, double dt) {
  PAMA_NO_CONTRACT
  return temp + heating * dt;
}

// both sweeps of one (column, member).  temp, heating and the fields of F point at element 0 and get off + k level; zint points at (0, e)
// with stride zs; sfc_temp (NULL: the lowest level's temp), olr, down_sfc and up_sfc point at element 0 and get off.
// Downward, k = nz-1 .. 0: D[k] = D[k+1] t_k + e_k from D[nz] = lw_down_top; D[k+1] - D[k] is parked in heating(k).  Upward, k = 0 .. nz-1:
// t_k and e_k are formed again from the same inputs (temp(k) is still the one of entry: it is replaced only after level k has been
// read), U[k+1] = U[k] t_k + e_k from U[0] = sigma Ts^4, heating(k) is finished and, where dt != 0, temp(k) takes it.
// The loads of AHEAD levels are requested before the first of them is used.  Nothing that is written overlaps anything that is read
// but temp and heating themselves (the entry point refuses it)
template <class IDX>
PAMA_D void column(double *temp, const Fields &F, const double *zint, const double *sfc_temp, IDX off, IDX level, IDX zs, int nz,
                   const Params &P, double *heating, double *olr, double *down_sfc, double *up_sfc) {
  const double *rd = F.rho_d + off, *rv = F.rho_v + off;
  // an absent species points at rho_d and is never read
  const double *l0 = P.num_liquid > 0 ? F.liquid[0] + off : rd, *l1 = P.num_liquid > 1 ? F.liquid[1] + off : rd;
  const double *i0 = P.num_ice > 0 ? F.ice[0] + off : rd, *i1 = P.num_ice > 1 ? F.ice[1] + off : rd;
  double *T = temp + off, *H = heating + off;
  const double ts = sfc_temp ? sfc_temp[off] : T[0];

  double D = P.lw_down_top, zi_p = zint[(IDX)nz * zs];
  for (int k0 = nz - 1; k0 >= 0; k0 -= AHEAD) {
    double a_rd[AHEAD], a_rv[AHEAD], a_L[AHEAD], a_I[AHEAD], a_T[AHEAD], a_zi[AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const IDX kc = (IDX)(k0 - b > 0 ? k0 - b : 0), o = kc * level;
      a_rd[b] = rd[o]; a_rv[b] = rv[o]; a_T[b] = T[o];
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
      double t, e;
      cell(P, a_rd[b], a_rv[b], a_L[b], a_I[b], a_T[b], difference(zi_p, a_zi[b]), t, e);
      const double Dk = attenuate(D, t, e);
      H[(IDX)k * level] = difference(D, Dk);
      D = Dk;
      zi_p = a_zi[b];
    }
  }
  down_sfc[off] = D;

  double U = surface_emission(P.sigma, ts), zi_k = zint[0];
  up_sfc[off] = U;
  for (int k0 = 0; k0 < nz; k0 += AHEAD) {
    double a_rd[AHEAD], a_rv[AHEAD], a_L[AHEAD], a_I[AHEAD], a_T[AHEAD], a_zi[AHEAD], a_H[AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const IDX kc = (IDX)(k0 + b < nz ? k0 + b : nz - 1), o = kc * level;
      a_rd[b] = rd[o]; a_rv[b] = rv[o]; a_T[b] = T[o]; a_H[b] = H[o];
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
      const double dz = difference(a_zi[b], zi_k);
      double t, e;
      cell(P, a_rd[b], a_rv[b], a_L[b], a_I[b], a_T[b], dz, t, e);
      const double Up = attenuate(U, t, e);
      const double h = heating_rate(P, a_H[b], U, Up, a_rd[b], a_rv[b], dz);
      H[(IDX)k * level] = h;
      if (P.dt != 0.0) T[(IDX)k * level] = apply(a_T[b], h, P.dt);
      U = Up;
      zi_k = a_zi[b];
    }
  }
  olr[off] = U;
}

}  // namespace grayrad
}  // namespace pama
