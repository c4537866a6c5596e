// surface_device.h -- the arithmetic of the bulk surface fluxes over a slab ocean (a bulk aerodynamic scheme with the closed-form
// stability functions of Louis 1979, and a slab of water that takes the net energy), as device functions that are plain inline C++
// outside hipcc: the HIP kernel in modules_kernels.hip calls them, and tests/emu/surface_emu.cpp compiles the same bodies with g++
// (-ffp-contract=off).  The method is not part of the reference tree; the yardstick is the numpy restatement of the contract in
// tests/surface_ref.py, held bit for bit (include/pam_amd_modules.h at pam_amd_surface_fluxes).
// Only level 0 of the (nz, ny, nx, nens) fields is read, so the offset of a thread's (row, column, member) into every array is its own
// flat index t = (j nx + i) nens + e: one index width serves, and no product with a level exists that a narrower one would save.
// zmid row 0, cn and cstar (nens) are per member.  Contraction into fma is switched off inside each body, so the device and the host
// give the same bits.  The only transcendental is the contract's own exponential, through pama::sgs::saturation_ratio.
#pragma once

#include "sgs_device.h"      // saturation_ratio over exp_c; msa_device.h: PAMA_D, PAMA_NO_CONTRACT

namespace pama {
namespace surface {

struct Params {
  double gust, wetness, grav, gc, cp_d, R_v, latvap;      // gc = grav / cp_d, formed once on the host (sgs::ratio)
  double cap, dt;                                         // slab_heat_capacity [J/m2/K]
};

// w = sqrt((u u + v v) + gust gust)
PAMA_D double wind(double u, double v, double gust) {
  PAMA_NO_CONTRACT
  const double a = u * u;
  const double b = v * v;
  const double s = a + b;
  const double g = gust * gust;
  return std::sqrt(s + g);
}

// t (1 + 0.608 q)
PAMA_D double virt(double t, double q) {
  PAMA_NO_CONTRACT
  const double a = 0.608 * q;
  const double f = 1.0 + a;
  return t * f;
}

// rib = ((grav z) (tva - tvs)) / (tvs (w w))
PAMA_D double richardson(double grav, double z, double tva, double tvs, double w) {
  PAMA_NO_CONTRACT
  const double gz = grav * z;
  const double d = tva - tvs;
  const double n = gz * d;
  const double ww = w * w;
  return n / (tvs * ww);
}

// Louis 1979: unstable 1 - (9.4 rib) / (1 + cstar sqrt(-rib)); else 1 / ((1 + 4.7 rib) (1 + 4.7 rib)).  A NaN rib is not < 0, takes the
// second branch and stays a NaN
PAMA_D double stability_function(double rib, double cstar) {
  PAMA_NO_CONTRACT
  if (rib < 0.0) {
    const double n = 9.4 * rib;
    const double r = std::sqrt(-rib);
    const double d = 1.0 + cstar * r;
    return 1.0 - n / d;
  }
  const double d = 1.0 + 4.7 * rib;
  return 1.0 / (d * d);
}

// ((rho c) (ch w)) (a - b): both fluxes, W/m2, positive upward
PAMA_D double bulk(double rho, double c, double ch, double w, double a, double b) {
  PAMA_NO_CONTRACT
  const double rc = rho * c;
  const double cw = ch * w;
  const double d = a - b;
  return (rc * cw) * d;
}

PAMA_D double difference(double a, double b) {
  PAMA_NO_CONTRACT
  return a - b;
}

// Ts + (dt (((sw) + (lw)) - (shf + lhf))) / cap
PAMA_D double slab_step(double Ts, double sw, double lw, double shf, double lhf, double dt, double cap) {
  PAMA_NO_CONTRACT
  const double r = sw + lw;
  const double t = shf + lhf;
  const double net = r - t;
  const double e = dt * net;
  return Ts + e / cap;
}

// one (row, column, member): every pointer points at the element itself (level 0 of the fields at t, zmid, cn, cstar at e).  Every load
// is requested before the first value is used; the saturation exponential is most of the arithmetic.  SLAB: sfc_temp is stepped after
// the fluxes, which come from its value at entry; lw_down and sw_down are NULL in pairs with lw_up and sw_up, and an absent pair
// contributes exactly 0.0 (the same choice for every thread of a launch).  Without SLAB no radiation input is read and sfc_temp is
// not written
template <bool SLAB>
PAMA_D void column(const double *temp, const double *rho_d, const double *rho_v, const double *uvel, const double *vvel, const double *zmid,
                   const double *cn, const double *cstar, double *sfc_temp, const double *lw_down, const double *lw_up, const double *sw_down,
                   const double *sw_up, const Params &P, double *sfc_shf, double *sfc_lhf) {
  PAMA_NO_CONTRACT
  const double T = *temp, rd = *rho_d, rv = *rho_v, u = *uvel, v = *vvel, Ts = *sfc_temp, z = *zmid, c_n = *cn, c_s = *cstar;
  double lwd = 0.0, lwu = 0.0, swd = 0.0, swu = 0.0;
  if constexpr (SLAB) {
    if (lw_down) { lwd = *lw_down; lwu = *lw_up; }
    if (sw_down) { swd = *sw_down; swu = *sw_up; }
  }
  const double rho = rd + rv;
  const double qv = rv / rho;
  const double w = wind(u, v, P.gust);
  const double sa = T + P.gc * z;
  const double qs = P.wetness * sgs::saturation_ratio(Ts, rho, P.R_v);
  const double tva = virt(sa, qv), tvs = virt(Ts, qs);
  const double rib = richardson(P.grav, z, tva, tvs, w);
  const double ch = c_n * stability_function(rib, c_s);
  const double shf = bulk(rho, P.cp_d, ch, w, Ts, sa);
  const double lhf = bulk(rho, P.latvap, ch, w, qs, qv);
  *sfc_shf = shf;
  *sfc_lhf = lhf;
  if constexpr (SLAB) {
    const double sw = sw_down ? difference(swd, swu) : 0.0;
    const double lw = lw_down ? difference(lwd, lwu) : 0.0;
    *sfc_temp = slab_step(Ts, sw, lw, shf, lhf, P.dt, P.cap);
  }
}

}  // namespace surface
}  // namespace pama
