// ice1m_device.h -- the arithmetic of the one-moment ice microphysics (option micro = "ice1m"): five water species (vapour, cloud
// liquid, cloud ice, rain, snow) as mass densities, sedimentation of rain, snow and cloud ice in per-column sub-cycles, and in every
// cell melting, freezing, a saturation adjustment over a liquid/ice mixture, collection, riming, evaporation and sublimation.  Device
// functions that are plain inline C++ outside hipcc: the HIP kernel in modules_kernels.hip calls them, and tests/emu/ice1m_emu.cpp
// compiles the same bodies with g++ (-ffp-contract=off).  The method is not part of the reference tree; the yardstick is the numpy
// restatement of the contract in tests/ice1m_ref.py, held bit for bit (include/pam_amd_modules.h at pam_amd_ice1m_time_step, DESIGN.md
// section 8).  Fields are (nz, ny, nx, nens), members fastest; zint is (nz + 1, nens).  A thread owns a (column, member): `off` is its
// offset into level 0, `level` = ny nx nens the stride of a level, `zs` = nens the stride of a row of zint.
// Contraction into fma is switched off inside each body; divisions and square roots are IEEE; the only transcendental is the contract's
// exp_c; there is no pow: every exponent is a chain of square roots.
#pragma once

#include <cmath>

#include "sgs_device.h"      // exp_c; msa_device.h: PAMA_D, PAMA_NO_CONTRACT

namespace pama {
namespace ice1m {

constexpr int AHEAD = 4;                 // levels whose loads are requested before the first of them is used
constexpr int MAX_SUB = 64;              // the cap of the sub-cycle count
constexpr double CFL = 0.8;              // the Courant number a sub-cycle may reach
constexpr double T0 = 273.16, TH = 233.16, TW = 253.16;      // melting point, homogeneous freezing, where the liquid fraction w begins
constexpr double LV = 2.5e6, LS = 2.834e6, LF = LS - LV;

PAMA_D double s8(double x) { return std::sqrt(std::sqrt(std::sqrt(x))); }      // x^(1/8)
PAMA_D double s16(double x) { return std::sqrt(s8(x)); }                       // x^(1/16)
PAMA_D double pos(double x) { return x < 0.0 ? 0.0 : x; }                      // max(x, 0) that keeps a NaN
PAMA_D double least(double a, double b) { return b < a ? b : a; }              // min(a, b) that keeps a NaN a

// p875(q) = q / s8(q) and p8125(q) = q / s16(q)^3, both 0 at q == 0
PAMA_D double p875(double q) {
  PAMA_NO_CONTRACT
  return q == 0.0 ? 0.0 : q / s8(q);
}
PAMA_D double p8125(double q) {
  PAMA_NO_CONTRACT
  if (q == 0.0) return 0.0;
  const double t = s16(q);
  return q / ((t * t) * t);
}

struct Fall { double r, s, i; };         // of rain, snow and cloud ice: a speed or a flux

// v_r = (13.1 s8(rr)) fac, v_s = (1.7 s16(rs)) fac, v_i = 0.4 where ri > 0 (else 0.0); fac = sqrt(rho0 / (rd + rv))
PAMA_D Fall speeds(double rr, double rs, double ri, double rd, double rv, double rho0) {
  PAMA_NO_CONTRACT
  const double rho = rd + rv;
  const double fac = std::sqrt(rho0 / rho);
  Fall v;
  v.r = (13.1 * s8(rr)) * fac;
  v.s = (1.7 * s16(rs)) * fac;
  v.i = ri > 0.0 ? 0.4 : 0.0;
  return v;
}

// c raised to the greatest (v dt) / dz of the three; a NaN takes c over and stays
PAMA_D double courant(const Fall &v, double dt, double dz, double c) {
  PAMA_NO_CONTRACT
  const double x[3] = {(v.r * dt) / dz, (v.s * dt) / dz, (v.i * dt) / dz};
  for (int i = 0; i < 3; i++)
    if (x[i] > c || x[i] != x[i]) c = x[i];
  return c;
}

// 1 where c <= 0.8 or c is a NaN, else min(ceil(c / 0.8), 64)
PAMA_D int sub_cycles(double c) {
  PAMA_NO_CONTRACT
  if (!(c > CFL)) return 1;
  const double n = std::ceil(c / CFL);
  return n >= (double)MAX_SUB ? MAX_SUB : (int)n;
}

// the fluxes F_x = v_x r_x of one level, each speed clipped to vmax = ((0.8 dz) nsub) / dt
PAMA_D Fall fluxes(double rr, double rs, double ri, double rd, double rv, double rho0, double dz, double dt, double nsub) {
  PAMA_NO_CONTRACT
  const Fall v = speeds(rr, rs, ri, rd, rv, rho0);
  const double vmax = ((CFL * dz) * nsub) / dt;
  Fall F;
  F.r = (v.r > vmax ? vmax : v.r) * rr;
  F.s = (v.s > vmax ? vmax : v.s) * rs;
  F.i = (v.i > vmax ? vmax : v.i) * ri;
  return F;
}

// r + q (F_above - F), q = dts / dz
PAMA_D double settle(double r, double q, double f_above, double f) {
  PAMA_NO_CONTRACT
  const double d = f_above - f;
  return r + q * d;
}

// the share of a surface rate of one sub-cycle: (F dts) / (1000 dt)
PAMA_D double surface_rate(double f, double dts, double dt) {
  PAMA_NO_CONTRACT
  return (f * dts) / (1000.0 * dt);
}

struct Cell { double rv, rc, ri, rr, rs, T; };
struct Sat { double tc, rsw, rsi; };

// rsw = esw / (R_v T), esw = 610.94 exp_c((17.625 tc) / (243.04 + tc)); rsi = esi / (R_v T), esi = 611.21 exp_c((22.587 tc) / (273.86 + tc));
// tc = T - 273.15 as saturation_ratio has it
PAMA_D Sat saturation(double T, double R_v) {
  PAMA_NO_CONTRACT
  Sat S;
  S.tc = T - 273.15;
  const double rvt = R_v * T;
  const double xw = (17.625 * S.tc) / (243.04 + S.tc);
  const double esw = 610.94 * sgs::exp_c(xw);
  S.rsw = esw / rvt;
  const double xi = (22.587 * S.tc) / (273.86 + S.tc);
  const double esi = 611.21 * sgs::exp_c(xi);
  S.rsi = esi / rvt;
  return S;
}

// melt (T > T0): cloud ice to cloud liquid, then snow to rain, limited by H = (cprd (T - T0)) / Lf
PAMA_D void melt(Cell &c, double cprd) {
  PAMA_NO_CONTRACT
  if (!(c.T > T0)) return;
  const double H = (cprd * (c.T - T0)) / LF;
  const double mi = least(c.ri, H);
  c.ri = c.ri - mi;
  c.rc = c.rc + mi;
  const double H2 = H - mi;
  const double ms = least(c.rs, H2);
  c.rs = c.rs - ms;
  c.rr = c.rr + ms;
  c.T = c.T - (LF * (mi + ms)) / cprd;
}

// freeze (T < Th): cloud liquid to cloud ice, then rain to snow, limited by H = (cprd (Th - T)) / Lf
PAMA_D void freeze(Cell &c, double cprd) {
  PAMA_NO_CONTRACT
  if (!(c.T < TH)) return;
  const double H = (cprd * (TH - c.T)) / LF;
  const double fc = least(c.rc, H);
  c.rc = c.rc - fc;
  c.ri = c.ri + fc;
  const double H2 = H - fc;
  const double fr = least(c.rr, H2);
  c.rr = c.rr - fr;
  c.rs = c.rs + fr;
  c.T = c.T + (LF * (fc + fr)) / cprd;
}

// one Newton step towards rsat = rsi + w (rsw - rsi), w = clamp((T - 253.16) / 20, 0, 1), the dw/dT term neglected
PAMA_D void adjust(Cell &c, double cprd, double R_v) {
  PAMA_NO_CONTRACT
  const Sat S = saturation(c.T, R_v);
  const double w0 = (c.T - TW) / 20.0;
  const double w = w0 < 0.0 ? 0.0 : (w0 > 1.0 ? 1.0 : w0);
  const double omw = 1.0 - w;
  const double rsat = S.rsi + w * (S.rsw - S.rsi);
  const double L = w * LV + omw * LS;
  const double rT = 1.0 / c.T;
  const double bw = 243.04 + S.tc, bi = 273.86 + S.tc;
  const double sw = (17.625 * 243.04) / (bw * bw) - rT;
  const double si = (22.587 * 273.86) / (bi * bi) - rT;
  const double slope = (w * S.rsw) * sw + (omw * S.rsi) * si;
  const double x = (c.rv - rsat) / (1.0 + (L / cprd) * slope);
  if (x > 0.0) {
    const double dc = w * x;
    const double di = x - dc;
    c.rv = c.rv - x;
    c.rc = c.rc + dc;
    c.ri = c.ri + di;
    c.T = c.T + (LV * dc + LS * di) / cprd;
  } else if (x < 0.0) {
    const double e = least(-x, c.rc + c.ri);
    const double el = least(e, c.rc);
    const double ei = least(e - el, c.ri);
    c.rc = c.rc - el;
    c.ri = c.ri - ei;
    c.rv = c.rv + (el + ei);
    c.T = c.T - (LV * el + LS * ei) / cprd;
  }
}

// Kessler's implicit form: autoconversion and accretion of liquid to rain, of ice to snow (g = exp_c(0.025 (T - T0))), and riming of
// cloud liquid onto snow where T < T0.  pr and ps are formed once, from rr and rs as they enter
PAMA_D void collect(Cell &c, double rd, double cprd, double dt) {
  PAMA_NO_CONTRACT
  const double pr = p875(c.rr / rd);
  const double ps = p8125(c.rs / rd);
  const double dtk = dt * 1.0e-3;
  const double a = pos(c.rc - 1.0e-3 * rd);
  const double rc1 = pos(c.rc - dtk * a) / (1.0 + (dt * 2.2) * pr);
  c.rr = c.rr + (c.rc - rc1);
  c.rc = rc1;
  const double g = sgs::exp_c(0.025 * (c.T - T0));
  const double b = pos(c.ri - 1.0e-4 * rd);
  const double ri1 = pos(c.ri - (dtk * g) * b) / (1.0 + (dt * g) * ps);
  c.rs = c.rs + (c.ri - ri1);
  c.ri = ri1;
  if (c.T < T0) {
    const double rc2 = c.rc / (1.0 + (dt * 2.0) * ps);
    const double dr = c.rc - rc2;
    c.rs = c.rs + dr;
    c.rc = rc2;
    c.T = c.T + (LF * dr) / cprd;
  }
}

// what a precipitating species r loses to a subsaturated vapour: the least of r, 0.5 (rsat - rv) and ((dt coef) (1 - rv / rsat)) sqrt(r)
PAMA_D double loss(double r, double rv, double rsat, double dt, double coef) {
  PAMA_NO_CONTRACT
  const double half = 0.5 * (rsat - rv);
  const double rate = ((dt * coef) * (1.0 - rv / rsat)) * std::sqrt(r);
  return least(least(r, half), rate);
}

// rain evaporates against rsw (1e-4, Lv), then snow sublimates against rsi (5e-5, Ls); both at the T the step begins with
PAMA_D void evaporate(Cell &c, double cprd, double R_v, double dt) {
  PAMA_NO_CONTRACT
  const Sat S = saturation(c.T, R_v);
  if (c.rv < S.rsw && c.rr > 0.0) {
    const double l = loss(c.rr, c.rv, S.rsw, dt, 1.0e-4);
    c.rr = c.rr - l;
    c.rv = c.rv + l;
    c.T = c.T - (LV * l) / cprd;
  }
  if (c.rv < S.rsi && c.rs > 0.0) {
    const double l = loss(c.rs, c.rv, S.rsi, dt, 5.0e-5);
    c.rs = c.rs - l;
    c.rv = c.rv + l;
    c.T = c.T - (LS * l) / cprd;
  }
}

// the local processes of one cell, in the contract's order
PAMA_D void local(Cell &c, double rd, double dt, double cp_d, double R_v) {
  PAMA_NO_CONTRACT
  const double cprd = cp_d * rd;
  melt(c, cprd);
  freeze(c, cprd);
  adjust(c, cprd, R_v);
  collect(c, rd, cprd, dt);
  evaporate(c, cprd, R_v, dt);
}

// what a launch is given.  Every pointer points at element 0 of its array
struct Args {
  double *rv, *rc, *ri, *rr, *rs, *temp, *precl, *preci;
  const double *rd, *zint;
  double dt, R_v, cp_d;
};

// the read-only pre-pass: the sub-cycle count of one (column, member) from the state at entry
template <class IDX>
PAMA_D int count_sub_cycles(const Args &A, IDX off, IDX level, IDX zs, int e, int nz, double rho0) {
  PAMA_NO_CONTRACT
  const double *RV = A.rv + off, *RI = A.ri + off, *RR = A.rr + off, *RS = A.rs + off, *RD = A.rd + off, *Z = A.zint + e;
  double c = 0.0, z_lo = Z[0];
  for (int k0 = 0; k0 < nz; k0 += AHEAD) {
    double a_rv[AHEAD], a_ri[AHEAD], a_rr[AHEAD], a_rs[AHEAD], a_rd[AHEAD], a_z[AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const IDX k = (IDX)(k0 + b < nz ? k0 + b : nz - 1);
      const IDX o = k * level;
      a_rv[b] = RV[o]; a_ri[b] = RI[o]; a_rr[b] = RR[o]; a_rs[b] = RS[o]; a_rd[b] = RD[o];
      a_z[b] = Z[(k + 1) * zs];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      if (k0 + b >= nz) break;
      const Fall v = speeds(a_rr[b], a_rs[b], a_ri[b], a_rd[b], a_rv[b], rho0);
      c = courant(v, A.dt, a_z[b] - z_lo, c);
      z_lo = a_z[b];
    }
  }
  return sub_cycles(c);
}

// one sub-cycle of one (column, member): an upward pass in place.  The values of the level itself are carried in registers; the loads
// are those of levels k0 + 1 .. k0 + AHEAD, still old, which give F(k + 1).  LAST: the local processes of the cell follow its
// sedimentation, and all six fields are stored; otherwise only the three falling species are read and written
template <class IDX, bool LAST>
PAMA_D void pass(const Args &A, IDX off, IDX level, IDX zs, int e, int nz, double nsub, double dts, double rho0, double &pl, double &pi) {
  PAMA_NO_CONTRACT
  double *RV = A.rv + off, *RC = A.rc + off, *RI = A.ri + off, *RR = A.rr + off, *RS = A.rs + off, *T = A.temp + off;
  const double *RD = A.rd + off, *Z = A.zint + e;
  double c_rv = RV[0], c_ri = RI[0], c_rr = RR[0], c_rs = RS[0], c_rd = RD[0], c_rc = 0.0, c_t = 0.0;
  if (LAST) { c_rc = RC[0]; c_t = T[0]; }
  double z_lo = Z[0], z_hi = Z[zs];
  Fall F = fluxes(c_rr, c_rs, c_ri, c_rd, c_rv, rho0, z_hi - z_lo, A.dt, nsub);
  pl = pl + surface_rate(F.r, dts, A.dt);
  pi = pi + surface_rate(F.s + F.i, dts, A.dt);
  for (int k0 = 0; k0 < nz; k0 += AHEAD) {
    double a_rv[AHEAD], a_ri[AHEAD], a_rr[AHEAD], a_rs[AHEAD], a_rd[AHEAD], a_rc[AHEAD], a_t[AHEAD], a_z[AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const IDX kf = (IDX)(k0 + b + 1 < nz ? k0 + b + 1 : nz - 1);      // the level above, whose fields are loaded
      const IDX o = kf * level;
      a_rv[b] = RV[o]; a_ri[b] = RI[o]; a_rr[b] = RR[o]; a_rs[b] = RS[o]; a_rd[b] = RD[o];
      a_rc[b] = LAST ? RC[o] : 0.0;
      a_t[b] = LAST ? T[o] : 0.0;
      a_z[b] = Z[(kf + 1) * zs];                                         // its upper interface
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const int k = k0 + b;
      if (k >= nz) break;
      const IDX o = (IDX)k * level;
      Fall Fn{0.0, 0.0, 0.0};
      if (k < nz - 1) Fn = fluxes(a_rr[b], a_rs[b], a_ri[b], a_rd[b], a_rv[b], rho0, a_z[b] - z_hi, A.dt, nsub);
      const double q = dts / (z_hi - z_lo);
      Cell c;
      c.rr = settle(c_rr, q, Fn.r, F.r);
      c.rs = settle(c_rs, q, Fn.s, F.s);
      c.ri = settle(c_ri, q, Fn.i, F.i);
      if (LAST) {
        c.rv = c_rv; c.rc = c_rc; c.T = c_t;
        local(c, c_rd, A.dt, A.cp_d, A.R_v);
        RV[o] = c.rv; RC[o] = c.rc; T[o] = c.T;
      }
      RI[o] = c.ri; RR[o] = c.rr; RS[o] = c.rs;
      c_rv = a_rv[b]; c_ri = a_ri[b]; c_rr = a_rr[b]; c_rs = a_rs[b]; c_rd = a_rd[b]; c_rc = a_rc[b]; c_t = a_t[b];
      z_lo = z_hi; z_hi = a_z[b];
      F = Fn;
    }
  }
}

// the whole of one (column, member).  dt == 0: no field is read or written, and both rates are +0.0
template <class IDX>
PAMA_D void column(const Args &A, IDX off, IDX level, IDX zs, int e, int nz) {
  PAMA_NO_CONTRACT
  double pl = 0.0, pi = 0.0;
  if (A.dt != 0.0) {
    const double rho0 = A.rd[off] + A.rv[off];
    const int nsub = count_sub_cycles<IDX>(A, off, level, zs, e, nz, rho0);
    const double dts = A.dt / (double)nsub;
    for (int s = 0; s < nsub - 1; s++) pass<IDX, false>(A, off, level, zs, e, nz, (double)nsub, dts, rho0, pl, pi);
    pass<IDX, true>(A, off, level, zs, e, nz, (double)nsub, dts, rho0, pl, pi);
  }
  A.precl[off] = pl;
  A.preci[off] = pi;
}

}  // namespace ice1m
}  // namespace pama
