// kessler_device.h -- per-column arithmetic of the Kessler microphysics kernels (physics/micro/kessler/Microphysics.h:120-268
// timeStep, :346-457 kessler()), as PAMA_D functions: the HIP kernels in modules_kernels.hip call them (they keep the LDS staging of
// the pow tables, the wavefront shuffle and the atomic minimum), and tests/emu/kessler_emu.cpp compiles the same bodies with g++
// (-ffp-contract=off).  The host build differs from the device's in three places only: fast_rcp is a true divide there, the
// compiler does not contract a * b + c into fma, and exp / sqrt are glibc's -- so the two agree to rounding, not bit for bit.
// Columns are independent; col = (j*nx+i)*nens+e is the fastest index of every (nz, ncol) array, so consecutive lanes
// read consecutive doubles at every level.
#pragma once
#include <math.h>
#include <string.h>

#include "awfl_device.h"   // pow_pos_fast + its tables, fast_rcp

namespace pama {
namespace kessler {

// Every x^y of the scheme has a non-negative base: it goes through pow_pos_fast (awfl_device.h: ~65 instructions, 0.52 ulp against
// 80-bit powl, 0 -> 0) instead of the device library's pow (~260-440 instructions, half of them for negative / special bases) -- six of
// them per cell and sub-cycle made the column kernel VALU-bound (round 5: 4.2 -> 2.9 ms per timeStep at 1024 x 32x32x60).  T: its
// tables, staged in LDS by the kernels (two dependent per-lane look-ups per pow).
PAMA_D double kpow(double x, double y, const PowTab *T) { return pow_pos_fast(x, y, T); }
PAMA_D double krcp(double x) { return fast_rcp(x); }
PAMA_D double kdiv(double a, double b) { return a * fast_rcp(b); }
// x^y (y > 0) where the base is an amount of rain: most cells of most columns hold none and 0^y = 0 exactly, so a wavefront without rain
// skips the evaluation (a branch over ~65 instructions: taken per wavefront); any other base -- negative and NaN included -- goes
// through kpow as before.  Same values either way.
PAMA_D double kpow_rain(double x, double y, const PowTab *T) {
  double r = 0.0;
  if (x != 0.0) r = kpow(x, y, T);
  return r;
}
PAMA_D double kessler_velqr(double qr, double r, double rhalf, const PowTab *T) {
  return 36.34 * kpow_rain(qr * r, 0.1364, T) * rhalf;   // :375, :449
}

// The sedimentation time-step limit of kessler "main 1" (:376-386, the input of the global minimum :389-390) of ONE column over the
// levels k0, k0 + kstep, ... < nz - 1; touches nothing.  Returns the bit pattern of the smallest dt2d: positive doubles order like
// their bit patterns; ~0 = no level looked at; 0 = "this state is not usable" (NaN or negative fall speed), which wins every
// minimum and fails the host's "limit must be positive" test.
PAMA_D unsigned long long kessler_limit_column(int nz, long long ncol, int nens, long long col, unsigned k0, unsigned kstep,
                                               const double *__restrict__ rho_r, const double *__restrict__ rho_dry,
                                               const double *__restrict__ zmid, double dt, const PowTab *PT) {
  unsigned long long bits = ~0ull;
  const int e = (int)(col % nens);
  const double rho0 = rho_dry[col];
  for (int k = k0; k < nz - 1; k += kstep) {
    const long long idx = (long long)k * ncol + col;
    const double rho = rho_dry[idx];
    const double qr = rho_r[idx] / rho;
    const double velqr = kessler_velqr(qr, 0.001 * rho, sqrt(rho0 / rho), PT);
    double dt2d = dt;
    if (velqr > 1.e-10) dt2d = 0.8 * (zmid[(long long)(k + 1) * nens + e] - zmid[(long long)k * nens + e]) / velqr;
    unsigned long long db;
#if defined(__HIP_DEVICE_COMPILE__)
    db = (unsigned long long)__double_as_longlong(dt2d);
#else
    memcpy(&db, &dt2d, 8);
#endif
    const unsigned long long b = (velqr >= 0 && dt2d > 0) ? db : 0ull;
    bits = b < bits ? b : bits;
  }
  return bits;
}

// The whole of timeStep for one column: the conversions :167-174 (densities -> mixing ratios, T -> theta through the Exner
// function of the incoming state), kessler "main 2" + "main 3" (:394-453) for all sub-cycles, the conversions back :243-250.  One
// thread marches one column upwards: sed(k) needs the not-yet-adjusted values of levels k and k+1, which an upward march has at
// hand.  The FIRST sub-cycle reads the coupler's arrays as they came (rounds 4-5 converted them in place in a kernel of their own:
// 11 more array passes of the 26); the LAST writes densities and temperature.  SINGLE (one sub-cycle, the usual case): nothing else
// is stored.  Otherwise the mixing ratios and theta live IN PLACE in the coupler arrays between sub-cycles and the Exner function
// of the incoming state in `exner` (nz x ncol doubles of scratch).  velqr, r, rhalf, pc are pure functions of stored values and are
// recomputed (bitwise the same as the reference's stored temporaries).
// IDX: unsigned when a field is below 2^29 doubles (one register of offset for all six arrays on top of their scalar bases).
template <bool SINGLE, class IDX>
PAMA_D void kessler_column(int nz, long long ncol, int nens, long long col_, double *qv_a, double *qc_a, double *qr_a,
                           const double *__restrict__ rho_dry, double *theta_a, double *precl, const double *__restrict__ zmid,
                           double *exner, double dt, int rainsplit, double Rd, double Rv, double cp, double p0, const PowTab *PT) {
  const IDX col = (IDX)col_, nc = (IDX)ncol;
  const int e = (int)(col_ % nens);
  const double psl = p0 / 100, rhoqr = 1000., lv = 2.5e6, rp0 = 1 / p0;
  const double dt0 = dt / (double)rainsplit;   // (uniform: scalar-side IEEE divisions stay)
  const double rho0 = rho_dry[col];
  double pr = 0;                                                                  // timeStep :176 precl = 0
  for (int nt = 0; nt < (SINGLE ? 1 : rainsplit); nt++) {
    const bool first = SINGLE || nt == 0, last = SINGLE || nt == rainsplit - 1;
    // level-k values carried from the previous iteration's "k+1" loads
    double rho_k = rho0, z_k = zmid[e], qr_k = qr_a[col];
    if (first) qr_k = kdiv(qr_k, rho_k);                                               // :169
    double r_k = 0.001 * rho_k, rhalf_k = sqrt(kdiv(rho0, rho_k));
    double vel_k = kessler_velqr(qr_k, r_k, rhalf_k, PT);
    double z_km1 = 0;
    pr = pr + rho0 * qr_k * vel_k / rhoqr;   // (a constant divisor: the compiler's reciprocal)                                       // :397
    for (int k = 0; k < nz; k++) {
      const IDX idx = (IDX)k * nc + col;
      double sed, rho_n = 0, z_n = 0, qr_n = 0, r_n = 0, rhalf_n = 0, vel_n = 0;
      if (k == nz - 1) {
        sed = kdiv(-dt0 * qr_k * vel_k, 0.5 * (z_k - z_km1));                        // :400
      } else {
        rho_n = rho_dry[idx + nc]; z_n = zmid[(long long)(k + 1) * nens + e]; qr_n = qr_a[idx + nc];
        if (first) qr_n = kdiv(qr_n, rho_n);
        r_n = 0.001 * rho_n; rhalf_n = sqrt(kdiv(rho0, rho_n));
        vel_n = kessler_velqr(qr_n, r_n, rhalf_n, PT);
        sed = kdiv(dt0 * (r_n * qr_n * vel_n - r_k * qr_k * vel_k), r_k * (z_n - z_k));   // :403
      }
      double qc = qc_a[idx], qv = qv_a[idx], theta = theta_a[idx], qr = qr_k, pk, pnorm = 0;
      if (first) {                                                                // :167-174
        const double rv = qv, T = theta;
        const double pressure = Rd * rho_k * T + Rv * rv * T;
        pnorm = pressure * rp0;
        pk = kpow(pnorm, Rd / cp, PT);
        const double rrho = krcp(rho_k);
        qv = rv * rrho; qc = qc * rrho; theta = kdiv(T, pk);
        if (!SINGLE) exner[idx] = pk;
      } else {
        pk = exner[idx];
      }
      // :374 pc = 3.8 / (pk^(cp/Rd) psl).  pk^(cp/Rd) IS pressure / p0 up to the rounding of two pows (a few ulp): where the pressure
      // is at hand (a first sub-cycle) the pow is not taken
      const double pc = kdiv(3.8, (first ? pnorm : kpow(pk, cp / Rd, PT)) * psl);
      // autoconversion and accretion (:412-414)
      const double qrprod = qc - kdiv(qc - dt0 * fmax(0.001 * (qc - 0.001), 0.), 1 + dt0 * 2.2 * kpow_rain(qr, 0.875, PT));
      qc = fmax(qc - qrprod, 0.);
      qr = fmax(qr + qrprod + sed, 0.);
      // saturation vapour mixing ratio (:417-422)
      const double tmp = pk * theta - 36.;
      const double rtmp = krcp(tmp);
      const double qvs = pc * exp(17.27 * (pk * theta - 273.) * rtmp);
      const double prod = kdiv(qv - qvs, 1. + qvs * (4093. * lv / cp) * (rtmp * rtmp));
      // evaporation of rain (:425-430)
      const double rq = r_k * qr;
      const double rqvs = krcp(qvs);
      double rq_a = 0.0, rq_b = 0.0;                            // rq^0.2046, rq^0.525: one logarithm for the two; none without rain
      if (rq != 0.0) {
        const PowLog2 lrq = pow_log2_dd(rq, PT);
        rq_a = pow_exp2_dd(rq, 0.2046, lrq, PT);
        rq_b = pow_exp2_dd(rq, 0.525, lrq, PT);
      }
      const double tmp1 = dt0 * kdiv((1.6 + 124.9 * rq_a) * rq_b, 2550000. * pc * (rqvs * (1 / 3.8)) + 540000.) *
                          (fmax(qvs - qv, 0.) * kdiv(rqvs, r_k));
      const double tmp2 = fmax(-prod - qc, 0.);
      const double ern = fmin(tmp1, fmin(tmp2, qr));
      // saturation adjustment (:433-439)
      const double cond = fmax(prod, -qc);
      theta = theta + kdiv(lv, cp * pk) * (cond - ern);
      qv = fmax(qv - cond + ern, 0.);
      qc = qc + cond;
      qr = qr - ern;
      if (last) {   // timeStep :243-250 (temp from the OLD Exner function)
        qv_a[idx] = qv * rho_k; qc_a[idx] = qc * rho_k; qr_a[idx] = qr * rho_k; theta_a[idx] = theta * pk;
      } else {
        qv_a[idx] = qv; qc_a[idx] = qc; qr_a[idx] = qr; theta_a[idx] = theta;
      }
      z_km1 = z_k;
      rho_k = rho_n; z_k = z_n; qr_k = qr_n; r_k = r_n; rhalf_k = rhalf_n; vel_k = vel_n;
    }
  }
  precl[col] = pr / (double)rainsplit;                                            // :452
}

}  // namespace kessler
}  // namespace pama
