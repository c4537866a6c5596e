// awfl_device.h -- device-side arithmetic of the MI355X-native AWFL dycore step (gfx950, fp64).
//
// Kernel BODIES live here as device functions taking explicit (line / cell, member) coordinates; the
// __global__ wrappers are in awfl_kernels.hip.  The same bodies are compiled by g++ into the host-side
// emulation harness under tests/emu/ (test infrastructure only: it lets the index logic be checked against
// the oracle without a GPU; the product library never contains or calls it).
//
// What is computed (reference: E3SM-Project/PAM dynamics/awfl/Dycore.h, WenoLimiter.h):
//   * weno5_*            WenoLimiter.h:98-181 compute_weno_coefs<5> + Dycore.h:591-604 reconstruct, restated as
//                        ONE polynomial per cell evaluated at both cell edges (the reference evaluates the same
//                        polynomial twice, once from each adjacent face, Dycore.h:345-359).
//   * flux_line_body     Dycore.h:334-519: acoustic characteristic upwind + advective upwind fluxes.
//   * fct_mult_body      Dycore.h:525-550: FCT positivity limiter, expressed as a per-cell multiplier.
//   * update_body        Dycore.h:553-584 (flux divergence + gravity), :162-221 (SSPRK3 combines, clipping,
//                        next FCT seed), fused with the NEXT stage's Dycore.h:310-321 (pressure, divide by rho)
//                        and :662-710 (vertical ghost cells).
//   * flux_x_update_body the fused x-sweep of the default stage: x fluxes + the complete update of the state and of water vapour
//                        (Dycore.h:334-386, :553-584, :162-221, :525-550); x_tracer_sweep: the further tracers, swept twice
//                        (FCT multipliers, then the complete update); tracer_fixup_line_body, pressure_tail_body: the tail.
//   * pow_pos_fast       every x^y of the step (positive bases): Dycore.h:310-321, :682-709, :1313-1387.
//   * init_prim_body     Dycore.h:1370-1387 (coupler -> dycore state), :130-134 (clip), fused with :310-321,:662-710.
//   * coupler_to_halo_arrays_body / halo_arrays_to_coupler_body   the two converts with the reference's argument lists
//                        (Dycore.h:1336-1388, :1281-1331).
//   * finalize_body      Dycore.h:1313-1330 (dycore state -> coupler).
//   * cfl_body           Dycore.h:86-101.
//   * pint_body / hydro_mean_body   Dycore.h:1450-1501 (declare_current_profile_as_hydrostatic).
//
// Data layout (all fp64, nens fastest, as the coupler: pam_coupler.h:259-263):
//   prim[f][kz][j][i][e]   f: 0 rho, 1 pressure, 2 u, 3 v, 4 w, 5 theta, 6.. tracer mixing ratios (rho_t/rho)
//                          kz in [0, nz+6): 3 ghost levels below and above (x,y are periodic: index wrap, no halo)
//   flux_d[l][face][..][e] l: 0 mass flux, 1 u, 2 v, 3 w, 4 theta, 5.. tracers.  x: nx faces (face nx == face 0),
//                          y: ny faces, z: nz+1 faces.
//   seed[t][k][j][i][e]    FCT "mass available" seed (Dycore.h:156-159,173,197) -- also the exact conserved rho_t.
//   mult[t][k][j][i][e]    FCT multiplier of the cell (1 when not limited).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "awfl_constants.h"

#if defined(__HIPCC__)
#define PAMA_D __device__ __forceinline__
#else
#define PAMA_D inline
#endif

namespace pama {

constexpr int HS = 3;          // ghost levels (Dycore.h:23)
constexpr int MAXT = 50;       // pam_const.h:24 max_fields
constexpr int FLUX_THREADS = 256;
constexpr int FLUX_WAVES = FLUX_THREADS / 64;
#ifndef PAMA_FLUX_NF
#define PAMA_FLUX_NF 2
#endif
constexpr int FLUX_NF = PAMA_FLUX_NF;   // advected fields swept together (independent polynomial chains per iteration)
constexpr int FLUX_MAX_SPAN = 64; // longest span one wavefront sweeps without a cut (a 61-face column, a 64-cell line)
constexpr int VZ_STRIDE = 31;  // per-level vertical table in difference form (struct VTable)

enum PrimField { P_RHO = 0, P_PRES = 1, P_U = 2, P_V = 3, P_W = 4, P_THETA = 5, P_TR0 = 6 };

struct TracerPtrs { double *p[MAXT]; };

struct Params {
  int nens, nx, ny, nz, nt;
  int sim2d;          // ny == 1 (Dycore.h:279)
  int grav_balance;   // option balance_hydrostasis_with_gravity (Dycore.h:284)
  int vz_per_ens;     // 0: vertical matrices identical for every ensemble member (wave-uniform table)
  int seg;            // shortest span a sweep line may be cut into when the ensemble alone does not fill the chip
  int flat_cells;     // pointwise kernels: the launch grid is flat over every cell (small ensembles: nx*nens does not fill a workgroup)
  double dx, dy, rdx, rdy;
  double C0, gamma, grav, R_d, R_v;
  long long sx, sy, sz;   // cell strides in doubles: nens, nx*nens, ny*nx*nens
  long long prim_fs;      // (nz+6)*sz
  long long ncell;        // nz*sz
  long long fz_fs;        // (nz+1)*sz
  const double *dz;       // (nz,nens)
  const double *grav_var; // (nz,nens)
  const double *hy_dens;  // (nz,nens)
  const double *hy_pres;  // (nz,nens)
  const double *vz;       // vertical difference-form tables: (nz+2,VZ_STRIDE) or (nz+2,VZ_STRIDE,nens)
  const struct PowTab *pw;   // tables of pow_pos_fast
  unsigned long long pos_mask, mass_mask;  // tracer_positive / tracer_adds_mass bit sets
  int idWV;
  int yz_fold;            // fused stage, 3-D member lanes: the z sweep adds the y differences of the state variables to its own and stores
                          // ONE field per variable, the y+z part of the divergence (yz_divergence); the x-sweep loads that field only
  const double *rdz;      // (nz,nens) fast_rcp(dz), formed once on the device (the z sweep of a folded stage reads it level by level)
};

// ------------------------------------------------------------------------------------------------
// reciprocal: v_rcp_f64 seed + two Newton steps (error ~1 ulp); the host emulation uses a true divide.
PAMA_D double fast_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  double y = __builtin_amdgcn_rcp(x);
  double r = fma(-x, y, 1.0);
  y = fma(y, r, y);
  r = fma(-x, y, 1.0);
  y = fma(y, r, y);
  return y;
#else
  return 1.0 / x;
#endif
}

// reciprocal for the two WENO weight normalisations: one Newton step (measured on gfx950, tools/probe/rcp_precision.hip:
// v_rcp_f64 alone 4.6e-8, one step 2.2e-15, two steps exact).  A relative error e in a normalisation factor moves an edge
// value by ~e x (spread of the candidate polynomials at the edge), far below one ulp of the value itself.
PAMA_D double weno_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  double y = __builtin_amdgcn_rcp(x);
  double r = fma(-x, y, 1.0);
  return fma(y, r, y);
#else
  return 1.0 / x;
#endif
}

// x^y for x > 0 -- every pow of the step has a density, a potential temperature or a pressure as its base, and the pressure pass
// of a stage (Dycore.h:310-321: p = C0 (rho theta)^gamma in every cell) is nothing but this function.  The device library's
// pow() costs 440 vector instructions (half of them for negative / special bases and integer exponents), its powr() 214; this
// one ~75, with a smaller error: 0.52 ulp measured against 80-bit powl over 3.6e6 samples (tests/test_pow_pos.py; glibc: 0.51).
//   x = m 2^e, m in [1,2); the top 7 mantissa bits pick c_i = 1 + (i + 1/2)/128 from a table: r = m/c_i - 1 in ONE fma
//   (1/c_i is stored with 24 bits, so the rounding of the fma is 2^-53 |r|, |r| <= 2^-8);
//   log2 x = (e + lh_i) + r/ln2 + [ll_i + r^2 q(r)]: -log2(1/c_i) = lh_i + ll_i with lh_i a multiple of 2^-32 (e + lh_i is exact),
//   r/ln2 as an exact product (fma residual) against a two-word 1/ln2, the leading two terms added with a two-sum -> a double-double;
//   z = y log2 x, again with the fma residual; z = k/64 + f, |f| <= 2^-7: 2^z = 2^(k>>6) T_(k&63) (1 + P(f)), T_j = 2^(j/64) in two words.
// The tables (PowTab: 128 x 3 + 64 x 2 doubles) are built once per handle on the host in 80-bit arithmetic (awfl_vertical.h).
struct PowLog { double ic, lh, ll; };
struct PowExp { double th, tl; };
struct PowTab { PowLog lg[128]; PowExp ex[64]; };
// the two halves of x^y, for callers that raise ONE base to several exponents (the Kessler column kernel): log2 x as a double-double,
// then 2^(y log2 x).  pow_pos_fast is their composition, operation for operation what it was as one function.
struct PowLog2 { double hi, lo; };
PAMA_D PowLog2 pow_log2_dd(double x, const PowTab *T) {
#pragma clang fp contract(off)
  int e;
  double m = frexp(x, &e) * 2.0;                            // x = m 2^e, m in [1, 2)
  e -= 1;
  unsigned long long bits;
#if defined(__HIP_DEVICE_COMPILE__)
  bits = (unsigned long long)__double_as_longlong(m);
#else
  memcpy(&bits, &m, 8);
#endif
  const int i = (int)((bits >> 45) & 127ull);
  const double ic = T->lg[i].ic, lh = T->lg[i].lh, ll = T->lg[i].ll;
  const double r = fma(m, ic, -1.0);
  const double Khi = 1.4426950408889634, Klo = 2.0355273740931033e-17;      // 1/ln 2
  const double th = r * Khi;
  double tl = fma(r, Khi, -th);
  tl = fma(r, Klo, tl);
  double q = -0.18033688011112042;                          // log2(1+r) - r/ln2 = r^2 q(r): -K/8, K/7, ... -K/2
  q = fma(q, r, 0.20609929155556620);
  q = fma(q, r, -0.24044917348149390);
  q = fma(q, r, 0.28853900817779268);
  q = fma(q, r, -0.36067376022224085);
  q = fma(q, r, 0.48089834696298783);
  q = fma(q, r, -0.72134752044448170);
  const double lo = fma(r * r, q, tl + ll);
  const double A = (double)e + lh;                          // exact
  const double s = A + th, bb = s - A;                      // two-sum
  const double err = (A - (s - bb)) + (th - bb);
  PowLog2 L;
  L.hi = s; L.lo = err + lo;
  return L;
}
PAMA_D double pow_exp2_dd(double x, double y, const PowLog2 L, const PowTab *T) {
#pragma clang fp contract(off)
  const double zh = y * L.hi;
  double zl = fma(y, L.hi, -zh);
  zl = fma(y, L.lo, zl);
  const double kd = rint(zh * 64.0);
  double f = fma(kd, -0.015625, zh);                        // exact
  f += zl;
  double p = 1.5403530393381609e-4;                         // 2^f - 1 = f (ln2 + f (ln2^2/2 + ... + f ln2^6/720))
  p = fma(p, f, 1.3333558146428443e-3);
  p = fma(p, f, 9.6181291076284772e-3);
  p = fma(p, f, 5.5504108664821580e-2);
  p = fma(p, f, 2.4022650695910071e-1);
  p = fma(p, f, 6.9314718055994531e-1);
  p = p * f;
  // a base that is not positive and finite only occurs in a state that has already blown up: keep the C library's answers
  // (0 -> 0 and +inf -> +inf for y > 0, the other way round for y < 0; negative or NaN -> NaN) -- decided BEFORE kd is converted
  // to an integer (a NaN / infinite kd would be undefined behaviour in the host build of this function)
  if (!(x > 0.0)) return (x == 0.0) ? (y > 0.0 ? 0.0 : INFINITY) : NAN;
  if (!(x < INFINITY)) return y > 0.0 ? INFINITY : 0.0;
  // (x finite and positive from here on: |log2 x| <= 1075, so kd = 64 y log2 x fits an int for every |y| < 3e4 -- the step's exponents
  // are gamma, gamma - 1 and their reciprocals)
  const int k = (int)kd;
  const int j = k & 63, n = k >> 6;                         // k = 64 n + j, 0 <= j < 64 (arithmetic shift)
  const double t2h = T->ex[j].th, t2l = T->ex[j].tl;
  return ldexp(fma(t2h, p, t2l) + t2h, n);
}
PAMA_D double pow_pos_fast(double x, double y, const PowTab *T) { return pow_exp2_dd(x, y, pow_log2_dd(x, T), T); }

PAMA_D double pow_pos(const Params &P, double x, double y) { return pow_pos_fast(x, y, P.pw); }

// Convexified ideal weights (WenoLimiter.h:39-44 + :94), sigma, and derived constants.
struct WenoConsts {
  double idl[4], sigma, ridl3;
  double c0[4], c1[4], c2[4], idl3x[4];   // map_weights pieces: idl+idl^2, 1-2idl, idl^2, 3*idl
};
PAMA_D WenoConsts weno_consts() {
  WenoConsts w;
  const double raw[4] = AWFL_WENO_IDL_INIT;
  double sum = ((raw[0] + raw[1]) + raw[2]) + raw[3];
  for (int i = 0; i < 4; i++) w.idl[i] = raw[i] / (sum + 1.0e-20);
  w.sigma = AWFL_WENO_SIGMA;
  w.ridl3 = 1.0 / w.idl[3];
  for (int i = 0; i < 4; i++) {
    w.c0[i] = w.idl[i] + w.idl[i] * w.idl[i];
    w.c1[i] = 1.0 - 2.0 * w.idl[i];
    w.c2[i] = w.idl[i] * w.idl[i];
    w.idl3x[i] = 3.0 * w.idl[i];
  }
#if defined(__HIP_DEVICE_COMPILE__)
  // The addends of map_weights' multiply-adds for weights 1 and 3 (weights 0 and 2 share theirs: idl0 == idl2) do not fit the scalar
  // file beside the other literals of a sweep, and the compiler keeps them in vector registers.  As KNOWN constants it rebuilds each
  // one in the destination of its v_fmac (a v_mov_b64 per use: 6 of ~135 vector instructions per polynomial); as opaque values
  // it reads them as the third operand of a v_fma.  Same arithmetic, same bits.
  asm("" : "+v"(w.idl3x[1]), "+v"(w.c0[1]), "+v"(w.c2[1]), "+v"(w.idl3x[3]), "+v"(w.c0[3]), "+v"(w.c2[3]));
  // c2 of weights 0 and 2 meets a second constant in its multiply-add (c1 w + c2: one scalar operand per instruction): same cure
  asm("" : "+v"(w.c2[0]));
  if (raw[0] == raw[2]) w.c2[2] = w.c2[0];
#endif
  return w;
}

// ------------------------------------------------------------------------------------------------
// WENO5 polynomial of one cell, evaluated at the left (x=-1/2) and right (x=+1/2) edge of the cell.
//
// Same algorithm as WenoLimiter.h:98-181 + Dycore.h:591-604, re-expressed in DIFFERENCE FORM: with
// d_m = u_m - u_{m-1} (m = 1..4), every non-constant coefficient of every candidate polynomial is a linear form in
// the d_m only (a constant field has a constant polynomial), and the constant coefficient is the centre value plus a
// linear form in the d_m (the polynomial reproduces the centre cell average).  The candidates therefore need
// 12 + 16 multiply-adds instead of 27 + 25, the constant coefficients are never formed, and
//      even = u2 + sum_i w_i E_i ,  odd = sum_i w_i O_i ,  left = even - odd ,  right = even + odd
// with E_i = (a0_i - u2) + a2_i/4 (+ a4/16), O_i = a1_i/2 (+ a3/8).  The bridge polynomial (WenoLimiter.h:128-136) is
// linear in the stencil and is folded into the upper-polynomial coefficients.
// Non-linear part (WenoLimiter.h:141-180: TV, sigma blend, weights, convexify, map, convexify, weighted sum): weno5_table (vertical)
// and weno5_const (uniform grid) form the TVs, both end in weno5_tail.
// UNIFORM (constant-matrix directions): the x^2 coefficient of every lower candidate is half the second difference, so
// a2 holds the second difference itself and the factor 1/4 moves into the TV constant.
// Every multiply-add below has an explicit rounding point (fma = one rounding; nothing else is contracted): the same
// source must give the same bits in every kernel it is inlined into (x/y/z sweeps, the fused x-sweep, the KAT hook), and the
// backend's own contraction choices depend on the surrounding code (seen on gfx950: tv*tv + 1e-20 fused in one kernel and
// not in another -- visible only where tv^2 ~ 1e-20, i.e. at the edges of tracer blobs).
// UNIFORM, scaling: the total variation of a lower candidate is a1^2 + K2U (2 a2)^2 with K2U = 13/12.  weno5_const forms every
// x coefficient (a1 of the candidates, h1..h4 of the upper polynomial) with literal factors, so it delivers them divided by
// sqrt(K2U) at no cost: all four TVs then come out divided by K2U -- a1'^2 + (2 a2)^2 is one multiply and one fma instead of two
// multiplies and an fma, three instructions per polynomial less -- and the weights, which are ratios of 1/(tv^2 + eps), are those of
// the unscaled TVs when the two eps constants carry the factor (tv^2 + eps = K2U^2 (tv'^2 + eps / K2U^2); the eps added to the sum
// of the unnormalised weights gets K2U^2).  The odd part and the upper polynomial's share of the even part are linear in the scaled
// coefficients: the factor moves into their constants.
constexpr double csqrt_(double v) {      // compile-time square root (Newton; v > 0)
  double x = v > 1.0 ? v : 1.0;
  for (int i = 0; i < 200; i++) x = 0.5 * (x + v / x);
  return x;
}
constexpr double WENO_K2U = 0.25 * AWFL_TV3_A2A2;            // uniform grid: a2 holds the second difference = 2 a2
constexpr double WENO_SQRT_K2U = csqrt_(WENO_K2U), WENO_RSQRT_K2U = 1.0 / WENO_SQRT_K2U;
// Weights with the ideal weights folded into the denominators: w_i = idl_i/d_i / (sum_k idl_k/d_k + eps) is unchanged when every
// idl_k/d_k is replaced by idl_0/d_k' with d_k' = d_k idl_k/idl_0 and the eps by eps/idl_0.  idl_0 == idl_2 (checked below), so only
// d_1' and d_3' carry a factor, and it rides on the tv^2 term of their multiply-add (tv (tv r) + eps r): two multiplies instead of
// the four idl_i x_i products.
constexpr double weno_idl_c(int i) {
  constexpr double raw[4] = AWFL_WENO_IDL_INIT;
  return raw[i] / ((((raw[0] + raw[1]) + raw[2]) + raw[3]) + 1.0e-20);   // the same arithmetic as weno_consts
}
constexpr double WENO_R1 = weno_idl_c(0) / weno_idl_c(1), WENO_R3 = weno_idl_c(0) / weno_idl_c(3);
static_assert(weno_idl_c(0) == weno_idl_c(2), "weights 0 and 2 share their ideal weight");
constexpr double WENO_BLEND_LO = (1.0 - AWFL_WENO_SIGMA) / 3.0;   // tv3 = lo_avg + (tv3 - lo_avg) sigma = LO (tv0+tv1+tv2) + sigma tv3

// The tail of every polynomial: from the four (folded) denominators d_i' to the two edge values.
//   w_i = x_i / (x_0 + x_1 + x_2 + x_3 + eps' d_0'd_1'd_2'd_3'),  x_i = prod_{k != i} d_k'   (one reciprocal, WenoLimiter.h:163-166);
//   the eps term is x_3 d_3' eps', added as x_3 (1 + eps' d_3').  The eps added to the SUM matters when the TVs are large (pressure
//   stencils: sum ~ 1e-17), so it is kept.
//   map_weights (WenoLimiter.h:11-19) then convexify, again with one reciprocal; the normalisation 1/sum(m) is applied to the two
//   weighted sums instead of to the four weights.
//   lo_e / lo_o: the lower candidates' even / odd parts (sum_i m_i a2_i, sum_i m_i a1_i); e3 / o3: those of the upper polynomial,
//   each multiplied by m3; kse: the factor of lo_e in the even part; codd: the factor of the odd part.
PAMA_D void weno5_tail(double u2, double d0, double d1, double d2, double d3, double eps_sum, const double (&a1)[3],
                       const double (&a2)[3], double e3, double o3, double kse, double codd, const WenoConsts &wc, double &left,
                       double &right) {
#pragma clang fp contract(off)
  const double p01 = d0 * d1, p23 = d2 * d3;
  const double x0 = d1 * p23, x1 = d0 * p23, x2 = d3 * p01, x3 = d2 * p01;
  const double rs = weno_rcp(fma(x3, fma(eps_sum, d3, 1.0), (x0 + x1) + x2));
  const double xx[4] = {x0, x1, x2, x3};
  double num[4], den[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const double w = xx[i] * rs;
    num[i] = w * fma(w, fma(xx[i], rs, -wc.idl3x[i]), wc.c0[i]);     // w (c0 + w (w - 3 idl))
    den[i] = fma(wc.c1[i], w, wc.c2[i]);
  }
  const double q01 = den[0] * den[1], q23 = den[2] * den[3];
  const double y0 = den[1] * q23, y1 = den[0] * q23, y2 = den[3] * q01, y3 = den[2] * q01;
  const double m0 = num[0] * y0, m1 = num[1] * y1, m2 = num[2] * y2, m3 = num[3] * y3;
  const double rm = weno_rcp(fma(num[3], y3, fma(num[2], y2, fma(num[1], y1, m0))));
  // even part.  Every candidate reproduces the average of the centre cell, which in the candidates' coordinate is centred
  // at 0 with width w (1 on the uniform grid; dz(k)/dz(k-1) in the vertical, whose matrices are normalised by the cell
  // below): a0 + a2 w^2/12 (+ a4 w^4/80) = u2.  Its value at x = +-1/2 minus u2 is therefore
  // a2 (1/4 - w^2/12) (+ a4 (1/16 - w^4/80)) and needs no coefficients of its own.
  const double lo_e = fma(m0, a2[0], fma(m1, a2[1], m2 * a2[2]));
  const double se = fma(kse, lo_e, m3 * e3);
  // odd part: a1/2 (+ a3/8 for the upper polynomial); left / right = u2 + (se -+ codd so) / sum(m)
  const double so = fma(m3, o3, fma(m0, a1[0], fma(m1, a1[1], m2 * a1[2])));
  left = fma(rm, fma(-codd, so, se), u2);
  right = fma(rm, fma(codd, so, se), u2);
}

// Difference-form coefficient tables.  Lower candidate i uses (d_{i+1}, d_{i+2}); the upper polynomial uses d_1..d_4.
//   lo1[i][2], lo2[i][2]      x and x^2 coefficients of candidate i
//   hi[p-1][4]   p=1..4       bridged upper coefficients; the x^3 and x^4 rows are scaled by sqrt(39.1125), sqrt(625.8)
//                             (their weights in coefs_to_tv<5>)
//   k2, k4                    even-part factors 1/4 - w^2/12 and (1/16 - w^4/80)/sqrt(625.8), w = width of the centre cell
// The vertical tables store the factored form of this (VTable, make_vtable); the uniform grid uses it through make_uniform_upper.
struct DTable { double lo1[3][2], lo2[3][2], hi[4][4], k2, k4; };

// conversion of a stencil-form linear functional  sum_s c_s u_{s0+s}  (cells s0..s0+n-1 of the 5-stencil, centre = 2)
// to difference form: coefficient of d_m (m = 1..4), dropping (sum c_s) u2 (=0 or u2, handled by the caller).
//   u0-u2 = -d1-d2, u1-u2 = -d2, u3-u2 = d3, u4-u2 = d3+d4
constexpr double dcoef(const double c[5], int m) {
  return m == 1 ? -c[0] : m == 2 ? -c[0] - c[1] : m == 3 ? c[3] + c[4] : c[4];
}

// Build the difference-form table from the stencil-form matrices recon_lo[i][s][ii] (vert_weno_recon_lower /
// TransformMatrices.h:1218) and recon_hi[s][ii] (vert_sten_to_coefs / TransformMatrices.h:970) and the ideal weights.
constexpr DTable make_dtable(const double lo[3][3][3], const double hi[5][5], const double idl[4], double w) {
  DTable t{};
  double lod[3][3][4] = {};   // [i][ii][m-1] full-width difference form of the lower candidates
  for (int i = 0; i < 3; i++)
    for (int ii = 0; ii < 3; ii++) {
      double c[5] = {0, 0, 0, 0, 0};
      for (int s = 0; s < 3; s++) c[i + s] = lo[i][s][ii];
      for (int m = 1; m <= 4; m++) lod[i][ii][m - 1] = dcoef(c, m);
    }
  double hid[5][4] = {};      // [ii][m-1]
  for (int ii = 0; ii < 5; ii++) {
    double c[5] = {hi[0][ii], hi[1][ii], hi[2][ii], hi[3][ii], hi[4][ii]};
    for (int m = 1; m <= 4; m++) {
      double v = dcoef(c, m);
      if (ii < 3)
        for (int i = 0; i < 3; i++) v -= idl[i] * lod[i][ii][m - 1];   // bridge, WenoLimiter.h:129-133
      hid[ii][m - 1] = v / idl[3];                                    // WenoLimiter.h:134-136
    }
  }
  for (int i = 0; i < 3; i++)
    for (int q = 0; q < 2; q++) {
      t.lo1[i][q] = lod[i][1][i + q];
      t.lo2[i][q] = lod[i][2][i + q];
    }
  for (int pp = 1; pp <= 4; pp++)
    for (int m = 0; m < 4; m++)
      t.hi[pp - 1][m] = hid[pp][m] * (pp == 3 ? AWFL_TV5_SQRT_A3A3 : (pp == 4 ? AWFL_TV5_SQRT_A4A4 : 1.0));
  t.k2 = 0.25 - w * w / 12.0;
  t.k4 = (0.0625 - w * w * w * w / 80.0) / AWFL_TV5_SQRT_A4A4;
  return t;
}

constexpr DTable make_const_dtable() {
  constexpr double S5[5][5] = AWFL_STEN_TO_COEFS_INIT;
  constexpr double W3[3][3][3] = AWFL_WENO_LOWER_INIT;
  constexpr double raw[4] = AWFL_WENO_IDL_INIT;
  double sum = ((raw[0] + raw[1]) + raw[2]) + raw[3];
  double idl[4] = {raw[0] / (sum + 1.0e-20), raw[1] / (sum + 1.0e-20), raw[2] / (sum + 1.0e-20), raw[3] / (sum + 1.0e-20)};
  return make_dtable(W3, S5, idl, 1.0);
}

constexpr double cabs_(double x) { return x < 0 ? -x : x; }

// The STORED vertical table of a level (awfl_vertical.h; VZ_STRIDE doubles in this order), made from the level's DTable:
//   lo1, lo2   the lower candidates' rows, lo2 times sqrt(13/3), the weight of a2^2 in coefs_to_tv<3> (TransformMatrices.h:188-193):
//              the candidates' TV is then a1^2 + a2'^2 -- one multiply and one fma -- and the even part, linear in a2', takes k2s
//   r          the upper polynomial's blended TV.  tvb = LO (tv0+tv1+tv2) + sigma tv3 (WenoLimiter.h:141-151) is one positive
//              definite quadratic form of the four differences (the lower TVs alone are: candidates 0 and 2 cover (d0, d1) and (d2, d3)),
//              stored as the rows of its Cholesky factor, times sqrt(R3) so that d3 = tvb'^2 + eps R3 needs no multiply of its own:
//                  tvb' = sqrt(R3) tvb = z0^2 + z1^2 + z2^2 + z3^2,   z0 = r0 . (d0..d3), z1 = r1 . (d1..d3), z2 = r2 . (d2, d3), z3 = r3 d3
//              -- 14 instructions, where h1..h4 (16), their TV (7) and the blend (3) took 26.  Every term is a square: nothing cancels.
//   e3, o3     the upper polynomial's even and odd parts, k2 h2 + k4 h4 and h1 + h3 / (4 sqrt(c3)), as rows of d
//   k2s        k2 / sqrt(13/3), the factor of the lower candidates' even part (their a2 is scaled)
struct VTable { double lo1[3][2], lo2[3][2], r[10], e3[4], o3[4], k2s; };
static_assert(sizeof(VTable) == VZ_STRIDE * sizeof(double), "VTable layout");

// piv: the four pivots of the factorisation (all > 0 for a positive definite form; awfl_vertical.h checks them).  root: the square
// root used for the scale factors and the pivots (std::sqrt on the host, csqrt_ at compile time).
template <class Root>
constexpr VTable make_vtable(const DTable &t, Root root, double (&piv)[4]) {
  VTable v{};
  const double sq = root(AWFL_TV3_A2A2);
  for (int i = 0; i < 3; i++)
    for (int q = 0; q < 2; q++) {
      v.lo1[i][q] = t.lo1[i][q];
      v.lo2[i][q] = t.lo2[i][q] * sq;
    }
  v.k2s = t.k2 / sq;
  constexpr double K13 = AWFL_TV5_A1A3 / AWFL_TV5_SQRT_A3A3, K24 = AWFL_TV5_A2A4 / AWFL_TV5_SQRT_A4A4;
  // the form sqrt(R3) tvb on d: LO x the lower TVs (stored rows), sigma x coefs_to_tv<5> of h1..h4 (TransformMatrices.h:871-876)
  const double s3 = root(WENO_R3), clo = s3 * WENO_BLEND_LO, chi = s3 * AWFL_WENO_SIGMA;
  double Q[4][4] = {};
  for (int i = 0; i < 3; i++) {
    double va[4] = {}, vb[4] = {};
    va[i] = v.lo1[i][0]; va[i + 1] = v.lo1[i][1];
    vb[i] = v.lo2[i][0]; vb[i + 1] = v.lo2[i][1];
    for (int a = 0; a < 4; a++)
      for (int b = 0; b < 4; b++) Q[a][b] += clo * (va[a] * va[b] + vb[a] * vb[b]);
  }
  const double(&h)[4][4] = t.hi;
  for (int a = 0; a < 4; a++)
    for (int b = 0; b < 4; b++)
      Q[a][b] += chi * (h[0][a] * h[0][b] + 0.5 * K13 * (h[0][a] * h[2][b] + h[2][a] * h[0][b]) + AWFL_TV5_A2A2 * h[1][a] * h[1][b] +
                        0.5 * K24 * (h[1][a] * h[3][b] + h[3][a] * h[1][b]) + h[2][a] * h[2][b] + h[3][a] * h[3][b]);
  // Cholesky, Q = R^T R with R upper triangular: row j of R is z_j's row
  double R[4][4] = {};
  for (int j = 0; j < 4; j++) {
    piv[j] = Q[j][j];
    const double s = piv[j] > 0.0 ? root(piv[j]) : 1.0;
    R[j][j] = s;
    for (int k = j + 1; k < 4; k++) R[j][k] = Q[j][k] / s;
    for (int a = j + 1; a < 4; a++)
      for (int b = j + 1; b < 4; b++) Q[a][b] -= R[j][a] * R[j][b];
  }
  int n = 0;
  for (int j = 0; j < 4; j++)
    for (int k = j; k < 4; k++) v.r[n++] = R[j][k];
  for (int m = 0; m < 4; m++) {
    v.e3[m] = t.k2 * t.hi[1][m] + t.k4 * t.hi[3][m];
    v.o3[m] = t.hi[0][m] + (0.25 / AWFL_TV5_SQRT_A3A3) * t.hi[2][m];
  }
  return v;
}

// compile-time proof of the cell-average identity weno5_tail relies on, on the generated uniform-grid constants:
// (a0 - u2) = -a2/12 for the lower candidates and -(a2/12 + a4/80) for the full quartic (stencil form, per stencil value)
constexpr bool uniform_even_identity_holds() {
  constexpr double S5[5][5] = AWFL_STEN_TO_COEFS_INIT;
  constexpr double W3[3][3][3] = AWFL_WENO_LOWER_INIT;
  for (int i = 0; i < 3; i++)
    for (int s_ = 0; s_ < 3; s_++) {
      const double centre = (i + s_ == 2) ? 1.0 : 0.0;
      if (cabs_(W3[i][s_][0] + W3[i][s_][2] / 12.0 - centre) > 1e-15) return false;
    }
  for (int s_ = 0; s_ < 5; s_++) {
    const double centre = (s_ == 2) ? 1.0 : 0.0;
    if (cabs_(S5[s_][0] + S5[s_][2] / 12.0 + S5[s_][4] / 80.0 - centre) > 1e-15) return false;
  }
  return true;
}
static_assert(uniform_even_identity_holds(), "uniform-grid candidates must reproduce the centre cell average");

// Horizontal directions: constant matrices (uniform grid).  All coefficients are compile-time literals, and the mirror
// symmetry of the uniform stencil (u_m -> u_{4-m}, i.e. d0 <-> -d3, d1 <-> -d2) splits every form of the polynomial into the sums
// and differences of the outer and inner first differences, s03 = d0+d3, s12 = d1+d2 (odd under the mirror) and t03 = d3-d0,
// a2_1 = d2-d1 (even).  The upper polynomial enters the step only through
//   * its blended TV  tvb = LO (tv0+tv1+tv2) + sigma tv3 (WenoLimiter.h:141-151), a quadratic form of d invariant under the mirror, so
//     without cross terms between (s03, s12) and (t03, a2_1): two 2x2 forms, each a sum of two squares (Cholesky).  Scaled by a
//     constant LAM (its 1/LAM^2 moves into d3's factor), and with the one-variable squares matched to tv1 = (S/2)^2 s12^2 + a2_1^2:
//         LAM tvb = l1^2 + l3^2 + tv1 + ETA a2_1^2,   l1 = A1 s03 + B1 s12,   l3 = A3 t03 + B3 a2_1
//     -- with l1, l3 seven instructions, where forming h1..h4, their TV and the blend took 19;
//   * its even and odd parts in the weighted sums: X = (h2 / 6 + a4 / 16 (scaled)) (t03, a2_1) and H = (h1 / 2 + h3 / 8) (s03, s12).
struct UniformUpper { double lam, a1, b1, a3, b3, eta, xt, xa, hs, hc, cross; };
constexpr UniformUpper make_uniform_upper() {
  constexpr DTable T = make_const_dtable();
  constexpr double S = WENO_RSQRT_K2U, K13 = AWFL_TV5_A1A3 / AWFL_TV5_SQRT_A3A3, K24 = AWFL_TV5_A2A4 / AWFL_TV5_SQRT_A4A4;
  // the quadratic form of tvb on d (every x coefficient divided by sqrt(K2U), a2 doubled: the scaling of the lower TVs)
  double Q[4][4] = {};
  for (int i = 0; i < 3; i++) {
    double va[4] = {}, vb[4] = {};
    va[i] = S * T.lo1[i][0]; va[i + 1] = S * T.lo1[i][1];
    vb[i] = -1.0; vb[i + 1] = 1.0;
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) Q[r][c] += WENO_BLEND_LO * (va[r] * va[c] + vb[r] * vb[c]);
  }
  double h[4][4] = {};
  for (int q = 0; q < 4; q++)
    for (int m = 0; m < 4; m++) h[q][m] = S * T.hi[q][m];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++)
      Q[r][c] += AWFL_WENO_SIGMA * (h[0][r] * h[0][c] + 0.5 * K13 * (h[0][r] * h[2][c] + h[2][r] * h[0][c]) +
                                    AWFL_TV5_A2A2 * h[1][r] * h[1][c] + 0.5 * K24 * (h[1][r] * h[3][c] + h[3][r] * h[1][c]) +
                                    h[2][r] * h[2][c] + h[3][r] * h[3][c]);
  // to the basis (s03, s12, t03, a2_1): d = P b
  const double P[4][4] = {{0.5, 0, -0.5, 0}, {0, 0.5, 0, -0.5}, {0, 0.5, 0, 0.5}, {0.5, 0, 0.5, 0}};
  double M[4][4] = {};
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++)
      for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) M[r][c] += P[a][r] * Q[a][b] * P[b][c];
  UniformUpper U{};
  const double ce = M[1][1] - M[0][1] * M[0][1] / M[0][0], co = M[3][3] - M[2][3] * M[2][3] / M[2][2];
  U.lam = 0.25 * S * S / ce;
  U.a1 = csqrt_(U.lam * M[0][0]); U.b1 = U.lam * M[0][1] / U.a1;
  U.a3 = csqrt_(U.lam * M[2][2]); U.b3 = U.lam * M[2][3] / U.a3;
  U.eta = U.lam * co - 1.0;
  // X = h2/6 + 0.05 h4/sqrt(c4) and H = h1 + 0.25 h3/sqrt(c3) (true coefficients; H then times S, the scale of the lower a1)
  double x[4] = {}, hh[4] = {};
  for (int m = 0; m < 4; m++) {
    x[m] = T.hi[1][m] / 6.0 + 0.05 * T.hi[3][m] / AWFL_TV5_SQRT_A4A4;
    hh[m] = S * (T.hi[0][m] + 0.25 * T.hi[2][m] / AWFL_TV5_SQRT_A3A3);
  }
  U.xt = x[3]; U.xa = x[2];     // X = xt t03 + xa a2_1 (antisymmetric)
  U.hs = hh[0]; U.hc = hh[1];   // H = hs s03 + hc s12  (symmetric)
  for (int r = 0; r < 2; r++)
    for (int c = 2; c < 4; c++) U.cross = cabs_(M[r][c]) > U.cross ? cabs_(M[r][c]) : U.cross;
  return U;
}
constexpr bool uniform_upper_ok() {
  // the blocks of tvb do not couple (mirror symmetry), and the odd block's residual square is positive
  constexpr UniformUpper U = make_uniform_upper();
  return U.cross < 1e-15 && U.lam > 0.0 && U.eta > -1.0 && U.a1 > 0.0 && U.a3 > 0.0;
}
static_assert(uniform_upper_ok(), "uniform-grid blended TV: positive definite blocks");

PAMA_D void weno5_const(const double u[5], const WenoConsts &wc, double &left, double &right) {
#pragma clang fp contract(off)
  constexpr DTable T = make_const_dtable();
  static_assert(T.hi[0][0] == T.hi[0][3] && T.hi[0][1] == T.hi[0][2], "x coefficient: symmetric");
  static_assert(T.hi[1][0] == -T.hi[1][3] && T.hi[1][1] == -T.hi[1][2], "x^2 coefficient: antisymmetric");
  static_assert(T.hi[2][0] == T.hi[2][3] && T.hi[2][1] == T.hi[2][2] && T.hi[2][0] == -T.hi[2][1], "x^3 coefficient");
  static_assert(T.hi[3][0] == -T.hi[3][3] && T.hi[3][1] == -T.hi[3][2] && cabs_(T.hi[3][1] + 3.0 * T.hi[3][0]) < 1e-14,
                "x^4 coefficient");
  static_assert(T.lo1[1][0] == 0.5 && T.lo1[1][1] == 0.5, "centred candidate slope");
  // on the uniform grid every lower candidate has a2 = (d_{i+1} - d_i)/2 exactly
  static_assert(T.lo2[0][0] == -0.5 && T.lo2[0][1] == 0.5 && T.lo2[1][0] == -0.5 && T.lo2[1][1] == 0.5 &&
                T.lo2[2][0] == -0.5 && T.lo2[2][1] == 0.5, "uniform-grid x^2 coefficients are half second differences");
  constexpr UniformUpper U = make_uniform_upper();
  constexpr double EPS_TV = 1.0e-20 / (WENO_K2U * WENO_K2U);      // added to tv^2 (the TVs are divided by K2U, see above weno5_tail)
  constexpr double EPS_SUM = 1.0e-20 * (WENO_K2U * WENO_K2U);     // added to the sum of the unnormalised weights
  const double d[4] = {u[1] - u[0], u[2] - u[1], u[3] - u[2], u[4] - u[3]};
  const double s03 = d[0] + d[3], s12 = d[1] + d[2], t03 = d[3] - d[0];
  double a1[3], a2[3];
  a2[0] = d[1] - d[0];
  a2[1] = d[2] - d[1];
  a2[2] = d[3] - d[2];
  constexpr double S = WENO_RSQRT_K2U;     // every x coefficient is delivered divided by sqrt(K2U) (see above weno5_tail)
  a1[0] = fma(S * T.lo1[0][1], d[1], (S * T.lo1[0][0]) * d[0]);
  a1[1] = (S * 0.5) * s12;
  a1[2] = fma(S * T.lo1[2][1], d[3], (S * T.lo1[2][0]) * d[2]);
  const double sq1 = a2[1] * a2[1];
  const double tv0 = fma(a1[0], a1[0], a2[0] * a2[0]), tv1 = fma(a1[1], a1[1], sq1), tv2 = fma(a1[2], a1[2], a2[2] * a2[2]);
  const double l1 = fma(U.a1, s03, U.b1 * s12), l3 = fma(U.a3, t03, U.b3 * a2[1]);
  const double tvb = fma(l1, l1, fma(l3, l3, fma(U.eta, sq1, tv1)));      // LAM x the blended TV of the upper polynomial
  constexpr double R3L = WENO_R3 / (U.lam * U.lam);
  const double d0 = fma(tv0, tv0, EPS_TV), d1 = fma(tv1, tv1 * WENO_R1, EPS_TV * WENO_R1);
  const double d2 = fma(tv2, tv2, EPS_TV), d3 = fma(tvb, tvb * R3L, EPS_TV * WENO_R3);
  weno5_tail(u[2], d0, d1, d2, d3, EPS_SUM / weno_idl_c(0), a1, a2, fma(U.xt, t03, U.xa * a2[1]), fma(U.hs, s03, U.hc * s12),
             1.0 / 12.0, 0.5 * WENO_SQRT_K2U, wc, left, right);
}

// Vertical direction: per-level difference-form table built at init from the cell-edge locations
// (Dycore.h:904-937 + TransformMatrices_variable.h -> awfl_vertical.h), used as Dycore.h:454-469.
// tab points at VZ_STRIDE doubles (struct VTable) with element stride `ts` (1 for the ensemble-uniform table, nens otherwise).
template <class TabPtr>
PAMA_D void weno5_table(const double u[5], TabPtr tab, long long ts, const WenoConsts &wc, double &left,
                        double &right) {
#pragma clang fp contract(off)
  constexpr double EPS_TV = 1.0e-20;    // added to tv^2
  const double d[4] = {u[1] - u[0], u[2] - u[1], u[3] - u[2], u[4] - u[3]};
  double a1[3], a2[3], tv[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    a1[i] = fma(tab[(1 + 2 * i) * ts], d[i + 1], tab[(0 + 2 * i) * ts] * d[i]);
    a2[i] = fma(tab[(7 + 2 * i) * ts], d[i + 1], tab[(6 + 2 * i) * ts] * d[i]);
    tv[i] = fma(a1[i], a1[i], a2[i] * a2[i]);
  }
  // sqrt(R3) x the blended TV of the upper polynomial, a sum of four squares (VTable)
  const double z0 = fma(tab[12 * ts], d[0], fma(tab[13 * ts], d[1], fma(tab[14 * ts], d[2], tab[15 * ts] * d[3])));
  const double z1 = fma(tab[16 * ts], d[1], fma(tab[17 * ts], d[2], tab[18 * ts] * d[3]));
  const double z2 = fma(tab[19 * ts], d[2], tab[20 * ts] * d[3]);
  const double z3 = tab[21 * ts] * d[3];
  const double tvb = fma(z0, z0, fma(z1, z1, fma(z2, z2, z3 * z3)));
  const double e3 = fma(tab[22 * ts], d[0], fma(tab[23 * ts], d[1], fma(tab[24 * ts], d[2], tab[25 * ts] * d[3])));
  const double o3 = fma(tab[26 * ts], d[0], fma(tab[27 * ts], d[1], fma(tab[28 * ts], d[2], tab[29 * ts] * d[3])));
  const double d0 = fma(tv[0], tv[0], EPS_TV), d1 = fma(tv[1], tv[1] * WENO_R1, EPS_TV * WENO_R1);
  const double d2 = fma(tv[2], tv[2], EPS_TV), d3 = fma(tvb, tvb, EPS_TV * WENO_R3);
  weno5_tail(u[2], d0, d1, d2, d3, 1.0e-20 / weno_idl_c(0), a1, a2, e3, o3, tab[30 * ts], 0.5, wc, left, right);
}

// The factored form of the constant (uniform-grid) table: positive pivots, and every stored coefficient finite
constexpr bool vertical_upper_ok() {
  double piv[4] = {};
  const VTable v = make_vtable(make_const_dtable(), csqrt_, piv);
  for (int j = 0; j < 4; j++)
    if (!(piv[j] > 0.0)) return false;
  for (int m = 0; m < 10; m++)
    if (!(cabs_(v.r[m]) < 1e100)) return false;
  return v.r[0] > 0.0 && v.r[4] > 0.0 && v.r[7] > 0.0 && v.r[9] > 0.0;
}
static_assert(vertical_upper_ok(), "vertical table: the blended TV of the uniform grid must factor with positive pivots");

// ------------------------------------------------------------------------------------------------
// Arithmetic shared by the unfused stage (flux kernel + update kernel) and the fused x-sweep (flux_x_update_body).  The two
// paths must produce the same bits, so every multiply-add here has an explicit rounding point: fma() where one rounding
// is meant, and no implicit contraction of anything else (the compiler's own contraction choices depend on the
// surrounding code, which differs between the two kernels).
//
// A product that is rounded on its own: never contracted into a neighbouring add/subtract (the AMDGPU backend fuses
// aggressively, also when the product has other uses -- and differently in different kernels).
PAMA_D double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}

// Acoustic characteristic flux at a face (Dycore.h:341-366, :477-496 for the vertical walls): face mass flux and pressure.
// The two characteristic variables are each one cell's: w1 comes from the left-edge values of the cell on the right of the face, w2 from
// the right-edge values of the cell on its left -- a sweep that meets the two cells far apart (the closing face of a periodic line)
// keeps w1 instead of the two edge values.
PAMA_D double acoustic_w1(double ru_R, double pp_R) {
#pragma clang fp contract(off)
  const double cs = 350.0;                                    // Dycore.h:335
  return 0.5 * fma(-cs, ru_R, pp_R);
}
PAMA_D double acoustic_w2(double ru_L, double pp_L) {
#pragma clang fp contract(off)
  const double cs = 350.0;
  return 0.5 * fma(cs, ru_L, pp_L);
}
PAMA_D void acoustic_face_w(double w1, double w2, bool wall, double &ruf, double &ppf) {
#pragma clang fp contract(off)
  const double rcs = 1.0 / 350.0;
  ppf = w1 + w2;
  ruf = (w2 - w1) * rcs;
  if (wall) ruf = 0.0;                                        // Dycore.h:496
}
PAMA_D void acoustic_face(double ru_L, double ru_R, double pp_L, double pp_R, bool wall, double &ruf, double &ppf) {
  if (wall) { ru_L = 0.0; ru_R = 0.0; }                       // Dycore.h:477,482
  acoustic_face_w(acoustic_w1(ru_R, pp_R), acoustic_w2(ru_L, pp_L), wall, ruf, ppf);
}

// -(dFx)/dx - (dFy)/dy - (dFz)/dz of one variable (Dycore.h:553-571), reciprocal multiplies (<= 1 ulp per term).  This association
// ((x + y) + z) is the one of the density and of every tracer.
PAMA_D double flux_divergence(const Params &P, double xlo, double xhi, double ylo, double yhi, double zlo, double zhi,
                              double rdzk) {
#pragma clang fp contract(off)
  double tend = (xlo - xhi) * P.rdx;
  if (!P.sim2d) tend = fma(ylo - yhi, P.rdy, tend);
  return fma(zlo - zhi, rdzk, tend);
}

// The momentum components and rho*theta in 3-D: x + (y + z).  The y+z part depends on nothing the x direction produces, so the z
// sweep of the fused stage can form it (it then reads the y sweep's differences instead of the x-sweep: P.yz_fold) and hand ONE field
// per variable to the x-sweep.  Every path -- folded or not, sweeps or tiles, the three-kernel stage, the host emulation -- forms it
// with this function, so they all agree bit for bit.  dyv / dzv = F[c] - F[c+1] of the y / z direction (what the DIFF sweeps store).
PAMA_D double yz_divergence(const Params &P, double dyv, double dzv, double rdzk) {
#pragma clang fp contract(off)
  return fma(dzv, rdzk, dyv * P.rdy);
}
// divergence of a state variable from its two x faces and the y+z part
PAMA_D double flux_divergence_g(const Params &P, double xlo, double xhi, double yz) {
#pragma clang fp contract(off)
  return fma(xlo - xhi, P.rdx, yz);
}
// the same from the y and z differences (2-D: there is no y part and the association stays (x + z))
PAMA_D double flux_divergence_d(const Params &P, double xlo, double xhi, double dyv, double dzv, double rdzk) {
#pragma clang fp contract(off)
  if (P.sim2d) return fma(dzv, rdzk, (xlo - xhi) * P.rdx);
  return flux_divergence_g(P, xlo, xhi, yz_divergence(P, dyv, dzv, rdzk));
}

// gravity source of the vertical momentum (Dycore.h:562-566): mode A -variable_gravity*rho, mode B -grav*(rho - hy_dens)
//   gcoef = gravity_coef(P, ke): the (level, member) entry the mode needs.  Sweeps that own a whole x line load it ONCE: inside the
//   loop the compiler cannot hoist it (its stores may alias anything) and the load sits at the end of a dependency chain,
//   where its full round trip -- behind every outstanding store -- stalls the wavefront once per cell.
PAMA_D double gravity_coef(const Params &P, long long ke) { return P.grav_balance ? P.grav_var[ke] : P.hy_dens[ke]; }
PAMA_D double add_gravity(const Params &P, double tend, double rho_in, double gcoef) {
#pragma clang fp contract(off)
  if (P.grav_balance) return fma(-gcoef, rho_in, tend);
  return fma(-P.grav, rho_in - gcoef, tend);
}

// SSPRK3 combines (Dycore.h:162-221):
//   STAGE 1: out = in' + dt T     STAGE 2: out = 3/4 q0' + 1/4 in' + 1/4 dt T     STAGE 3: out = 1/3 q0' + 2/3 in' + 2/3 dt T
template <int STAGE>
PAMA_D double rk_combine(double m_0, double m_in, double dt_dyn, double tend) {
#pragma clang fp contract(off)
  if (STAGE == 1) return fma(dt_dyn, tend, m_in);
  if (STAGE == 2) return fma((1.0 / 4.0) * dt_dyn, tend, fma(1.0 / 4.0, m_in, (3.0 / 4.0) * m_0));
  return fma((2.0 / 3.0) * dt_dyn, tend, fma(2.0 / 3.0, m_in, (1.0 / 3.0) * m_0));
}
// FCT seed of the next stage (Dycore.h:173-174,197-198); after stage 3 the exact conserved tracer mass
template <int STAGE>
PAMA_D double next_seed(double m_0, double m_in, double v) {
#pragma clang fp contract(off)
  if (STAGE == 1) return fma(1.0 / 4.0, v, (3.0 / 4.0) * m_in);
  if (STAGE == 2) return fma(2.0 / 3.0, v, (1.0 / 3.0) * m_0);
  return v;
}
// A lower bound L <= seed of the FCT seed that stage STAGE of a positive-definite tracer READS in a cell, from what that stage has in
// registers anyway: m_0 = mul_rn(q_0, rho_0) and m_in = mul_rn(q_in, rho_in), its own sub-step-start and stage-input masses (q_in, rho_in:
// the stage-input mixing ratio and density as loaded).  The x-sweep compares the mass leaving the cell with fct_mass_available(L) first
// and loads the seed only where that does not settle the answer (finish_tracer_cell); fct_mass_available is monotone, so
// mass_out <= available(L) implies mass_out <= available(seed): multiplier exactly 1, no flag, the very bits of the loading path.
// Holds for seeds made by THIS library's chain inside one timeStep: init_prim_body, then every stage's next_seed (state pass, fix-up
// pass, tile kernels, one-kernel update -- all through tracer_new_value).  A stage run on buffers the caller may have written
// (pam_amd_awfl_debug_stage) keeps the load.
//   STAGE 2  reads next_seed<1> = fma(1/4, v, (3/4) m_in') of stage 1, whose input IS this sub-step's start: m_in' = mul_rn of the same two
//            doubles as m_0, and (3/4) m_0 here is the very product there.  v = fmax(0, .) >= 0 (a NaN becomes 0), so the exact sum is
//            >= (3/4) m_0, a double, and rounding to nearest cannot go below a double that the exact value is not below.  L = (3/4) m_0.
//   STAGE 3  reads next_seed<2> = fma(2/3, v, (1/3) m_0) with the same m_0 (both stages combine with the sub-step's start): L = (1/3) m_0.
//            (m_0 a NaN: seed and L are NaN, fmax(NaN, 0) = 0 on both sides -- and the comparison sends the row to the load.)
//   STAGE 1  reads the conserved mass S >= 0 itself (init_prim_body: the clipped coupler value; next_seed<3>: the clipped v), while the
//            producer stored q_in = rn(S y), y = fast_rcp(rho_in) = (1 + e) / rho_in, and rho_in.  |e| <= 2^-52: v_rcp_f64 is good to
//            2^-23 at worst (measured 4.6e-8), a Newton step y(1 + rn(1 - x y)) squares the error and adds one rounding of the fma each
//            way, 2^-46 + 2^-53 after the first, < 2^-52 after the second (the host's 1/x: 2^-53).  Without underflow
//            m_in = S (1 + e)(1 + d1)(1 + d2), |d| <= 2^-53, so m_in < S (1 + 2^-50) and
//            L = rn(m_in (1 - 2^-48)) <= S (1 + 2^-50)(1 - 2^-48)(1 + 2^-53) < S.
//            "Without underflow" (or overflow) is checked, not assumed: 2^-900 <= q_in <= 2^900 and 2^-100 <= rho_in <= 2^100 put S y,
//            q_in rho_in and L a hundred binades inside the normal range (and send NaNs, zeros and negative densities the other way);
//            anything else gets L = 0 <= S -- a cell with no vapour at all, or a state no bound should be trusted on, loads its seed.
template <int STAGE>
PAMA_D double seed_lower_bound(double m_0, double m_in, double q_in, double rho_in) {
#pragma clang fp contract(off)
  if (STAGE == 2) return (3.0 / 4.0) * m_0;
  if (STAGE == 3) return (1.0 / 3.0) * m_0;
  const bool normal = (q_in >= 0x1p-900) & (q_in <= 0x1p900) & (rho_in >= 0x1p-100) & (rho_in <= 0x1p100);
  return normal ? m_in * (1.0 - 0x1p-48) : 0.0;
}

// ------------------------------------------------------------------------------------------------
// Wave-uniform addressing.  In the fused x-sweep every lane of a wavefront works on the SAME x line (k, j) and differs only
// in the ensemble member, so every address is  (uniform base)  +  member * 8 bytes.  uni()/uniw() tell the compiler that a
// pointer is wave-uniform (readfirstlane of an already-uniform value costs nothing): the base then lives in scalar
// registers, is advanced by the scalar unit, and the access becomes `global_load v, v_member_offset, s[base]` -- one VGPR of
// address for ALL streams instead of a 64-bit per-lane pointer (two VGPRs + vector adds) per stream.  ONLY for pointers
// that really are identical across the wavefront.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(1))) double *gc_ptr;
typedef __attribute__((address_space(1))) double *g_ptr;
PAMA_D gc_ptr uni(const double *p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (gc_ptr)(((unsigned long long)hi << 32) | lo);
}
PAMA_D g_ptr uniw(double *p) { return (g_ptr)uni(p); }
// a wave-uniform integer computed on the vector unit (e.g. a division) moved to a scalar register for good: the empty asm
// keeps the compiler from folding the readfirstlane away and continuing on the vector unit
// The ensemble-uniform vertical tables are written once in init and never by a kernel: read them through the constant
// address space so that they are fetched with scalar loads whatever stores the kernel makes through other pointers.
typedef const __attribute__((address_space(4))) double *const_ptr;
PAMA_D const_ptr as_constant(const double *p) { return (const_ptr)(unsigned long long)p; }
PAMA_D int uni_int(int v) {
  int r = __builtin_amdgcn_readfirstlane(v);
  asm volatile("" : "+s"(r));
  return r;
}
#else
typedef const double *gc_ptr;
typedef double *g_ptr;
PAMA_D gc_ptr uni(const double *p) { return p; }
PAMA_D g_ptr uniw(double *p) { return p; }
typedef const double *const_ptr;
PAMA_D const_ptr as_constant(const double *p) { return p; }
PAMA_D int uni_int(int v) { return v; }
#endif
// Streaming policy.  A stage moves ~37 GB through a 256 MB last-level cache, and the few lines that ARE read twice (the cells of the
// periodic wrap, the stage-input density, the j+1 / k+1 faces shared with the neighbouring line) have to survive there behind
// some 25 streams per trip that are touched exactly once.  ld_once / st_once make the same `scalar base + lane offset` access
// as uni(p)[e] / uniw(p)[e] and mark it non-temporal (the `nt` bit of global_load / global_store: the line is the first to be
// evicted).  A hint only: values, ordering and addressing are those of the plain access, which is also what the host
// emulation and a build with the group's macro at 0 make.  Measured (round 19, docs/experiments.md): the bytes the kernels fetch do
// not change with it, the C2 step gains about 1 %, and only X1 and F1 together are ahead of the parent reliably; X2 lost and is off.
// One macro per group of sites, so that each can be measured alone:
//   PAMA_STREAM_X1   x-sweep state pass, loads: the y/z differences, the sub-step-start values, water vapour's seed
//   PAMA_STREAM_F1   flux sweeps, stores: the per-cell flux differences of the state variables (DIFF), read once by the x-sweep
//   PAMA_STREAM_X2   x-sweep state pass, stores: water vapour's x flux (read again only where the limiter acts)
#ifndef PAMA_STREAM_POLICY
#define PAMA_STREAM_POLICY 1
#endif
#ifndef PAMA_STREAM_X1
#define PAMA_STREAM_X1 PAMA_STREAM_POLICY
#endif
#ifndef PAMA_STREAM_F1
#define PAMA_STREAM_F1 PAMA_STREAM_POLICY
#endif
#ifndef PAMA_STREAM_X2
#define PAMA_STREAM_X2 0
#endif
template <int NT>
PAMA_D double ld_once(gc_ptr p, unsigned e) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (NT != 0) return __builtin_nontemporal_load(p + e);
#endif
  return p[e];
}
template <int NT>
PAMA_D void st_once(g_ptr p, unsigned e, double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (NT != 0) { __builtin_nontemporal_store(v, p + e); return; }
#endif
  p[e] = v;
}
// The member index of a lane as the compiler must see it for `scalar base + 32-bit lane offset` addressing: an unsigned
// value whose top bits are KNOWN to be zero (nens < 2^28), so that 8*e cannot wrap in 32 bits.
PAMA_D unsigned member_offset(int e) { return (unsigned)e & 0x0fffffffu; }

// store_adv / store_rho_pres-style ghost handling with wave-uniform addressing: `cu` = offset of (j, i, member 0) inside a
// level (uniform), `e` = member (per lane).
PAMA_D void store_adv_u(const Params &P, double *prim, int pf, int k, long long cu, unsigned e, double val, double ghost_val) {
  double *f = prim + (long long)pf * P.prim_fs + cu;
  uniw(f + (long long)(k + HS) * P.sz)[e] = val;
  if (k == 0)
    for (int kk = 0; kk < HS; kk++) uniw(f + (long long)(HS - 1 - kk) * P.sz)[e] = ghost_val;     // Dycore.h:670,675
  if (k == P.nz - 1)
    for (int kk = 0; kk < HS; kk++) uniw(f + (long long)(HS + P.nz + kk) * P.sz)[e] = ghost_val;  // Dycore.h:671,676
}

// ------------------------------------------------------------------------------------------------
// Flux kernel geometry.  One "line" = the cells along the sweep direction for fixed other indices and
// ensemble member; an "item" = (line, iens) flattened with iens fastest so that a wavefront's 64 lanes read
// 64 consecutive doubles (512 B, fully coalesced) for nens >= 64.  A thread sweeps a span of faces of its line
// (the whole line when there are enough lines x members to fill the chip); consecutive wavefronts take consecutive
// spans of the same 64 items, so the overlap cells between neighbouring spans are L1/L2 hits.
struct LineGeom {
  int dir;             // 0 x, 1 y, 2 z
  int n;               // cells along the line
  int nfaces;          // x,y: n (periodic); z: n+1
  long long cs;        // cell stride along the line (doubles)
  long long fs_flux;   // field stride of this direction's flux array
};

PAMA_D LineGeom line_geom(const Params &P, int dir) {
  LineGeom g;
  g.dir = dir;
  if (dir == 0) { g.n = P.nx; g.nfaces = P.nx; g.cs = P.sx; g.fs_flux = P.ncell; }
  else if (dir == 1) { g.n = P.ny; g.nfaces = P.ny; g.cs = P.sy; g.fs_flux = P.ncell; }
  else { g.n = P.nz; g.nfaces = P.nz + 1; g.cs = P.sz; g.fs_flux = P.fz_fs; }
  return g;
}

PAMA_D int wrap(int c, int n) {
  c %= n;
  return c < 0 ? c + n : c;
}

// 2-D (ny == 1): the v tendency is zero whatever the fluxes are (Dycore.h:559 `if (sim2d) ... = 0`), so the fused stage (DIFF
// sweeps + x-sweep) neither reconstructs v nor stores / loads its flux differences.  The three-kernel stage keeps every face
// flux (the kernel-level parity tests compare them all with the oracle).
#if defined(__HIPCC__)
#define PAMA_HD __host__ __device__ inline
#else
#define PAMA_HD inline
#endif
// The fused stage treats ONE tracer differently from the others: water vapour (index idWV; every microphysics registers it,
// Dycore.h:83) is a smooth positive field in which the limiter is idle almost everywhere -- it rides with the state pass of the
// fused x-sweep and is finished there, with a sparse fix-up afterwards.  The others (cloud, rain, ice ...: blobs with exact zeros
// around them, limited in a large part of their cells) get the two-phase sweeps.  i-th further tracer -> tracer index:
PAMA_HD int further_tracer(const Params &P, int i) { return i < P.idWV ? i : i + 1; }
PAMA_HD bool skip_advected_v(const Params &P, bool diff) { return diff && P.sim2d; }
// advected fields a sweep visits after pass 1 (everything but the normal velocity; see above), in pairs (host: launch geometry)
PAMA_HD int flux_sweep_pairs(const Params &P, bool diff) { return (3 + P.nt - (skip_advected_v(P, diff) ? 1 : 0) + 1) / 2; }

// The work units of a sweep launch, one per WAVEFRONT.  Unit u names (line, block of 64 members, span of the line, selector) with the
// selector (a pair of advected fields, a group of tracers; nsel == 1: none) fastest, then the span, then the member block: consecutive
// wavefronts take the selectors and the consecutive spans of the same 64 items.  The host fills one, asks it for the size of the launch
// and checks its limit; the kernel builds the same numbers from its arguments and asks it what a wavefront works on -- the count
// and the decode stand next to each other here and nowhere else.
struct SweepUnits {
  int n1, n2, ne, nblk, nspan, nsel;     // lines of the sweep: n1 x n2 (the two directions across it); members of the range and their
                                         // blocks of 64; spans per line; selectors per span
  struct Unit { int us, grp, sel; };     // us: (line, member block, span); grp: (line, member block)
  struct Lane { int line, blk; };
  PAMA_HD long long count() const { return (long long)n1 * n2 * nblk * nspan * nsel; }
  PAMA_HD long long workgroups(int waves) const { return (count() + waves - 1) / waves; }
  static constexpr long long MAX_UNITS = 0x3fffffffll;                  // the decode is 32-bit: at most 2^30 wavefronts per launch
  PAMA_HD bool fits() const { return count() <= MAX_UNITS; }
  // u, and with it every quotient, is wave-uniform: uni_int keeps them in scalar registers.  has_sel false: u carries no selector
  PAMA_D Unit decode(int u, bool has_sel = true) const {
    Unit w;
    const int us = has_sel ? uni_int(u / nsel) : u;
    w.us = us;
    w.sel = has_sel ? u - us * nsel : 0;
    w.grp = uni_int(us / nspan);
    return w;
  }
  PAMA_D int span(const Unit &w) const { return w.us - w.grp * nspan; }
  // the (line, member block) of group grp (whole lines without selectors: of the unit itself); the wavefront's lanes are the block's
  // members: lane l works on member el = blk * 64 + l of the range
  PAMA_D Lane place(int grp) const {
    Lane m;
    m.line = uni_int(grp / nblk);
    m.blk = grp - m.line * nblk;
    return m;
  }
  PAMA_D bool holds(const Lane &m, int el) const { return m.line < n1 * n2 && el < ne; }
};
PAMA_HD SweepUnits sweep_units(int n1, int n2, int ne, int nspan, int nsel) { return SweepUnits{n1, n2, ne, (ne + 63) >> 6, nspan, nsel}; }

// Body of the reconstruction + flux kernel for one lane.
//   DIR      sweep direction
//   line     wave-uniform index of the line: x: k*ny + j, y: k*nx + i, z: j*nx + i        e   ensemble member of this lane
//   f0,span  the wavefront sweeps the faces f0 .. min(f0+span, nfaces)-1 of its line (normally the whole line)
// All 64 lanes of a wavefront work on the same line and differ in the member only, so every address is a wave-uniform
// base + member (uni()/uniw(): scalar addressing, one VGPR of address for all streams).
// The span is swept once per quantity with a 5-cell sliding window in registers, so every state value is loaded once
// per sweep (plus the 5-cell overlap at the start of a span):
//   pass 1   rho*u_n, p and u_n together: the acoustic pair gives the face mass flux ruf and face pressure ppf
//            (Dycore.h:341-366); ruf goes to flux field 0; the normal-momentum flux ruf*upwind(u_n) + ppf is finished in the
//            same pass, so ppf never needs storing;
//   pass 2.. FLUX_NF advected fields at a time (the other velocity components, theta, tracers), upwinded by the ruf read
//            back from flux field 0 (the lane's own store: L2-resident; no LDS, so residency is bounded by registers only)
//            (Dycore.h:367-385).
// Every cell polynomial is computed once and evaluated at both edges; the only redundant polynomial is the one of cell
// f0-1 at the start of the span.
//   DIFF     (the fused stage's y/z sweeps) the four momentum/theta variables are stored as the flux difference of each
//            cell, F[c] - F[c+1] -- exactly the subtraction the divergence performs (flux_divergence), so the consumer loads ONE
//            value per cell, variable and direction instead of two faces of which one belongs to a neighbouring line.  The
//            mass flux (the later passes upwind with its faces) and the tracers (the FCT limiter works on faces) keep the
//            face form.  Periodic lines must then be swept whole (f0 = 0, span >= n).
// Reference: Dycore.h:334-519.  `prim` holds rho, p, and the density-divided u,v,w,theta,tracers (Dycore.h:310-321)
// with vertical ghosts already filled (Dycore.h:662-710).
// Where a lane of a sweep works: the wave-uniform offsets of the line's cell 0 inside a prim field (pbase) and of its face 0 inside a
// flux field (fbase), the lane's own element offset on top of both (eu, < 2^28: scalar base + 32-bit lane offset addressing) and the
// ensemble member whose per-member tables it reads (et).
//   member lanes (member_lane): the 64 lanes are 64 consecutive MEMBERS of ONE line; eu = member.  Full lanes when nens is a
//                multiple of 64 -- the layout every large ensemble runs with.
//   flat lanes   (flat_lane, the y and z sweeps of small ensembles): nens is the fastest axis and x the next, so for a sweep along y
//                or z the (x, member) pairs of a row -- and, row after row, everything that is not the sweep direction -- form ONE
//                flat index space whose 64 consecutive items sit in consecutive lanes: the stencil stays in the lane (its neighbours
//                are sy / sz doubles away in memory), accesses stay coalesced along the fastest (x, nens) axes, and a wavefront is
//                full whenever nx*nens (times the rows that are packed with it) reaches 64, whatever nens is.
struct LineLane { long long pbase, fbase; unsigned eu; int et; };
template <int DIR>
PAMA_D LineLane member_lane(const Params &P, int line, int e) {
  LineLane ll;
  ll.eu = member_offset(e);
  ll.et = e;
  if (DIR == 0) {  // line = k*ny + j
    const int k = uni_int(line / P.ny), j = line - k * P.ny;
    ll.pbase = (long long)(k + HS) * P.sz + (long long)j * P.sy;
    ll.fbase = (long long)k * P.sz + (long long)j * P.sy;
  } else if (DIR == 1) {  // line = k*nx + i
    const int k = uni_int(line / P.nx), i = line - k * P.nx;
    ll.pbase = (long long)(k + HS) * P.sz + (long long)i * P.sx;
    ll.fbase = (long long)k * P.sz + (long long)i * P.sx;
  } else {  // line = j*nx + i ; cell c lives at kz = c + HS
    ll.pbase = (long long)HS * P.sz + (long long)line * P.sx;
    ll.fbase = (long long)line * P.sx;
  }
  return ll;
}
// item q of the flat index space of a y sweep ((level, x, member): nz * nx*nens items) or a z sweep ((y, x, member): ny * nx*nens)
PAMA_HD long long flat_items(const Params &P, int dir) { return (long long)(dir == 1 ? P.nz : P.ny) * P.nx * P.nens; }
template <int DIR>
PAMA_D LineLane flat_lane(const Params &P, unsigned q) {
  static_assert(DIR == 1 || DIR == 2, "flat lanes: y and z sweeps (the x direction has its own tile kernels)");
  LineLane ll;
  ll.pbase = (long long)HS * P.sz;
  ll.fbase = 0;
  const unsigned row = (unsigned)P.nx * (unsigned)P.nens;                // (x, member) pairs of a row: contiguous in memory
  if (DIR == 1) {
    const unsigned k = q / row, r = q - k * row;
    ll.eu = member_offset((int)(k * (unsigned)P.sz + r));
    ll.et = (int)(r % (unsigned)P.nens);
  } else {
    ll.eu = member_offset((int)q);                                        // (y, x, member) is contiguous as it stands
    ll.et = (int)(q % (unsigned)P.nens);
  }
  return ll;
}

// Where a z sweep takes the vertical WENO table of a level from (weno5_table; level = cell index + 1, Dycore.h:454-469).  A sweep
// announces the levels it will use, in ascending order: pass_begin(first, last), then per level trip_begin(level) ... weno(level)
// ... trip_end(level).
//   ZTabConst   every member has the same vertical grid (set_grid(..., realConst1d), pam_coupler.h:184-202): ONE table, read through
//               the constant address space with scalar loads -- the coefficients are scalar operands of the polynomial's instructions
//   ZTabLane    per-member grids (set_grid(..., realConst2d), pam_coupler.h:163-181; Dycore.h:897-940 builds the matrices per
//               (k, iens) unconditionally), each lane reads its member's 31 coefficients from global memory: the flat-lane sweeps of
//               small ensembles, the host emulation
//   ZTabLds     (awfl_kernels.hip) per-member grids, member lanes: the wavefronts of a workgroup sweep different columns of the SAME
//               64 members in step, and the level's table of those members is staged in LDS once per workgroup
struct ZTabConst {
  const double *vz;
  // one grid for the ensemble: 1/dz of a level is wave-uniform -- a scalar load (member 0's entry), no vector memory operation
  PAMA_D double rdz(const Params &P, int k, int) const { return as_constant(P.rdz + (long long)k * P.nens)[0]; }
  PAMA_D void pass_begin(int, int) {}
  PAMA_D void trip_begin(int) {}
  PAMA_D void trip_end(int) {}
  PAMA_D void weno(const double u[5], int level, const WenoConsts &wc, double &L, double &R) const {
    weno5_table(u, as_constant(vz + (long long)level * VZ_STRIDE), 1, wc, L, R);
  }
};
struct ZTabLane {
  const double *vz;
  long long nens;
  int e;
  PAMA_D double rdz(const Params &P, int k, int e_) const { return P.rdz[(long long)k * P.nens + e_]; }
  PAMA_D void pass_begin(int, int) {}
  PAMA_D void trip_begin(int) {}
  PAMA_D void trip_end(int) {}
  PAMA_D void weno(const double u[5], int level, const WenoConsts &wc, double &L, double &R) const {
    weno5_table(u, vz + (long long)level * VZ_STRIDE * nens + e, nens, wc, L, R);
  }
};

//   FOLD     (DIR == 2, DIFF, 3-D) the y sweep has run in an EARLIER launch: the z sweep loads the y difference of each state variable
//            of the cell it closes (fold_y: the y flux array) and stores yz_divergence() -- the y+z part of the variable's divergence --
//            instead of its own difference: the x-sweep then loads one value per variable instead of two (P.yz_fold)
template <int DIR, bool DIFF, class ZT, bool FOLD = false>
PAMA_D void flux_line_body_zt(const Params &P, const double *__restrict__ prim, double *__restrict__ flux, const LineLane &ll,
                              int f0, int span, int pair_sel, ZT &zt, const double *__restrict__ fold_y = nullptr) {
  static_assert(!FOLD || (DIR == 2 && DIFF), "only the z sweep of the fused stage folds the y differences in");
  const unsigned eu = ll.eu;
  const int e = ll.et;
  const LineGeom g = line_geom(P, DIR);
  const WenoConsts wc = weno_consts();
  // base offset of the line's cell 0 inside a prim field, and of its face 0 inside a flux field (wave-uniform)
  const long long pbase = ll.pbase, fbase = ll.fbase;
  const int fend = (f0 + span < g.nfaces) ? f0 + span : g.nfaces;     // exclusive: the faces this span owns
  // DIFF: the five state variables leave as flux DIFFERENCES of cells (F[c] - F[c+1], what the divergence needs), so the
  // sweep also computes the face that closes its last cell: face fend, or the periodic face n == face 0 (same bits)
  const int cl = DIFF ? (fend < g.n ? fend : g.n) : fend - 1;          // last face needed (inclusive)
  const bool periodic = (DIR != 2);
  // DIFF on a periodic line (swept whole: f0 = 0): the closing face n IS face 0.  It is formed once, after the loops, from the right
  // edges of cell n-1 (the last trip's) and the left edges of cell 0 (the prologue's, see cpro): n polynomial sets for n cells -- no
  // polynomial of cell -1 == cell n-1 for its right edges only and no second trip over cell 0
  const bool reuse0 = DIFF && periodic && f0 == 0 && cl == g.n;
  const int cloop = reuse0 ? cl - 1 : cl;                               // last face the loops compute
  const int ncomp = (DIR == 0) ? P_U : (DIR == 1 ? P_V : P_W);         // normal velocity field
  // z: faces 0 and nz are walls, the cells beyond them (-1: the prologue's; nz: the last trip's) are ghosts.  A wall face has no mass
  // flux, so the only edge value of a ghost cell that a result needs is the pressure's.  The other polynomials of ghost cell -1, and
  // those of ghost cell nz in the pair sweeps, are not built: wave-uniform branches outside the loops (f0, nz and the span are
  // scalar); the loads, the stores and the table hooks of every trip stay
  const bool wall_lo = (DIR == 2) && f0 == 0;
  // last trip of the pair sweeps' loops: a span that ends at the top wall makes its last trip, the one of ghost cell nz, after them
  const int cin = ((DIR == 2) && cloop == P.nz) ? cloop - 1 : cloop;
  // the cell the prologue builds.  Normally f0-1, for its right edges (face f0).  A whole periodic line starts with cell 0 instead and
  // keeps its LEFT edges for the closing face: the loops then run over the faces 1 .. n-1 like those of any other span
  const int cpro = reuse0 ? 0 : f0 - 1;

  auto cell_off = [&](int c) -> long long {
    if (DIR == 2) return pbase + (long long)(c > P.nz + 2 ? P.nz + 2 : c) * g.cs;   // ghosts exist for c in [-3, nz+2]
    // periodic (Dycore.h:629-657); c in [-3, n+2] and n >= 3: no division, stays on the scalar unit
    return pbase + (long long)(c < 0 ? c + g.n : (c >= g.n ? c - g.n : c)) * g.cs;
  };
  // vertical table of cell c (level index c+1): tab[m] for the ensemble-uniform table, tab[m*nens + e] per member
  auto weno = [&](const double u[5], int c, double &L, double &R) {
    if (DIR != 2) { weno5_const(u, wc, L, R); return; }
    zt.weno(u, c + 1, wc, L, R);
  };
  // FOLD: what the store of a closed cell cc needs besides the z difference -- the y difference of the variable and 1/dz of the cell
  // (requested at the top of the trip that closes the cell, on EVERY trip: see flux_x_update_body on s_waitcnt counts)
  auto fold_cell = [&](int c) -> int { return c > 0 ? c - 1 : 0; };      // the cell trip c closes (clamped: trip f0 closes none)
  auto folded = [&](double dzv, double dyv, double rdzv) -> double { return yz_divergence(P, dyv, dzv, rdzv); };
  // DIFF: the store of a closed cell's difference by the trips of the loops.  The x-sweep reads it once (PAMA_STREAM_F1).  Trip 1 of a
  // whole periodic line goes through here too, although what it parks in cell 0's slot is loaded back by this lane behind the loop: one
  // reload per line.  Telling that trip apart cost the loops of the y sweep 6 to 25 instructions each (a second copy of every store
  // behind a scalar branch), which an FP64-issue-bound kernel pays for on every trip.  The values parked BEFORE the loops and the
  // stores behind them (the closing face) stay plain accesses.
  auto st_diff = [&](double *p, double val) __attribute__((always_inline)) { st_once<PAMA_STREAM_F1>(uniw(p), eu, val); };
  const int nadv = 4 + P.nt;
  double *fl0 = flux + fbase;                                          // flux field 0 of this line: the face mass flux

  // pair_sel: -1 = the whole sweep in this wavefront; 0 = pass 1 only; p >= 1 = only the p-th pair of advected fields (small
  // ensembles: the passes of a sweep are spread over wavefronts, pass 1 in a launch of its own before the pairs)
  // ---------------- pass 1: acoustic pair + normal momentum (Dycore.h:341-366, :368-385 for u_n) -------------
  if (pair_sel <= 0) {
    const double *pr = prim + (long long)P_RHO * P.prim_fs;
    const double *pn = prim + (long long)ncomp * P.prim_fs;
    const double *pp = prim + (long long)P_PRES * P.prim_fs;
    double *fln = flux + (long long)(1 + ncomp - P_U) * g.fs_flux + fbase;
    double wm[5], wp[5], wn[5];   // windows: rho*u_n product, pressure, u_n
#pragma unroll
    for (int s = 0; s < 5; s++) {                          // the window of the prologue's cell (f0-1: cells f0-3..f0+1)
      const long long o = cell_off(cpro - 2 + s);
      wn[s] = uni(pn + o)[eu];
      wm[s] = mul_rn(uni(pr + o)[eu], wn[s]);
      wp[s] = uni(pp + o)[eu];
    }
    double prevR_m, prevR_p, prevR_n;
    if (DIR == 2) { zt.pass_begin(f0, cloop + 1); zt.trip_begin(f0); }     // (levels f0 .. cloop + 1, in this order)
    {                                                      // cell f0-1: only its right-edge values are needed (face f0)
      double Lm0 = 0.0, Lp0, Ln0 = 0.0;                   // (cell 0 of a whole periodic line: both edges)
      weno(wp, cpro, Lp0, prevR_p);
      if (wall_lo) {
        // face 0 of a column is a wall: acoustic_face() zeroes both rho*w arguments and returns ruf = +0.0, so of ghost cell -1 only
        // the pressure's edge value reaches a result -- rho*w's is replaced by 0.0 and w's multiplied by +0.0 (fma(+0, ., ppf)):
        // any finite value gives the same number (at most the sign of a zero differs)
        prevR_m = 0.0; prevR_n = 0.0;
      } else {
        weno(wm, cpro, Lm0, prevR_m);
        weno(wn, cpro, Ln0, prevR_n);
      }
      if (reuse0) {
        // A whole periodic line: what face n == face 0 needs of cell 0 -- its characteristic variable w1 and the left edge of u_n --
        // waits in memory, not in registers, in two output slots of this lane that no trip writes: the mass flux of face 0 and
        // the difference of cell n-1 (both are stored after the loop, from these values)
        uniw(fl0)[eu] = acoustic_w1(Lm0, Lp0);
        uniw(fln + (long long)(g.n - 1) * g.cs)[eu] = Ln0;
      }
      const long long on = cell_off(cpro + 3);
      const double nn = uni(pn + on)[eu];
#pragma unroll
      for (int s = 0; s < 4; s++) { wm[s] = wm[s + 1]; wp[s] = wp[s + 1]; wn[s] = wn[s + 1]; }
      wn[4] = nn; wm[4] = mul_rn(uni(pr + on)[eu], nn); wp[4] = uni(pp + on)[eu];
    }
    if (DIR == 2) zt.trip_end(f0);
    // DIFF: the previous face's normal-momentum flux.  A whole periodic line starts from 0.0: its first trip, face 1, then parks
    // 0.0 - F[1] in cell 0's own output slot, where it waits for face 0 (after the loop)
    double Fpn = 0.0;
    const double *fyn = FOLD ? fold_y + (long long)(1 + ncomp - P_U) * P.ncell + fbase : nullptr;
    // one trip: face c between cells c-1 and c, from the windows of cell c (cells c-2..c+2, in um / up / un)
    auto trip = [&](int c, const double (&um)[5], const double (&up)[5], const double (&un)[5]) __attribute__((always_inline)) {
      double dyv = 0.0, rdzv = 0.0;
      if (FOLD) {
        dyv = uni(fyn + (long long)fold_cell(c) * g.cs)[eu];
        rdzv = zt.rdz(P, fold_cell(c), e);
      }
      double Lm, Rm, Lp, Rp, Ln, Rn;
      weno(um, c, Lm, Rm);
      weno(up, c, Lp, Rp);
      weno(un, c, Ln, Rn);
      const bool wall = (DIR == 2) && (c == 0 || c == P.nz);   // Dycore.h:477,482,496
      double ruf, ppf;
      acoustic_face(prevR_m, Lm, prevR_p, Lp, wall, ruf, ppf);
      const double val = (ruf > 0.0) ? prevR_n : Ln;            // upwind (Dycore.h:368)
      const double fn = fma(ruf, val, ppf);
      // the mass flux always leaves as FACES: the later passes upwind with it (face n of a periodic line is face 0)
      if (!(DIFF && periodic && c == g.n)) uniw(fl0 + (long long)c * g.cs)[eu] = ruf;
      if (DIFF) {
        if (c > f0) st_diff(fln + (long long)(c - 1) * g.cs, FOLD ? folded(Fpn - fn, dyv, rdzv) : Fpn - fn);   // cell c-1 is closed by faces c-1 and c
        Fpn = fn;
      } else {
        uniw(fln + (long long)c * g.cs)[eu] = fn;
      }
      prevR_m = Rm; prevR_p = Rp; prevR_n = Rn;
    };
    if constexpr (DIR == 2) {
      // z: the windows rotate their slots as in the pair sweeps below (trip r of five uses the slots (r, .. r+4) mod 5 and overwrites
      // slot r with the cell that enters): no window is moved, and neighbouring cells of a round share their differences.  The y
      // sweep keeps moving windows: rotated, its three windows would also share second differences and their squares, and those
      // live ranges cost the 128-register budget 108 B of scratch (docs/experiments.md).
      // (pass 1 builds ghost cell nz whole: making its last trip after the loop with the pressure polynomial alone costs every
      // trip of the loop more scalar-register spills than the two polynomials are worth, and the kernel 8 B of scratch)
#pragma clang loop unroll(disable)
      for (int c = f0; c <= cloop;) {
#pragma unroll
        for (int r = 0; r < 5; r++) {
          if (c > cloop) break;
          if (DIR == 2) zt.trip_begin(c + 1);
          const long long on = cell_off(c + 3);            // the next cell entering the window
          const double nn = uni(pn + on)[eu], nm = mul_rn(uni(pr + on)[eu], nn), np_ = uni(pp + on)[eu];
          const double um[5] = {wm[r % 5], wm[(r + 1) % 5], wm[(r + 2) % 5], wm[(r + 3) % 5], wm[(r + 4) % 5]};
          const double up[5] = {wp[r % 5], wp[(r + 1) % 5], wp[(r + 2) % 5], wp[(r + 3) % 5], wp[(r + 4) % 5]};
          const double un[5] = {wn[r % 5], wn[(r + 1) % 5], wn[(r + 2) % 5], wn[(r + 3) % 5], wn[(r + 4) % 5]};
          trip(c, um, up, un);
          wm[r % 5] = nm; wp[r % 5] = np_; wn[r % 5] = nn;
          if (DIR == 2) zt.trip_end(c + 1);
          c++;
        }
      }
    } else {
#pragma clang loop unroll(disable)
      for (int c = cpro + 1; c <= cloop; c++) {
        if (DIR == 2) zt.trip_begin(c + 1);
        const long long on = cell_off(c + 3);              // the next cell entering the window
        const double nn = uni(pn + on)[eu], nm = mul_rn(uni(pr + on)[eu], nn), np_ = uni(pp + on)[eu];
        trip(c, wm, wp, wn);
#pragma unroll
        for (int s = 0; s < 4; s++) { wm[s] = wm[s + 1]; wp[s] = wp[s + 1]; wn[s] = wn[s + 1]; }
        wm[4] = nm; wp[4] = np_; wn[4] = nn;
        if (DIR == 2) zt.trip_end(c + 1);
      }
    }
    if (reuse0) {
      // face n == face 0, from the right edges of cell n-1 and what was kept of cell 0; its mass flux is stored here, before
      // any pair sweep reads it.  It closes the last cell and, with the parked 0.0 - F[1] loaded back (this lane's own store), cell 0:
      // F[0] + (0.0 - F[1]) is F[0] - F[1] rounded once (the negation is exact; only the sign of a zero can differ)
      double ruf, ppf;
      const double w1 = uni(fl0)[eu], Ln0 = uni(fln + (long long)(g.n - 1) * g.cs)[eu];
      acoustic_face_w(w1, acoustic_w2(prevR_m, prevR_p), false, ruf, ppf);
      const double fn = fma(ruf, (ruf > 0.0) ? prevR_n : Ln0, ppf);
      uniw(fl0)[eu] = ruf;
      uniw(fln + (long long)(g.n - 1) * g.cs)[eu] = Fpn - fn;
      const double mF1 = uni(fln)[eu];
      uniw(fln)[eu] = fn + mF1;
    }
  }
  // ---------------- the other advected quantities (Dycore.h:367-385), FLUX_NF fields per sweep ------------------
  // One polynomial is a long dependent chain (differences -> coefficients -> TVs -> weights -> map -> blend); with few
  // wavefronts per SIMD a single chain per iteration leaves issue slots empty, several independent chains fill them.
  // NS: the first NS fields of the sweep are state variables whose DIFFERENCE is stored (DIFF only; the sweep order puts the
  // state variables first), the others store faces
  auto sweep = [&](auto nf_tag, auto ns_tag, const int *fa) __attribute__((always_inline)) {
    constexpr int NF = decltype(nf_tag)::value;
    constexpr int NS = decltype(ns_tag)::value;
    const double *q[NF];
    double *fl[NF];
    double w[NF][5], prevR[NF];
#pragma unroll
    for (int n = 0; n < NF; n++) {
      q[n] = prim + (long long)(P_U + fa[n]) * P.prim_fs;
      fl[n] = flux + (long long)(1 + fa[n]) * g.fs_flux + fbase;
    }
#pragma unroll
    for (int s = 0; s < 5; s++) {
      const long long o = cell_off(cpro - 2 + s);
#pragma unroll
      for (int n = 0; n < NF; n++) w[n][s] = uni(q[n] + o)[eu];
    }
    if (DIR == 2) { zt.pass_begin(f0, cloop + 1); zt.trip_begin(f0); }
    {
      const long long on = cell_off(cpro + 3);
#pragma unroll
      for (int n = 0; n < NF; n++) {
        // wall face 0: its mass flux is +0.0, never > 0, so the upwind value is cell 0's left edge and ghost cell -1 has no reader:
        // its polynomials are not built
        double L0 = 0.0;
        if (wall_lo) prevR[n] = 0.0;
        else weno(w[n], cpro, L0, prevR[n]);
        // A whole periodic line: cell 0's left edge is what face n == face 0 needs of it.  It waits in memory, not in a register, in
        // the output slot of this lane that no trip writes: the difference of cell n-1, or face 0 of a face-form field
        if (reuse0) uniw(fl[n] + (n < NS ? (long long)(g.n - 1) * g.cs : 0))[eu] = L0;
#pragma unroll
        for (int s = 0; s < 4; s++) w[n][s] = w[n][s + 1];
        w[n][4] = uni(q[n] + on)[eu];
      }
    }
    if (DIR == 2) zt.trip_end(f0);
    const double *fyq[NF];
#pragma unroll
    for (int n = 0; n < NF; n++) fyq[n] = (FOLD && n < NS) ? fold_y + (long long)(1 + fa[n]) * P.ncell + fbase : nullptr;
    // the previous face's flux.  A whole periodic line starts from 0.0: its first trip, face 1, then parks 0.0 - F[1] in cell 0's own
    // output slot, where it waits for face 0 (after the loop)
    double Fp[NF];
#pragma unroll
    for (int n = 0; n < NF; n++) Fp[n] = 0.0;
    // The window does not move: trip r of five uses the slots (r, r+1, .. r+4) mod 5 and overwrites slot r -- the oldest cell --
    // with the cell that enters; after five trips the naming is back where it started.  (Shifting the window costs 4 v_mov_b64
    // per field and trip, 6 % of the vector instructions of a sweep.)
    int c = cpro + 1;
#pragma clang loop unroll(disable)
    for (; c <= cin;) {
#pragma unroll
      for (int r = 0; r < 5; r++) {
        if (c > cin) break;
        if (DIR == 2) zt.trip_begin(c + 1);
        const long long on = cell_off(c + 3);
        double nq[NF], L[NF], R[NF], dyv[NF], rdzv = 0.0;
#pragma unroll
        for (int n = 0; n < NF; n++) nq[n] = uni(q[n] + on)[eu];
#pragma unroll
        for (int n = 0; n < NF; n++) dyv[n] = (FOLD && n < NS) ? uni(fyq[n] + (long long)fold_cell(c) * g.cs)[eu] : 0.0;
        if (FOLD && NS > 0) rdzv = zt.rdz(P, fold_cell(c), e);
        // this lane's own store of pass 1 (the periodic face n is face 0)
        const double ruf = uni(fl0 + (long long)((DIFF && periodic && c == g.n) ? 0 : c) * g.cs)[eu];
#pragma unroll
        for (int n = 0; n < NF; n++) {
          const double u[5] = {w[n][r % 5], w[n][(r + 1) % 5], w[n][(r + 2) % 5], w[n][(r + 3) % 5], w[n][(r + 4) % 5]};
          weno(u, c, L[n], R[n]);
        }
        const bool up = ruf > 0.0;                              // upwind (Dycore.h:368)
#pragma unroll
        for (int n = 0; n < NF; n++) {
          const double F = mul_rn(ruf, up ? prevR[n] : L[n]);
          if (n < NS) {
            if (c > f0) st_diff(fl[n] + (long long)(c - 1) * g.cs, FOLD ? folded(Fp[n] - F, dyv[n], rdzv) : Fp[n] - F);
            Fp[n] = F;
          } else if (c < fend) {
            uniw(fl[n] + (long long)c * g.cs)[eu] = F;
          }
          prevR[n] = R[n];
          w[n][r % 5] = nq[n];
        }
        if (DIR == 2) zt.trip_end(c + 1);
        c++;
      }
    }
    if (DIR == 2 && c <= cloop) {
      // The last trip, face nz: a wall.  Its mass flux is +0.0, so the flux of every field is mul_rn(+0.0, left edge of ghost cell nz):
      // a zero for any finite edge value.  No polynomial of the ghost cell is built and 0.0 stands in for the edge value.  Only the
      // sign bit of that zero can differ from the built polynomial's (a face-form field stores it as it is), and it reaches an
      // output only as the sign of a zero.  The trip's loads of the mass flux and the fold terms, its stores and its table hooks stay;
      // the window has no cell left to take in.  (c == nz here: the loop's own counter)
      zt.trip_begin(c + 1);
      double dyv[NF], rdzv = 0.0;
#pragma unroll
      for (int n = 0; n < NF; n++) dyv[n] = (FOLD && n < NS) ? uni(fyq[n] + (long long)fold_cell(c) * g.cs)[eu] : 0.0;
      if (FOLD && NS > 0) rdzv = zt.rdz(P, fold_cell(c), e);
      const double ruf = uni(fl0 + (long long)c * g.cs)[eu];
#pragma unroll
      for (int n = 0; n < NF; n++) {
        const double F = mul_rn(ruf, 0.0);
        if (n < NS) {
          if (c > f0) st_diff(fl[n] + (long long)(c - 1) * g.cs, FOLD ? folded(Fp[n] - F, dyv[n], rdzv) : Fp[n] - F);
        } else if (c < fend) {
          uniw(fl[n] + (long long)c * g.cs)[eu] = F;
        }
      }
      zt.trip_end(c + 1);
    }
    if (reuse0) {                                                // face n == face 0: upwinded by face 0's mass flux (pass 1's store)
      const double ruf0 = uni(fl0)[eu];
      const bool up0 = ruf0 > 0.0;
#pragma unroll
      for (int n = 0; n < NF; n++) {
        const double L0 = uni(fl[n] + (n < NS ? (long long)(g.n - 1) * g.cs : 0))[eu];
        const double Fc = mul_rn(ruf0, up0 ? prevR[n] : L0);
        if (n < NS) {
          // closes the last cell and, with the parked 0.0 - F[1] loaded back (this lane's own store), cell 0: F[0] + (0.0 - F[1]) is
          // F[0] - F[1] rounded once (the negation is exact; only the sign of a zero can differ)
          uniw(fl[n] + (long long)(g.n - 1) * g.cs)[eu] = Fp[n] - Fc;
          const double mF1 = uni(fl[n])[eu];
          uniw(fl[n])[eu] = Fc + mF1;
        } else {
          uniw(fl[n])[eu] = Fc;
        }
      }
    }
  };
  // dispatch: NF fields per sweep, of which the leading ns are state variables in difference form
  auto run = [&](int nf, const int *fa) __attribute__((always_inline)) {
    int ns = 0;
    if (DIFF)
      for (int n = 0; n < nf; n++) ns += (fa[n] < 4) ? 1 : 0;
    using std::integral_constant;
    if (nf == 1) { if (ns == 1) sweep(integral_constant<int, 1>{}, integral_constant<int, 1>{}, fa); else sweep(integral_constant<int, 1>{}, integral_constant<int, 0>{}, fa); }
    else if (nf == 2) {
      if (ns == 2) sweep(integral_constant<int, 2>{}, integral_constant<int, 2>{}, fa);
      else if (ns == 1) sweep(integral_constant<int, 2>{}, integral_constant<int, 1>{}, fa);
      else sweep(integral_constant<int, 2>{}, integral_constant<int, 0>{}, fa);
    }
  };
  static_assert(FLUX_NF == 2, "the sweep dispatch is written for two fields per sweep");
  if (pair_sel == 0) return;
  int fa[FLUX_NF], nfa = 0, ipair = 0;
  for (int a = 0; a < nadv; a++) {
    if (P_U + a == ncomp) continue;
    if (skip_advected_v(P, DIFF) && a == 1) continue;
    fa[nfa++] = a;
    if (nfa == FLUX_NF) {
      ipair++;
      if (pair_sel < 0 || pair_sel == ipair) run(FLUX_NF, fa);
      nfa = 0;
    }
  }
  if (nfa == 1) {
    ipair++;
    if (pair_sel < 0 || pair_sel == ipair) run(1, fa);
  }
}

// the table of the sweep chosen by VZ_PER_ENS: one for the ensemble / the lane's own member's, straight from global memory
template <int DIR, bool VZ_PER_ENS, bool DIFF, bool FOLD = false>
PAMA_D void flux_line_body(const Params &P, const double *__restrict__ prim, double *__restrict__ flux, const LineLane &ll,
                           int f0, int span, int pair_sel = -1, const double *__restrict__ fold_y = nullptr) {
  if constexpr (VZ_PER_ENS) {
    ZTabLane zt{P.vz, (long long)P.nens, ll.et};
    flux_line_body_zt<DIR, DIFF, ZTabLane, FOLD>(P, prim, flux, ll, f0, span, pair_sel, zt, fold_y);
  } else {
    ZTabConst zt{P.vz};
    flux_line_body_zt<DIR, DIFF, ZTabConst, FOLD>(P, prim, flux, ll, f0, span, pair_sel, zt, fold_y);
  }
}
// lanes = members of one line (the layout of large ensembles; also what the host emulation runs)
template <int DIR, bool VZ_PER_ENS, bool DIFF, bool FOLD = false>
PAMA_D void flux_line_body(const Params &P, const double *__restrict__ prim, double *__restrict__ flux, int line, int e,
                           int f0, int span, int pair_sel = -1, const double *__restrict__ fold_y = nullptr) {
  flux_line_body<DIR, VZ_PER_ENS, DIFF, FOLD>(P, prim, flux, member_lane<DIR>(P, line, e), f0, span, pair_sel, fold_y);
}

// ------------------------------------------------------------------------------------------------
// Stores of one cell's density-divided variables (Dycore.h:310-321) and, for the first/last level, of the 3 ghost
// levels below/above (Dycore.h:662-710, intended semantics: ghost theta = theta of the boundary cell).
// Fields are stored one at a time as they are produced, so no per-thread array is needed (no scratch).
PAMA_D void store_adv(const Params &P, double *prim, int pf, int k, long long c2, double val, double ghost_val) {
  double *f = prim + (long long)pf * P.prim_fs;
  f[(long long)(k + HS) * P.sz + c2] = val;
  if (k == 0)
    for (int kk = 0; kk < HS; kk++) f[(long long)(HS - 1 - kk) * P.sz + c2] = ghost_val;     // Dycore.h:670,675
  if (k == P.nz - 1)
    for (int kk = 0; kk < HS; kk++) f[(long long)(HS + P.nz + kk) * P.sz + c2] = ghost_val;  // Dycore.h:671,676
}

// density and pressure of the cell + their hydrostatically extrapolated ghosts (Dycore.h:682-709)
template <bool STORE_RHO = true>   // false: the interior density is already in place (the fused x-sweep wrote it)
PAMA_D void store_rho_pres(const Params &P, double *prim, int k, long long c2, int e, double rho, double th,
                           double rho_theta, bool subtract_hy) {
#pragma clang fp contract(off)
  double *fr = prim + (long long)P_RHO * P.prim_fs, *fp = prim + (long long)P_PRES * P.prim_fs;
  const long long o = (long long)(k + HS) * P.sz + c2;
  double pres = P.C0 * pow_pos(P, rho_theta, P.gamma);
  if (subtract_hy) pres -= P.hy_pres[(long long)k * P.nens + e];
  if (STORE_RHO) fr[o] = rho;
  fp[o] = pres;
  const bool bot = (k == 0), top = (k == P.nz - 1);
  if (bot || top) {
    const double gm1 = P.gamma - 1.0;
    const double rho0_gm1 = pow_pos(P, rho, gm1);
    const double theta0_g = pow_pos(P, th, P.gamma);
    const double dzk = P.dz[(long long)k * P.nens + e];
    const double coef = P.grav * gm1 * dzk / (P.gamma * P.C0 * theta0_g);
    for (int kk = 0; kk < HS; kk++) {
      const int kz = bot ? (HS - 1 - kk) : (HS + P.nz + kk);
      const long long og = (long long)kz * P.sz + c2;
      const double arg = bot ? rho0_gm1 + coef * (kk + 1) : rho0_gm1 - coef * (kk + 1);
      const double rho_g = pow_pos(P, arg, 1.0 / gm1);
      double p_g = pres;                                          // mode B: copy (Dycore.h:678-681)
      if (P.grav_balance) p_g = P.C0 * pow_pos(P, rho_g * th, P.gamma);    // mode A (Dycore.h:691-694)
      fr[og] = rho_g;
      fp[og] = p_g;
    }
  }
}

// A cell and its flattened index (nens fastest).  The pointwise kernels get k and j from the launch grid and split only
// (i, member) per thread with one 32-bit division: a 64-bit div/mod decomposition of the flat index costs several
// hundred VALU instructions per thread, which matters because these kernels co-run with the FP64-bound flux kernel.
struct CellId { int k, j, i, e; long long idx; };

// decompose a flattened cell index (nens fastest) -> k, j, i, e
PAMA_D void cell_coords(const Params &P, long long idx, int &k, int &j, int &i, int &e) {
  e = (int)(idx % P.nens);
  long long r = idx / P.nens;
  i = (int)(r % P.nx); r /= P.nx;
  j = (int)(r % P.ny);
  k = (int)(r / P.ny);
}
PAMA_D CellId cell_of(const Params &P, long long idx) {
  CellId c;
  cell_coords(P, idx, c.k, c.j, c.i, c.e);
  c.idx = idx;
  return c;
}

// Coupler fields -> prim (+ghosts) and seed.  Dycore.h:1370-1387, :130-134.
// gcm != nullptr selects the use_gcm_data branch of declare_current_profile_as_hydrostatic (Dycore.h:1415-1434):
// gcm[0..4] = gcm_density_dry, gcm_temp, gcm_water_vapor, gcm_cloud_water, gcm_cloud_ice, each (nz,nens).
PAMA_D void init_prim_body(const Params &P, const double *__restrict__ rho_d_c, const double *__restrict__ u_c,
                           const double *__restrict__ v_c, const double *__restrict__ w_c,
                           const double *__restrict__ temp_c, const TracerPtrs &trc, const double *const *gcm,
                           double *__restrict__ prim, double *__restrict__ seed, bool subtract_hy, const CellId &c) {
  const int k = c.k, j = c.j, i = c.i, e = c.e;
  const long long idx = c.idx;
  const long long c2 = (long long)j * P.sy + (long long)i * P.sx + e;
  double rho, ru, rv, rw, rt;
  if (gcm) {
    const long long c = (long long)k * P.nens + e;
    double rho_d = gcm[0][c], rho_v = gcm[2][c];
    rho = gcm[0][c] + gcm[2][c] + gcm[3][c] + gcm[4][c];
    double p = (rho_d * P.R_d + rho_v * P.R_v) * gcm[1][c];
    ru = 0; rv = 0; rw = 0;
    rt = pow_pos(P, p / P.C0, 1.0 / P.gamma);
  } else {
    double rho_d = rho_d_c[idx], temp = temp_c[idx];
    double rho_v = trc.p[P.idWV][idx];
    double press = rho_d * P.R_d * temp + rho_v * P.R_v * temp;
    rho = rho_d;
    for (int t = 0; t < P.nt; t++)
      if ((P.mass_mask >> t) & 1ull) rho += trc.p[t][idx];
    double theta = pow_pos(P, press / P.C0, 1.0 / P.gamma) / rho;
    ru = rho * u_c[idx]; rv = rho * v_c[idx]; rw = rho * w_c[idx]; rt = rho * theta;
  }
  const double rrho = fast_rcp(rho);
  const double th = rt * rrho;
  store_rho_pres(P, prim, k, c2, e, rho, th, rt, subtract_hy);
  store_adv(P, prim, P_U, k, c2, ru * rrho, ru * rrho);
  store_adv(P, prim, P_V, k, c2, rv * rrho, rv * rrho);
  store_adv(P, prim, P_W, k, c2, rw * rrho, 0.0);
  store_adv(P, prim, P_THETA, k, c2, th, th);
  for (int t = 0; t < P.nt; t++) {
    double r = 0.0;
    if (!gcm) {
      r = trc.p[t][idx];
      if ((P.pos_mask >> t) & 1ull) r = fmax(0.0, r);           // Dycore.h:130-134
    }
    seed[(long long)t * P.ncell + idx] = r;                      // Dycore.h:156-159
    store_adv(P, prim, P_TR0 + t, k, c2, r * rrho, r * rrho);
  }
}

// prim + seed -> coupler fields.  Dycore.h:1313-1330.
PAMA_D void finalize_body(const Params &P, const double *__restrict__ prim, const double *__restrict__ seed,
                          double *__restrict__ rho_d_c, double *__restrict__ u_c, double *__restrict__ v_c,
                          double *__restrict__ w_c, double *__restrict__ temp_c, const TracerPtrs &trc, const CellId &c) {
  const int k = c.k, j = c.j, i = c.i, e = c.e;
  const long long idx = c.idx;
  const long long o = (long long)(k + HS) * P.sz + (long long)j * P.sy + (long long)i * P.sx + e;
  double rho = prim[P_RHO * P.prim_fs + o];
  double theta = prim[P_THETA * P.prim_fs + o];
  double press = P.C0 * pow_pos(P, rho * theta, P.gamma);
  double rho_v = seed[(long long)P.idWV * P.ncell + idx];
  double rho_d = rho;
  for (int t = 0; t < P.nt; t++) {
    double r = seed[(long long)t * P.ncell + idx];
    if ((P.mass_mask >> t) & 1ull) rho_d -= r;
    trc.p[t][idx] = r;
  }
  rho_d_c[idx] = rho_d;
  u_c[idx] = prim[P_U * P.prim_fs + o];
  v_c[idx] = prim[P_V * P.prim_fs + o];
  w_c[idx] = prim[P_W * P.prim_fs + o];
  temp_c[idx] = press / (rho_d * P.R_d + rho_v * P.R_v);
}

// The reference's own signatures of the two converts take the caller's HALO'D arrays (Dycore.h:1281-1283, :1336-1338):
// state(5, nz+6, ny+6, nx+6, nens) = rho, rho u, rho v, rho w, rho theta and tracers(NT, ...) = tracer densities, interior at
// [hs+k][hs+j][hs+i].  These two bodies are that interface (the resident state of the handle is not involved): coupler fields ->
// interior of the arrays (Dycore.h:1370-1387; halos untouched) and back (Dycore.h:1313-1330).
PAMA_D long long halo_index(const Params &P, int l, int k, int j, int i, int e) {
  return ((((long long)l * (P.nz + 2 * HS) + (k + HS)) * (P.ny + 2 * HS) + (j + HS)) * (P.nx + 2 * HS) + (i + HS)) * P.nens + e;
}
PAMA_D void coupler_to_halo_arrays_body(const Params &P, const double *__restrict__ rho_d_c, const double *__restrict__ u_c,
                                        const double *__restrict__ v_c, const double *__restrict__ w_c,
                                        const double *__restrict__ temp_c, const TracerPtrs &trc, double *__restrict__ state,
                                        double *__restrict__ tracers, const CellId &c) {
  const long long idx = c.idx;
  const double rho_d = rho_d_c[idx], temp = temp_c[idx], rho_v = trc.p[P.idWV][idx];
  const double press = rho_d * P.R_d * temp + rho_v * P.R_v * temp;
  double rho = rho_d;
  for (int t = 0; t < P.nt; t++)
    if ((P.mass_mask >> t) & 1ull) rho += trc.p[t][idx];
  const double theta = pow_pos(P, press / P.C0, 1.0 / P.gamma) / rho;
  state[halo_index(P, 0, c.k, c.j, c.i, c.e)] = rho;
  state[halo_index(P, 1, c.k, c.j, c.i, c.e)] = rho * u_c[idx];
  state[halo_index(P, 2, c.k, c.j, c.i, c.e)] = rho * v_c[idx];
  state[halo_index(P, 3, c.k, c.j, c.i, c.e)] = rho * w_c[idx];
  state[halo_index(P, 4, c.k, c.j, c.i, c.e)] = rho * theta;
  for (int t = 0; t < P.nt; t++) tracers[halo_index(P, t, c.k, c.j, c.i, c.e)] = trc.p[t][idx];
}
PAMA_D void halo_arrays_to_coupler_body(const Params &P, const double *__restrict__ state, const double *__restrict__ tracers,
                                        double *__restrict__ rho_d_c, double *__restrict__ u_c, double *__restrict__ v_c,
                                        double *__restrict__ w_c, double *__restrict__ temp_c, const TracerPtrs &trc, const CellId &c) {
  const long long idx = c.idx;
  const double rho = state[halo_index(P, 0, c.k, c.j, c.i, c.e)];
  const double u = state[halo_index(P, 1, c.k, c.j, c.i, c.e)] / rho, v = state[halo_index(P, 2, c.k, c.j, c.i, c.e)] / rho;
  const double w = state[halo_index(P, 3, c.k, c.j, c.i, c.e)] / rho, theta = state[halo_index(P, 4, c.k, c.j, c.i, c.e)] / rho;
  const double press = P.C0 * pow_pos(P, rho * theta, P.gamma);
  const double rho_v = tracers[halo_index(P, P.idWV, c.k, c.j, c.i, c.e)];
  double rho_d = rho;
  for (int t = 0; t < P.nt; t++) {
    const double r = tracers[halo_index(P, t, c.k, c.j, c.i, c.e)];
    if ((P.mass_mask >> t) & 1ull) rho_d -= r;
    trc.p[t][idx] = r;
  }
  rho_d_c[idx] = rho_d; u_c[idx] = u; v_c[idx] = v; w_c[idx] = w;
  temp_c[idx] = press / (rho_d * P.R_d + rho_v * P.R_v);
}

// CFL time step of one cell (Dycore.h:86-99); the caller min-reduces.
PAMA_D double cfl_body(const Params &P, const double *__restrict__ rho_d_c, const double *__restrict__ u_c,
                       const double *__restrict__ v_c, const double *__restrict__ w_c,
                       const double *__restrict__ temp_c, const double *__restrict__ rho_v_c, double cfl, long long idx) {
  // level and member of the cell (for dz): two 32-bit divisions where the grid allows -- the five 64-bit ones of cell_coords were most
  // of this kernel's instructions (it is a reduction over six fields: 0.87 -> ms at C2)
  long long ke;
  if (P.ncell <= 0xffffffffll) {
    const unsigned c = (unsigned)idx;
    ke = (long long)(c / (unsigned)P.sz) * P.nens + (long long)(c % (unsigned)P.nens);
  } else {
    ke = (idx / P.sz) * P.nens + idx % P.nens;
  }
  double rho_d = rho_d_c[idx], rho_v = rho_v_c[idx], temp = temp_c[idx];
  double rho = rho_d + rho_v;
  double p = (rho_d * P.R_d + rho_v * P.R_v) * temp;
  double cs = sqrt(P.gamma * p / rho);
  double dtx = cfl * P.dx / (fabs(u_c[idx]) + cs);
  double dty = cfl * P.dy / (fabs(v_c[idx]) + cs);
  double dtz = cfl * P.dz[ke] / (fabs(w_c[idx]) + cs);
  // a dry density, a total density or a temperature that is not positive is no state to take a time step from, yet two wrong signs
  // cancel in p / rho (rho_d < -rho_v R_v / R_d, or rho_v < -rho_d: p and rho both negative), cs comes out real and the cell would pass
  // for a healthy one.  With all three positive a negative p gives a NaN cs by itself.  NaN: the caller's reduction keeps it and reports 0
  return (rho_d > 0.0 && rho > 0.0 && temp > 0.0) ? fmin(fmin(dtx, dty), dtz) : NAN;
}

// ------------------------------------------------------------------------------------------------
// Row flags of the FCT multiplier.  The limiter acts in few cells (edges of clouds and rain shafts; never in a smooth positive
// field such as water vapour), so `mult` is 1.0 almost everywhere -- and the tracer update would still read seven of them per
// cell and tracer.  A *row* is (tracer, cell, block of 64 consecutive members), i.e. what one wavefront of the pointwise kernels
// touches per access; flags[row] == seq says "some member of this row was limited by THIS stage's FCT kernel" (seq is the
// stage's launch number, so the flags are never cleared).  The update loads a multiplier only from flagged rows and uses the
// exact value 1.0 otherwise (F * 1.0 == F bitwise): same results, 7 loads per cell and tracer fewer almost everywhere.
//   sparse_store   (FCT kernel) every wavefront of the launch IS one row (member range aligned to 64) and the caller does not
//                  need a complete `mult`: an unflagged row's multipliers are not even stored.  Otherwise (ragged ranges, the
//                  three-kernel stage, the host emulation) they are always stored.
//   any            one int per block of 64 members: == seq when some row of that member block was flagged in this stage (the
//                  fix-up launch leaves at once where it is not).  PER MEMBER BLOCK, not one word: member ranges of one handle
//                  advance on their own streams, and a range that is already a stage ahead must not overwrite the answer of a
//                  range that is about to look (one shared word did exactly that at full C2 size: tools/soak_configs.py)
//   lines          (nt, nz, ny, ceil(nens/64)) ints, same convention: == seq when some row of the x line (k, j) of that tracer and
//                  member block was flagged in this stage.  The fix-up pass of the fused stage (tracer_fixup_line_body) is driven by
//                  them: a wavefront per (tracer, x line, member block) looks at its own line flag and those of the four
//                  neighbouring lines and leaves unless one of them is set.
struct FctRows {
  int *flags;          // (nt, nz, ny, ceil(nens/64), nx); nullptr: no flags, every multiplier is stored and loaded
  int *any;
  int *lines;          // (nt, nz, ny, ceil(nens/64)); nullptr where the stage structure has no use for them
  int seq;
  int sparse_store;
  const int *seq_base; // nullptr, or (a timeStep replayed from a captured HIP graph) a device word that `seq` is relative to: the
                       // launch parameters of a graph are frozen at capture, the stage number advances with every replay
};
// first thing in every kernel that takes FctRows: the stage's flag value as this launch must see it
PAMA_D void fct_rows_resolve(FctRows &r) {
  if (r.seq_base) r.seq += *r.seq_base;
}
PAMA_D long long fct_rows_per_tracer(const Params &P) { return (long long)P.nz * P.ny * P.nx * ((P.nens + 63) >> 6); }
// layout (tracer, level, y, member block, x)
PAMA_D long long fct_row(const Params &P, int k, int j, int i, int e) {
  return (((long long)k * P.ny + j) * ((P.nens + 63) >> 6) + (e >> 6)) * P.nx + i;
}
PAMA_D long long fct_lines_per_tracer(const Params &P) { return (long long)P.nz * P.ny * ((P.nens + 63) >> 6); }
PAMA_D long long fct_line(const Params &P, int k, int j, int e) { return ((long long)k * P.ny + j) * ((P.nens + 63) >> 6) + (e >> 6); }
// "some lane of this wavefront": for decisions to STORE something for the whole row (the host emulation, which runs lane by
// lane, always stores) ...
PAMA_D bool wave_any(bool x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __any(x) != 0;
#else
  return true;
#endif
}
// ... and for decisions to SKIP work that is only needed by lanes with x (correct lane by lane, which is what the host
// emulation does; the device takes one wave-uniform branch)
PAMA_D bool wave_any_or_lane(bool x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __any(x) != 0;
#else
  return x;
#endif
}

// FCT multiplier of a positive-definite tracer in one cell (Dycore.h:533-540) from the mass seed and the six face fluxes:
// 1 unless the fluxes leaving the cell in `dt` carry more than the mass available.
//   rdzk = fast_rcp(dzk).  The three divisions by the grid spacings are reciprocal multiplies (<= 1 ulp each, as in
//   flux_divergence); the one true division -- the multiplier itself -- is executed only by wavefronts with a limited member.
PAMA_D double fct_multiplier(const Params &P, double seed_v, double xlo, double xhi, double ylo, double yhi, double zlo,
                             double zhi, double dzk, double rdzk, double dt) {
#pragma clang fp contract(off)
  const double mass_available = fmax(seed_v, 0.0) * P.dx * P.dy * dzk;
  const double flux_out_x = (fmax(xhi, 0.0) - fmin(xlo, 0.0)) * P.rdx;
  const double flux_out_y = P.sim2d ? 0.0 : (fmax(yhi, 0.0) - fmin(ylo, 0.0)) * P.rdy;
  const double flux_out_z = (fmax(zhi, 0.0) - fmin(zlo, 0.0)) * rdzk;
  const double mass_out = (flux_out_x + flux_out_y + flux_out_z) * dt * P.dx * P.dy * dzk;
  const bool limited = mass_out > mass_available;
  double m = 1.0;
  if (wave_any_or_lane(limited)) m = limited ? mass_available / mass_out : 1.0;
  return m;
}
// Its two sides once more, as functions of their own: the x-sweep forms both before it has the seed (finish_tracer_cell, seed_lower_bound).
// SPELLED A SECOND TIME on purpose -- fct_multiplier written in terms of these two changed the compiler's code for every kernel that
// calls it (docs/experiments.md, "Kernel entry layer"); tests/test_seed_bound.py holds the two spellings to the same bits.
// fct_mass_available is MONOTONE in the seed: fmax, then three rounded products by positive factors (init rejects xlen, ylen and
// dz <= 0), and rounding to nearest preserves <=.
PAMA_D double fct_mass_available(const Params &P, double seed_v, double dzk) {
#pragma clang fp contract(off)
  return fmax(seed_v, 0.0) * P.dx * P.dy * dzk;
}
PAMA_D double fct_mass_out(const Params &P, double xlo, double xhi, double ylo, double yhi, double zlo, double zhi, double dzk,
                           double rdzk, double dt) {
#pragma clang fp contract(off)
  const double flux_out_x = (fmax(xhi, 0.0) - fmin(xlo, 0.0)) * P.rdx;
  const double flux_out_y = P.sim2d ? 0.0 : (fmax(yhi, 0.0) - fmin(ylo, 0.0)) * P.rdy;
  const double flux_out_z = (fmax(zhi, 0.0) - fmin(zlo, 0.0)) * rdzk;
  return (flux_out_x + flux_out_y + flux_out_z) * dt * P.dx * P.dy * dzk;
}

// FCT multiplier of one cell and tracer (Dycore.h:533-540): 1 when the cell is not limited.
//   t0   first tracer to do (test hook)
PAMA_D void fct_mult_body(const Params &P, const double *__restrict__ fx, const double *__restrict__ fy,
                          const double *__restrict__ fz, const double *__restrict__ seed, double *__restrict__ mult,
                          const FctRows &rows, double dt, const CellId &c, int t0 = 0) {
  const int k = c.k, j = c.j, i = c.i, e = c.e;
  const long long idx = c.idx;
  const double dzk = P.dz[(long long)k * P.nens + e];
  const double rdzk = fast_rcp(dzk);
  const long long ip1 = idx + ((i == P.nx - 1) ? -(long long)(P.nx - 1) * P.sx : P.sx);
  const long long jp1 = idx + ((j == P.ny - 1) ? -(long long)(P.ny - 1) * P.sy : P.sy);
  for (int t = t0; t < P.nt; t++) {
    double m = 1.0;
    if ((P.pos_mask >> t) & 1ull) {
      const double *tx = fx + (long long)(5 + t) * P.ncell;
      const double *ty = fy + (long long)(5 + t) * P.ncell;
      const double *tz = fz + (long long)(5 + t) * P.fz_fs;
      m = fct_multiplier(P, seed[(long long)t * P.ncell + idx], tx[idx], tx[ip1], P.sim2d ? 0.0 : ty[idx],
                         P.sim2d ? 0.0 : ty[jp1], tz[idx], tz[idx + P.sz], dzk, rdzk, dt);
    }
    bool store = true;
    if (rows.flags) {
      const bool limited = (m != 1.0);
      if (limited) {
        rows.flags[(long long)t * fct_rows_per_tracer(P) + fct_row(P, k, j, i, e)] = rows.seq;
        rows.any[e >> 6] = rows.seq;
      }
      if (rows.sparse_store) store = wave_any(limited);
    }
    if (store) mult[(long long)t * P.ncell + idx] = m;
  }
}

// Limited tracer flux through a face, given the raw flux F, the multipliers of the cell on the low side (ml) and
// on the high side (mh) of the face.  `seam`: the face is the periodic duplicate pair (face 0 == face n), where the
// reference reconciles the two copies with min() (Dycore.h:574-579): a negative flux stays unlimited there (quirk Q4).
PAMA_D double limited_flux(double F, double ml, double mh, bool seam) {
  if (F > 0.0) return mul_rn(F, ml);
  if (F < 0.0) return seam ? F : mul_rn(F, mh);
  return F;
}



// The flags of the cell's own row and of its six neighbours' (tracer t): was the row flagged by this stage's limiter?  All seven
// are requested unconditionally (a guarded load is a branch with a full memory round trip behind it): in 2-D the y offsets are
// 0, at the walls the z offsets are clamped to the cell itself (and the answer forced to false).
struct NearFlags { bool c, im1, ip1, jm1, jp1, km1, kp1; };
PAMA_D bool any_of(const NearFlags &g) { return g.c | g.im1 | g.ip1 | g.jm1 | g.jp1 | g.km1 | g.kp1; }
PAMA_D NearFlags fct_near_flags(const Params &P, const FctRows &rows, int t, int k, int j, int i, int e) {
  const long long lstride = (long long)((P.nens + 63) >> 6) * P.nx;     // from one x line to the next in y (same member block)
  const int *fl = rows.flags + (long long)t * fct_rows_per_tracer(P) + fct_row(P, k, j, i, e);
  const long long r_ip1 = (i == P.nx - 1) ? -(long long)(P.nx - 1) : 1, r_im1 = (i == 0) ? (long long)(P.nx - 1) : -1;
  const long long r_jp1 = ((j == P.ny - 1) ? -(long long)(P.ny - 1) : 1) * lstride, r_jm1 = ((j == 0) ? (long long)(P.ny - 1) : -1) * lstride;
  const long long r_kz = (long long)P.ny * lstride;
  const bool zl = (k > 0), zh = (k < P.nz - 1);
  const int sq = rows.seq;
  const int a0 = fl[0], a1 = fl[r_im1], a2 = fl[r_ip1], a3 = fl[r_jm1], a4 = fl[r_jp1], a5 = fl[zl ? -r_kz : 0], a6 = fl[zh ? r_kz : 0];
  NearFlags g;
  g.c = (a0 == sq); g.im1 = (a1 == sq); g.ip1 = (a2 == sq); g.jm1 = (a3 == sq); g.jp1 = (a4 == sq);
  g.km1 = zl & (a5 == sq); g.kp1 = zh & (a6 == sq);
  return g;
}
PAMA_D bool fct_flagged_near(const Params &P, const FctRows &rows, int t, int k, int j, int i, int e) {
  return any_of(fct_near_flags(P, rows, t, k, j, i, e));
}

// New conserved value and next FCT seed of one tracer in one cell from its six (limited) face fluxes: divergence, SSPRK3
// combine, clipping (Dycore.h:553-584, :162-221).  q_in / q_0: stage-input / sub-step-start mixing ratio (re-formed as (m/rho)*rho,
// quirk Q5).
template <int STAGE>
PAMA_D void tracer_new_value(const Params &P, int t, double f_x, double f_xp1, double f_y, double f_yp1, double f_z, double f_zp1,
                             double q_in, double q_0, double rho_in, double rho_0, double rdzk, double dt_dyn, double &v,
                             double &new_seed) {
  const double tend = flux_divergence(P, f_x, f_xp1, f_y, f_yp1, f_z, f_zp1, rdzk);
  const double m_in = mul_rn(q_in, rho_in);
  double m_0 = 0.0;
  if (STAGE > 1) m_0 = mul_rn(q_0, rho_0);
  v = rk_combine<STAGE>(m_0, m_in, dt_dyn, tend);
  if ((P.pos_mask >> t) & 1ull) v = fmax(0.0, v);
  new_seed = next_seed<STAGE>(m_0, m_in, v);
}

// Stage update of ONE tracer in one cell (Dycore.h:553-584 with the FCT-limited fluxes, :162-221): shared by the one-kernel
// update (update_body) and by the fix-up pass that follows the fused x-sweeps (tracer_fixup_line_body), so that both paths
// perform the same arithmetic.  rho_in / rho_0: density of the stage input / sub-step start; rrho: reciprocal of the NEW
// density.  Loads of prim_in/prim0 happen before the store (alias-safe).
//   only_near_flagged   (fix-up) the sweep has already stored the update the cell gets when neither it nor a neighbour is
//                       limited (and the cell's own multiplier + row flag): redo the cell only where one of the seven rows is flagged
template <int STAGE>
PAMA_D void tracer_update_one(const Params &P, int t, const double *prim_in, const double *prim0, double *prim_out,
                              const double *__restrict__ fx, const double *__restrict__ fy, const double *__restrict__ fz,
                              const double *__restrict__ mult, const FctRows &rows, double *__restrict__ seed, double dt_dyn,
                              const CellId &c, double rho_in, double rho_0, double rrho, double rdzk, bool only_near_flagged) {
  const int k = c.k, j = c.j, i = c.i, e = c.e;
  const long long idx = c.idx;
  const long long c2 = (long long)j * P.sy + (long long)i * P.sx + e;
  const long long o = (long long)(k + HS) * P.sz + c2;
  const long long ip1 = idx + ((i == P.nx - 1) ? -(long long)(P.nx - 1) * P.sx : P.sx);
  const long long im1 = idx + ((i == 0) ? (long long)(P.nx - 1) * P.sx : -P.sx);
  const long long jp1 = idx + ((j == P.ny - 1) ? -(long long)(P.ny - 1) * P.sy : P.sy);
  const long long jm1 = idx + ((j == 0) ? (long long)(P.ny - 1) * P.sy : -P.sy);
  const double *tx = fx + (long long)(5 + t) * P.ncell, *ty = fy + (long long)(5 + t) * P.ncell;
  const double *tz = fz + (long long)(5 + t) * P.fz_fs;
  const double *mt = mult + (long long)t * P.ncell;
  if (only_near_flagged && rows.flags) {
    if (!wave_any_or_lane(fct_flagged_near(P, rows, t, k, j, i, e))) return;
  }
  // Multipliers of the cell and its six neighbours: loaded only when one of their rows was flagged by this stage's limiter,
  // else exactly 1.0.  ONE wave-uniform branch: the seven flags and every other input of the cell are requested first and are
  // in flight together; in the (rare) flagged case all seven multipliers are loaded unconditionally and the ones from unflagged
  // rows (possibly never written) are discarded by the select.
  const bool zlo = (k > 0), zhi = (k < P.nz - 1);
  double m_c = 1.0, m_im1 = 1.0, m_ip1 = 1.0, m_jm1 = 1.0, m_jp1 = 1.0, m_km1 = 1.0, m_kp1 = 1.0;
  const double Fx = tx[idx], Fxp1 = tx[ip1], Fz = tz[idx], Fzp1 = tz[idx + P.sz];
  const double Fy = P.sim2d ? 0.0 : ty[idx], Fyp1 = P.sim2d ? 0.0 : ty[jp1];
  const int pf = P_TR0 + t;
  const double q_in = prim_in[pf * P.prim_fs + o];
  const double q_0 = (STAGE > 1) ? prim0[pf * P.prim_fs + o] : 0.0;
  if (rows.flags) {
    const NearFlags g = fct_near_flags(P, rows, t, k, j, i, e);
    if (wave_any(any_of(g))) {
      const double l_c = mt[idx], l_im1 = mt[im1], l_ip1 = mt[ip1], l_jm1 = mt[jm1], l_jp1 = mt[jp1];
      const double l_km1 = mt[zlo ? idx - P.sz : idx], l_kp1 = mt[zhi ? idx + P.sz : idx];
      m_c = g.c ? l_c : 1.0; m_im1 = g.im1 ? l_im1 : 1.0; m_ip1 = g.ip1 ? l_ip1 : 1.0;
      m_jm1 = g.jm1 ? l_jm1 : 1.0; m_jp1 = g.jp1 ? l_jp1 : 1.0;
      m_km1 = g.km1 ? l_km1 : 1.0; m_kp1 = g.kp1 ? l_kp1 : 1.0;
    }
  } else {
    m_c = mt[idx]; m_im1 = mt[im1]; m_ip1 = mt[ip1];
    if (!P.sim2d) { m_jm1 = mt[jm1]; m_jp1 = mt[jp1]; }
    if (zlo) m_km1 = mt[idx - P.sz];
    if (zhi) m_kp1 = mt[idx + P.sz];
  }
  double f_x = limited_flux(Fx, m_im1, m_c, i == 0);
  double f_xp1 = limited_flux(Fxp1, m_c, m_ip1, i == P.nx - 1);
  double f_y = 0.0, f_yp1 = 0.0;
  if (!P.sim2d) {
    f_y = limited_flux(Fy, m_jm1, m_c, j == 0);
    f_yp1 = limited_flux(Fyp1, m_c, m_jp1, j == P.ny - 1);
  }
  // vertical: wall faces carry zero flux; interior faces are shared with the cell below / above
  const double f_z = limited_flux(Fz, m_km1, m_c, false);
  const double f_zp1 = limited_flux(Fzp1, m_c, m_kp1, false);
  double v, new_seed;
  tracer_new_value<STAGE>(P, t, f_x, f_xp1, f_y, f_yp1, f_z, f_zp1, q_in, q_0, rho_in, rho_0, rdzk, dt_dyn, v, new_seed);
  seed[(long long)t * P.ncell + idx] = new_seed;
  store_adv(P, prim_out, pf, k, c2, v * rrho, v * rrho);
}

// every tracer of the cell (the one-kernel update of the three-kernel stage)
template <int STAGE>
PAMA_D void tracer_update_part(const Params &P, const double *prim_in, const double *prim0, double *prim_out,
                               const double *__restrict__ fx, const double *__restrict__ fy, const double *__restrict__ fz,
                               const double *__restrict__ mult, const FctRows &rows, double *__restrict__ seed, double dt_dyn,
                               const CellId &c, double rho_in, double rho_0, double rrho, double rdzk) {
  for (int t = 0; t < P.nt; t++)
    tracer_update_one<STAGE>(P, t, prim_in, prim0, prim_out, fx, fy, fz, mult, rows, seed, dt_dyn, c, rho_in, rho_0, rrho, rdzk, false);
}

// Fix-up pass of the fused stage.  Every tracer has been advanced by its x-sweep (water vapour in the state pass of
// flux_x_update_body, the others in x_tracer_sweep) with the update a cell gets when neither it nor one of its six neighbours is
// limited, and the sweeps have stored the multipliers of limited cells, their row flags and -- per tracer, x line and member
// block -- a line flag.  This pass redoes, with the complete arithmetic (tracer_update_one), exactly the neighbourhoods of flagged
// rows.  Work unit: (tracer t, x line (k, j), block of 64 members), lanes = members: five line flags (the line itself and its
// four neighbours in y and z; the x neighbours of a cell are on the line) decide whether the wavefront has anything to do at
// all -- where the limiter is idle (a smooth positive field such as water vapour) it leaves after one round of loads -- and on
// the lines that do, each cell looks at its seven row flags (Dycore.h:525-550, :572-584, :162-221).
template <int STAGE>
PAMA_D void tracer_fixup_line_body(const Params &P, const double *prim_in, const double *prim0, double *prim_out,
                                   const double *__restrict__ fx, const double *__restrict__ fy, const double *__restrict__ fz,
                                   const double *__restrict__ mult, const FctRows &rows, double *__restrict__ seed, double dt_dyn,
                                   int t, int k, int j, int e) {
  {
    const int *ln = rows.lines + (long long)t * fct_lines_per_tracer(P);
    const int sq = rows.seq;
    const bool zl = (k > 0), zh = (k < P.nz - 1);
    const int jm = (j == 0) ? P.ny - 1 : j - 1, jp = (j == P.ny - 1) ? 0 : j + 1;
    const int a0 = ln[fct_line(P, k, j, e)], a1 = ln[fct_line(P, k, jm, e)], a2 = ln[fct_line(P, k, jp, e)];
    const int a3 = ln[fct_line(P, zl ? k - 1 : k, j, e)], a4 = ln[fct_line(P, zh ? k + 1 : k, j, e)];
    if (!wave_any_or_lane((a0 == sq) | (a1 == sq) | (a2 == sq) | (a3 == sq) | (a4 == sq))) return;
  }
  const double rdzk = fast_rcp(P.dz[(long long)k * P.nens + e]);
  for (int i = 0; i < P.nx; i++) {
    if (!wave_any_or_lane(fct_flagged_near(P, rows, t, k, j, i, e))) continue;
    CellId c;
    c.k = k; c.j = j; c.i = i; c.e = e;
    c.idx = (((long long)k * P.ny + j) * P.nx + i) * P.nens + e;
    const long long o = (long long)(k + HS) * P.sz + (long long)j * P.sy + (long long)i * P.sx + e;
    const double rho_new = prim_out[P_RHO * P.prim_fs + o];
    const double rho_in = prim_in[P_RHO * P.prim_fs + o];
    const double rho_0 = (STAGE > 1) ? prim0[P_RHO * P.prim_fs + o] : 0.0;
    tracer_update_one<STAGE>(P, t, prim_in, prim0, prim_out, fx, fy, fz, mult, rows, seed, dt_dyn, c, rho_in, rho_0,
                             fast_rcp(rho_new), rdzk, false);   // (the seven flags were just looked at)
  }
}

// The same fix-up with one lane per CELL (small ensembles: a wavefront per (line, member block) would be one lane): the five line
// flags, then the seven row flags of the cell, then the complete update.  Cells of a wavefront that is in here for a neighbour's
// sake are redone with multipliers of exactly 1: the value the state pass already stored, bit for bit.
template <int STAGE>
PAMA_D void tracer_fixup_cell_body(const Params &P, const double *prim_in, const double *prim0, double *prim_out,
                                   const double *__restrict__ fx, const double *__restrict__ fy, const double *__restrict__ fz,
                                   const double *__restrict__ mult, const FctRows &rows, double *__restrict__ seed, double dt_dyn,
                                   int t, const CellId &c) {
  const int k = c.k, j = c.j, e = c.e;
  {
    const int *ln = rows.lines + (long long)t * fct_lines_per_tracer(P);
    const int sq = rows.seq;
    const bool zl = (k > 0), zh = (k < P.nz - 1);
    const int jm = (j == 0) ? P.ny - 1 : j - 1, jp = (j == P.ny - 1) ? 0 : j + 1;
    const int a0 = ln[fct_line(P, k, j, e)], a1 = ln[fct_line(P, k, jm, e)], a2 = ln[fct_line(P, k, jp, e)];
    const int a3 = ln[fct_line(P, zl ? k - 1 : k, j, e)], a4 = ln[fct_line(P, zh ? k + 1 : k, j, e)];
    if (!wave_any_or_lane((a0 == sq) | (a1 == sq) | (a2 == sq) | (a3 == sq) | (a4 == sq))) return;
  }
  if (!wave_any_or_lane(fct_flagged_near(P, rows, t, k, j, c.i, e))) return;
  const double rdzk = fast_rcp(P.dz[(long long)k * P.nens + e]);
  const long long o = (long long)(k + HS) * P.sz + (long long)j * P.sy + (long long)c.i * P.sx + e;
  const double rho_new = prim_out[P_RHO * P.prim_fs + o];
  const double rho_in = prim_in[P_RHO * P.prim_fs + o];
  const double rho_0 = (STAGE > 1) ? prim0[P_RHO * P.prim_fs + o] : 0.0;
  tracer_update_one<STAGE>(P, t, prim_in, prim0, prim_out, fx, fy, fz, mult, rows, seed, dt_dyn, c, rho_in, rho_0,
                           fast_rcp(rho_new), rdzk, false);
}

// Pointwise remainder of the fused stage: the next stage's pressure (Dycore.h:310-321) and the density / pressure ghosts
// (:682-709).  The state variables and every tracer were advanced by the fused x-sweeps (flux_x_update_body), which left the
// new density, the new theta and -- in the pressure slot -- the new rho*theta in prim_out: a pow per cell and nothing else, so
// few registers and full occupancy (kept out of the register-critical sweep loop; VALU-bound on the pow).
PAMA_D void pressure_tail_body(const Params &P, double *prim_out, const CellId &c) {
  const long long c2 = (long long)c.j * P.sy + (long long)c.i * P.sx + c.e;
  const long long o = (long long)(c.k + HS) * P.sz + c2;
  // theta and the new density are needed for the density/pressure ghosts only, i.e. on the two boundary levels
  const bool boundary = (c.k == 0 || c.k == P.nz - 1);
  const double th = boundary ? prim_out[P_THETA * P.prim_fs + o] : 0.0;
  const double rho_theta = prim_out[P_PRES * P.prim_fs + o];
  const double rho_new = boundary ? prim_out[P_RHO * P.prim_fs + o] : 0.0;
  store_rho_pres<false>(P, prim_out, c.k, c2, c.e, rho_new, th, rho_theta, !P.grav_balance);
}

// Flux divergence + gravity (Dycore.h:553-584), SSPRK3 combine of this stage (Dycore.h:162-221), clipping, next
// FCT seed, then the next stage's pressure / division by rho / vertical ghosts (store_adv, store_rho_pres).
//   STAGE 1: out = in' + dt T                      seed = 3/4 in' + 1/4 out
//   STAGE 2: out = 3/4 q0' + 1/4 in' + 1/4 dt T    seed = 1/3 q0' + 2/3 out
//   STAGE 3: out = 1/3 q0' + 2/3 in' + 2/3 dt T    seed = out (exact conserved tracer mass for the next sub-step)
// in' / q0' are the conserved values re-formed as (m/rho)*rho exactly as the reference's in-place round trip
// (Dycore.h:316-320,527-532).  prim_in is the stage input, prim0 the sub-step start (STAGE>1).
// prim_out may alias prim_in (stage 2) or prim0 (stage 3): the update is pointwise (every input of the cell is read
// before its outputs are written), so no __restrict__ on those.
template <int STAGE>
PAMA_D void update_body(const Params &P, const double *prim_in, const double *prim0,
                        double *prim_out, const double *__restrict__ fx, const double *__restrict__ fy,
                        const double *__restrict__ fz, const double *__restrict__ mult, const FctRows &rows,
                        double *__restrict__ seed, double dt_dyn, const CellId &c) {
  const int k = c.k, j = c.j, i = c.i, e = c.e;
  const long long idx = c.idx;
  const long long c2 = (long long)j * P.sy + (long long)i * P.sx + e;
  const long long o = (long long)(k + HS) * P.sz + c2;
  const long long ke = (long long)k * P.nens + e;
  const double dzk = P.dz[ke];
  const double rdzk = fast_rcp(dzk);
  const long long ip1 = idx + ((i == P.nx - 1) ? -(long long)(P.nx - 1) * P.sx : P.sx);
  const long long im1 = idx + ((i == 0) ? (long long)(P.nx - 1) * P.sx : -P.sx);
  const long long jp1 = idx + ((j == P.ny - 1) ? -(long long)(P.ny - 1) * P.sy : P.sy);
  const long long jm1 = idx + ((j == 0) ? (long long)(P.ny - 1) * P.sy : -P.sy);
  const double rho_in = prim_in[P_RHO * P.prim_fs + o];
  const double rho_0 = (STAGE > 1) ? prim0[P_RHO * P.prim_fs + o] : 0.0;
  // state variables: l = 0 rho, 1 rho u, 2 rho v, 3 rho w, 4 rho theta (all inputs read before any store)
  double qs[5];
#pragma unroll
  for (int l = 0; l < 5; l++) {
    const double *sx_ = fx + (long long)l * P.ncell, *sy_ = fy + (long long)l * P.ncell, *sz_ = fz + (long long)l * P.fz_fs;
    const double ylo = P.sim2d ? 0.0 : sy_[idx], yhi = P.sim2d ? 0.0 : sy_[jp1];   // no y-flux array in 2-D
    // (density: (x + y) + z; momentum and rho*theta: x + (y + z) -- see yz_divergence)
    double tend = (l == 0) ? flux_divergence(P, sx_[idx], sx_[ip1], ylo, yhi, sz_[idx], sz_[idx + P.sz], rdzk)
                           : flux_divergence_d(P, sx_[idx], sx_[ip1], ylo - yhi, sz_[idx] - sz_[idx + P.sz], rdzk);
    if (l == 3) tend = add_gravity(P, tend, rho_in, gravity_coef(P, ke));
    if (l == 2 && P.sim2d) tend = 0.0;
    const int pf = (l == 0) ? P_RHO : P_U + (l - 1);
    double m_in = prim_in[pf * P.prim_fs + o];
    if (l > 0) m_in = mul_rn(m_in, rho_in);
    double m_0 = 0.0;
    if (STAGE > 1) {
      m_0 = prim0[pf * P.prim_fs + o];
      if (l > 0) m_0 = mul_rn(m_0, rho_0);
    }
    qs[l] = rk_combine<STAGE>(m_0, m_in, dt_dyn, tend);
  }
  const double rrho = fast_rcp(qs[0]);
  const double th = qs[4] * rrho;
  tracer_update_part<STAGE>(P, prim_in, prim0, prim_out, fx, fy, fz, mult, rows, seed, dt_dyn, c, rho_in, rho_0, rrho, rdzk);
  store_rho_pres(P, prim_out, k, c2, e, qs[0], th, qs[4], !P.grav_balance);
  store_adv(P, prim_out, P_U, k, c2, qs[1] * rrho, qs[1] * rrho);
  store_adv(P, prim_out, P_V, k, c2, qs[2] * rrho, qs[2] * rrho);
  store_adv(P, prim_out, P_W, k, c2, qs[3] * rrho, 0.0);
  store_adv(P, prim_out, P_THETA, k, c2, th, th);
}

// FCT multiplier of one tracer in one cell, formed inside an x-sweep with all six face fluxes of the cell at hand (Dycore.h:525-540):
// final for THIS cell.  Row flag set where it is not 1.
//   DENSE   false (water vapour, state pass): stored only in rows with a limited member, and the line flag and the "any" word are set
//           (the fix-up pass reads multipliers through the flags);  true (further tracers, phase 1): always stored -- phase 2 reads
//           it without looking at flags
//   ix: offset of the cell inside an interior-sized field (wave-uniform)
template <bool DENSE>
PAMA_D void own_multiplier_cell(const Params &P, int t, double *__restrict__ mult, const FctRows &rows, int k, int j, int i, int e,
                                unsigned eu, long long ix, double F_lo, double F_hi, double yl, double yh, double zl, double zh,
                                double seed_v, double dzk, double rdzk, double dt_stage) {
  const bool pos = ((P.pos_mask >> t) & 1ull) != 0;
  const double m_t = pos ? fct_multiplier(P, seed_v, F_lo, F_hi, yl, yh, zl, zh, dzk, rdzk, dt_stage) : 1.0;
  const bool limited = (m_t != 1.0);
  double *mt = mult + (long long)t * P.ncell + ix;
  if (rows.flags) {
    if (limited) {
      rows.flags[(long long)t * fct_rows_per_tracer(P) + fct_row(P, k, j, i, e)] = rows.seq;
      if (!DENSE && rows.lines) rows.lines[(long long)t * fct_lines_per_tracer(P) + fct_line(P, k, j, e)] = rows.seq;
      if (!DENSE) rows.any[e >> 6] = rows.seq;  // ("some row of water vapour in this member block": the fix-up pass has work)
    }
    // (sparse: only where a wavefront IS a row -- 64 members of one cell.  In the tile kernels a row may be narrower than a
    // wavefront and straddle two of them: the half without a limited member must still store its multipliers, the row is flagged)
    if (DENSE || !rows.sparse_store || wave_any(limited)) uniw(mt)[eu] = m_t;
  } else {
    uniw(mt)[eu] = m_t;
  }
}
// ... its flag and store part for a multiplier the caller has formed (finish_tracer_cell<., true>; a second spelling, as fct_mass_out)
template <bool DENSE>
PAMA_D void own_multiplier_store(const Params &P, int t, double *__restrict__ mult, const FctRows &rows, int k, int j, int i, int e,
                                 unsigned eu, long long ix, double m_t) {
  const bool limited = (m_t != 1.0);
  double *mt = mult + (long long)t * P.ncell + ix;
  if (rows.flags) {
    if (limited) {
      rows.flags[(long long)t * fct_rows_per_tracer(P) + fct_row(P, k, j, i, e)] = rows.seq;
      if (!DENSE && rows.lines) rows.lines[(long long)t * fct_lines_per_tracer(P) + fct_line(P, k, j, e)] = rows.seq;
      if (!DENSE) rows.any[e >> 6] = rows.seq;  // ("some row of water vapour in this member block": the fix-up pass has work)
    }
    // (sparse: only where a wavefront IS a row -- 64 members of one cell.  In the tile kernels a row may be narrower than a
    // wavefront and straddle two of them: the half without a limited member must still store its multipliers, the row is flagged)
    if (DENSE || !rows.sparse_store || wave_any(limited)) uniw(mt)[eu] = m_t;
  } else {
    uniw(mt)[eu] = m_t;
  }
}

// Tracer 0 of one cell finished inside the state pass of the fused x-sweep (Dycore.h:525-550, :572-584, :162-221): its own
// multiplier (above), and the cell's update as it is unless the cell or a neighbour is limited -- tracer_fixup_line_body redoes
// exactly those neighbourhoods afterwards.  (Water vapour: a smooth positive field, the limiter is idle almost everywhere.)
//   cu: offset of (j, i, member 0) inside a level
//   LAZY_SEED   the caller has NOT loaded the seed (seed_v is ignored).  The mass leaving the cell is compared with what a lower bound of
//               the seed makes available (seed_lower_bound, from values the update needs anyway); only a wavefront in which that does
//               not settle some member's answer loads the seed and runs fct_multiplier as it is.  Elsewhere the multiplier is exactly
//               1, as fct_multiplier would have found: same stores, same flags.  `!(a <= b)`: a NaN on either side takes the load.
//               A tracer that is not positive-definite never had a use for its seed.
#ifndef PAMA_SEED_SKIP_NOTE
#define PAMA_SEED_SKIP_NOTE(P, t, k, j, i, e, loaded)     // (the host emulation counts the rows of either path)
#endif
template <int STAGE, bool LAZY_SEED = false>
PAMA_D void finish_tracer_cell(const Params &P, int t, double *prim_out, double *__restrict__ seed, double *__restrict__ mult,
                               const FctRows &rows, int k, int j, int i, int e, unsigned eu, long long cu, long long ix,
                               double F_lo, double F_hi, double yl, double yh, double zl, double zh, double seed_v, double q_in,
                               double q_0, double rho_in, double rho_0, double rrho, double dzk, double rdzk, double dt_dyn,
                               double dt_stage) {
  if constexpr (LAZY_SEED) {
    double m_t = 1.0;
    if ((P.pos_mask >> t) & 1ull) {
      const double m_in = mul_rn(q_in, rho_in), m_0 = (STAGE > 1) ? mul_rn(q_0, rho_0) : 0.0;
      const double at_least = fct_mass_available(P, seed_lower_bound<STAGE>(m_0, m_in, q_in, rho_in), dzk);
      const double mass_out = fct_mass_out(P, F_lo, F_hi, yl, yh, zl, zh, dzk, rdzk, dt_stage);
      const bool open = !(mass_out <= at_least);
      if (wave_any_or_lane(open))
        m_t = fct_multiplier(P, ld_once<PAMA_STREAM_X1>(uni(seed + (long long)t * P.ncell + ix), eu), F_lo, F_hi, yl, yh, zl, zh, dzk, rdzk, dt_stage);
      PAMA_SEED_SKIP_NOTE(P, t, k, j, i, e, open);
    }
    own_multiplier_store<false>(P, t, mult, rows, k, j, i, e, eu, ix, m_t);
  } else {
    own_multiplier_cell<false>(P, t, mult, rows, k, j, i, e, eu, ix, F_lo, F_hi, yl, yh, zl, zh, seed_v, dzk, rdzk, dt_stage);
  }
  double v, new_seed;
  tracer_new_value<STAGE>(P, t, F_lo, F_hi, yl, yh, zl, zh, q_in, q_0, rho_in, rho_0, rdzk, dt_dyn, v, new_seed);
  uniw(seed + (long long)t * P.ncell + ix)[eu] = new_seed;
  store_adv_u(P, prim_out, P_TR0 + t, k, cu, eu, v * rrho, v * rrho);
}

// x sweeps of the further tracers in the fused stage (advected-field indices fa[0..NF): 5 = tracer 1, ...), NF at a time, over the
// cells c0..c0+span-1 of one periodic x line; upwinded by the face mass flux the state pass left in flux_x field 0 (Dycore.h:367-385).
// These tracers (cloud, rain, ice ...: blobs with exact zeros around them) are limited in a large part of their cells, stage after
// stage, so the "finish in the sweep, redo the few limited neighbourhoods" scheme of water vapour would redo most cells.  Instead the
// line is swept TWICE and the x fluxes never reach memory:
//   PHASE 1   x fluxes -> with the y/z faces and the mass seed of the cell: its FCT multiplier (own_multiplier_cell; Dycore.h:525-540),
//             stored for EVERY cell (a complete field: no flags to consult in phase 2).  Nothing else is written.
//   PHASE 2   (a later launch: the multipliers of the neighbouring lines must be complete) the same x fluxes again -- same inputs,
//             same code, same bits -- and the complete update of every cell: the six faces limited by the multipliers of the cell
//             and its six neighbours (Dycore.h:541-548, :572-579), divergence, SSPRK3 combine, clipping, next seed (:553-584, :162-221;
//             the arithmetic of tracer_update_one).  The multipliers along the line slide through registers (one load per cell),
//             those of the y/z neighbours are loaded (two / four per cell, shared with the neighbouring lines' sweeps through L2).
// Against "x faces -> FCT kernel -> pointwise update" this trades one more polynomial per tracer and cell (the sweeps are
// HBM-bound) for ~4 of 14 field passes per tracer and stage, and two launches for none of the flag traffic.  One polynomial
// per cell and phase.
//   have_close / ruf_close   the mass flux through the face that closes the span's last cell (face c1; it belongs to the next span, or
//                            is the periodic face nx == face 0), handed over in a register when this sweep runs inline after the state
//                            pass of the same wavefront -- another wavefront of the SAME launch may still be writing it to flux_x.  In
//                            a launch of its own (awfl_xtr_kernel) it is read from flux_x like the others.
template <int NF, int STAGE, int PHASE, bool AHEAD = false>
PAMA_D void x_tracer_sweep(const Params &P, const double *__restrict__ prim_in, const double *__restrict__ prim0,
                           double *__restrict__ prim_out, const double *__restrict__ fx, const double *__restrict__ fy,
                           const double *__restrict__ fz, double *__restrict__ seed, double *__restrict__ mult,
                           const FctRows &rows, int line, int e, int c0, int span, const int *fa, double dt_dyn, double dt_stage,
                           bool have_close, double ruf_close) {
  const unsigned eu = member_offset(e);
  const WenoConsts wc = weno_consts();
  const int nx = P.nx;
  const int c1 = (c0 + span < nx) ? c0 + span : nx;      // cells c0 .. c1-1, faces c0 .. c1
  const int k = uni_int(line / P.ny), j = line - k * P.ny;
  const long long cu0 = (long long)j * P.sy;
  const long long pbase = (long long)(k + HS) * P.sz + cu0, fbase = (long long)k * P.sz + cu0;
  const long long jp1 = (j == P.ny - 1) ? -(long long)(P.ny - 1) * P.sy : P.sy;
  const long long jm1 = (j == 0) ? (long long)(P.ny - 1) * P.sy : -P.sy;
  const long long ke = (long long)k * P.nens + e;
  const double dzk = P.dz[ke];
  const double rdzk = fast_rcp(dzk);
  const bool have_y = !P.sim2d;
  const bool zlo = (k > 0), zhi = (k < P.nz - 1);
  const double *ruf_line = fx + fbase;
  auto cell_off = [&](int c) -> long long { return pbase + (long long)(c < 0 ? c + nx : (c >= nx ? c - nx : c)) * P.sx; };
  const double *q[NF], *q0p[NF], *fyt[NF], *fzt[NF];
  int tt[NF];
  double w[NF][5], prevR[NF], F_prev[NF];
#pragma unroll
  for (int n = 0; n < NF; n++) {
    tt[n] = fa[n] - 4;                                   // tracer index
    q[n] = prim_in + (long long)(P_U + fa[n]) * P.prim_fs;
    q0p[n] = prim0 + (long long)(P_U + fa[n]) * P.prim_fs;
    fyt[n] = fy + (long long)(1 + fa[n]) * P.ncell;
    fzt[n] = fz + (long long)(1 + fa[n]) * P.fz_fs;
    F_prev[n] = 0.0;
  }
  const double *pr = prim_in + (long long)P_RHO * P.prim_fs, *r0 = prim0 + (long long)P_RHO * P.prim_fs;
  const double *rn = prim_out + (long long)P_RHO * P.prim_fs;   // the new density: written by the state pass (an earlier launch)
  // PHASE 2: multipliers of the line's cells, sliding: before trip c (mA, mB) = cells (c-2, c-1); the trip loads cell c
  const double *mline[NF];
  double mA[NF], mB[NF];
#pragma unroll
  for (int n = 0; n < NF; n++) {
    mline[n] = mult + (long long)tt[n] * P.ncell + fbase;
    mA[n] = mB[n] = 1.0;
    if (PHASE == 2) mB[n] = uni(mline[n] + (long long)(c0 == 0 ? nx - 1 : c0 - 1) * P.sx)[eu];
  }
#pragma unroll
  for (int s = 0; s < 5; s++) {                          // cells c0-3..c0+1: the window of cell c0-1
    const long long o = cell_off(c0 - 3 + s);
#pragma unroll
    for (int n = 0; n < NF; n++) w[n][s] = uni(q[n] + o)[eu];
  }
  {                                                      // cell c0-1: only its right-edge value is needed (face c0)
    const long long on = cell_off(c0 + 2);
#pragma unroll
    for (int n = 0; n < NF; n++) {
      double L;
      weno5_const(w[n], wc, L, prevR[n]);
#pragma unroll
      for (int s = 0; s < 4; s++) w[n][s] = w[n][s + 1];
      w[n][4] = uni(q[n] + on)[eu];
    }
  }
  // everything one trip loads: the cell that enters the windows (c + 3), the face mass flux of face c, and what the cell this trip
  // completes (cc = c - 1) needs besides its x fluxes -- loaded on EVERY trip, also the first one, which completes no cell (see
  // flux_x_update_body: s_waitcnt counts are a static minimum over all paths)
  struct Trip {
    double nq[NF], ruf, rho_in, rho_0, rho_new;
    double yl[NF], yh[NF], zl[NF], zh[NF], sd[NF], q_0[NF], m_new[NF], m_jm1[NF], m_jp1[NF], m_km1[NF], m_kp1[NF];
  };
  auto load_trip = [&](int c, Trip &T) {
    const long long on = cell_off(c + 3);
#pragma unroll
    for (int n = 0; n < NF; n++) T.nq[n] = uni(q[n] + on)[eu];
    T.ruf = uni(ruf_line + (long long)(c == nx ? 0 : c) * P.sx)[eu];
    const int cc = c > c0 ? c - 1 : c0;
    const long long o = pbase + (long long)cc * P.sx, ix = fbase + (long long)cc * P.sx;
    T.rho_in = 0.0; T.rho_0 = 0.0; T.rho_new = 1.0;
    if (PHASE == 2) {
      T.rho_in = uni(pr + o)[eu];
      T.rho_0 = (STAGE > 1) ? uni(r0 + o)[eu] : 0.0;
      T.rho_new = uni(rn + o)[eu];
    }
#pragma unroll
    for (int n = 0; n < NF; n++) {
      T.yl[n] = have_y ? uni(fyt[n] + ix)[eu] : 0.0;
      T.yh[n] = have_y ? uni(fyt[n] + ix + jp1)[eu] : 0.0;
      T.zl[n] = uni(fzt[n] + ix)[eu];
      T.zh[n] = uni(fzt[n] + ix + P.sz)[eu];
      T.sd[n] = (PHASE == 1) ? uni(seed + (long long)tt[n] * P.ncell + ix)[eu] : 0.0;
      T.q_0[n] = (PHASE == 2 && STAGE > 1) ? uni(q0p[n] + o)[eu] : 0.0;
      T.m_jm1[n] = T.m_jp1[n] = T.m_km1[n] = T.m_kp1[n] = T.m_new[n] = 1.0;
      if (PHASE == 2) {
        T.m_new[n] = uni(mline[n] + (long long)(c == nx ? 0 : c) * P.sx)[eu];                       // cell c: the x neighbour of cell cc
        if (have_y) { T.m_jm1[n] = uni(mline[n] + (long long)cc * P.sx + jm1)[eu]; T.m_jp1[n] = uni(mline[n] + (long long)cc * P.sx + jp1)[eu]; }
        if (zlo) T.m_km1[n] = uni(mline[n] + (long long)cc * P.sx - P.sz)[eu];
        if (zhi) T.m_kp1[n] = uni(mline[n] + (long long)cc * P.sx + P.sz)[eu];
      }
    }
  };
  // AHEAD (experiment (b) of VERDICT r3 / r4): trip c + 1's loads are requested before trip c's polynomials are built -- one more
  // trip of latency hidden per wavefront, one more set of loaded values (2 + 6 NF doubles in 2-D) in registers
  Trip Tn;
  if (AHEAD) load_trip(c0, Tn);
#pragma clang loop unroll(disable)
  for (int c = c0; c <= c1; c++) {                       // window = cells c-2..c+2; face c1 closes the last cell
    Trip T;
    if (AHEAD) {
      T = Tn;
      if (c < c1) load_trip(c + 1, Tn);
    } else {
      load_trip(c, T);
    }
    double L[NF], R[NF];
    double ruf = T.ruf;
    if (have_close && c == c1) ruf = ruf_close;
    const int cc = c > c0 ? c - 1 : c0;
    const long long ix = fbase + (long long)cc * P.sx;
    const double rho_in = T.rho_in, rho_0 = T.rho_0, rho_new = T.rho_new;
    const double (&nq)[NF] = T.nq, (&yl)[NF] = T.yl, (&yh)[NF] = T.yh, (&zl)[NF] = T.zl, (&zh)[NF] = T.zh, (&sd)[NF] = T.sd, (&q_0)[NF] = T.q_0;
    const double (&m_new)[NF] = T.m_new, (&m_jm1)[NF] = T.m_jm1, (&m_jp1)[NF] = T.m_jp1, (&m_km1)[NF] = T.m_km1, (&m_kp1)[NF] = T.m_kp1;
#pragma unroll
    for (int n = 0; n < NF; n++) weno5_const(w[n], wc, L[n], R[n]);
    const bool up = ruf > 0.0;                              // upwind (Dycore.h:368)
    const double rrho = (PHASE == 2) ? fast_rcp(rho_new) : 0.0;
#pragma unroll
    for (int n = 0; n < NF; n++) {
      const double F = mul_rn(ruf, up ? prevR[n] : L[n]);
      if (c > c0) {                                         // cell cc = c-1 is complete; window element 1 is its stage-input value
        if (PHASE == 1) {
          own_multiplier_cell<true>(P, tt[n], mult, rows, k, j, cc, e, eu, ix, F_prev[n], F, yl[n], yh[n], zl[n], zh[n], sd[n], dzk, rdzk, dt_stage);
        } else {                                            // multipliers of cells cc-1, cc, cc+1: mA, mB, m_new
          const double f_x = limited_flux(F_prev[n], mA[n], mB[n], cc == 0);
          const double f_xp1 = limited_flux(F, mB[n], m_new[n], cc == nx - 1);
          double f_y = 0.0, f_yp1 = 0.0;
          if (have_y) {
            f_y = limited_flux(yl[n], m_jm1[n], mB[n], j == 0);
            f_yp1 = limited_flux(yh[n], mB[n], m_jp1[n], j == P.ny - 1);
          }
          const double f_z = limited_flux(zl[n], m_km1[n], mB[n], false);
          const double f_zp1 = limited_flux(zh[n], mB[n], m_kp1[n], false);
          double v, new_seed;
          tracer_new_value<STAGE>(P, tt[n], f_x, f_xp1, f_y, f_yp1, f_z, f_zp1, w[n][1], q_0[n], rho_in, rho_0, rdzk, dt_dyn, v, new_seed);
          uniw(seed + (long long)tt[n] * P.ncell + ix)[eu] = new_seed;
          store_adv_u(P, prim_out, P_TR0 + tt[n], k, cu0 + (long long)cc * P.sx, eu, v * rrho, v * rrho);
        }
      }
      F_prev[n] = F;
      prevR[n] = R[n];
      mA[n] = mB[n];
      mB[n] = m_new[n];
#pragma unroll
      for (int s = 0; s < 4; s++) w[n][s] = w[n][s + 1];
      w[n][4] = nq[n];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// In-sweep pressure of the fused x-sweep (NT = 1).  The sweep loop has no register left for the pow that turns a cell's new rho*theta
// into the next stage's pressure, so a lane parks the rho*theta of every cell it completes in a slot of its own (on the device: LDS,
// XSTASH_CELLS x XSTASH_LANES doubles per wavefront; a lane reads only what it wrote, so nothing synchronises) and works the slots off
// behind the loop, where nothing of the loop is live any more.  NoStash switches all of it off at compile time.
constexpr int XSTASH_CELLS = 32;     // cells of a span that a stash holds: longer spans keep the separate pressure pass
constexpr int XSTASH_LANES = 64;     // slots of one cell: a lane's cell n is slot[n * XSTASH_LANES]
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) double *stash_ptr;
#else
typedef double *stash_ptr;
#endif
struct NoStash { static constexpr bool on = false; };
// slot: the lane's slot of the span's first cell (one address register, advanced by one vector add per trip of the sweep loop; forming
// the lane's part anew on every trip from the member offset costs no register but more scalar spills: measured, docs/experiments.md)
struct LineStash { static constexpr bool on = true; stash_ptr slot; };

// The pressure pass of the cells c0 .. c1-1 of line (k, j) by the lane that has just completed them: pressure_tail_body's values
// (rho*theta from the stash instead of prim_out[P_PRES]; on the two boundary levels theta and the new density are the lane's own
// stores to prim_out, read back in program order) through the same store_rho_pres<false>.  P.pw: on the device the caller's LDS copy.
// The member comes as the offset `eu` the sweep addresses with, behind an opaque copy: whatever the epilogue derives from it per lane
// (the addresses of dz and hy_pres, the cell's offset) is then formed here, behind the loop, instead of living across it in registers.
PAMA_D void xsweep_pressure_epilogue(const Params &P, double *prim_out, const NoStash &, int, long long, unsigned, int, int) {}
PAMA_D void xsweep_pressure_epilogue(const Params &P, double *prim_out, const LineStash &stash, int k, long long cu0, unsigned eu, int c0, int c1) {
  const bool boundary = (k == 0 || k == P.nz - 1);
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(eu));
#endif
  const int e = (int)eu;
#pragma clang loop unroll(disable)
  for (int cc = c0; cc < c1; cc++) {
    const long long cu = cu0 + (long long)cc * P.sx, c2 = cu + e;
    const long long ou = (long long)(k + HS) * P.sz + cu;         // the cell of member 0 inside a prim field (uniform)
    const double th = boundary ? uni(prim_out + P_THETA * P.prim_fs + ou)[eu] : 0.0;
    const double rho_theta = stash.slot[(cc - c0) * XSTASH_LANES];
    const double rho_new = boundary ? uni(prim_out + P_RHO * P.prim_fs + ou)[eu] : 0.0;
    store_rho_pres<false>(P, prim_out, k, c2, e, rho_new, th, rho_theta, !P.grav_balance);
  }
}

// ------------------------------------------------------------------------------------------------
// FUSED x-sweep: reconstruction + fluxes in x (as flux_line_body<0>) AND, in the same pass, the stage update of the five
// state variables of every cell of the line (as update_body), with the y and z flux differences of the cell read from the
// arrays the y/z sweeps (flux_line_body<.., DIFF = true>) wrote earlier.  Reference: Dycore.h:334-386 (x fluxes), :553-571 (divergence, gravity), :162-221 (SSPRK3
// combine), next stage's :310-321 (divide by rho) and :662-710 (vertical ghosts of the advected variables).
//
// Why: in the three-kernel stage every x face flux of the state makes a round trip through HBM (written by the flux
// kernel, read back by the update kernel) and the update kernel re-reads the stage input the x-sweep has just had in
// registers.  Here a wavefront owns a whole periodic x line (k, j) of 64 members: when faces c-1 and c of a variable are
// known, cell c-1 is complete -- its x flux difference never leaves the registers, its stage-input value is the window
// element the polynomial was built from, and only the y/z flux differences and the sub-step-start value are loaded.  The
// x fluxes of the state are never stored (except the mass flux, for the tracer sweeps), nor are those of the further tracers
// (x_tracer_sweep forms them twice); only water vapour's is kept, for the fix-up pass (tracer_fixup_line_body).
//
// Passes over the line (5-cell sliding windows, one polynomial per cell, as flux_line_body):
//   state    rho*u, p, u, v, w, theta and water vapour together (seven independent polynomial chains per cell): face mass flux
//            ruf and face pressure, the x fluxes of all five state variables, and the complete update of every cell: new density,
//            u, v, w, theta density-divided to prim_out (+ vertical ghosts when k is a boundary level); the new rho*theta goes to
//            prim_out[P_PRES] for the pressure pass that follows (pressure_tail_body: next stage's pressure and density/pressure
//            ghosts); water vapour finished as well (own FCT multiplier, the update an unlimited neighbourhood gets).  ruf is
//            also written to flux_x field 0 for the tracer sweeps (the lane's own line, L2-resident; no LDS, so residency is
//            bounded by registers only).  Each input is read exactly once.
//   tracers  phase 1 of the further tracers' sweeps (x_tracer_sweep), FLUX_NF at a time, upwinded by the ruf read back.
// prim_in, prim0 and prim_out must be three different buffers: the line is periodic (cells 0..2 are read again at the
// end of the sweep) and later passes re-read the stage-input density, so nothing may be updated in place.
// Bit-for-bit the arithmetic of flux_line_body<0> + update_body (shared helpers above; tests/test_fused_stage.py).
//   line   wave-uniform index of the x line: k * ny + j          e   ensemble member of this lane
//   tracers_inline   phase 1 of the further tracers here (else the caller launches awfl_xtr_kernel<., 1>)
//   FOLD   the z sweep has folded the y differences of the state variables into the field it stores (flux_line_body_zt<., FOLD>;
//          P.yz_fold, 3-D only): the z array holds the y+z part of each variable's divergence and the y differences are not loaded
//   stash  NoStash: the new rho*theta goes to prim_out[P_PRES] and pressure_tail_body follows in a pass of its own.  LineStash
//          (NT = 1 -- no further tracers are swept and no mass flux is kept for them; spans of at most XSTASH_CELLS cells): the lane keeps the rho*theta of the cells it completes in slots of its
//          own and, behind the sweep loop, makes the next stage's pressure of them itself (xsweep_pressure_epilogue: the arithmetic
//          of pressure_tail_body on the same doubles -- same bits, no pressure pass, rho*theta never leaves the CU)
//   LAZY_SEED  water vapour's FCT seed is loaded only by wavefronts that cannot tell without it (finish_tracer_cell; seeds of this
//          library's own chain only: seed_lower_bound)
template <int STAGE, bool FOLD = false, class Stash = NoStash, bool LAZY_SEED = false>
PAMA_D void flux_x_update_body(const Params &P, const double *__restrict__ prim_in, const double *__restrict__ prim0,
                               double *__restrict__ prim_out, double *__restrict__ fx, const double *__restrict__ fy,
                               const double *__restrict__ fz, double *__restrict__ seed, double *__restrict__ mult,
                               const FctRows &rows, int line, int e, int c0, int span, double dt_dyn, double dt_stage,
                               bool tracers_inline, const Stash stash = Stash()) {
  const unsigned eu = member_offset(e);
  const WenoConsts wc = weno_consts();
  const int nx = P.nx;
  const int c1 = (c0 + span < nx) ? c0 + span : nx;      // this wavefront owns the cells c0 .. c1-1 (faces c0 .. c1)
  const int k = uni_int(line / P.ny), j = line - k * P.ny;   // (integer division runs on the vector unit: re-assert uniformity)
  const long long cu0 = (long long)j * P.sy;                          // (j, i=0, member 0) inside a level
  const long long pbase = (long long)(k + HS) * P.sz + cu0;            // cell i=0 inside a prim field (uniform)
  const long long fbase = (long long)k * P.sz + cu0;                   // cell / face i=0 inside an interior-sized field
  const long long jp1 = (j == P.ny - 1) ? -(long long)(P.ny - 1) * P.sy : P.sy;   // offset of the (j+1) neighbour
  const long long ke = (long long)k * P.nens + e;
  const double dzk = P.dz[ke];
  const double rdzk = fast_rcp(dzk);
  const double gcoef = gravity_coef(P, ke);
  const bool have_y = !P.sim2d;
  double ruf_close = 0.0;                                              // mass flux through the face that closes the span (face c1)
  double *ruf_line = fx + fbase;                                       // flux_x field 0 of this line: the mass flux
  // periodic wrap of c in [-3, nx+2] without a division (nx >= 3): stays on the scalar unit
  auto cell_off = [&](int c) -> long long { return pbase + (long long)(c < 0 ? c + nx : (c >= nx ? c - nx : c)) * P.sx; };

  // ---------------- state pass: rho*u, p, u, v, w, theta in ONE sweep + the update of all five state variables --------
  // (Dycore.h:341-386; :553-571; :162-221).  Six windows, six independent polynomial chains per cell; the stage-input
  // density, the sub-step-start values and the y/z face fluxes of a cell are loaded once, at the top of the iteration
  // that completes the cell, and are consumed ~700 vector instructions later.
  {
    constexpr int NQ = 4;                                  // advected state variables: u (the normal velocity), v, w, theta
    const double *pr = prim_in + (long long)P_RHO * P.prim_fs;
    const double *pp = prim_in + (long long)P_PRES * P.prim_fs;
    const double *r0 = prim0 + (long long)P_RHO * P.prim_fs;
    double *out_rho = prim_out + (long long)P_RHO * P.prim_fs, *out_rt = prim_out + (long long)P_PRES * P.prim_fs;
    double wm[5], wp[5], wq[NQ][5], wt[5];                 // wt: water vapour (tracer idWV) rides along
    const int tr = P.idWV;                                 // the tracer that rides with the state (water vapour)
    const double *pt = prim_in + (long long)(P_TR0 + tr) * P.prim_fs;
    double *flt = fx + (long long)(5 + tr) * P.ncell + fbase;   // its x flux
    const bool more_tracers = !Stash::on && P.nt > 1;      // the tracer sweeps below need the mass flux (LineStash: NT = 1, none follow)
    auto load_cell = [&](long long o, double &m, double &p, double (&qv)[NQ]) {
#pragma unroll
      for (int n = 0; n < NQ; n++) qv[n] = uni(prim_in + (long long)(P_U + n) * P.prim_fs + o)[eu];
      m = mul_rn(uni(pr + o)[eu], qv[0]);
      p = uni(pp + o)[eu];
    };
#pragma unroll
    for (int s = 0; s < 5; s++) {                          // cells c0-3..c0+1: the window of cell c0-1
      double qv[NQ];
      load_cell(cell_off(c0 - 3 + s), wm[s], wp[s], qv);
#pragma unroll
      for (int n = 0; n < NQ; n++) wq[n][s] = qv[n];
      wt[s] = uni(pt + cell_off(c0 - 3 + s))[eu];
    }
    double prevR_m, prevR_p, prevR_q[NQ], prevR_t;
    {                                                      // cell c0-1: only its right-edge values are needed (face c0)
      double L;
      weno5_const(wm, wc, L, prevR_m);
      weno5_const(wp, wc, L, prevR_p);
      weno5_const(wt, wc, L, prevR_t);
#pragma unroll
      for (int n = 0; n < NQ; n++) {
        if (n == 1 && !have_y) { prevR_q[n] = 0.0; continue; }
        weno5_const(wq[n], wc, L, prevR_q[n]);
      }
      double nm, np_, nq[NQ];
      load_cell(cell_off(c0 + 2), nm, np_, nq);
      const double nt0 = uni(pt + cell_off(c0 + 2))[eu];
#pragma unroll
      for (int s = 0; s < 4; s++) {
        wm[s] = wm[s + 1]; wp[s] = wp[s + 1]; wt[s] = wt[s + 1];
#pragma unroll
        for (int n = 0; n < NQ; n++) wq[n][s] = wq[n][s + 1];
      }
      wm[4] = nm; wp[4] = np_; wt[4] = nt0;
#pragma unroll
      for (int n = 0; n < NQ; n++) wq[n][4] = nq[n];
    }
    double F_prev[1 + NQ], Ft_prev = 0.0;                  // face fluxes of rho, rho u, rho v, rho w, rho theta; of water vapour
#pragma unroll
    for (int l = 0; l <= NQ; l++) F_prev[l] = 0.0;
    // everything cell cc needs besides its x fluxes
    // y0*/z0*: the two y / z faces of the mass flux; dy, dz: flux differences of the other variables (DIFF sweeps)
    //   t*: water vapour -- its y/z face fluxes, FCT mass seed and sub-step-start mixing ratio
    struct CellIn { double rho_in, rho_0, q0[NQ], y0l, y0h, z0l, z0h, dy[1 + NQ], dz[1 + NQ], tyl, tyh, tzl, tzh, tseed, tq0; };
    const double *fyt = fy + (long long)(5 + tr) * P.ncell, *fzt = fz + (long long)(5 + tr) * P.fz_fs;
    const double *pt0 = prim0 + (long long)(P_TR0 + tr) * P.prim_fs;
    const double *sdt = seed + (long long)tr * P.ncell;
    auto load_in = [&](int cc, CellIn &ci) {
      const long long o = pbase + (long long)cc * P.sx, ix = fbase + (long long)cc * P.sx;
      ci.rho_in = uni(pr + o)[eu];
      ci.rho_0 = (STAGE > 1) ? ld_once<PAMA_STREAM_X1>(uni(r0 + o), eu) : 0.0;
#pragma unroll
      for (int n = 0; n < NQ; n++) ci.q0[n] = (STAGE > 1) ? ld_once<PAMA_STREAM_X1>(uni(prim0 + (long long)(P_U + n) * P.prim_fs + o), eu) : 0.0;
      ci.y0l = have_y ? uni(fy + ix)[eu] : 0.0;
      ci.y0h = have_y ? uni(fy + ix + jp1)[eu] : 0.0;
      ci.z0l = uni(fz + ix)[eu];
      ci.z0h = uni(fz + ix + P.sz)[eu];
#pragma unroll
      for (int l = 1; l <= NQ; l++) {
        ci.dy[l] = (have_y && !FOLD) ? ld_once<PAMA_STREAM_X1>(uni(fy + (long long)l * P.ncell + ix), eu) : 0.0;
        ci.dz[l] = (l == 2 && !have_y) ? 0.0 : ld_once<PAMA_STREAM_X1>(uni(fz + (long long)l * P.fz_fs + ix), eu);   // 2-D: no v tendency, nothing stored
      }
      ci.tyl = have_y ? uni(fyt + ix)[eu] : 0.0;
      ci.tyh = have_y ? uni(fyt + ix + jp1)[eu] : 0.0;
      ci.tzl = uni(fzt + ix)[eu];
      ci.tzh = uni(fzt + ix + P.sz)[eu];
      ci.tseed = LAZY_SEED ? 0.0 : ld_once<PAMA_STREAM_X1>(uni(sdt + ix), eu);
      ci.tq0 = (STAGE > 1) ? ld_once<PAMA_STREAM_X1>(uni(pt0 + o), eu) : 0.0;
    };
    // finish cell cc: F_lo/F_hi = its two x faces; m_in_u = rho*u of the stage input (the product window), q_in = v, w, theta
    auto finish = [&](int cc, const CellIn &ci, const double (&Flo)[1 + NQ], const double (&Fhi)[1 + NQ], double m_in_u,
                      double v_in, double w_in, double th_in, double Ft_lo, double Ft_hi, double qt_in) {
      const long long o = pbase + (long long)cc * P.sx;
      const double q0 = rk_combine<STAGE>(ci.rho_0, ci.rho_in, dt_dyn,
                                          flux_divergence(P, Flo[0], Fhi[0], ci.y0l, ci.y0h, ci.z0l, ci.z0h, rdzk));
      const double rrho = fast_rcp(q0);
      uniw(out_rho + o)[eu] = q0;
      const double q_in[NQ] = {0.0, v_in, w_in, th_in};
#pragma unroll
      for (int n = 0; n < NQ; n++) {
        const int l = 1 + n;                               // 1 rho u, 2 rho v, 3 rho w, 4 rho theta
        double tend = FOLD ? flux_divergence_g(P, Flo[l], Fhi[l], ci.dz[l]) : flux_divergence_d(P, Flo[l], Fhi[l], ci.dy[l], ci.dz[l], rdzk);
        if (l == 3) tend = add_gravity(P, tend, ci.rho_in, gcoef);
        if (l == 2 && P.sim2d) tend = 0.0;
        const double m_in = (n == 0) ? m_in_u : mul_rn(q_in[n], ci.rho_in);
        const double m_0 = (STAGE > 1) ? mul_rn(ci.q0[n], ci.rho_0) : 0.0;
        const double v = rk_combine<STAGE>(m_0, m_in, dt_dyn, tend);
        store_adv_u(P, prim_out, P_U + n, k, cu0 + (long long)cc * P.sx, eu, v * rrho, (l == 3) ? 0.0 : v * rrho);
        // the new rho*theta goes where the pressure belongs: pressure_tail_body turns it into the next stage's pressure
        // (a pow per cell, kept out of this register-critical loop)
        // (LineStash: it stays in the lane's own slot of this cell until the epilogue behind the loop)
        if (l == 4) {
          if constexpr (Stash::on) stash.slot[(cc - c0) * XSTASH_LANES] = v;
          else uniw(out_rt + o)[eu] = v;
        }
      }
      // Tracer 0 (Dycore.h:525-550, :572-584, :162-221): finished here like the further tracers in x_tracer_sweep
      finish_tracer_cell<STAGE, LAZY_SEED>(P, tr, prim_out, seed, mult, rows, k, j, cc, e, eu, cu0 + (long long)cc * P.sx, fbase + (long long)cc * P.sx,
                                           Ft_lo, Ft_hi, ci.tyl, ci.tyh, ci.tzl, ci.tzh, ci.tseed, qt_in, ci.tq0, ci.rho_in, ci.rho_0, rrho, dzk,
                                           rdzk, dt_dyn, dt_stage);
    };
    // Faces c0 .. c1: the last one closes the last cell.  It belongs to the next span (or is the periodic face nx == face 0)
    // and is computed here a second time, with the same bits -- one polynomial set per span instead of a dependency.
#pragma clang loop unroll(disable)
    for (int c = c0; c <= c1; c++) {                       // window = cells c-2..c+2
      double nm, np_, nq[NQ];
      load_cell(cell_off(c + 3), nm, np_, nq);
      const double nt0 = uni(pt + cell_off(c + 3))[eu];
      // consumed at the bottom of this iteration.  Loaded on EVERY trip, also the first one, which completes no cell (it
      // loads cell c0's values, to be loaded again by the next trip): s_waitcnt vmcnt(N) is a static count of the memory
      // operations that may still be outstanding, the compiler takes the minimum over all paths that reach the wait, and
      // a first trip without these loads made that minimum 2-4 -- every trip then began by draining the previous trip's
      // stores (seen in the ISA: vmcnt(4) right after the window loads, vmcnt(2) at the loop tail).
      CellIn ci;
      load_in(c > c0 ? c - 1 : c0, ci);
      double Lm, Rm, Lp, Rp, Lq[NQ], Rq[NQ];
      weno5_const(wm, wc, Lm, Rm);
      weno5_const(wp, wc, Lp, Rp);
#pragma unroll
      for (int n = 0; n < NQ; n++) {
        if (n == 1 && !have_y) { Lq[n] = Rq[n] = 0.0; continue; }   // 2-D: the v flux is never used (skip_advected_v)
        weno5_const(wq[n], wc, Lq[n], Rq[n]);
      }
      double Lt, Rt;
      weno5_const(wt, wc, Lt, Rt);
      double ruf, ppf, F[1 + NQ];
      acoustic_face(prevR_m, Lm, prevR_p, Lp, false, ruf, ppf);
      const bool up = ruf > 0.0;                             // upwind (Dycore.h:368)
      const double Ft = mul_rn(ruf, up ? prevR_t : Lt);      // x flux of water vapour (Dycore.h:367-385)
      if (c < c1) {                                          // the faces this span owns
        if (more_tracers) uniw(ruf_line + (long long)c * P.sx)[eu] = ruf;   // for the tracer sweeps
        st_once<PAMA_STREAM_X2>(uniw(flt + (long long)c * P.sx), eu, Ft);   // (read again where the limiter acts: tracer_fixup_line_body)
      }
      ruf_close = ruf;                                       // (after the last trip: face c1)
      F[0] = ruf;
      F[1] = fma(ruf, up ? prevR_q[0] : Lq[0], ppf);
#pragma unroll
      for (int n = 1; n < NQ; n++) F[1 + n] = mul_rn(ruf, up ? prevR_q[n] : Lq[n]);
      if (c > c0) finish(c - 1, ci, F_prev, F, wm[1], wq[1][1], wq[2][1], wq[3][1], Ft_prev, Ft, wt[1]);   // window element 1 is cell c-1
#pragma unroll
      for (int l = 0; l <= NQ; l++) F_prev[l] = F[l];
      Ft_prev = Ft;
      prevR_m = Rm; prevR_p = Rp; prevR_t = Rt;
#pragma unroll
      for (int n = 0; n < NQ; n++) prevR_q[n] = Rq[n];
#pragma unroll
      for (int s = 0; s < 4; s++) {
        wm[s] = wm[s + 1]; wp[s] = wp[s + 1]; wt[s] = wt[s + 1];
#pragma unroll
        for (int n = 0; n < NQ; n++) wq[n][s] = wq[n][s + 1];
      }
      wm[4] = nm; wp[4] = np_; wt[4] = nt0;
#pragma unroll
      for (int n = 0; n < NQ; n++) wq[n][4] = nq[n];
    }
  }
  // nothing of the loop is live here: the pow per cell that the loop has no register for
  if constexpr (Stash::on) xsweep_pressure_epilogue(P, prim_out, stash, k, cu0, eu, c0, c1);

  // ---------------- the other tracers (Dycore.h:367-385): inline here, or -- small ensembles, where a wavefront per line is
  // too little parallelism for a chain this long -- by awfl_xtr_kernel, one wavefront per (line, pair of tracers)
  if (!Stash::on && tracers_inline) {
    for (int i = 0; i < P.nt - 1; i += FLUX_NF) {          // water vapour went with the state pass
      const int fa[2] = {4 + further_tracer(P, i), 4 + further_tracer(P, i + 1)};
      if (i + 1 < P.nt - 1) x_tracer_sweep<2, STAGE, 1>(P, prim_in, prim0, prim_out, fx, fy, fz, seed, mult, rows, line, e, c0, span, fa, dt_dyn, dt_stage, true, ruf_close);
      else x_tracer_sweep<1, STAGE, 1>(P, prim_in, prim0, prim_out, fx, fy, fz, seed, mult, rows, line, e, c0, span, fa, dt_dyn, dt_stage, true, ruf_close);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// TILE form of the x direction: one lane per CELL instead of one lane per member of a line that is swept serially.
//
// With nens the fastest axis and x the next, a periodic x line of `nx` cells and `nens` members is ONE contiguous run of nx*nens
// doubles, and the stencil neighbours of a lane's cell are the lanes `nens` positions to its left and right.  A workgroup takes a
// tile of `rows` rows of that run -- a row = (one cell) x (W consecutive members), W = nens when the whole ensemble fits a row
// (small ensembles: rows follow each other without a gap, the lanes of a wavefront are 64 consecutive (x, member) pairs whatever
// nens is), else a block of members -- and every lane
//   0  stages the tile: it loads the stage-input values of ITS cell (in a tile with halo rows the lanes of the first rows also the
//      two cells beyond the halo row on each side) into an LDS image of the tile: every value leaves global memory once;
//   A  reads the 5-point stencils from that image (the lanes W and 2W slots to either side; inside a whole-line tile they wrap around
//      the tile's rows), builds the ONE polynomial set of its own cell (the same weno5_const on the same five values as the sweeps:
//      same bits) and puts the right-edge values into a second LDS region;
//   B  takes the right-edge values of the cell to its left from LDS, forms the fluxes through its own left face (acoustic pair +
//      upwinding, as flux_x_update_body) and puts them into LDS;
//   C  takes the fluxes of its right face from the lane to its right and finishes its cell exactly as the sweep does (divergence,
//      gravity, SSPRK3 combine, vertical ghosts, water vapour's own FCT multiplier and provisional update).
// A tile is either a whole periodic line (`halo` 0: the neighbour rows wrap inside the tile; several short lines share a
// workgroup) or `tc` cells of it with one halo row on each side (the left one only builds polynomials, the right one also the face
// that closes the tile; both recompute what the neighbouring tile computes, with the same bits).
// What this buys over the sweep: no serial chain along the line (a wavefront per 64 cells instead of per 64 lines), lanes that are
// full whenever nx*nens reaches 64, and half the registers (4 waves per SIMD).  What it costs: the LDS round trips, four workgroup
// barriers and the halo rows.  Launches that fill the chip with one wavefront per line span keep the sweep (measured: DESIGN.md
// section 6).
// Reference: Dycore.h:334-386 (x fluxes), :553-571, :162-221, next stage's :310-321 (divide), :662-710 (ghosts), :525-550 + :572-584
// (water vapour); x_tile_tracer_*: :367-385, :525-548, :572-584 for the further tracers.
struct XTileGeom {
  int W;       // lanes per row
  int nmb;     // member blocks per line: ceil(nens / W)
  int tc;      // cells a tile completes
  int halo;    // 0: a tile is a whole periodic line; 1: tc cells + one halo row on each side
  int ntl;     // tiles per line
  int lpb;     // lines per workgroup (halo == 0 only)
};
PAMA_HD int xtile_rows(const XTileGeom &G) { return G.tc + 2 * G.halo; }
PAMA_HD int xtile_threads(const XTileGeom &G) { return G.W * xtile_rows(G) * G.lpb; }
// automatic geometry (w_req / tc_req / lpb_req > 0 override: tuning and tests; results never depend on the geometry)
//   ncu: compute units of the device (0: unknown -- the host emulation).  Whole-line tiles of a small grid are a LATENCY problem: the
//   launch is over when the most loaded CU is, so the lines per workgroup are chosen to minimise (workgroups per CU, rounded up) x
//   (lanes per workgroup), ties going to 256-lane workgroups (one wavefront per SIMD) -- measured on MI355X (round 5,
//   profiles/r05_ab_experiments.txt): 32x32x60 with one member 6 -> 8 lines (320 -> 240 workgroups on 256 CUs) 14.5 -> 13.9 us, with two
//   members 3 -> 4 lines (640 -> 480) 17.0 -> 15.7 us.
PAMA_HD XTileGeom xtile_geometry(const Params &P, int w_req, int tc_req, int lpb_req, int ncu = 0) {
  XTileGeom G;
  G.W = (P.nens <= 64) ? P.nens : 64;
  // fewer than 64 members whose whole line does not fit a workgroup: rows of an even share of the members (at least 16: 128-byte
  // runs) so that a tile is still a whole periodic line -- no halo rows (measured, 48 members on 32x32x60: rows of all 48 members in
  // 16-cell tiles with halo rows 0.31 ms per stage, whole lines 0.24)
  // ... and a whole line of 512 lanes rather than 1024: at 97-105 VGPRs a CU holds 16 wavefronts of this kernel -- ONE workgroup of
  // 1024 lanes, whose four barriers then stall the whole CU, or two of 512 that fill each other's waits (measured, 32x32x60: 32
  // members 1.77 -> 1.91 G, 48 members 1.82 -> 2.01 G with rows of 16; 256-lane tiles lose again: 16 members 1.69 -> 1.64)
  if (P.nens < 64 && (long long)P.nx * P.nens > 512) {
    const int nmb = (int)(((long long)P.nx * P.nens + 511) / 512), w = (P.nens + nmb - 1) / nmb;
    if (w >= 16 && P.nx * w <= 1024) G.W = w;
    else if ((long long)P.nx * P.nens > 1024) {
      const int nmb2 = (int)(((long long)P.nx * P.nens + 1023) / 1024), w2 = (P.nens + nmb2 - 1) / nmb2;
      if (w2 >= 16 && P.nx * w2 <= 1024) G.W = w2;
    }
  }
  if (w_req > 0) G.W = w_req < P.nens ? w_req : P.nens;
  if (G.W > 1024 / 3) G.W = 64;
  G.nmb = (P.nens + G.W - 1) / G.W;
  const int max_threads = 1024;
  if (tc_req <= 0 && P.nx * G.W <= max_threads) {        // a whole periodic line per tile
    G.halo = 0; G.tc = P.nx; G.ntl = 1;
    // lines per workgroup: the fewest that fill their wavefronts (lanes used / lanes launched within 3 % of the best any
    // count reaches) with at least 192 lanes
    const int row = P.nx * G.W, most = max_threads / row;
    auto used = [&](int l) { return (double)(l * row) / (double)(((l * row + 63) / 64) * 64); };
    double best = 0.0;
    for (int l = 1; l <= most; l++) best = used(l) > best ? used(l) : best;
    G.lpb = most;
    for (int l = 1; l <= most; l++)
      if (used(l) >= best - 0.03 && (l * row >= 192 || l == most)) { G.lpb = l; break; }
    if (ncu > 0) {
      const long long nlines = (long long)P.nz * P.ny;
      long long best_cost = -1;
      int best_dist = 0;
      for (int l = 1; l <= most; l++) {
        if (used(l) < best - 0.03) continue;
        const int T = ((l * row + 63) / 64) * 64;
        const long long nwg = (long long)G.nmb * ((nlines + l - 1) / l);
        const long long cost = ((nwg + ncu - 1) / ncu) * T;
        const int dist = T > 256 ? T - 256 : 256 - T;
        if (best_cost < 0 || cost < best_cost || (cost == best_cost && dist < best_dist)) { best_cost = cost; best_dist = dist; G.lpb = l; }
      }
    }
    if (lpb_req > 0) G.lpb = lpb_req < most ? lpb_req : most;
    if (G.lpb < 1) G.lpb = 1;
  } else {
    G.halo = 1; G.lpb = 1;
    int tc = tc_req > 0 ? tc_req : 14;
    if (tc > P.nx) tc = P.nx;
    while (tc > 1 && (tc + 2) * G.W > max_threads) tc--;
    G.ntl = (P.nx + tc - 1) / tc;
    G.tc = tc_req > 0 ? tc : (P.nx + G.ntl - 1) / G.ntl;   // automatic: even tiles
  }
  return G;
}
// lanes of the tile kernels address with `uniform field base + 32-bit lane offset`: every field must stay below 2^28 doubles
PAMA_HD bool xtile_supported(const Params &P) { return P.prim_fs < (1ll << 28) && P.fz_fs < (1ll << 28) && (long long)P.nz * P.ny < (1ll << 30); }

// A lane of a tile kernel: its cell, its roles and its neighbours.
struct XLane {
  int k, j, i, e;                       // level, y index, cell (wrapped into [0, nx)), member
  bool poly, face, upd;                 // builds polynomials / forms its left face / completes its cell
  int slot, slot_l, slot_r;             // LDS slots: own, of the row to the left, of the row to the right
  unsigned po, io, ke;                  // offsets of the cell inside a prim field / an interior-sized field; of (level, member)
  // the STAGED tile: every stage-input value of the tile is loaded from global memory ONCE (each lane its own cell; in a tile with
  // halo rows the first lanes also the two cells beyond the halo row on each side) into LDS, and the 5-point stencils are read
  // from there (Dycore.h:629-657: periodic in x -- inside a whole-line tile the stencil wraps around the tile's rows)
  int s5[5];                            // LDS elements (inside one staged field) of the cells i-2 .. i+2
  int nstage;                           // cells this lane stages (0 .. 3): its own first
  unsigned stage_po[3];                 // their prim offsets
  int stage_el[3];                      // their LDS elements
};
// LDS elements of one staged field of a tile kernel's workgroup
PAMA_HD int xtile_stage_rows(const XTileGeom &G) { return xtile_rows(G) + 4 * G.halo; }
PAMA_HD int xtile_stage_elems(const XTileGeom &G) { return G.lpb * xtile_stage_rows(G) * G.W; }
// (bx, by): workgroup index (tile of a line and member block; group of lines); (tx, ty, tz): lane inside it = (member of the row,
// row, line of the group)
PAMA_D XLane xtile_lane(const Params &P, const XTileGeom &G, int bx, int by, int tx, int ty, int tz) {
  XLane X;
  const int rows = xtile_rows(G);
  const int mb = bx / G.ntl, tl = bx - mb * G.ntl;
  const int line = by * G.lpb + tz;
  const int c0 = tl * G.tc;
  const int tcl = (c0 + G.tc <= P.nx) ? G.tc : P.nx - c0;           // cells this tile really holds
  const int nrow = tcl + 2 * G.halo;
  X.e = mb * G.W + tx;
  const bool valid = line < P.nz * P.ny && X.e < P.nens && ty < nrow;
  X.k = P.sim2d ? line : line / P.ny;
  X.j = P.sim2d ? 0 : line - X.k * P.ny;
  if (!valid) { X.k = 0; X.j = 0; X.e = 0; }
  const int c = c0 - G.halo + (valid ? ty : G.halo);                  // -1 .. nx
  X.i = c < 0 ? c + P.nx : (c >= P.nx ? c - P.nx : c);
  X.poly = valid;
  X.face = valid && (G.halo == 0 || ty >= 1);
  X.upd = valid && ty >= G.halo && ty < G.halo + tcl;
  X.slot = (tz * rows + ty) * G.W + tx;
  X.slot_l = (ty > 0) ? X.slot - G.W : X.slot + (nrow - 1) * G.W;   // (halo 0: the periodic neighbour; halo 1: unused)
  X.slot_r = (ty < nrow - 1) ? X.slot + G.W : X.slot - (nrow - 1) * G.W;
  const unsigned lrow = (unsigned)(X.j * P.nx) * (unsigned)P.nens + (unsigned)X.e;       // (j, i = 0, e) inside a level
  const unsigned sx = (unsigned)P.nens;
  auto at = [&](int ii) -> unsigned { return lrow + (unsigned)(ii < 0 ? ii + P.nx : (ii >= P.nx ? ii - P.nx : ii)) * sx; };
  const unsigned lev_p = (unsigned)(X.k + HS) * (unsigned)P.sz, lev_i = (unsigned)X.k * (unsigned)P.sz;
  X.po = member_offset((int)(lev_p + at(X.i)));
  X.io = member_offset((int)(lev_i + at(X.i)));
  X.ke = (unsigned)X.k * (unsigned)P.nens + (unsigned)X.e;
  // staged tile: rows of a line's slab in LDS = [2 cells below the tile's rows] + the rows + [2 cells above] with halo rows, the rows
  // alone in a whole-line tile (the stencil wraps)
  const int srows = xtile_stage_rows(G), sbase = tz * srows;
  const int shift = 2 * G.halo;
#pragma unroll
  for (int s = 0; s < 5; s++) {
    int r = ty + s - 2;
    if (G.halo == 0) r = r < 0 ? r + nrow : (r >= nrow ? r - nrow : r);
    X.s5[s] = (sbase + r + shift) * G.W + tx;
  }
  X.nstage = 0;
  if (valid) {
    X.stage_po[0] = X.po;
    X.stage_el[0] = (sbase + ty + shift) * G.W + tx;
    X.nstage = 1;
    if (G.halo) {
      // the four cells beyond the halo rows (c0-3, c0-2 | c0+tcl+1, c0+tcl+2) are staged by the lanes of the first rows: row r of
      // the four by the lanes with ty == r, and (a tile of three rows only) the fourth by the lanes of row 0 as well
      auto extra = [&](int r, int n) {
        const int cc = (r < 2) ? c0 - 3 + r : c0 + tcl + 1 + (r - 2);
        const int srow = (r < 2) ? r : nrow + r;          // (rows 0, 1 | nrow + 2, nrow + 3 of the slab)
        X.stage_po[n] = member_offset((int)(lev_p + at(cc)));
        X.stage_el[n] = (sbase + srow) * G.W + tx;
      };
      if (ty < 4) { extra(ty, 1); X.nstage = 2; }
      if (ty + nrow < 4) { extra(ty + nrow, 2); X.nstage = 3; }
    }
  }
  return X;
}

// store_adv with a per-lane offset: `lo` = offset of the cell inside a level
PAMA_D void store_adv_l(const Params &P, double *prim, int pf, int k, unsigned lo, double val, double ghost_val) {
  g_ptr f = uniw(prim + (long long)pf * P.prim_fs);
  const unsigned sz = (unsigned)P.sz;
  f[member_offset((int)((unsigned)(k + HS) * sz + lo))] = val;
  if (k == 0)
    for (int kk = 0; kk < HS; kk++) f[member_offset((int)((unsigned)(HS - 1 - kk) * sz + lo))] = ghost_val;        // Dycore.h:670,675
  if (k == P.nz - 1)
    for (int kk = 0; kk < HS; kk++) f[member_offset((int)((unsigned)(HS + P.nz + kk) * sz + lo))] = ghost_val;     // Dycore.h:671,676
}

// store_rho_pres<false> with a per-lane offset (the pressure pass of a cell inside the tile kernel: pressure_tail_body's arithmetic
// on the values the lane still holds): `lo` = offset of the cell inside a level, `ke` = (level, member) entry
PAMA_D void store_pres_l(const Params &P, double *prim, int k, unsigned lo, unsigned ke, double rho, double th, double rho_theta,
                         bool subtract_hy) {
#pragma clang fp contract(off)
  g_ptr fr = uniw(prim + (long long)P_RHO * P.prim_fs), fp = uniw(prim + (long long)P_PRES * P.prim_fs);
  const unsigned sz = (unsigned)P.sz;
  double pres = P.C0 * pow_pos(P, rho_theta, P.gamma);
  if (subtract_hy) pres -= P.hy_pres[ke];
  fp[member_offset((int)((unsigned)(k + HS) * sz + lo))] = pres;
  const bool bot = (k == 0), top = (k == P.nz - 1);
  if (bot || top) {
    const double gm1 = P.gamma - 1.0;
    const double rho0_gm1 = pow_pos(P, rho, gm1);
    const double theta0_g = pow_pos(P, th, P.gamma);
    const double dzk = P.dz[ke];
    const double coef = P.grav * gm1 * dzk / (P.gamma * P.C0 * theta0_g);
    for (int kk = 0; kk < HS; kk++) {
      const int kz = bot ? (HS - 1 - kk) : (HS + P.nz + kk);
      const unsigned og = member_offset((int)((unsigned)kz * sz + lo));
      const double arg = bot ? rho0_gm1 + coef * (kk + 1) : rho0_gm1 - coef * (kk + 1);
      const double rho_g = pow_pos(P, arg, 1.0 / gm1);
      double p_g = pres;                                          // mode B: copy (Dycore.h:678-681)
      if (P.grav_balance) p_g = P.C0 * pow_pos(P, rho_g * th, P.gamma);    // mode A (Dycore.h:691-694)
      fr[og] = rho_g;
      fp[og] = p_g;
    }
  }
}

// ---- state tile (the arithmetic of flux_x_update_body's state pass, cell by cell) --------------------------------------------
// fields of the state tile, in LDS order: 0 rho*u, 1 pressure, 2 u, 3 v, 4 w, 5 theta, 6 water vapour
constexpr int XT_NS = 7;    // right-edge values a lane hands to its right neighbour
constexpr int XT_NF = 6;    // face fluxes a lane hands to its left neighbour: rho, rho u, rho v, rho w, rho theta, vapour
// phase 0: the lane's share of the staged tile.  fields[f]: prim field index of staged field f; st: the staged fields, TS elements
// each; own[f]: the values of the lane's own cell (kept in registers: the centre of its stencils)
//   fmask: bit f set = staged field f is needed (the parts of the state pass stage only their own fields)
template <int NSF>
PAMA_D void xtile_stage(const Params &P, const double *__restrict__ prim_in, const XLane &X, const int (&fields)[NSF], double *st, int TS,
                        double (&own)[NSF], unsigned fmask = ~0u) {
  // every load is issued before the first LDS store (a loop of load -> store per cell would wait for each load in turn)
  double v1[NSF], v2[NSF];
  const bool has0 = X.nstage > 0, has1 = X.nstage > 1, has2 = X.nstage > 2;
#pragma unroll
  for (int f = 0; f < NSF; f++) {
    const bool need = ((fmask >> f) & 1u) != 0;
    gc_ptr fp = uni(prim_in + (long long)fields[f] * P.prim_fs);
    own[f] = (has0 && need) ? fp[X.stage_po[0]] : 0.0;
    v1[f] = (has1 && need) ? fp[X.stage_po[1]] : 0.0;
    v2[f] = (has2 && need) ? fp[X.stage_po[2]] : 0.0;
  }
#pragma unroll
  for (int f = 0; f < NSF; f++) {
    if (!((fmask >> f) & 1u)) continue;
    if (has0) st[f * TS + X.stage_el[0]] = own[f];
    if (has1) st[f * TS + X.stage_el[1]] = v1[f];
    if (has2) st[f * TS + X.stage_el[2]] = v2[f];
  }
}
// WAVEFRONT-SHUFFLE form of the tile exchange.  When a whole periodic line of a tile (nx rows of W lanes) lies inside ONE wavefront
// -- nx * W divides 64: the C2 / C1 grid with 1 or 2 members, 16-cell lines with up to 4 -- every value a lane exchanges with its
// neighbours (the four outer stencil values of each quantity, the right-edge values of the cell to its left, the fluxes of its right
// face) is held by another lane of the same wavefront, and the tile kernels fetch it with wavefront shuffles (ds_bpermute_b32 pairs:
// the LDS crossbar, no LDS memory): no LDS image, no workgroup barrier.  Same values into the same helpers: same bits as the LDS form.
struct XShuf { int ln[5]; int l, r; };     // wavefront lanes of the cells i-2 .. i+2 (periodic inside the line), of the left / right cell
PAMA_HD bool xtile_line_in_wavefront(const Params &P, const XTileGeom &G) {
  return G.halo == 0 && P.nx * G.W <= 64 && 64 % (P.nx * G.W) == 0;
}
// lane: the lane's index inside its wavefront (the workgroup's linear thread index & 63); (tx, ty): member of the row, row
PAMA_D XShuf xtile_shuffle_lanes(const Params &P, const XTileGeom &G, int lane, int tx, int ty) {
  XShuf S;
  const int base = lane - (ty * G.W + tx);             // first lane of the line
#pragma unroll
  for (int s = 0; s < 5; s++) {
    int r = ty + s - 2;
    r = r < 0 ? r + P.nx : (r >= P.nx ? r - P.nx : r);
    S.ln[s] = base + r * G.W + tx;
  }
  S.l = S.ln[1];
  S.r = S.ln[3];
  return S;
}
#if defined(__HIP_DEVICE_COMPILE__)
PAMA_D double xtile_shfl(double v, int src_lane) { return __shfl(v, src_lane, 64); }
#else
PAMA_D double xtile_shfl(double v, int) { return v; }     // (host emulation: the tile kernels are emulated in their LDS form)
#endif
// the stage-input values of the lane's own cell (whole-line tiles: every lane stages exactly its own cell)
template <int NSF>
PAMA_D void xtile_load_own(const Params &P, const double *__restrict__ prim_in, const XLane &X, const int (&fields)[NSF], double (&own)[NSF],
                           unsigned fmask = ~0u) {
#pragma unroll
  for (int f = 0; f < NSF; f++)
    own[f] = (X.nstage > 0 && ((fmask >> f) & 1u)) ? uni(prim_in + (long long)fields[f] * P.prim_fs)[X.stage_po[0]] : 0.0;
}
// staged fields (rho, p, u, v, w, theta, vapour) a part of the state pass needs
PAMA_HD unsigned xtile_part_fields(int part) {
  return 0x7u | ((part & 2) ? 0x18u : 0u) | ((part & 4) ? 0x60u : 0u);
}
PAMA_D void xtile_state_fields(const Params &P, int (&fields)[XT_NS]) {
  fields[0] = P_RHO; fields[1] = P_PRES; fields[2] = P_U; fields[3] = P_V; fields[4] = P_W; fields[5] = P_THETA; fields[6] = P_TR0 + P.idWV;
}
// A: one polynomial per field of the lane's own cell, stencils from the staged tile (staged fields: rho, p, u, v, w, theta, vapour).
// cen: the stage-input values the update needs again: rho*u, v, w, theta, vapour (window element of the cell in the sweep) and the
// density
//   nb(f, s): the value of staged field f in the cell s - 2 cells away (s = 0, 1, 3, 4) -- from the LDS image of the tile, or (a line
//   that lies inside ONE wavefront) from the lane that holds it, by a wavefront shuffle (XShuf below)
// PARTS of the state pass (round 5).  The state pass of a cell is one chain -- seven polynomials, the face, the finish, the pressure.
// On a small grid with idle SIMDs it is cut into three parts that run BESIDE each other in workgroups of their own (z slices of the
// launch), each rebuilding what it needs of the others instead of waiting for it -- the polynomials of rho*u and p, the face mass flux
// and the new density: the same products in the same functions, hence the same bits:
//   XP_U   the acoustic part: u (normal momentum: mass flux x upwinded u + face pressure), and it STORES the new density and the face
//          mass flux;                      XP_VW  v and w (gravity);
//   XP_T   theta, the next stage's pressure (+ density / pressure ghosts) and water vapour (own multiplier, update, seed, x flux).
// XP_ALL = the whole pass in one lane (every case where the chip is busy anyway).
constexpr int XP_U = 1, XP_VW = 2, XP_T = 4, XP_ALL = 7;
template <int PART = XP_ALL, class Neighbour>
PAMA_D void xtile_state_polys_from(const Params &P, Neighbour &&nb, const double (&own)[XT_NS], double (&L)[XT_NS], double (&R)[XT_NS],
                                   double (&cen)[6]) {
  const WenoConsts wc = weno_consts();
  auto stencil = [&](int f, double (&u)[5]) {
#pragma unroll
    for (int s = 0; s < 5; s++) u[s] = (s == 2) ? own[f] : nb(f, s);
  };
#pragma unroll
  for (int f = 0; f < XT_NS; f++) L[f] = R[f] = 0.0;
  cen[1] = cen[2] = cen[3] = cen[4] = 0.0;
  double r[5], u[5], w[5];
  stencil(0, r);
  stencil(2, u);
#pragma unroll
  for (int s = 0; s < 5; s++) w[s] = mul_rn(r[s], u[s]);
  cen[0] = w[2];
  cen[5] = r[2];
  weno5_const(w, wc, L[0], R[0]);
  if (PART & XP_U) weno5_const(u, wc, L[2], R[2]);
  stencil(1, w);
  weno5_const(w, wc, L[1], R[1]);
  if (PART & XP_VW) {
    cen[1] = own[3];
    if (!P.sim2d) {
      stencil(3, w);
      weno5_const(w, wc, L[3], R[3]);
    }                                                         // 2-D: the v flux is never used (skip_advected_v)
    stencil(4, w);
    cen[2] = w[2];
    weno5_const(w, wc, L[4], R[4]);
  }
  if (PART & XP_T) {
    stencil(5, w);
    cen[3] = w[2];
    weno5_const(w, wc, L[5], R[5]);
    stencil(6, w);
    cen[4] = w[2];
    weno5_const(w, wc, L[6], R[6]);
  }
}
PAMA_D void xtile_state_polys(const Params &P, const XLane &X, const double *st, int TS, const double (&own)[XT_NS],
                              double (&L)[XT_NS], double (&R)[XT_NS], double (&cen)[6]) {
  xtile_state_polys_from(P, [&](int f, int s) { return st[f * TS + X.s5[s]]; }, own, L, R, cen);
}
// B: the fluxes through the lane's LEFT face from the right-edge values of the cell to its left (Rl) and its own left-edge values
// (Dycore.h:341-386).  own_face: the face belongs to this tile (its cell is one the tile completes): the mass flux (when further
// tracers follow) and water vapour's flux go to flux_x as in the sweep.
template <int PART = XP_ALL>
PAMA_D void xtile_state_face(const Params &P, double *__restrict__ fx, const XLane &X, const double (&L)[XT_NS],
                             const double (&Rl)[XT_NS], bool own_face, double (&F)[XT_NF]) {
  double ruf, ppf;
  acoustic_face(Rl[0], L[0], Rl[1], L[1], false, ruf, ppf);
  const bool up = ruf > 0.0;                               // upwind (Dycore.h:368)
#pragma unroll
  for (int n = 0; n < XT_NF; n++) F[n] = 0.0;
  F[0] = ruf;
  if (PART & XP_U) {
    if (own_face && P.nt > 1) uniw(fx)[X.io] = ruf;         // for the tracer tiles
    F[1] = fma(ruf, up ? Rl[2] : L[2], ppf);
  }
  if (PART & XP_VW) {
#pragma unroll
    for (int n = 1; n < 3; n++) F[1 + n] = mul_rn(ruf, up ? Rl[2 + n] : L[2 + n]);
  }
  if (PART & XP_T) {
    const double Ft = mul_rn(ruf, up ? Rl[6] : L[6]);
    if (own_face) uniw(fx + (long long)(5 + P.idWV) * P.ncell)[X.io] = Ft;   // (read again where the limiter acts: tracer_fixup_line_body)
    F[4] = mul_rn(ruf, up ? Rl[5] : L[5]);
    F[5] = Ft;
  }
}
// C: the lane's cell complete (the `finish` of flux_x_update_body): Flo / Fhi = the fluxes through its left / right face.
// PART (above): which variables this lane finishes; the new density is formed by every part (same function, same inputs) and stored by XP_U
template <int STAGE, int PART = XP_ALL>
PAMA_D void xtile_state_finish(const Params &P, const double *__restrict__ prim_in, const double *__restrict__ prim0,
                               double *__restrict__ prim_out, const double *__restrict__ fy, const double *__restrict__ fz,
                               double *__restrict__ seed, double *__restrict__ mult, const FctRows &rows, const XLane &X,
                               const double (&Flo)[XT_NF], const double (&Fhi)[XT_NF], const double (&cen)[6], double dt_dyn,
                               double dt_stage, bool with_pressure) {
  const bool have_y = !P.sim2d;
  const int k = X.k, j = X.j;
  const unsigned po = X.po, io = X.io;
  const unsigned jp1 = member_offset((int)(io + (unsigned)((j == P.ny - 1) ? -(long long)(P.ny - 1) * P.sy : P.sy)));
  const unsigned kp1 = member_offset((int)(io + (unsigned)P.sz));
  const double dzk = P.dz[X.ke];
  const double rdzk = fast_rcp(dzk);
  const double gcoef = (PART & XP_VW) ? gravity_coef(P, X.ke) : 0.0;
  const int tr = P.idWV;
  const double rho_in = cen[5];
  const double rho_0 = (STAGE > 1) ? uni(prim0 + (long long)P_RHO * P.prim_fs)[po] : 0.0;
  // which of the four momentum / theta variables (n = 0 rho u, 1 rho v, 2 rho w, 3 rho theta) this part finishes
  const bool mine[4] = {(PART & XP_U) != 0, (PART & XP_VW) != 0, (PART & XP_VW) != 0, (PART & XP_T) != 0};
  double q0[4];
#pragma unroll
  for (int n = 0; n < 4; n++) q0[n] = (STAGE > 1 && mine[n]) ? uni(prim0 + (long long)(P_U + n) * P.prim_fs)[po] : 0.0;
  const double y0l = have_y ? uni(fy)[io] : 0.0, y0h = have_y ? uni(fy)[jp1] : 0.0;
  const double z0l = uni(fz)[io], z0h = uni(fz)[kp1];
  double dy[5], dz[5];
#pragma unroll
  for (int l = 1; l <= 4; l++) {
    dy[l] = (have_y && mine[l - 1]) ? uni(fy + (long long)l * P.ncell)[io] : 0.0;
    dz[l] = ((l == 2 && !have_y) || !mine[l - 1]) ? 0.0 : uni(fz + (long long)l * P.fz_fs)[io];     // 2-D: no v tendency, nothing stored
  }
  double tyl = 0.0, tyh = 0.0, tzl = 0.0, tzh = 0.0, tseed = 0.0, tq0 = 0.0;
  if (PART & XP_T) {
    tyl = have_y ? uni(fy + (long long)(5 + tr) * P.ncell)[io] : 0.0;
    tyh = have_y ? uni(fy + (long long)(5 + tr) * P.ncell)[jp1] : 0.0;
    tzl = uni(fz + (long long)(5 + tr) * P.fz_fs)[io];
    tzh = uni(fz + (long long)(5 + tr) * P.fz_fs)[kp1];
    tseed = uni(seed + (long long)tr * P.ncell)[io];
    tq0 = (STAGE > 1) ? uni(prim0 + (long long)(P_TR0 + tr) * P.prim_fs)[po] : 0.0;
  }
  const unsigned lo = po - (unsigned)(k + HS) * (unsigned)P.sz;                     // the cell inside its level

  const double qn = rk_combine<STAGE>(rho_0, rho_in, dt_dyn, flux_divergence(P, Flo[0], Fhi[0], y0l, y0h, z0l, z0h, rdzk));
  const double rrho = fast_rcp(qn);
  if (PART & XP_U) uniw(prim_out + (long long)P_RHO * P.prim_fs)[po] = qn;
  const double q_in[4] = {0.0, cen[1], cen[2], cen[3]};
#pragma unroll
  for (int n = 0; n < 4; n++) {
    if (!mine[n]) continue;
    const int l = 1 + n;                                   // 1 rho u, 2 rho v, 3 rho w, 4 rho theta
    double tend = flux_divergence_d(P, Flo[l], Fhi[l], dy[l], dz[l], rdzk);
    if (l == 3) tend = add_gravity(P, tend, rho_in, gcoef);
    if (l == 2 && P.sim2d) tend = 0.0;
    const double m_in = (n == 0) ? cen[0] : mul_rn(q_in[n], rho_in);
    const double m_0 = (STAGE > 1) ? mul_rn(q0[n], rho_0) : 0.0;
    const double v = rk_combine<STAGE>(m_0, m_in, dt_dyn, tend);
    store_adv_l(P, prim_out, P_U + n, k, lo, v * rrho, (l == 3) ? 0.0 : v * rrho);
    if (l == 4) {
      // the new rho*theta: with_pressure -- the next stage's pressure and the density / pressure ghosts at once (small ensembles: one
      // launch less per stage; the arithmetic of pressure_tail_body on the same doubles); else pressure_tail_body makes them of it
      if (with_pressure) store_pres_l(P, prim_out, k, lo, X.ke, qn, v * rrho, v, !P.grav_balance);
      else uniw(prim_out + (long long)P_PRES * P.prim_fs)[po] = v;
    }
  }
  if (PART & XP_T) {
    // water vapour (finish_tracer_cell): its own multiplier (sparse store + flags) and the update an unlimited neighbourhood gets
    own_multiplier_cell<false>(P, tr, mult, rows, k, j, X.i, X.e, io, 0, Flo[5], Fhi[5], tyl, tyh, tzl, tzh, tseed, dzk, rdzk, dt_stage);
    double v, new_seed;
    tracer_new_value<STAGE>(P, tr, Flo[5], Fhi[5], tyl, tyh, tzl, tzh, cen[4], tq0, rho_in, rho_0, rdzk, dt_dyn, v, new_seed);
    uniw(seed + (long long)tr * P.ncell)[io] = new_seed;
    store_adv_l(P, prim_out, P_TR0 + tr, k, lo, v * rrho, v * rrho);
  }
}

// ---- tracer tiles (the arithmetic of x_tracer_sweep, cell by cell): NF further tracers per lane ------------------------------
template <int NF, class Neighbour>
PAMA_D void xtile_tracer_polys_from(const Params &P, Neighbour &&nb, const double (&own)[NF], double (&L)[NF], double (&R)[NF],
                                    double (&cen)[NF]) {
  const WenoConsts wc = weno_consts();
#pragma unroll
  for (int n = 0; n < NF; n++) {
    double w[5];
#pragma unroll
    for (int s = 0; s < 5; s++) w[s] = (s == 2) ? own[n] : nb(n, s);
    cen[n] = w[2];
    weno5_const(w, wc, L[n], R[n]);
  }
}
template <int NF>
PAMA_D void xtile_tracer_polys(const Params &P, const XLane &X, const double *st, int TS, const double (&own)[NF], double (&L)[NF],
                               double (&R)[NF], double (&cen)[NF]) {
  xtile_tracer_polys_from<NF>(P, [&](int n, int s) { return st[n * TS + X.s5[s]]; }, own, L, R, cen);
}
// the fluxes through the lane's left face, upwinded by the face mass flux the state kernel left in flux_x field 0 (Dycore.h:367-385)
//   have_ruf / ruf_reg: the mass flux through the lane's left face handed over in a register (phase 1 inline in the state kernel: the
//   lane has just formed it); else it is read from flux_x (a launch of its own)
template <int NF>
PAMA_D void xtile_tracer_face(const Params &P, const double *__restrict__ fx, const XLane &X, const double (&L)[NF],
                              const double (&Rl)[NF], double (&F)[NF], bool have_ruf = false, double ruf_reg = 0.0) {
  const double ruf = have_ruf ? ruf_reg : uni(fx)[X.io];
  const bool up = ruf > 0.0;
#pragma unroll
  for (int n = 0; n < NF; n++) F[n] = mul_rn(ruf, up ? Rl[n] : L[n]);
}
// PHASE 1: the cell's FCT multipliers (a complete field); PHASE 2 (a later launch): the complete limited update
template <int NF, int STAGE, int PHASE>
PAMA_D void xtile_tracer_finish(const Params &P, const double *__restrict__ prim_in, const double *__restrict__ prim0,
                                double *__restrict__ prim_out, const double *__restrict__ fy, const double *__restrict__ fz,
                                double *__restrict__ seed, double *__restrict__ mult, const FctRows &rows, const XLane &X,
                                const int *fa, const double (&Flo)[NF], const double (&Fhi)[NF], const double (&cen)[NF],
                                double dt_dyn, double dt_stage) {
  const bool have_y = !P.sim2d;
  const int k = X.k, j = X.j, i = X.i;
  const unsigned po = X.po, io = X.io;
  const unsigned sx = (unsigned)P.nens, sy = (unsigned)P.sy, sz = (unsigned)P.sz;
  const unsigned jp1 = member_offset((int)((j == P.ny - 1) ? io - (unsigned)(P.ny - 1) * sy : io + sy));
  const unsigned jm1 = member_offset((int)((j == 0) ? io + (unsigned)(P.ny - 1) * sy : io - sy));
  const unsigned ip1 = member_offset((int)((i == P.nx - 1) ? io - (unsigned)(P.nx - 1) * sx : io + sx));
  const unsigned im1 = member_offset((int)((i == 0) ? io + (unsigned)(P.nx - 1) * sx : io - sx));
  const unsigned kp1 = member_offset((int)(io + sz));
  const bool zlo = (k > 0), zhi = (k < P.nz - 1);
  const unsigned km1 = zlo ? member_offset((int)(io - sz)) : io;
  const double dzk = P.dz[X.ke];
  const double rdzk = fast_rcp(dzk);
  double rho_in = 0.0, rho_0 = 0.0, rho_new = 1.0;
  if (PHASE == 2) {
    rho_in = uni(prim_in + (long long)P_RHO * P.prim_fs)[po];
    rho_0 = (STAGE > 1) ? uni(prim0 + (long long)P_RHO * P.prim_fs)[po] : 0.0;
    rho_new = uni(prim_out + (long long)P_RHO * P.prim_fs)[po];        // written by the state kernel (an earlier launch)
  }
  const double rrho = (PHASE == 2) ? fast_rcp(rho_new) : 0.0;
  const unsigned lo = po - (unsigned)(k + HS) * sz;
#pragma unroll
  for (int n = 0; n < NF; n++) {
    const int t = fa[n] - 4;                               // tracer index
    gc_ptr fyt = uni(fy + (long long)(1 + fa[n]) * P.ncell), fzt = uni(fz + (long long)(1 + fa[n]) * P.fz_fs);
    const double yl = have_y ? fyt[io] : 0.0, yh = have_y ? fyt[jp1] : 0.0;
    const double zl = fzt[io], zh = fzt[kp1];
    if (PHASE == 1) {
      const double sd = uni(seed + (long long)t * P.ncell)[io];
      own_multiplier_cell<true>(P, t, mult, rows, k, j, i, X.e, io, 0, Flo[n], Fhi[n], yl, yh, zl, zh, sd, dzk, rdzk, dt_stage);
    } else {
      gc_ptr mt = uni(mult + (long long)t * P.ncell);
      const double q_0 = (STAGE > 1) ? uni(prim0 + (long long)(P_U + fa[n]) * P.prim_fs)[po] : 0.0;
      const double m_c = mt[io], m_im1 = mt[im1], m_ip1 = mt[ip1];
      double m_jm1 = 1.0, m_jp1 = 1.0, m_km1 = 1.0, m_kp1 = 1.0;
      if (have_y) { m_jm1 = mt[jm1]; m_jp1 = mt[jp1]; }
      if (zlo) m_km1 = mt[km1];
      if (zhi) m_kp1 = mt[kp1];
      const double f_x = limited_flux(Flo[n], m_im1, m_c, i == 0);
      const double f_xp1 = limited_flux(Fhi[n], m_c, m_ip1, i == P.nx - 1);
      double f_y = 0.0, f_yp1 = 0.0;
      if (have_y) {
        f_y = limited_flux(yl, m_jm1, m_c, j == 0);
        f_yp1 = limited_flux(yh, m_c, m_jp1, j == P.ny - 1);
      }
      const double f_z = limited_flux(zl, m_km1, m_c, false);
      const double f_zp1 = limited_flux(zh, m_c, m_kp1, false);
      double v, new_seed;
      tracer_new_value<STAGE>(P, t, f_x, f_xp1, f_y, f_yp1, f_z, f_zp1, cen[n], q_0, rho_in, rho_0, rdzk, dt_dyn, v, new_seed);
      uniw(seed + (long long)t * P.ncell)[io] = new_seed;
      store_adv_l(P, prim_out, P_TR0 + t, k, lo, v * rrho, v * rrho);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// TILE form of the fused stage's y and z sweeps (flux_line_body<DIR, ., DIFF = true>, cell by cell): a lane per CELL.
// The lanes of a row are W consecutive doubles of the axis that is contiguous across the sweep direction ((x, member) for a y
// sweep, (y, x, member) for a z sweep), the rows of a tile follow the sweep direction: the stencil neighbours of a lane's cell are
// the same lane of the rows above and below, sy / sz doubles away in memory.  Every lane builds the ONE polynomial of its cell per
// quantity, hands the right-edge values to the next row through LDS, forms the fluxes through its LOWER face, and -- for the four
// state variables that leave as flux differences -- takes the flux of its upper face back from the next row.  Quantities go in
// groups of FT_NG: group 0 = the acoustic triple (rho*u_n, p, u_n: face mass flux + normal momentum flux), then the other advected
// state variables, then the tracers (faces only).  Same helpers on the same five values as the sweep: same bits.
// y tiles are periodic like the x tiles (whole lines, or cells + one halo row per side); z tiles are `tc` levels + one halo row
// below and above (the ghost levels exist in prim; the walls are faces 0 and nz), a row being exactly one wavefront (W = 64) so
// that the level's WENO table is fetched with scalar loads as in the sweep.
// Reference: Dycore.h:387-519 (y and z fluxes), WenoLimiter.h:98-181.
constexpr int FT_NG = 3;
struct FTileGeom {
  int W;       // lanes per row
  int nch;     // chunks of W lanes of the contiguous axis
  int tc;      // cells (y) / levels (z) a tile completes
  int halo;    // y: 0 = whole periodic line, 1 = halo rows; z: always 1
  int ntl;     // tiles along the sweep direction
  int lpb;     // y: levels per workgroup (whole-line tiles of short rows); z: 1
};
PAMA_HD int ftile_rows(const FTileGeom &G) { return G.tc + 2 * G.halo; }
PAMA_HD int ftile_threads(const FTileGeom &G) { return G.W * ftile_rows(G) * G.lpb; }
// (per-member vertical grids: a lane of a z tile holds its member's 31 coefficients of the level across the polynomials of a group --
// the tile kernel then runs with workgroups of at most 512 lanes, i.e. a register budget of 256: no scratch)
PAMA_HD int ftile_max_threads(const Params &P) { return P.vz_per_ens ? 512 : 1024; }
PAMA_HD FTileGeom ftile_geometry(const Params &P, int dir, int tc_req) {
  FTileGeom G;
  const int maxT = ftile_max_threads(P);
  const long long plane = (dir == 1) ? (long long)P.nx * P.nens : P.sz;     // contiguous lanes across the sweep direction
  const int n = (dir == 1) ? P.ny : P.nz;
  if (dir == 1) {
    const int nchunk = (int)((plane + 63) / 64);
    G.W = (int)((plane + nchunk - 1) / nchunk);                              // even chunks of at most 64 lanes
    G.nch = nchunk;
    if (tc_req <= 0 && n * G.W <= 256) {                                      // short lines: whole periodic lines, several levels per workgroup
      G.halo = 0; G.tc = n; G.ntl = 1;
      G.lpb = 256 / (n * G.W);
      if (G.lpb < 1) G.lpb = 1;
      if (G.lpb > P.nz) G.lpb = P.nz;
    } else {
      G.halo = 1; G.lpb = 1;
      int tc = tc_req > 0 ? tc_req : (G.W >= 32 ? 512 : 256) / G.W - 2;
      if (tc < 2) tc = 2;
      if (tc > n) tc = n;
      while (tc > 1 && (tc + 2) * G.W > maxT) tc--;
      G.ntl = (n + tc - 1) / tc;
      G.tc = tc_req > 0 ? tc : (n + G.ntl - 1) / G.ntl;
    }
  } else {
    G.W = 64; G.nch = (int)((plane + 63) / 64);
    G.halo = 1; G.lpb = 1;
    int tc = tc_req > 0 ? tc_req : 6;
    if (tc > n) tc = n;
    if (tc > maxT / 64 - 2) tc = maxT / 64 - 2;
    G.ntl = (n + tc - 1) / tc;
    G.tc = tc_req > 0 ? tc : (n + G.ntl - 1) / G.ntl;
  }
  return G;
}

struct FLane {
  bool poly, face, own, pay, wall;     // builds polynomials / forms its lower face / stores that face / stores its cell's differences
  int slot, slot_l, slot_r;            // LDS slots: own, of the row below (towards lower indices), of the row above
  int lev, et;                         // z: index of the cell's vertical table (level + 1); member (per-member tables)
  unsigned o5[5];                      // prim offsets of the cells c-2 .. c+2 along the sweep direction
  unsigned fo;                         // offset of the lane's lower face / of its cell inside a flux field of this direction
};
template <int DIR>
PAMA_D FLane ftile_lane(const Params &P, const FTileGeom &G, int bx, int by, int tx, int ty, int tz) {
  static_assert(DIR == 1 || DIR == 2, "y and z sweeps");
  FLane X;
  const int rows = ftile_rows(G);
  const int chunk = bx / G.ntl, tl = bx - chunk * G.ntl;
  const int c0 = tl * G.tc;
  const unsigned sz = (unsigned)P.sz, sy = (unsigned)P.sy;
  X.slot = (tz * rows + ty) * G.W + tx;
  X.wall = false; X.lev = 0; X.own = false;
  if (DIR == 1) {
    const int k = by * G.lpb + tz;
    const unsigned q = (unsigned)(chunk * G.W + tx);
    const int tcl = (c0 + G.tc <= P.ny) ? G.tc : P.ny - c0;
    const int nrow = tcl + 2 * G.halo;
    const bool valid = k < P.nz && q < (unsigned)P.nx * (unsigned)P.nens && tx < G.W && ty < nrow;
    const int c = c0 - G.halo + (valid ? ty : G.halo);
    const int j = c < 0 ? c + P.ny : (c >= P.ny ? c - P.ny : c);
    X.poly = valid;
    X.face = valid && (G.halo == 0 || ty >= 1);
    X.pay = valid && ty >= G.halo && ty < G.halo + tcl;
    X.own = X.pay;
    X.slot_l = (ty > 0) ? X.slot - G.W : X.slot + (nrow - 1) * G.W;
    X.slot_r = (ty < nrow - 1) ? X.slot + G.W : X.slot - (nrow - 1) * G.W;
    const unsigned kk = valid ? (unsigned)k : 0u, qq = valid ? q : 0u;
    const unsigned base = (kk + HS) * sz + qq;
#pragma unroll
    for (int s = 0; s < 5; s++) {
      const int jj = j + s - 2;
      X.o5[s] = member_offset((int)(base + (unsigned)(jj < 0 ? jj + P.ny : (jj >= P.ny ? jj - P.ny : jj)) * sy));
    }
    X.fo = member_offset((int)(kk * sz + (unsigned)j * sy + qq));
    X.et = (int)(qq % (unsigned)P.nens);
  } else {
    const unsigned p = (unsigned)(chunk * G.W + tx);
    const int tcl = (c0 + G.tc <= P.nz) ? G.tc : P.nz - c0;
    const int nrow = tcl + 2;
    const bool valid = p < sz && ty < nrow;
    const int c = c0 - 1 + (valid ? ty : 1);                                  // -1 .. nz
    X.poly = valid;
    X.face = valid && ty >= 1;
    X.pay = valid && ty >= 1 && ty <= tcl;
    X.own = X.pay || (valid && ty == tcl + 1 && c0 + tcl == P.nz);            // the top row of the top tile stores face nz
    X.wall = (c == 0 || c == P.nz);
    X.slot_l = X.slot - G.W;
    X.slot_r = X.slot + G.W;
    const unsigned pp = valid ? p : 0u;
#pragma unroll
    for (int s = 0; s < 5; s++) X.o5[s] = member_offset((int)((unsigned)(c + s - 2 + HS) * sz + pp));
    X.fo = member_offset((int)((unsigned)(c < 0 ? 0 : c) * sz + pp));
    X.lev = c + 1;
    X.et = (int)(pp % (unsigned)P.nens);
  }
  return X;
}
// the polynomial of the lane's cell: uniform-grid constants in y, the level's table in z (scalar loads when the table is the same
// for every member: a row of a z tile is one wavefront, the level is wave-uniform)
template <int DIR, bool VZ_PER_ENS>
PAMA_D void ftile_weno(const Params &P, const FLane &X, const WenoConsts &wc, const double (&u)[5], double &L, double &R) {
  if (DIR != 2) { weno5_const(u, wc, L, R); return; }
  if (VZ_PER_ENS) {
    weno5_table(u, P.vz + (long long)X.lev * VZ_STRIDE * P.nens + X.et, (long long)P.nens, wc, L, R);
  } else {
    weno5_table(u, as_constant(P.vz + (long long)uni_int(X.lev) * VZ_STRIDE), 1, wc, L, R);
  }
}
// group 0, A: rho*u_n, p, u_n
//   WITH_N false: only rho*u_n and p (what the face mass flux needs) -- the workgroups that take one group of advected quantities
//   BESIDE the acoustic workgroup rebuild the mass flux themselves (flux_tile_part)
template <int DIR, bool VZ_PER_ENS, bool WITH_N = true>
PAMA_D void ftile_acoustic_polys(const Params &P, const double *__restrict__ prim, const FLane &X, double (&L)[FT_NG], double (&R)[FT_NG]) {
  const WenoConsts wc = weno_consts();
  const int ncomp = (DIR == 1) ? P_V : P_W;
  gc_ptr fr = uni(prim + (long long)P_RHO * P.prim_fs), fn = uni(prim + (long long)ncomp * P.prim_fs), fp = uni(prim + (long long)P_PRES * P.prim_fs);
  double m[5], p[5], n[5];
#pragma unroll
  for (int s = 0; s < 5; s++) {
    n[s] = fn[X.o5[s]];
    m[s] = mul_rn(fr[X.o5[s]], n[s]);
    p[s] = fp[X.o5[s]];
  }
  ftile_weno<DIR, VZ_PER_ENS>(P, X, wc, m, L[0], R[0]);
  ftile_weno<DIR, VZ_PER_ENS>(P, X, wc, p, L[1], R[1]);
  if (WITH_N) ftile_weno<DIR, VZ_PER_ENS>(P, X, wc, n, L[2], R[2]);
  else L[2] = R[2] = 0.0;
}
// group 0, B: face mass flux (stored as a face by the lane that owns it) and normal-momentum flux (Dycore.h:341-366,:477-496)
template <int DIR>
PAMA_D void ftile_acoustic_face(const Params &P, double *__restrict__ flux, const FLane &X, const double (&L)[FT_NG],
                                const double (&Rl)[FT_NG], double &ruf, double &fn) {
  double ppf;
  acoustic_face(Rl[0], L[0], Rl[1], L[1], (DIR == 2) && X.wall, ruf, ppf);
  const double val = (ruf > 0.0) ? Rl[2] : L[2];            // upwind (Dycore.h:368)
  fn = fma(ruf, val, ppf);
  if (X.own) uniw(flux)[X.fo] = ruf;
}
// the advected quantities fa[0..nf) (advected-field indices: 0 u, 1 v, 2 w, 3 theta, 4.. tracers)
template <int DIR, bool VZ_PER_ENS>
PAMA_D void ftile_adv_polys(const Params &P, const double *__restrict__ prim, const FLane &X, const int *fa, int nf,
                            double (&L)[FT_NG], double (&R)[FT_NG]) {
  const WenoConsts wc = weno_consts();
#pragma unroll
  for (int n = 0; n < FT_NG; n++) {
    if (n >= nf) { L[n] = R[n] = 0.0; continue; }
    gc_ptr f = uni(prim + (long long)(P_U + fa[n]) * P.prim_fs);
    double w[5];
#pragma unroll
    for (int s = 0; s < 5; s++) w[s] = f[X.o5[s]];
    ftile_weno<DIR, VZ_PER_ENS>(P, X, wc, w, L[n], R[n]);
  }
}
// their fluxes through the lane's lower face; tracers leave as faces at once, state variables wait for the difference
template <int DIR>
PAMA_D void ftile_adv_face(const Params &P, double *__restrict__ flux, const FLane &X, const int *fa, int nf, const double (&L)[FT_NG],
                           const double (&Rl)[FT_NG], double ruf, double (&F)[FT_NG]) {
  const bool up = ruf > 0.0;
  const long long fs = (DIR == 2) ? P.fz_fs : P.ncell;
#pragma unroll
  for (int n = 0; n < FT_NG; n++) {
    if (n >= nf) { F[n] = 0.0; continue; }
    F[n] = mul_rn(ruf, up ? Rl[n] : L[n]);
    if (fa[n] >= 4 && X.own) uniw(flux + (long long)(1 + fa[n]) * fs)[X.fo] = F[n];
  }
}
// the cell's flux difference F[c] - F[c+1] of one state variable (advected index a; the normal velocity included)
template <int DIR>
PAMA_D void ftile_store_diff(const Params &P, double *__restrict__ flux, const FLane &X, int a, double F_lo, double F_hi) {
  const long long fs = (DIR == 2) ? P.fz_fs : P.ncell;
  uniw(flux + (long long)(1 + a) * fs)[X.fo] = F_lo - F_hi;
}
// the groups of a sweep after the acoustic one: advected indices in sweep order, FT_NG per group; the state variables come first
// and all sit in group 1.  Returns the number of groups (>= 1); grp[g][n] = advected index or -1
PAMA_HD int ftile_groups(const Params &P, int dir, int (*grp)[FT_NG], int max_groups) {
  const int ncomp_a = (dir == 1) ? 1 : 2;                    // advected index of the normal velocity
  int ng = 0, nf = 0;
  for (int n = 0; n < FT_NG; n++) grp[0][n] = -1;
  for (int a = 0; a < 4 + P.nt; a++) {
    if (a == ncomp_a) continue;
    if (a == 1 && P.sim2d) continue;                          // 2-D: v is neither reconstructed nor stored (skip_advected_v)
    if (nf == FT_NG) {
      ng++; nf = 0;
      if (ng >= max_groups) return ng;
      for (int n = 0; n < FT_NG; n++) grp[ng][n] = -1;
    }
    grp[ng][nf++] = a;
  }
  return ng + 1;
}

// ------------------------------------------------------------------------------------------------
// Optional idealised initial conditions of Dycore::init (Dycore.h:986-1090).  Both build the conserved cell averages
// with 9x9x9-point Gauss-Lobatto quadrature, accumulated in the reference's loop order (kk, jj, ii), and convert them to
// coupler fields exactly as convert_dynamics_to_coupler does (Dycore.h:1313-1330).
PAMA_D double sample_ellipse_cosine(double amp, double x, double y, double z, double x0, double y0, double z0, double xrad,
                                    double yrad, double zrad) {   // Dycore.h:753-766
  double dist = sqrt(((x - x0) / xrad) * ((x - x0) / xrad) + ((y - y0) / yrad) * ((y - y0) / yrad) +
                     ((z - z0) / zrad) * ((z - z0) / zrad)) * M_PI / 2.;
  if (dist <= M_PI / 2.) return amp * pow(cos(dist), 2.0);
  return 0.;
}

// conserved (rho, rho u, rho v, rho w, rho theta, rho_t...) -> coupler fields of one cell
PAMA_D void store_coupler_cell(const Params &P, double rho, double ru, double rv, double rw, double rt, double rho_v_wv,
                               double *__restrict__ rho_d_c, double *__restrict__ u_c, double *__restrict__ v_c,
                               double *__restrict__ w_c, double *__restrict__ temp_c, const TracerPtrs &trc, long long idx) {
  double theta = rt / rho;
  double press = P.C0 * pow_pos(P, rho * theta, P.gamma);
  double rho_d = rho;
  for (int t = 0; t < P.nt; t++) {
    double r = (t == P.idWV) ? rho_v_wv : 0.0;
    if ((P.mass_mask >> t) & 1ull) rho_d -= r;
    trc.p[t][idx] = r;
  }
  rho_d_c[idx] = rho_d;
  u_c[idx] = ru / rho;
  v_c[idx] = rv / rho;
  w_c[idx] = rw / rho;
  temp_c[idx] = press / (rho_d * P.R_d + rho_v_wv * P.R_v);
}

// DATA_SPEC_THERMAL (Dycore.h:1021-1088): theta = 300 K hydrostatic atmosphere + 2 K cos^2 bubble at (xlen/2, ylen/2, 2 km)
PAMA_D void init_thermal_body(const Params &P, double xlen, double ylen, double cp_d, double p0,
                              const double *__restrict__ zmid, double *__restrict__ rho_d_c, double *__restrict__ u_c,
                              double *__restrict__ v_c, double *__restrict__ w_c, double *__restrict__ temp_c,
                              const TracerPtrs &trc, const CellId &c) {
  const double qp[9] = AWFL_GLL9_PTS_INIT, qw[9] = AWFL_GLL9_WTS_INIT;
  const long long ke = (long long)c.k * P.nens + c.e;
  const double dzk = P.dz[ke], zm = zmid[ke];
  // hydrostatic background cell averages (Dycore.h:1035-1047)
  double hr = 0., hp = 0.;
  for (int kk = 0; kk < 9; kk++) {
    double z = zm + qp[kk] * dzk;
    const double theta0 = 300.;
    double exner = 1. - P.grav * z / (cp_d * theta0);            // hydro_const_theta, Dycore.h:739-748
    double p = p0 * pow(exner, (cp_d / P.R_d));
    double rt = pow_pos(P, (p / P.C0), (1.0 / P.gamma));
    double r = rt / theta0;
    hr += r * qw[kk];
    hp += P.C0 * pow_pos(P, r * theta0, P.gamma) * qw[kk];
  }
  const double ht = pow_pos(P, hp / P.C0, 1.0 / P.gamma) / hr;
  double sR = 0., sU = 0., sV = 0., sW = 0., sT = 0., sQ = 0.;
  for (int kk = 0; kk < 9; kk++)
    for (int jj = 0; jj < 9; jj++)
      for (int ii = 0; ii < 9; ii++) {
        double x = (c.i + 0.5) * P.dx + qp[ii] * P.dx;
        double y = (c.j + 0.5) * P.dy + qp[jj] * P.dy;
        if (P.sim2d) y = ylen / 2;
        double z = zm + qp[kk] * dzk;
        double rho = hr, u = 0, v = 0, w = 0, rho_v = 0;
        double theta = ht + sample_ellipse_cosine(2.0, x, y, z, xlen / 2, ylen / 2, 2000., 2000., 2000., 2000.);
        double wt = qw[ii] * qw[jj] * qw[kk];
        sR += rho * wt; sU += rho * u * wt; sV += rho * v * wt; sW += rho * w * wt; sT += rho * theta * wt;
        sQ += rho_v * wt;
      }
  store_coupler_cell(P, sR, sU, sV, sW, sT, sQ, rho_d_c, u_c, v_c, w_c, temp_c, trc, c.idx);
}

// init_supercell (Dycore.h:1096-1276): the column quantities (hydrostatic cell means, vapour density at the 9 GLL
// levels of each cell) are integrated on the host at init (awfl_vertical.h); this is the 3-D fill (Dycore.h:1233-1275).
//   hy_dens, hy_pres (nz,nens); dens_vap_gll (nz,9,nens)
PAMA_D void init_supercell_body(const Params &P, const double *__restrict__ zmid, const double *__restrict__ hy_dens,
                                const double *__restrict__ hy_pres, const double *__restrict__ dens_vap_gll,
                                double *__restrict__ rho_d_c, double *__restrict__ u_c, double *__restrict__ v_c,
                                double *__restrict__ w_c, double *__restrict__ temp_c, const TracerPtrs &trc,
                                const CellId &c) {
  const double qp[9] = AWFL_GLL9_PTS_INIT, qw[9] = AWFL_GLL9_WTS_INIT;
  const long long ke = (long long)c.k * P.nens + c.e;
  const double dzk = P.dz[ke], zm = zmid[ke];
  const double rho = hy_dens[ke];
  const double rt = pow_pos(P, hy_pres[ke] / P.C0, 1.0 / P.gamma);
  double sU = 0., sV = 0., sW = 0., sQ = 0.;
  for (int kk = 0; kk < 9; kk++) {
    const double zloc = zm + qp[kk] * dzk;
    const double zs = 5000, us = 30, uc = 15;
    const double uvel = zloc < zs ? us * (zloc / zs) - uc : us - uc;
    const double dens_vap = dens_vap_gll[((long long)c.k * 9 + kk) * P.nens + c.e];
    for (int jj = 0; jj < 9; jj++)
      for (int ii = 0; ii < 9; ii++) {
        double factor = qw[ii] * qw[jj] * qw[kk];
        sU += rho * uvel * factor; sV += rho * 0.0 * factor; sW += rho * 0.0 * factor;
        sQ += dens_vap * factor;
      }
  }
  store_coupler_cell(P, rho, sU, sV, sW, rt, sQ, rho_d_c, u_c, v_c, w_c, temp_c, trc, c.idx);
}

// ------------------------------------------------------------------------------------------------
// declare_current_profile_as_hydrostatic (Dycore.h:1439-1501).
// interface pressure 0.5*(p_L + p_R) at face k of column (j,i,e) from the vertical WENO (Dycore.h:1457-1482)
template <bool VZ_PER_ENS>
PAMA_D double pint_body(const Params &P, const double *__restrict__ prim, int kf, long long c2, int e) {
  const WenoConsts wc = weno_consts();
  const double *pp = prim + (long long)P_PRES * P.prim_fs;
  const long long vts = VZ_PER_ENS ? (long long)P.nens : 1;
  double w[5], L, R, Rl, Lr;
  // left state: right edge of cell kf-1 (stencil kf-3..kf+1); right state: left edge of cell kf
  for (int s = 0; s < 5; s++) w[s] = pp[(long long)(kf - 3 + s + HS) * P.sz + c2];
  const double *t0 = VZ_PER_ENS ? P.vz + ((long long)kf * VZ_STRIDE) * P.nens + e : P.vz + (long long)kf * VZ_STRIDE;
  weno5_table(w, t0, vts, wc, L, Rl);
  for (int s = 0; s < 5; s++) w[s] = pp[(long long)(kf - 2 + s + HS) * P.sz + c2];
  const double *t1 = VZ_PER_ENS ? P.vz + ((long long)(kf + 1) * VZ_STRIDE) * P.nens + e : P.vz + (long long)(kf + 1) * VZ_STRIDE;
  weno5_table(w, t1, vts, wc, Lr, R);
  return 0.5 * (Rl + Lr);
}

// The same mean of mode A from interface pressures computed beforehand -- ONE thread per (face, column) instead of one per (level,
// member) walking ny*nx columns with four polynomials each (hydro_pint_face: `pint` is (nz+1, ny, nx, nens), the layout of a z flux
// field); the sum runs over the same values in the same order: same bits as hydro_mean_body.
template <bool VZ_PER_ENS>
PAMA_D void hydro_pint_face(const Params &P, const double *__restrict__ prim, double *__restrict__ pint, int kf, int j, int i, int e) {
  const long long c2 = (long long)j * P.sy + (long long)i * P.sx + e;
  pint[(long long)kf * P.sz + c2] = pint_body<VZ_PER_ENS>(P, prim, kf, c2, e);
}
PAMA_D void hydro_mean_from_pint(const Params &P, const double *__restrict__ prim, const double *__restrict__ pint,
                                 double *__restrict__ grav_var, int k, int e) {
#pragma clang fp contract(off)
  const double r_nx_ny = 1. / (P.nx * P.ny);
  const long long ke = (long long)k * P.nens + e;
  const double dzk = P.dz[ke];
  double g = 0.0;
  for (int j = 0; j < P.ny; j++)
    for (int i = 0; i < P.nx; i++) {
      const long long c2 = (long long)j * P.sy + (long long)i * P.sx + e;
      const double dens = prim[P_RHO * P.prim_fs + (long long)(k + HS) * P.sz + c2];
      const double pu = pint[(long long)(k + 1) * P.sz + c2], pl = pint[(long long)k * P.sz + c2];
      g += -(pu - pl) / (dens * dzk) * r_nx_ny;
    }
  grav_var[ke] = g;
}

// horizontal means for level k, member e, accumulated in the reference's serial order (j outer, i inner), which
// makes the result deterministic (the reference uses atomicAdd, Dycore.h:1487,1499-1500).
// mode B (no gravity balance): the means of pressure and density, Dycore.h:1492-1501
// (the products are rounded before they are added, as the reference's atomicAdd of `value * r_nx_ny` does: a contracted fma shifts a
//  level's mean pressure by ~1e-10 Pa, which mode B differences over dz -- 1e-12 m/s in w after one sub-step, fuzz seed 1858)
PAMA_D void hydro_cell_mean_body(const Params &P, const double *__restrict__ prim, double *__restrict__ hy_dens,
                                 double *__restrict__ hy_pres, int k, int e) {
#pragma clang fp contract(off)
  const double r_nx_ny = 1. / (P.nx * P.ny);
  const long long ke = (long long)k * P.nens + e;
  double hp = 0.0, hd = 0.0;
  for (int j = 0; j < P.ny; j++)
    for (int i = 0; i < P.nx; i++) {
      const long long o = (long long)(k + HS) * P.sz + (long long)j * P.sy + (long long)i * P.sx + e;
      hp += prim[P_PRES * P.prim_fs + o] * r_nx_ny;
      hd += prim[P_RHO * P.prim_fs + o] * r_nx_ny;
    }
  hy_pres[ke] = hp;
  hy_dens[ke] = hd;
}
// both modes in one body, mode A with the interface pressures formed in place (Dycore.h:1450-1490).  The device runs mode A in two
// steps (hydro_pint_face, hydro_mean_from_pint); this direct form is what the host emulation checks the two steps against.
template <bool VZ_PER_ENS>
PAMA_D void hydro_mean_body(const Params &P, const double *__restrict__ prim, double *__restrict__ grav_var,
                            double *__restrict__ hy_dens, double *__restrict__ hy_pres, int k, int e) {
#pragma clang fp contract(off)
  if (!P.grav_balance) { hydro_cell_mean_body(P, prim, hy_dens, hy_pres, k, e); return; }
  const double r_nx_ny = 1. / (P.nx * P.ny);
  const long long ke = (long long)k * P.nens + e;
  double g = 0.0;
  const double dzk = P.dz[ke];
  for (int j = 0; j < P.ny; j++)
    for (int i = 0; i < P.nx; i++) {
      const long long c2 = (long long)j * P.sy + (long long)i * P.sx + e;
      double dens = prim[P_RHO * P.prim_fs + (long long)(k + HS) * P.sz + c2];
      double pu = pint_body<VZ_PER_ENS>(P, prim, k + 1, c2, e), pl = pint_body<VZ_PER_ENS>(P, prim, k, c2, e);
      g += -(pu - pl) / (dens * dzk) * r_nx_ny;
    }
  grav_var[ke] = g;
}

}  // namespace pama
