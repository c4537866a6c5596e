// lsforcing_device.h -- the arithmetic of the large-scale forcing (SAM's forcing + subsidence + nudging + coriolis, once per CRM step):
// a prescribed large-scale vertical velocity that advects every column, horizontally uniform tendencies of temp and vapour, a relaxation
// of the level means towards target profiles, and the Coriolis force about a geostrophic wind.  Device functions that are plain inline
// C++ outside hipcc: the HIP kernels in modules_kernels.hip call them, and tests/emu/lsforcing_emu.cpp compiles the same bodies with g++
// (-ffp-contract=off).  The method is not part of the reference tree; the yardstick is the numpy restatement of the contract in
// tests/lsforcing_ref.py, held bit for bit (include/pam_amd_modules.h at pam_amd_ls_forcing).
// Fields are (nz, ny, nx, nens), members fastest; profiles are (nz, nens); fcor is (nens).  A thread of the forcing owns a (column,
// member): `off` is its offset into level 0, `level` = ny nx nens the stride of a level, `zs` = nens the stride of a profile row.
// Contraction into fma is switched off inside each body, so the device and the host give the same bits.
#pragma once

#include "msa_device.h"      // PAMA_D, PAMA_NO_CONTRACT, and the slot order of the level means: NS, r_ncol, mean_add, fold

namespace pama {
namespace lsforcing {

constexpr int AHEAD = 4;                 // levels whose loads are requested before the first of them is used
constexpr int MAX_TRACERS = 64;          // tracers per call
constexpr int CHUNK = 4;                 // tracers that share one walk of the column, and with it the rho of every level
enum { X_T, X_Q, X_U, X_V, NX };         // the four nudged quantities: temp, qv = rho_v / rho, uvel, vvel
enum { N_TEMP, N_RHO_D, N_RHO_V, N_U, N_V, NFIELDS };      // the field table of the nudging

// ---- the level means and the nudging increments

PAMA_D double quotient(double a, double b) {
  PAMA_NO_CONTRACT
  return a / b;
}

PAMA_D double total_density(double rho_d, double rho_v) {
  PAMA_NO_CONTRACT
  return rho_d + rho_v;
}

// one slot's share of the level means of one (level, member), in msa's order (cell c belongs to slot c % 16, v r rounded before it is
// added); f[i] points at (k, 0, e) of field i.  A quantity that is not wanted is not read; qv is formed per cell before it enters
PAMA_D void mean_walk(const double *const *f, long long stride, int ncol, int slot, const bool (&want)[NX], double (&acc)[NX]) {
  const double r = msa::r_ncol(ncol);
  acc[X_T] = 0.0; acc[X_Q] = 0.0; acc[X_U] = 0.0; acc[X_V] = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
  for (int c = slot; c < ncol; c += msa::NS) {
    const long long o = (long long)c * stride;
    if (want[X_T]) acc[X_T] = msa::mean_add(acc[X_T], f[N_TEMP][o], r);
    if (want[X_Q]) {
      const double rv = f[N_RHO_V][o];
      acc[X_Q] = msa::mean_add(acc[X_Q], quotient(rv, total_density(f[N_RHO_D][o], rv)), r);
    }
    if (want[X_U]) acc[X_U] = msa::mean_add(acc[X_U], f[N_U][o], r);
    if (want[X_V]) acc[X_V] = msa::mean_add(acc[X_V], f[N_V][o], r);
  }
}

// inc = (dt rate) (target - mean)
PAMA_D double increment(double dt, double rate, double target, double mean) {
  PAMA_NO_CONTRACT
  const double a = dt * rate;
  const double d = target - mean;
  return a * d;
}

// ---- the forcing

// g of temp: temp + gc z, the quantity the SGS diffuses (gc = grav / cp_d, formed once on the host)
PAMA_D double static_energy(double temp, double gc, double z) {
  PAMA_NO_CONTRACT
  return temp + gc * z;
}

// first-order upwind in advective form.  w > 0 takes the level below, w < 0 the level above: adv = (w (g_hi - g_lo)) / (z_hi - z_lo),
// dg = -(dt adv).  The term exists (-> true) where the upwind level does; a NaN w makes dg that NaN.  One division, whichever way the
// wind blows, and no branch: neighbouring members may subside and rise
struct Upwind {
  double w, dz;        // dz = z_hi - z_lo of the upwind pair
  bool below, active;
};
PAMA_D Upwind upwind(double w, double z_m, double z, double z_p, bool has_below, bool has_above) {
  PAMA_NO_CONTRACT
  Upwind u;
  u.w = w;
  u.below = w > 0.0;
  u.dz = u.below ? z - z_m : z_p - z;
  u.active = (u.below && has_below) || (w < 0.0 && has_above) || w != w;
  return u;
}
PAMA_D double subsidence(const Upwind &u, double g_m, double g, double g_p, double dt) {
  PAMA_NO_CONTRACT
  const double d = u.below ? g - g_m : g_p - g;
  const double n = u.w * d;
  const double adv = n / u.dz;
  const double t = dt * adv;
  return u.w != u.w ? u.w : -t;
}

// d = dt tend + inc, an absent addend absent; -> whether there is one
PAMA_D bool uniform_increment(double dt, bool has_tend, double tend, bool has_inc, double inc, double &d) {
  PAMA_NO_CONTRACT
  d = 0.0;
  if (has_tend) {
    const double t = dt * tend;
    d = has_inc ? t + inc : t;
  } else if (has_inc) {
    d = inc;
  }
  return has_tend || has_inc;
}

// x + (dg + d), an absent addend absent; with neither, x keeps its bits
PAMA_D double plus_increments(double x, bool has_dg, double dg, bool has_d, double d) {
  PAMA_NO_CONTRACT
  if (has_dg && has_d) return x + (dg + d);
  if (has_dg) return x + dg;
  if (has_d) return x + d;
  return x;
}

// rho_x + rho (dg + d), the same way; then, where the tracer is flagged positive, what is below zero becomes 0.0 (a NaN stays)
PAMA_D double tracer_update(double x, double rho, bool has_dg, double dg, bool has_d, double d, bool positive) {
  PAMA_NO_CONTRACT
  if (!has_dg && !has_d) return x;
  const double s = has_dg && has_d ? dg + d : (has_dg ? dg : d);
  const double m = rho * s;
  const double r = x + m;
  return positive && r < 0.0 ? 0.0 : r;
}

// the trapezoidal rotation of the ageostrophic wind, neutral for any f dt: a = 0.5 (f dt); c1 = 1 - a a; c2 = 2 a; den = 1 + a a
struct Rotation { double c1, c2, den; };
PAMA_D Rotation rotation(double fcor, double dt) {
  PAMA_NO_CONTRACT
  const double fd = fcor * dt;
  const double a = 0.5 * fd;
  const double aa = a * a;
  return Rotation{1.0 - aa, 2.0 * a, 1.0 + aa};
}
// u' = ug + ((c1 du) + (c2 dv)) / den; v' = vg + ((c1 dv) - (c2 du)) / den
PAMA_D void rotate(const Rotation &R, double ug, double vg, double &u, double &v) {
  PAMA_NO_CONTRACT
  const double du = u - ug;
  const double dv = v - vg;
  const double a = R.c1 * du;
  const double b = R.c2 * dv;
  const double c = R.c1 * dv;
  const double d = R.c2 * du;
  const double nu = a + b;
  const double nv = c - d;
  u = ug + nu / R.den;
  v = vg + nv / R.den;
}

// what a launch is given.  Every pointer points at element 0 of its array.  The tracer table is the caller's with the vapour (rho_v
// itself, `vapour` its place, -1: not in the table) moved to the END: a walk reads rho_v for the rho of its levels, and rho is the one
// of entry for the whole call, so the walk that writes rho_v comes last.  Without subsidence only the vapour has anything to take, and
// the table is the vapour alone (or empty)
struct Args {
  double *uvel, *vvel, *temp;
  const double *rho_d, *rho_v, *zmid;
  const double *wsub, *temp_tend, *qv_tend, *inc[NX], *fcor, *ug, *vg;
  double dt, gc;
  int num_tracers, vapour;
  double *tr[MAX_TRACERS];
  unsigned char positive[MAX_TRACERS];
};

inline Args make_args(double *uvel, double *vvel, double *temp, int num_tracers, double *const *tracers, const unsigned char *positive,
                      const double *rho_d, const double *rho_v, const double *zmid, const double *wsub, const double *temp_tend,
                      const double *qv_tend, const double *const *inc, const double *fcor, const double *ug, const double *vg, double dt,
                      double gc) {
  Args A;
  A.uvel = uvel; A.vvel = vvel; A.temp = temp; A.rho_d = rho_d; A.rho_v = rho_v; A.zmid = zmid;
  A.wsub = wsub; A.temp_tend = temp_tend; A.qv_tend = qv_tend; A.fcor = fcor; A.ug = ug; A.vg = vg;
  for (int x = 0; x < NX; x++) A.inc[x] = inc ? inc[x] : nullptr;
  A.dt = dt; A.gc = gc;
  for (int i = 0; i < MAX_TRACERS; i++) { A.tr[i] = nullptr; A.positive[i] = 0; }
  int vapour = -1, n = 0;
  for (int i = 0; i < num_tracers; i++)
    if (tracers[i] == rho_v && vapour < 0) vapour = i;
  if (wsub)
    for (int i = 0; i < num_tracers; i++)
      if (i != vapour) { A.tr[n] = tracers[i]; A.positive[n] = positive[i]; n++; }
  A.vapour = -1;
  if (vapour >= 0 && (wsub || qv_tend || A.inc[X_Q])) { A.tr[n] = tracers[vapour]; A.positive[n] = positive[vapour]; A.vapour = n; n++; }
  A.num_tracers = n;
  return A;
}

// uvel, vvel and temp of one (column, member), walked upward; the values of entry of the level below and of the level itself are kept
// in registers, so the update is in place.  With SUBS the loads of levels k0+1 .. k0+AHEAD (the upper neighbours) are requested before
// level k0 is formed; without it there is no vertical coupling and the loads are the AHEAD levels themselves.  A field that nothing
// acts on is neither read nor written (the same for every thread of a launch)
template <class IDX, bool SUBS>
PAMA_D void walk_winds_temp(const Args &A, IDX off, IDX level, IDX zs, int e, int nz) {
  PAMA_NO_CONTRACT
  const bool coriolis = A.fcor != nullptr;
  const bool do_uv = SUBS || A.inc[X_U] || A.inc[X_V] || coriolis;
  const bool do_t = SUBS || A.temp_tend || A.inc[X_T];
  if (!do_uv && !do_t) return;
  double *U = A.uvel + off, *V = A.vvel + off, *T = A.temp + off;
  const double *Z = A.zmid + e;
  const double *W = SUBS ? A.wsub + e : nullptr;
  const double *TT = A.temp_tend ? A.temp_tend + e : nullptr, *IT = A.inc[X_T] ? A.inc[X_T] + e : nullptr;
  const double *IU = A.inc[X_U] ? A.inc[X_U] + e : nullptr, *IV = A.inc[X_V] ? A.inc[X_V] + e : nullptr;
  const double *UG = coriolis ? A.ug + e : nullptr, *VG = coriolis ? A.vg + e : nullptr;
  Rotation R{1.0, 0.0, 1.0};
  if (coriolis) R = rotation(A.fcor[e], A.dt);

  // the carried values of entry: level k-1 (_m) and level k (_c); g of temp beside temp itself
  double u_m = 0.0, v_m = 0.0, g_m = 0.0, z_m = 0.0, u_c = 0.0, v_c = 0.0, t_c = 0.0, g_c = 0.0, z_c = 0.0;
  if constexpr (SUBS) {
    z_c = Z[0];
    if (do_uv) { u_c = U[0]; v_c = V[0]; }
    if (do_t) { t_c = T[0]; g_c = static_energy(t_c, A.gc, z_c); }
    u_m = u_c; v_m = v_c; g_m = g_c; z_m = z_c;
  }
  for (int k0 = 0; k0 < nz; k0 += AHEAD) {
    double a_u[AHEAD], a_v[AHEAD], a_t[AHEAD], a_z[AHEAD], a_w[AHEAD], a_tt[AHEAD], a_it[AHEAD], a_iu[AHEAD], a_iv[AHEAD], a_ug[AHEAD],
        a_vg[AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const IDX kc = (IDX)(k0 + b < nz ? k0 + b : nz - 1);                       // the level itself
      const IDX kf = SUBS ? (IDX)(k0 + b + 1 < nz ? k0 + b + 1 : nz - 1) : kc;   // the level whose fields are loaded
      const IDX o = kf * level;
      a_u[b] = do_uv ? U[o] : 0.0;
      a_v[b] = do_uv ? V[o] : 0.0;
      a_t[b] = do_t ? T[o] : 0.0;
      a_z[b] = SUBS ? Z[kf * zs] : 0.0;
      a_w[b] = SUBS ? W[kc * zs] : 0.0;
      a_tt[b] = TT ? TT[kc * zs] : 0.0;
      a_it[b] = IT ? IT[kc * zs] : 0.0;
      a_iu[b] = IU ? IU[kc * zs] : 0.0;
      a_iv[b] = IV ? IV[kc * zs] : 0.0;
      a_ug[b] = coriolis ? UG[kc * zs] : 0.0;
      a_vg[b] = coriolis ? VG[kc * zs] : 0.0;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const int k = k0 + b;
      if (k >= nz) break;
      const IDX o = (IDX)k * level;
      double u, v, t, dg_u = 0.0, dg_v = 0.0, dg_t = 0.0;
      bool active = false;
      if constexpr (SUBS) {
        const double g_p = do_t ? static_energy(a_t[b], A.gc, a_z[b]) : 0.0;
        const Upwind up = upwind(a_w[b], z_m, z_c, a_z[b], k > 0, k < nz - 1);
        active = up.active;
        u = u_c; v = v_c; t = t_c;
        if (do_uv) {
          dg_u = subsidence(up, u_m, u_c, a_u[b], A.dt);
          dg_v = subsidence(up, v_m, v_c, a_v[b], A.dt);
        }
        if (do_t) dg_t = subsidence(up, g_m, g_c, g_p, A.dt);
        u_m = u_c; v_m = v_c; g_m = g_c; z_m = z_c;
        u_c = a_u[b]; v_c = a_v[b]; t_c = a_t[b]; g_c = g_p; z_c = a_z[b];
      } else {
        u = a_u[b]; v = a_v[b]; t = a_t[b];
      }
      if (do_t) {
        double d_t;
        const bool has_d = uniform_increment(A.dt, TT != nullptr, a_tt[b], IT != nullptr, a_it[b], d_t);
        T[o] = plus_increments(t, active, dg_t, has_d, d_t);
      }
      if (do_uv) {
        u = plus_increments(u, active, dg_u, IU != nullptr, a_iu[b]);
        v = plus_increments(v, active, dg_v, IV != nullptr, a_iv[b]);
        if (coriolis) rotate(R, a_ug[b], a_vg[b], u, v);
        U[o] = u;
        V[o] = v;
      }
    }
  }
}

// tracers first .. first + n - 1 of the table (n <= CHUNK) of one (column, member), walked upward the same way; g = rho_x / rho, rho =
// rho_d + rho_v of entry, formed once per level and shared by the chunk.  The vapour takes d_q = dt qv_tend + inc_q as well
template <class IDX, bool SUBS>
PAMA_D void walk_tracers(const Args &A, int first, int n, IDX off, IDX level, IDX zs, int e, int nz) {
  PAMA_NO_CONTRACT
  const double *RD = A.rho_d + off, *RV = A.rho_v + off;
  const double *Z = A.zmid + e;
  const double *W = SUBS ? A.wsub + e : nullptr;
  const double *QT = A.qv_tend ? A.qv_tend + e : nullptr, *IQ = A.inc[X_Q] ? A.inc[X_Q] + e : nullptr;
  double *X[CHUNK];
  bool pos[CHUNK];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < CHUNK; i++) {
    X[i] = (i < n ? A.tr[first + i] : A.tr[first]) + off;      // an absent one points at the first and is never touched
    pos[i] = i < n && A.positive[first + i] != 0;
  }
  const int iv = A.vapour - first;                            // the vapour's place in this chunk (the last, where it is in it)
  const bool vap_d = iv >= 0 && iv < n && (QT || IQ);

  double z_m = 0.0, z_c = 0.0, rho_c = 0.0, x_c[CHUNK], g_c[CHUNK], g_m[CHUNK];
  if constexpr (SUBS) {
    z_c = Z[0];
    z_m = z_c;
    rho_c = total_density(RD[0], RV[0]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < CHUNK; i++) {
      x_c[i] = i < n ? X[i][0] : 0.0;
      g_c[i] = quotient(x_c[i], rho_c);
      g_m[i] = g_c[i];
    }
  }
  for (int k0 = 0; k0 < nz; k0 += AHEAD) {
    double a_rd[AHEAD], a_rv[AHEAD], a_z[AHEAD], a_w[AHEAD], a_qt[AHEAD], a_iq[AHEAD], a_x[CHUNK][AHEAD];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const IDX kc = (IDX)(k0 + b < nz ? k0 + b : nz - 1);
      const IDX kf = SUBS ? (IDX)(k0 + b + 1 < nz ? k0 + b + 1 : nz - 1) : kc;
      const IDX o = kf * level;
      a_rd[b] = RD[o];
      a_rv[b] = RV[o];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int i = 0; i < CHUNK; i++) a_x[i][b] = i < n ? X[i][o] : 0.0;
      a_z[b] = SUBS ? Z[kf * zs] : 0.0;
      a_w[b] = SUBS ? W[kc * zs] : 0.0;
      a_qt[b] = QT ? QT[kc * zs] : 0.0;
      a_iq[b] = IQ ? IQ[kc * zs] : 0.0;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < AHEAD; b++) {
      const int k = k0 + b;
      if (k >= nz) break;
      const IDX o = (IDX)k * level;
      const double rho_f = total_density(a_rd[b], a_rv[b]);      // of the loaded level: k+1 with SUBS, else k
      double d_q = 0.0;
      const bool has_dq = vap_d && uniform_increment(A.dt, QT != nullptr, a_qt[b], IQ != nullptr, a_iq[b], d_q);
      if constexpr (SUBS) {
        const Upwind up = upwind(a_w[b], z_m, z_c, a_z[b], k > 0, k < nz - 1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < CHUNK; i++) {
          if (i >= n) break;
          const double g_p = quotient(a_x[i][b], rho_f);
          const double dg = subsidence(up, g_m[i], g_c[i], g_p, A.dt);
          X[i][o] = tracer_update(x_c[i], rho_c, up.active, dg, has_dq && i == iv, d_q, pos[i]);
          g_m[i] = g_c[i]; g_c[i] = g_p; x_c[i] = a_x[i][b];
        }
        z_m = z_c; z_c = a_z[b]; rho_c = rho_f;
      } else {      // the table is the vapour alone (make_args): place 0
        if (has_dq) X[0][o] = tracer_update(a_x[0][b], rho_f, false, 0.0, true, d_q, pos[0]);
      }
    }
  }
}

// the whole of one (column, member): the winds and temp, then the tracers by chunks, the vapour's chunk last (make_args)
template <class IDX, bool SUBS>
PAMA_D void column(const Args &A, IDX off, IDX level, IDX zs, int e, int nz) {
  walk_winds_temp<IDX, SUBS>(A, off, level, zs, e, nz);
  for (int first = 0; first < A.num_tracers; first += CHUNK) {
    const int n = A.num_tracers - first < CHUNK ? A.num_tracers - first : CHUNK;
    walk_tracers<IDX, SUBS>(A, first, n, off, level, zs, e, nz);
  }
}

}  // namespace lsforcing
}  // namespace pama
