// Host emulation of the fused stage with water vapour's FCT seed loaded only where it can matter (flux_x_update_body<., ., ., true>,
// finish_tracer_cell<., true>, seed_lower_bound), beside the always-loading form, and the bound itself on arrays of operands
// (tests/test_seed_bound.py).  The whole of xsweep_pressure_emu.cpp (and with it awfl_emu.cpp) is part of this translation unit.
// TEST INFRASTRUCTURE ONLY.
#include <vector>

namespace pama { struct Params; }
// every (cell, lane) that passes the comparison in finish_tracer_cell<., true> reports here: did the lane ask for the seed?
static void seed_skip_note(const pama::Params &P, int t, int k, int j, int i, int e, bool open);
#define PAMA_SEED_SKIP_NOTE(P, t, k, j, i, e, loaded) seed_skip_note(P, t, k, j, i, e, loaded)
#include "xsweep_pressure_emu.cpp"

// per row of water vapour (cell, block of 64 members -- what one wavefront of the device decides for): 0 not seen, 1 every lane so far
// skipped, 2 some lane asked for the seed (the wavefront loads)
static std::vector<unsigned char> g_rows;
static void seed_skip_note(const Params &P, int t, int k, int j, int i, int e, bool open) {
  if (t != P.idWV || g_rows.empty()) return;
  unsigned char &r = g_rows[(size_t)fct_row(P, k, j, i, e)];
  r = (open || r == 2) ? 2 : 1;
}

// awfl_xupd_kernel<STAGE, FOLD, PRESSURE, LAZY>: NT = 1, member lanes
template <int STAGE, bool LAZY>
static void xupd_seed_launch(Emu *h, const double *in, const double *p0, double *out, double dt, double dt_stage, bool pressure,
                             long long *counts) {
  const Params &P = h->P;
  const int span = h->span > 0 ? h->span : P.nx, nspan = (P.nx + span - 1) / span;
  std::vector<double> cells((size_t)XSTASH_CELLS * XSTASH_LANES);
  g_rows.assign((size_t)fct_rows_per_tracer(P), 0);
  for (int line = 0; line < P.nz * P.ny; line++)
    for (int sp = 0; sp < nspan; sp++)
      for (int e = 0; e < P.nens; e++) {
        double *fx = h->fx.data(), *fy = h->fy.data(), *fz = h->fz.data(), *sd = h->seed.data(), *mt = h->mult.data();
        if (pressure) {
          LineStash stash;
          stash.slot = cells.data() + (e & (XSTASH_LANES - 1));
          for (int n = 0; n < XSTASH_CELLS; n++) stash.slot[n * XSTASH_LANES] = NAN;
          if (P.yz_fold) flux_x_update_body<STAGE, true, LineStash, LAZY>(P, in, p0, out, fx, fy, fz, sd, mt, fct_rows(h), line, e, sp * span, span, dt, dt_stage, false, stash);
          else flux_x_update_body<STAGE, false, LineStash, LAZY>(P, in, p0, out, fx, fy, fz, sd, mt, fct_rows(h), line, e, sp * span, span, dt, dt_stage, false, stash);
        } else {
          if (P.yz_fold) flux_x_update_body<STAGE, true, NoStash, LAZY>(P, in, p0, out, fx, fy, fz, sd, mt, fct_rows(h), line, e, sp * span, span, dt, dt_stage, false);
          else flux_x_update_body<STAGE, false, NoStash, LAZY>(P, in, p0, out, fx, fy, fz, sd, mt, fct_rows(h), line, e, sp * span, span, dt, dt_stage, false);
        }
      }
  if (counts)
    for (unsigned char r : g_rows)
      if (r) counts[2 * (STAGE - 1) + (r == 2 ? 1 : 0)]++;
  g_rows.clear();
  poison_unflagged_mult(h);
}
template <int STAGE>
static void stage_seed(Emu *h, const double *in, const double *p0, double *out, double dt, double dt_stage, bool lazy, bool pressure,
                       long long *counts) {
  h->fct_seq++;
  flux_launch(h, in, 6, true);
  if (lazy) xupd_seed_launch<STAGE, true>(h, in, p0, out, dt, dt_stage, pressure, counts);
  else xupd_seed_launch<STAGE, false>(h, in, p0, out, dt, dt_stage, pressure, counts);
  if (pressure) fixup_launch<STAGE>(h, in, p0, out, dt);
  else tail_launch<STAGE>(h, in, p0, out, dt);
}

extern "C" {

// emu_time_step's fused stage (NT = 1, member lanes) with the seed always loaded (lazy 0) or only where it can matter (lazy 1), with the
// pressure pass of its own (pressure 0) or inside the sweep (1).  counts[2 (stage - 1) + p] += the rows of water vapour whose
// wavefront took the skip (p = 0) or the load (p = 1) in that stage (lazy 1 only).  -1 where the device does not run these kernels.
int emu_time_step_seed_skip(Emu *h, double *rho_d, double *u, double *v, double *w, double *T, double *tracers, double crm_dt,
                            double dt_hint, double *dt_out, int lazy, int pressure, long long *counts) {
  const Params &P = h->P;
  const int span = h->span > 0 ? h->span : P.nx;
  if (!h->fused || h->flat || h->xtile || P.nt != 1) return -1;
  if (pressure && (span < P.nx ? span : P.nx) > XSTASH_CELLS) return -1;
  emu_convert_coupler_to_dynamics(h, rho_d, u, v, w, T, tracers);
  double dt = dt_hint > 0 ? dt_hint : emu_compute_time_step(h, rho_d, u, v, w, T, tracers, 0.8);
  const int ncycles = (int)std::ceil(crm_dt / dt);
  dt = crm_dt / ncycles;
  if (dt_out) *dt_out = dt;
  double *A = h->prim0.data(), *B = h->prim1.data(), *C = h->prim2.data();
  for (int ic = 0; ic < ncycles; ic++) {
    std::fill(h->fx.begin(), h->fx.begin() + 5 * P.ncell, NAN);
    stage_seed<1>(h, A, A, B, dt, dt, lazy, pressure, counts);
    stage_seed<2>(h, B, A, C, dt, (1.0 / 4.0) * dt, lazy, pressure, counts);
    stage_seed<3>(h, C, A, B, dt, (2.0 / 3.0) * dt, lazy, pressure, counts);
    std::swap(A, B);
  }
  if (A != h->prim0.data()) h->prim0.swap(h->prim1);
  TracerPtrs tp = tptrs(h, tracers);
  for (long long idx = 0; idx < P.ncell; idx++) finalize_body(P, h->prim0.data(), h->seed.data(), rho_d, u, v, w, T, tp, cell_of(P, idx));
  return ncycles;
}

// the row flags, the "any" words and the line flags of the FCT multiplier as the last stage left them (out == nullptr: their number)
long long emu_fct_flags(Emu *h, int *out) {
  if (out) std::memcpy(out, h->fct_flags.data(), h->fct_flags.size() * sizeof(int));
  return (long long)h->fct_flags.size();
}

// The bound on n operand triples, producer and consumer with the library's own functions.
//   stage 1   a = the conserved mass before its clipping, b = the density the producer divides by.  Producer (init_prim_body, and every
//             stage-3 update through store_adv / store_adv_u): S = fmax(0, a), q = S * fast_rcp(b).  Consumer: m_in = mul_rn(q, b).
//   stage 2   a = q_0, b = rho_0, c = stage 1's new mass before its clipping.  Producer: next_seed<1>(., mul_rn(a, b), fmax(0, c)).
//   stage 3   the same with next_seed<2>(mul_rn(a, b), ., fmax(0, c)).
// seed: what the producer stores; low: seed_lower_bound as the consumer forms it; av_low / av_seed: fct_mass_available of the two.
void emu_seed_bound(int stage, long long n, const double *a, const double *b, const double *c, double dx, double dy, double dzk,
                    double *seed, double *low, double *av_low, double *av_seed) {
  Params P;
  std::memset(&P, 0, sizeof(P));
  P.dx = dx; P.dy = dy;
  for (long long i = 0; i < n; i++) {
    if (stage == 1) {
      const double S = fmax(0.0, a[i]), q = S * fast_rcp(b[i]);
      seed[i] = next_seed<3>(0.0, 0.0, S);
      low[i] = seed_lower_bound<1>(0.0, mul_rn(q, b[i]), q, b[i]);
    } else {
      const double m_0 = mul_rn(a[i], b[i]), v = fmax(0.0, c[i]);
      seed[i] = (stage == 2) ? next_seed<1>(0.0, m_0, v) : next_seed<2>(m_0, 0.0, v);
      low[i] = (stage == 2) ? seed_lower_bound<2>(m_0, 0.0, 0.0, 0.0) : seed_lower_bound<3>(m_0, 0.0, 0.0, 0.0);
    }
    av_low[i] = fct_mass_available(P, low[i], dzk);
    av_seed[i] = fct_mass_available(P, seed[i], dzk);
  }
}

}  // extern "C"
