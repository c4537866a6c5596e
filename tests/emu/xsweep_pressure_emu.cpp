// Host emulation of the fused stage with the pressure pass INSIDE the x-sweep (flux_x_update_body<., ., LineStash>; NT = 1, member
// lanes, spans of at most XSTASH_CELLS cells), beside the emulation of the separate pass that awfl_emu.cpp holds: the whole of
// awfl_emu.cpp is part of this translation unit, so one library runs both forms of the stage on the same handle type
// (tests/test_xsweep_pressure_emu.py).  TEST INFRASTRUCTURE ONLY.
#include "awfl_emu.cpp"

// awfl_xupd_kernel<STAGE, FOLD, true>: a wavefront's stash is XSTASH_CELLS x XSTASH_LANES doubles; a lane's slots are poisoned before
// its sweep (it may read only what it wrote in this sweep)
template <int STAGE>
static void xupd_pressure_launch(Emu *h, const double *in, const double *p0, double *out, double dt, double dt_stage) {
  const Params &P = h->P;
  const int span = h->span > 0 ? h->span : P.nx, nspan = (P.nx + span - 1) / span;
  std::vector<double> cells((size_t)XSTASH_CELLS * XSTASH_LANES);
  for (int line = 0; line < P.nz * P.ny; line++)
    for (int sp = 0; sp < nspan; sp++)
      for (int e = 0; e < P.nens; e++) {
        LineStash stash;
        stash.slot = cells.data() + (e & (XSTASH_LANES - 1));
        for (int n = 0; n < XSTASH_CELLS; n++) stash.slot[n * XSTASH_LANES] = NAN;
        if (P.yz_fold)
          flux_x_update_body<STAGE, true, LineStash>(P, in, p0, out, h->fx.data(), h->fy.data(), h->fz.data(), h->seed.data(), h->mult.data(),
                                                     fct_rows(h), line, e, sp * span, span, dt, dt_stage, false, stash);
        else
          flux_x_update_body<STAGE, false, LineStash>(P, in, p0, out, h->fx.data(), h->fy.data(), h->fz.data(), h->seed.data(), h->mult.data(),
                                                      fct_rows(h), line, e, sp * span, span, dt, dt_stage, false, stash);
      }
  poison_unflagged_mult(h);
}
// the tail that is left: water vapour's fix-up, one wavefront per (x line, member block) (awfl_trfix_kernel) -- no pressure pass
template <int STAGE>
static void fixup_launch(Emu *h, const double *in, const double *p0, double *out, double dt) {
  const Params &P = h->P;
  const FctRows rows = fct_rows(h);
  bool any = false;
  for (int b = 0; b < ((P.nens + 63) >> 6); b++) any = any || rows.any[b] == rows.seq;
  if (!any) return;
  for (int k = 0; k < P.nz; k++)
    for (int j = 0; j < P.ny; j++)
      for (int e = 0; e < P.nens; e++)
        tracer_fixup_line_body<STAGE>(P, in, p0, out, h->fx.data(), h->fy.data(), h->fz.data(), h->mult.data(), rows, h->seed.data(), dt, P.idWV, k, j, e);
}

extern "C" {

// emu_time_step's fused stage with the in-sweep pressure; -1 where the device keeps the separate pass (launch_xupd_sweeps)
int emu_time_step_xsweep_pressure(Emu *h, double *rho_d, double *u, double *v, double *w, double *T, double *tracers, double crm_dt,
                                  double dt_hint, double *dt_out) {
  const Params &P = h->P;
  const int span = h->span > 0 ? h->span : P.nx;
  if (!h->fused || h->flat || h->xtile || P.nt != 1 || (span < P.nx ? span : P.nx) > XSTASH_CELLS) return -1;
  emu_convert_coupler_to_dynamics(h, rho_d, u, v, w, T, tracers);
  double dt = dt_hint > 0 ? dt_hint : emu_compute_time_step(h, rho_d, u, v, w, T, tracers, 0.8);
  const int ncycles = (int)std::ceil(crm_dt / dt);
  dt = crm_dt / ncycles;
  if (dt_out) *dt_out = dt;
  double *A = h->prim0.data(), *B = h->prim1.data(), *C = h->prim2.data();
  for (int ic = 0; ic < ncycles; ic++) {
    std::fill(h->fx.begin(), h->fx.begin() + 5 * P.ncell, NAN);
    h->fct_seq++; flux_launch(h, A, 6, true); xupd_pressure_launch<1>(h, A, A, B, dt, dt); fixup_launch<1>(h, A, A, B, dt);
    h->fct_seq++; flux_launch(h, B, 6, true); xupd_pressure_launch<2>(h, B, A, C, dt, (1.0 / 4.0) * dt); fixup_launch<2>(h, B, A, C, dt);
    h->fct_seq++; flux_launch(h, C, 6, true); xupd_pressure_launch<3>(h, C, A, B, dt, (2.0 / 3.0) * dt); fixup_launch<3>(h, C, A, B, dt);
    std::swap(A, B);
  }
  if (A != h->prim0.data()) h->prim0.swap(h->prim1);
  TracerPtrs tp = tptrs(h, tracers);
  for (long long idx = 0; idx < P.ncell; idx++) finalize_body(P, h->prim0.data(), h->seed.data(), rho_d, u, v, w, T, tp, cell_of(P, idx));
  return ncycles;
}

}
