"""The GCM-coupled CRM loop on the CPU, no device (tests/mmf_loop_ref.py is the chain and its schedule): the chain run through the emulated
device bodies against the chain of the numpy restatements, bit for bit after every call; every scheme of every stack acts on the seeded
state; ten broken contracts each leave the gate of the free-running GPU comparison in a quantity the test names; and the conditions of
that gate, on the reference alone, for every stack."""
import numpy as np
import pytest

import mmf_loop_ref as mmf
from parity_gate import FLOOR_K, TOL_TIGHT, is_tight

STACK_NAMES = tuple(mmf.STACKS)
_RUNS = {}


def _traced(name):
    """the chain's run of a stack with the state after every call, once per stack and shared"""
    if name not in _RUNS:
        k = mmf.stack(name)
        trace = []
        B, log = mmf.chain(k, trace=trace)
        _RUNS[name] = (k, B, log, trace)
    return _RUNS[name]


def _emulated_kernels():
    """the g++-built device bodies behind the interface of the restatements.  Without a harness, and so left on numpy or the oracle in
    both chains: the forced radiation, the time and horizontal averages, the saturation adjustment and the surface friction as modules
    (their restatements are scalar loops of the same arithmetic), the dycore, the sponge layer, Kessler and the GCM forcing"""
    import p3_cases as pc
    import shoc_cases as sc
    from coldiag_emu_harness import EmuBackend as Coldiag
    from fluxprof_emu_harness import EmuBackend as Fluxprof
    from msa_emu_harness import EmuBackend as Msa
    from rad_emu_harness import BLOCK_SLOTS, THREAD_SLOTS, EmuBackend as Rad
    from sgs_emu_harness import EmuBackend as Sgs
    from vt_emu_harness import EmuBackend as Vt

    def p3(st, q, k, adjust, first_step, consts):
        state = dict(st, q=q, zint=k.zint)
        assert all(consts[n] == pc.ref.CONSTS[n] for n in pc.ref.CONSTS)
        out = pc.emulated(state, k.layout, adjust, first_step, num_tend_out=k.num_tend_out)[2]
        return out, [out["q%d" % t] for t in range(7)]

    def shoc(st, q, fu, fv, k, consts):
        state = dict(st, q=q, flx_u=fu, flx_v=fv, zint=k.zint, zmid=k.zmid)
        keep = sc.XLEN, sc.YLEN                      # shoc_cases.emulated reads the domain of its own cases from the module
        sc.XLEN, sc.YLEN = k.xlen, k.ylen
        try:
            _, _, out, qn = sc.emulated(state, k.layout, consts=consts)
        finally:
            sc.XLEN, sc.YLEN = keep
        return out, qn
    return dict(msa=Msa(), vt=Vt(), rad=Rad(THREAD_SLOTS), rad_feedback=Rad(BLOCK_SLOTS), coldiag=Coldiag(), fluxprof=Fluxprof(), sgs=Sgs(),
                p3=p3, shoc=shoc)


@pytest.mark.parametrize("name", ["mmf3d_p3shoc", "mmf2d_kessler"])
def test_chain_through_the_emulated_bodies_equals_the_numpy_chain_bit_for_bit(name):
    """every call of both GCM steps, the inits and the end-of-step calls included: each entry the DataManager would hold has the same bits in
    both chains.  mmf3d_p3shoc runs the P3 and SHOC coupling layers in layout 1; mmf2d_kessler the dry Smagorinsky closure and the
    single-condensate rows of every module"""
    k, _, log_w, want = _traced(name)
    got = []
    _, log = mmf.chain(k, trace=got, kernels=_emulated_kernels())
    assert log == log_w
    assert len(got) == len(want)
    for i, ((g, call, _, a), (g_w, call_w, _, b)) in enumerate(zip(got, want)):
        assert (g, call) == (g_w, call_w)
        bad = [n for n in b if not mmf.same_bits(np.ascontiguousarray(a[n]), np.ascontiguousarray(b[n]))]
        assert bad == [], (i, g, call, bad)
    print("%s: %d calls, %d entries at the end, all bits equal" % (name, len(want), len(want[-1][3])))


@pytest.mark.parametrize("name", STACK_NAMES)
def test_every_scheme_acts(name):
    """on the seeded state no part of the stack idles: the cease flag rose and fell and the weights are those of mmf_loop_ref.WEIGHTS;
    a hole-filling bit of the GCM-forcing mask is set; a VT scale sits at each clamp and strictly between; every aggregate, diagnostic and
    profile the stack's microphysics has was zero after its init and is non-zero at the end of each GCM step, and those it lacks are
    absent; t_prev == temp and q_prev == water_vapor after every P3 step, and P3's etime counts the CRM steps of both GCM steps; and every
    temperature tendency msa_accelerate saw lies a factor of ten or more from its crm_accel_max_ttend"""
    k, B, log, trace = _traced(name)
    assert tuple(tuple(w) for w in log["weights"]) == mmf.WEIGHTS[name]
    for g in range(k.gcm_steps):
        ceased = mmf.CEASED[name][g]
        assert any(log["cease"][g]) == ceased and log["flag"][g][-1] == ceased
        if ceased:      # the first accelerated step ceased, the flag stayed up, and no later step called msa_accelerate
            assert log["cease"][g][0] and all(log["flag"][g]) and not any(log["cease"][g][1:])
    rose = [S["accel_ceaseflag"][0] for g, call, _, S in trace if call in ("msa_init", "msa_accelerate")]
    if any(mmf.CEASED[name]):
        assert 1 in rose and rose[-1] == 0 and rose[rose.index(1):].count(0) > 0        # up in GCM step 0, down again at msa_init
    else:
        assert not any(rose)
    for g, worst, limit in B.log["max_ttend"]:
        assert worst >= 10 * limit or 10 * worst <= limit, (g, worst, limit)
    if k.forcing:
        masks = [m for per_step in log["masks"] for m in per_step]
        assert any(m & 0x7 for m in masks), masks
    else:
        assert log["masks"] == [[], []] and not any(n.startswith("gcm_forcing_tend_") for n in B.S)
    scales = np.concatenate([s[x].ravel() for s in B.log["vt_scale"] for x in s])
    lo, hi = 1.0 - mmf.VT_LIMIT, 1.0 + mmf.VT_LIMIT
    assert (scales == lo).any() and (scales == hi).any() and ((scales > lo) & (scales < hi) & (scales != 1.0)).any()
    accumulated = mmf.rad_names(k) + mmf.diag_names(k) + mmf.prof_names(k) + mmf.time_average_entries(k)
    inits = {"rad_aggregate_init": mmf.rad_names(k), "column_diagnostics_init": mmf.diag_names(k), "flux_profiles_init": mmf.prof_names(k),
             "time_average_init": mmf.time_average_entries(k)}
    seen = 0
    for g, call, _, S in trace:
        if call in inits:
            assert all(not S[n].any() for n in inits[call]), (g, call)
            seen += 1
        if call == "horizontal_average":
            idle = [n for n in accumulated + mmf.feedback_names(k) + mmf.vt_names(k, "feedback") if not S[n].any()]
            assert idle == [], (g, idle)
    assert seen == 4 * k.gcm_steps
    if k.micro == "kessler":
        assert not any(n in B.S for n in ("rad_qi", "crm_feedback_mean_qi", "crm_feedback_tend_qi", "diag_iwp", "diag_precip_ice", "cldfrac"))
        assert B.S["precl"].max() > 0 and B.S["diag_precip_liq"].max() > 0
    else:
        assert B.log["p3_prev_equal"] and all(B.log["p3_prev_equal"])
        steps = sum(len(w) for w in log["weights"])
        assert B.p3_etime == steps * k.dt and not B.p3_first
        assert ("cldfrac" in B.S) == k.shoc
    cloud = B.S[k.cloud] > 0
    assert cloud.any() and (B.S["precip_liquid" if k.micro == "kessler" else "rain"][0] > 0).any()      # rain in the lowest level
    print(name, log, B.log["max_ttend"])


# the stack each mutant runs on, and the quantity that must leave its gate (the docstring of the test lists the measured factors)
MUTANT_STACK = {m: "mmf3d_p3shoc" for m in mmf.MUTANTS}
MUTANT_STACK["msa_init_skipped"] = "mmf3d_members"
MUTANT_CAUGHT_BY = {"rad_aggregate_weight_one": "rad_temperature", "vt_forcing_unweighted": "vt_var_u", "gcm_forcing_after_dycore": "wvel",
                    "msa_diagnose_after_gcm_forcing": "uvel", "msa_init_skipped": "temp", "vt_init_skipped": "vt_feedback_t",
                    "rad_aggregate_init_skipped": "rad_temperature", "condensate_swapped": "rad_qc", "ice_num_adds_mass": "uvel",
                    "p3_adjusts_beside_shoc": "cloud_water"}


@pytest.mark.parametrize("mutant", mmf.MUTANTS)
def test_gate_sees_a_broken_contract(mutant):
    """each mutant of the chain (mmf_loop_ref.drive and Chain) differs from the chain by more than the free-running gate in the quantity
    MUTANT_CAUGHT_BY names.  Measured (seed 0), worst / gate of that quantity:

      rad_aggregate_weight_one        mmf3d_p3shoc   rad_temperature  0.667    / 1e-12    = 6.7e11  (a third of the GCM step is missing)
      vt_forcing_unweighted           mmf3d_p3shoc   vt_var_u         0.075    / 1e-12    = 7.5e10
      gcm_forcing_after_dycore        mmf3d_p3shoc   wvel             0.044    / 1.3e-12  = 3.3e10
      msa_diagnose_after_gcm_forcing  mmf3d_p3shoc   uvel             0.071    / 1e-12    = 7.1e10
      msa_init_skipped                mmf3d_members  temp             1.1e-3   / 1e-12    = 1.1e9   (GCM step 1 stays ceased: 4 steps of weight 1)
      vt_init_skipped                 mmf3d_p3shoc   vt_feedback_t    1.0      / 1.1e-12  = 8.9e11  (against the variances GCM step 0 began with)
      rad_aggregate_init_skipped      mmf3d_p3shoc   rad_temperature  0.993    / 1e-12    = 9.9e11  (twice the aggregate)
      condensate_swapped              mmf3d_p3shoc   rad_qc           0.948    / 1e-12    = 9.5e11
      ice_num_adds_mass               mmf3d_p3shoc   uvel             3.24     / 1e-12    = 3.2e12  (the dycore's total density)
      p3_adjusts_beside_shoc          mmf3d_p3shoc   cloud_water      0.587    / 1e-12    = 5.9e11"""
    k = mmf.stack(MUTANT_STACK[mutant])
    base, held, floor, _, _ = mmf.floors(k)
    gate = mmf.gates(k, base, floor)
    B, _ = mmf.chain(k, mutant)
    worst = mmf.errors(k, mmf.to_fields(k, B.S), B.S, base, held)
    n = MUTANT_CAUGHT_BY[mutant]
    beyond = {q: worst[q] / gate[q] for q in worst if gate[q] > 0 and worst[q] > gate[q]}
    print("%s: %s %.3g / %.3g = %.3g; beyond the gate: %d of %d" % (mutant, n, worst[n], gate[n], worst[n] / gate[n], len(beyond), len(worst)))
    assert worst[n] > gate[n], (n, worst[n], gate[n], sorted(beyond, key=beyond.get)[-5:])


@pytest.mark.parametrize("name", STACK_NAMES)
def test_conditions_of_the_free_running_gate_hold_on_the_reference(name):
    """parity_gate.noise_floor through the whole chain (three twins with one ulp of noise in temp): rho_d, temp and the vapour of the twins
    stay within TOL_TIGHT / 10; for every other compared quantity FLOOR_K x floor stays at or below a tenth of its cap (1e-8 for the
    winds and the tracers other than vapour, 1e-10 for the GCM-step outputs), so the cap is never what passes a case; and the
    count-like outputs (rad_cld, the four diag_cld*, prof_cld, the conditional mass fluxes) change by a count, not by rounding, so the
    twins must take the same weights, cease decisions and hole-filling masks, and the same classification in every cell of every CRM
    step: the cloud fraction of the aggregate, cloudy and upward of the mass fluxes, the pressure class, and the water path beyond its
    threshold"""
    k = mmf.stack(name)
    base, held, floor, logs, _ = mmf.floors(k)
    print(name, k.shape, {n: float("%.2g" % v) for n, v in floor.items()})
    for twin in logs[1:]:
        for what in ("weights", "cease", "flag", "masks"):
            assert twin[what] == logs[0][what], what
        assert len(twin["classes"]) == len(logs[0]["classes"])
        for step, (a, b) in enumerate(zip(twin["classes"], logs[0]["classes"])):
            differ = [n for n in b if not np.array_equal(a[n], b[n])]
            assert differ == [], (step, differ)
    for n, v in floor.items():
        if is_tight(n):
            assert v <= TOL_TIGHT / 10, (n, v)
        else:
            cap = mmf.CAP_COLUMN if n in mmf.outputs(k) else mmf.CAP_NOISE
            assert FLOOR_K * v <= cap / 10, (n, v, cap)
    assert set(mmf.outputs(k)) <= set(floor) and set(k.names) <= set(floor)
