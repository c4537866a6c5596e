"""compute_gcm_forcing_tendencies / apply_gcm_forcing_tendencies cell by cell, on every species (tests/gcm_forcing_cases.py has the
states, the per-level scale and the gate).

Without a GPU: what the named cases reach (every hole-filling bit at every member count, several species in the fallback in one call,
the number clamps, a level with nothing to pay with), the oracle's floor on them, that the per-level gate bites where the max-norm it
joins does not, that a member of a mixed ensemble is bit for bit the member run alone, and the hazard the module inherits from the
reference: a member without liquid in a call whose liquid fallback runs ends in 0/0.

On the GPU (-m gpu): every named case with the device read back and gated after each application, run-to-run determinism, the
device's fields on member shards against the whole call, and the hazard as the oracle has it."""
import copy
import re

import numpy as np
import pytest

import gcm_forcing_cases as gc

MIXED_70 = "n70_6x3x9_mixed"


def _union(run):
    u = 0
    for m in gc.masks(run):
        u |= m
    return u


# ---- without a GPU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", gc.NAMED_IDS)
def test_census_case_does_what_its_scenarios_declare(name):
    _, (nens, nx, ny, nz), _, scenarios = gc.BY_NAME[name]
    assert nens * nx * ny * nz < 25000
    ref = gc.reference(name)
    run, crm = ref["run"], ref["crm"]
    assert _union(run) == gc.declared_mask(scenarios, nx * ny), [bin(m) for m in gc.masks(run)]
    for s in run["steps"]:
        assert all(np.isfinite(v).all() for v in s["crm"].values()) and all(np.isfinite(v).all() for v in s["tend"].values())
        assert all(s["crm"][n].min() >= 0.0 for n in gc.WATER + gc.NUM)
    if nx * ny > 1:
        # gap 2: cloud-free (ice-free) cells beside cloudy ones -- the level pass runs on the FIRST application, whatever the scenario
        for w in ("cloud_water", "ice"):
            lev = (crm[w] == 0.0).any(axis=(1, 2)) & (crm[w] > 0.0).any(axis=(1, 2))
            assert lev.any(), w
        assert run["steps"][0]["mask"] & 0b110 == 0b110
    if "numclamp" in scenarios:
        out = run["steps"][-1]["crm"]
        for n in gc.NUM:
            assert ((out[n] == 0.0) & (crm[n] > 0.0)).any(), n


def _levels_with_nothing_to_pay(name):
    """(species, application) pairs in which the level pass ran with a level whose positive mass was exactly zero -- the `p > 0` false
    branch.  Certain when every cell of the level is zero afterwards and either was zero before (0 + t <= 0 in every cell: a positive t
    would have left them positive) or is the level's only cell (it went negative and was clamped)."""
    ref = gc.reference(name)
    ncol = ref["crm"]["temp"].shape[1] * ref["crm"]["temp"].shape[2]
    found, before = [], ref["crm"]
    for a, s in enumerate(ref["run"]["steps"]):
        for sp, w in enumerate(gc.WATER):
            empty = (s["crm"][w] == 0.0).all(axis=(1, 2)) & ((before[w] == 0.0).all(axis=(1, 2)) | (ncol == 1))
            if (s["mask"] >> sp) & 1 and empty.any():
                found.append((sp, a))
        before = s["crm"]
    return found


def test_census_named_cases_cover_every_bit_at_every_member_count():
    by_nens = {}
    two_in_fallback, nothing_to_pay = [], []
    for name, (nens, _, _, _), _, _ in gc.NAMED:
        run = gc.reference(name)["run"]
        by_nens[nens] = by_nens.get(nens, 0) | _union(run)
        if any(bin(m >> 4).count("1") >= 2 for m in gc.masks(run)):
            two_in_fallback.append(name)
        if _levels_with_nothing_to_pay(name):
            nothing_to_pay.append(name)
    assert sorted(by_nens) == sorted(sh[0] for sh in gc.SHAPES)
    for nens, u in by_nens.items():
        assert u == 0b1110111, (nens, bin(u))
    assert two_in_fallback and nothing_to_pay
    # ny*nx of every named shape against the slot counts of the two kernels (8 in compute, 16 in apply)
    assert sorted({sh[1] * sh[2] for sh in gc.SHAPES}) == [1, 5, 6, 7, 18, 25]


@pytest.mark.parametrize("name", gc.NAMED_IDS)
def test_oracle_floor_is_small_and_noise_moves_no_decision(name):
    """the twins leave every mask and every zero set as it was, and move no field or tendency by more than FLOOR_MAX in the gate's
    units: 4 x floor stays at or below the 1e-12 bar, so the gate derived per case is that bar"""
    ref = gc.reference(name)
    assert not ref["problems"], ref["problems"]
    assert set(ref["floor"]) == set(gc.CRM) | set(gc.TEND)
    for k, f in ref["floor"].items():
        assert f <= gc.FLOOR_MAX, (k, f)
        assert ref["tol"][k] == max(4.0 * f, 1e-12) <= gc.TOL_CAP


def test_per_level_gate_bites_where_the_max_norm_does_not():
    """one water cell of the level with the smallest scale, and one qv tendency, off by 1e-9 of themselves"""
    ref = gc.reference(MIXED_70)
    exp, crm, gcm, tol = ref["run"], ref["crm"], ref["gcm"], ref["tol"]
    gc.gate(copy.deepcopy(exp), exp, crm, gcm, tol)
    last = exp["steps"][-1]["crm"]
    S = gc.field_scale(crm, gcm, last)
    for w in gc.WATER:
        held = gc.level_max(last[w])
        cand = np.where(held >= 0.5 * S[w], S[w], np.inf)          # levels whose largest cell is of the level's scale
        k, e = np.unravel_index(np.argmin(cand), cand.shape)
        j, i = np.unravel_index(np.argmax(last[w][k, :, :, e]), last[w].shape[1:3])
        assert S[w][k, e] < 1e-3 * np.abs(last[w]).max()
        bad = copy.deepcopy(exp)
        bad["steps"][-1]["crm"][w][k, j, i, e] *= 1.0 + 1e-9
        err = np.abs(bad["steps"][-1]["crm"][w] - last[w]).max()
        assert 0 < err <= 1e-12 * np.abs(last[w]).max()             # the max-norm gate of tests/test_modules.py passes it
        with pytest.raises(AssertionError, match="'%s', [0-9.e-]+, %s" % (w, re.escape(repr(tol[w])))):
            gc.gate(bad, exp, crm, gcm, tol)
    n = gc.T + "qv"
    sc = gc.computed_scale(crm, gcm)[n]
    k, e = np.unravel_index(np.argmax(np.abs(exp["computed"][n]) / sc), sc.shape)
    bad = copy.deepcopy(exp)
    bad["computed"][n][k, e] *= 1.0 + 1e-9
    err = np.abs(bad["computed"][n] - exp["computed"][n]).max()
    assert 0 < err <= 1e-14 * max(np.abs(g).max() for g in gcm.values()) / gc.DT_GCM      # the bound of tests/test_modules.py
    with pytest.raises(AssertionError, match="'%s', [0-9.e-]+, %s" % (n, re.escape(repr(tol[n])))):
        gc.gate(bad, exp, crm, gcm, tol)


@pytest.mark.parametrize("name", ["n10_3x2x6_mixed", "n65_7x1x8_mixed"])
def test_member_of_a_mixed_ensemble_equals_the_member_run_alone(name):
    """the fallback decision is one flag over the whole call, and the fallback then runs on every member -- with nothing to remove
    where a member needed none.  So a member's bits do not depend on who else is in the call, though its own masks do
    (tests/test_member_chunks_premise.py pins the same for chunks that share their masks)"""
    ref = gc.reference(name)
    whole = ref["run"]
    differ = 0
    for e in range(ref["crm"]["temp"].shape[-1]):
        crm, gcm, dz = gc.members(ref["crm"], ref["gcm"], gc.grid_dz(ref["dz"]), e, e + 1)
        alone = gc.run_oracle(crm, gcm, dz)
        assert gc.same_bits(alone, gc.run_members(whole, e, e + 1), with_masks=False) is None, e
        differ += gc.masks(alone) != gc.masks(whole)
    assert differ >= 5


def _hazard():
    crm, gcm, dz = gc.hazard_state()
    return crm, gcm, dz, gc.run_oracle(crm, gcm, gc.grid_dz(dz))


def _nonfinite(run):
    """where a run is not finite: per application and array, the boolean map"""
    return [{n: ~np.isfinite(v) for grp in ("crm", "tend") for n, v in s[grp].items()} for s in run["steps"]]


def test_inherited_hazard_clear_sky_member_beside_a_liquid_fallback():
    """Parity with the reference is the contract, so this pins the reference's arithmetic and changes nothing: the clear-sky member
    gets 0 dz / 0 in the liquid fallback another member triggered, and run alone it stays finite."""
    crm, gcm, dz, whole = _hazard()
    assert not crm["cloud_water"][..., 0].any() and not gcm["gcm_cloud_water"][:, 0].any()
    first = [a for a, m in enumerate(gc.masks(whole)) if m & 32]
    assert first, gc.masks(whole)
    for a, bad in enumerate(_nonfinite(whole)):
        for n, b in bad.items():
            if a >= first[0] and n == "cloud_water":
                assert b[..., 0].all() and not b[..., 1:].any()
            elif a >= first[0] and n == gc.T + "rho_l":
                assert not b[:, 1:].any()                       # diagnosed before the fill: member 0's turns one application later
                assert b[:, 0].all() if a > first[0] else not b[:, 0].any()
            else:
                assert not b.any(), (a, n)
    alone = gc.run_oracle(*gc.members(crm, gcm, gc.grid_dz(dz), 0, 1))
    assert not any(b.any() for step in _nonfinite(alone) for b in step.values())
    assert all(m & 32 == 0 for m in gc.masks(alone))
    # the other members do not notice: they are what they are without member 0 in the call
    rest = gc.run_oracle(*gc.members(crm, gcm, gc.grid_dz(dz), 1, 12))
    assert gc.same_bits(rest, gc.run_members(whole, 1, 12)) is None


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------

def _device_run(crm, gcm, dz):
    """compute, then NAPP applications in a fresh coupler, everything read back after each: a run as gc.run_oracle returns it"""
    import torch
    import test_modules as tm
    from pam_amd import modules
    coupler, dm, zint = tm._gcm_gpu_coupler(crm, gcm, dz, gc.DT_GCM, gc.CRM_DT)
    assert np.array_equal(dm.get("vertical_cell_dz", readonly=True).cpu().numpy(), gc.grid_dz(dz))
    coupler.run_module("compute_gcm_forcing_tendencies", modules.compute_gcm_forcing_tendencies)
    run = dict(computed={n: dm.get(n, readonly=True).cpu().numpy() for n in gc.COMPUTED}, steps=[])
    for _ in range(gc.NAPP):
        out = {}
        coupler.run_module("apply_gcm_forcing_tendencies", lambda c: out.setdefault("m", modules.apply_gcm_forcing_tendencies(c)))
        torch.cuda.synchronize()
        run["steps"].append(dict(crm={n: dm.get(n, readonly=True).cpu().numpy() for n in gc.CRM},
                                 tend={n: dm.get(n, readonly=True).cpu().numpy() for n in gc.DIAGNOSED}, mask=out["m"]))
    for n in gc.COMPUTED:      # apply leaves the computed tendencies alone
        assert np.array_equal(run["computed"][n], dm.get(n, readonly=True).cpu().numpy()), n
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("name", gc.NAMED_IDS)
def test_gpu_gcm_forcing_named_case_matches_oracle_after_every_application(name):
    ref = gc.reference(name)
    got = _device_run(ref["crm"], ref["gcm"], ref["dz"])
    worst = gc.gate(got, ref["run"], ref["crm"], ref["gcm"], ref["tol"], what=name, case="gcm_forcing/" + name, floor=ref["floor"])
    print(name, "masks", gc.masks(got), "worst/gate", max(worst[k] / ref["tol"][k] for k in worst), max(worst, key=worst.get))


@pytest.mark.gpu
def test_gpu_gcm_forcing_is_deterministic_run_to_run():
    """the only atomics of the path are the atomicOr of the flags: two fresh couplers give the same bits"""
    ref = gc.reference("n130_5x5x7_mixed")
    a = _device_run(ref["crm"], ref["gcm"], ref["dz"])
    b = _device_run(ref["crm"], ref["gcm"], ref["dz"])
    assert gc.same_bits(a, b) is None


@pytest.mark.gpu
def test_gpu_gcm_forcing_member_shards_equal_the_whole_call():
    """the sharding contract (README, "Multi-GPU") where the shards' masks differ from the whole call's and from each other's"""
    ref = gc.reference(MIXED_70)
    whole = _device_run(ref["crm"], ref["gcm"], ref["dz"])
    differ = 0
    for lo, hi in ((0, 5), (5, 64), (64, 70)):
        crm, gcm, dz = gc.members(ref["crm"], ref["gcm"], ref["dz"], lo, hi)
        part = _device_run(crm, gcm, dz)
        assert gc.same_bits(part, gc.run_members(whole, lo, hi), with_masks=False) is None, (lo, hi)
        assert gc.masks(part) == gc.masks(gc.run_oracle(crm, gcm, gc.grid_dz(dz))), (lo, hi)
        differ += gc.masks(part) != gc.masks(whole)
    assert differ >= 1


@pytest.mark.gpu
def test_gpu_gcm_forcing_inherited_hazard_is_the_oracles():
    """a NaN in a field is no fault of the device: the clear-sky member's non-finite cells are the oracle's, and every other member
    passes the gate"""
    crm, gcm, dz, exp = _hazard()
    got = _device_run(crm, gcm, dz)
    assert gc.masks(got) == gc.masks(exp)
    for a, (bg, be) in enumerate(zip(_nonfinite(got), _nonfinite(exp))):
        for n in be:
            assert np.array_equal(bg[n], be[n]), (a, n)
    assert any(b.any() for step in _nonfinite(exp) for b in step.values())
    sub = gc.members(crm, gcm, dz, 1, 12)
    base = gc.run_members(exp, 1, 12)
    floor, problems = gc.oracle_floor(sub[0], sub[1], gc.grid_dz(sub[2]), base)
    assert not problems and max(floor.values()) <= gc.FLOOR_MAX
    gc.gate(gc.run_members(got, 1, 12), base, sub[0], sub[1], gc.tolerances(floor), what="hazard", case="gcm_forcing/hazard_members_1_11",
            floor=floor)
