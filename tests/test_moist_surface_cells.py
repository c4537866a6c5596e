"""saturation_adjustment held to the bit and surface_friction_init / compute_surface_friction held per cell and per member
(tests/moist_surface_cases.py has the cases, the gates and the reasoning; tests/moist_surface_ref.py the float64 restatement and its
mutants).  The CPU tests establish what the GPU tests rest on: every branch is reached and no committed cell is near a tie, the host
emulation is the restatement bit for bit, the reference is right (40 digits) and the restatement within E of it, and every mutant is
rejected by the new gates -- those marked OLD_GATE_ACCEPTS passed the gate of 1e-12 of the field's largest value."""
import ctypes as C

import numpy as np
import pytest

import moist_surface_cases as mc
import moist_surface_ref as ref
from pam_amd import capi

LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: saturation adjustment

@pytest.mark.parametrize("name", mc.SATURATION_IDS)
def test_every_branch_is_reached_and_no_committed_cell_is_near_a_tie(name):
    """from the restatement alone: condensation, evaporation and untouched cells in every case, and the smallest relative decision
    margin of an adjusted cell >= 1e-10 -- two orders above MARGIN, so no cell of a GPU test is exempt from bit equality.  (Measured:
    5.2e-8, 3.3e-6, 1.1e-6 for the three kessler shapes, 3.2e-8, 5.7e-6, 1.9e-6 for p3, 3.0e-7 and 1.0e-7 for kessler_order and
    p3_order, 1.7e-10 for specials -- its vapour of 1e3 --, 5.4e-8 for each of massy_0, _1, _55.)"""
    d = mc.saturation_case(name)
    info = d["info"]
    adjusted = info["branch"] > 0
    assert set(np.unique(info["branch"])) == {0, 1, 2}
    smallest = float(info["margin"][adjusted].min())
    print("%s: %d of %d cells adjusted, smallest margin %.3g" % (name, adjusted.sum(), adjusted.size, smallest))
    assert smallest >= mc.MIN_MARGIN
    assert info["iters"][adjusted].min() >= 1 and not info["iters"][~adjusted].any()


def test_the_special_cells_are_what_their_names_say():
    d = mc.saturation_case("specials")
    info, before, want = d["info"], d["before"], d["want"]
    at = {what: i for i, what in d["special"].items()}
    wavefronts = {i // 64 for i in at.values()}
    assert len(wavefronts) == len(at)                                        # each among 63 ordinary cells
    untouched = ("nan_rho_v", "nan_rho_c_subsaturated", "nan_temp", "negative_zero_cloud_subsaturated", "negative_cloud_subsaturated",
                 "negative_vapour_without_cloud")
    for what in untouched:
        assert info["branch"][at[what]] == 0, what
    i = at["negative_zero_cloud_subsaturated"]
    assert np.signbit(want["rho_c"][i]) and want["rho_c"][i] == 0
    i = at["nan_rho_c_supersaturated"]
    assert info["branch"][i] == 1 and np.isnan(want["rho_c"][i]) and np.isnan(want["temp"][i]) and want["rho_v"][i] < before["rho_v"][i]
    assert want["rho_c"][at["negative_cloud_below_what_condenses"]] == 0.0     # max(0, rho_c + x) still clamps at the end
    assert info["branch"][at["negative_vapour_with_cloud"]] == 2
    # brackets at or below 2 tol: one iteration moves exactly half
    for what, field in (("evaporation_bracket_2tol", "rho_c"), ("evaporation_bracket_tol", "rho_c"), ("evaporation_bracket_1e-10", "rho_c"),
                        ("evaporation_bracket_1e-13", "rho_c"), ("condensation_bracket_tol_cold", "rho_v"),
                        ("condensation_bracket_2tol_cold", "rho_v")):
        i = at[what]
        assert info["iters"][i] == 1 and want[field][i] == before[field][i] / 2, what
    assert info["iters"][at["evaporation_bracket_above_2tol"]] == 2 and info["iters"][at["condensation_bracket_above_2tol_cold"]] == 2
    for what in ("vapour_1e3", "vapour_1e6", "vapour_1e9", "cloud_1e3", "cloud_1e6", "cloud_1e9"):
        assert 30 <= info["iters"][at[what]] <= 50, (what, info["iters"][at[what]])
    for what in ("inf_rho_v", "inf_rho_c"):
        assert info["iters"][at[what]] == ref.MAX_ITER and d["capped"][at[what]], what
    assert d["capped"].sum() == 2


@pytest.mark.parametrize("name", mc.SATURATION_IDS)
def test_the_emulation_is_the_restatement_bit_for_bit_on_saturation(name):
    """the device body under g++ against the Python restatement, specials included: every cell but the two that end at the iteration
    cap, where the restatement raises and the expected values ARE the emulation's"""
    d = mc.saturation_case(name)
    rv, rc, t, it = mc.emu_adjust(d["rho_d"], d["massy"], *[d["before"][k] for k in mc.ADJUSTED])
    for k, a in zip(mc.ADJUSTED, (rv, rc, t)):
        assert mc.same_bits(a, d["want"][k]), k
    assert np.array_equal(it, d["info"]["iters"])
    assert mc.assert_adjusted_bits(dict(zip(mc.ADJUSTED, (rv, rc, t))), d["want"], d["info"], d["before"]) == 0


def test_reversing_the_55_tracers_changes_the_temperature_bits():
    """the order of the sum rho = rho_d + tracers shows in the last place of rho and from there in temp: reversing the list changes the
    bits of temp in at least 1 % of the adjusted cells, so bit equality on the GPU proves the registration order"""
    d = mc.saturation_case("massy_55")
    got, _ = mc._restate_cells(d["rho_d"], d["massy"][::-1], *[d["before"][k] for k in mc.ADJUSTED])
    adjusted = d["info"]["branch"] > 0
    changed = mc.differing(got["temp"], d["want"]["temp"]) & adjusted
    print("massy_55 reversed: temp differs in %d of %d adjusted cells" % (changed.sum(), adjusted.sum()))
    assert changed.sum() >= 0.01 * adjusted.sum()
    assert d["massy"][17] is d["before"]["rho_v"] and d["massy"][41] is d["before"]["rho_c"] and len(d["massy"]) == 55


# the mutants the gate of 1e-12 of the field's largest value let through, on every case it can be applied to (specials holds infinite
# and absurd values, so its largest value says nothing)
SAT_OLD_GATE_ACCEPTS = ("rho_reversed", "cp_reassociated", "temp_fused", "skip_below_1e-9")
SAT_OLD_CASES = [n for n in mc.SATURATION_IDS if n != "specials"]


@pytest.mark.parametrize("mutant", ref.SATURATION_MUTANTS)
def test_the_bit_gate_rejects_every_saturation_mutant(mutant):
    """one deliberate error in the restatement at a time, against the committed cases.  skip_below_1e-9 (an adjustment of less than
    1e-9 is not written) reaches the 24 trace clouds of 1e-14 .. 4e-14 in massy_1, whose evaporation moves rho_c by at most 2e-14
    against the old tolerance of 3e-14, and the trace clouds of 1e-10 and 1e-13 in specials."""
    rejected, old_accepts = [], []
    for name in mc.SATURATION_IDS:
        d = mc.saturation_case(name)
        got = mc.saturation_mutant(name, mutant)
        try:
            mc.assert_adjusted_bits(got, d["want"], d["info"], d["before"])
        except AssertionError:
            rejected.append(name)
        if name in SAT_OLD_CASES:
            old_accepts.append(mc.old_gate_accepts(got, d["want"], d["info"]))
    print("%s: rejected on %s; the old gate accepts it on %d of %d cases" % (mutant, rejected, sum(old_accepts), len(old_accepts)))
    assert rejected, mutant
    if mutant == "rho_reversed":
        # a list of none or one has no order; massy_55 through the C ABI and the two _order states through the module are built to show it
        assert set(rejected) >= {"massy_55", "kessler_order", "p3_order"} and not {"massy_0", "massy_1"} & set(rejected)
    elif mutant == "skip_below_1e-9":
        assert rejected == ["specials", "massy_1"]               # the only cases with clouds below 2e-9
    else:
        assert set(rejected) >= {"kessler_ragged_nens_16cols", "p3_ragged_nens_16cols"}
    if mutant in SAT_OLD_GATE_ACCEPTS:
        assert all(old_accepts), mutant
    else:
        assert not all(old_accepts), mutant


def test_the_bit_gate_rejects_a_trace_cloud_left_unwritten_and_a_last_place():
    d = mc.saturation_case("kessler_ragged_nens_16cols")
    trace = np.flatnonzero((d["info"]["branch"] == 2) & (d["before"]["rho_c"] < 1e-6))
    assert trace.size
    for k, i, value in (("rho_c", trace[0], d["before"]["rho_c"][trace[0]]),
                        ("temp", trace[0], np.nextafter(d["want"]["temp"][trace[0]], 0.0))):
        got = {n: np.array(a) for n, a in d["want"].items()}
        got[k][i] = value
        with pytest.raises(AssertionError):
            mc.assert_adjusted_bits(got, d["want"], d["info"], d["before"])
    got = {n: np.array(a) for n, a in d["want"].items()}
    untouched = np.flatnonzero(d["info"]["branch"] == 0)[0]
    got["rho_c"][untouched] = -0.0 if not np.signbit(got["rho_c"][untouched]) else 0.0
    with pytest.raises(AssertionError):
        mc.assert_adjusted_bits(got, d["want"], d["info"], d["before"])


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: surface friction

def test_the_chunk_arithmetic_of_the_named_cases():
    """the three lines of pam_amd_surface_friction_compute that split the columns, restated (mc.chunks): the partial and the empty
    chunks of capped_chunks, the split of uneven_chunks"""
    shape = lambda n: mc.chunks(mc.FRICTION_BY_NAME[n].nens, mc.FRICTION_BY_NAME[n].nx * mc.FRICTION_BY_NAME[n].ny)
    assert shape("ragged") == (2, 1, 20) and shape("few_columns") == (1, 1, 6) and shape("one_member") == (1, 1, 6)
    assert shape("three_chunks") == (1, 3, 48)
    assert shape("uneven_chunks") == (1, 2, 33)                               # 33 and 32 columns
    nblk, nchunk, chunk = shape("capped_chunks")
    assert (nblk, nchunk, chunk) == (2, 256, 65)                              # the count is capped at 512 workgroups
    held = [max(0, min(16385, (b + 1) * chunk) - b * chunk) for b in range(nchunk)]
    assert sum(held) == 16385 and held[:252] == [65] * 252 and held[252:] == [5, 0, 0, 0]
    assert mc.last_chunk_start(70, 16385) == 16380 and mc.last_chunk_start(5, 65) == 33 and mc.last_chunk_start(70, 20) == 0


@pytest.mark.parametrize("name", mc.FRICTION_IDS)
def test_the_friction_states_hold_what_the_old_gate_could_not_see(name):
    c = mc.FRICTION_BY_NAME[name]
    d = mc.friction_case(name)
    u, v = d["uvel"][0].reshape(-1, c.nens), d["vvel"][0].reshape(-1, c.nens)
    assert (np.hypot(u, v) < 1.0).any() and (np.hypot(u, v) > 1.0).any()      # the wind clamp on both sides
    assert d["zint"].shape == (4, c.nens) and (c.nens == 1 or np.unique(d["zint"][1] - d["zint"][0]).size == c.nens)
    assert d["z0"].min() >= 1e-5 and d["z0"].max() <= 1.0
    if c.nens >= 3:
        b = d["bflx"]
        assert (b == 0).any() and (b > 0).any() and (b < 0).any() and (d["z0"] == 1e-5).any() and (d["z0"] == 1.0).any()
    r = mc.case_reference(name)
    mag = np.abs(r["fu"].astype(np.float64))
    decades = np.log10(mag.max() / mag[mag > 0].min())
    print("%s: |sfc_mom_flx_u| spans %.1f decades" % (name, decades))
    if c.nens >= 70:
        assert decades >= 6
        assert np.array_equal(d["tau"], np.sort(d["tau"])[::-1])            # the smallest tau on the ragged last block
        if name == "ragged":
            assert np.abs(r["fu"][..., -1].astype(np.float64)).max() < 1e-9 * mag.max()     # the last member: 1e-11 of the others' wind
        start = mc.last_chunk_start(c.nens, c.nx * c.ny)
        if start:
            assert (np.hypot(u, v)[start:] < 1.0)[:, d["bflx"] <= 0].all()   # the last chunk is calm


@pytest.mark.parametrize("name", mc.ALL_FRICTION_STATES)
def test_the_slot_order_mean_is_within_the_summation_bound_of_the_exact_mean(name):
    """|mean~ - mean| <= (ncol + 1) u mean|f|: a product carries two roundings, an addend passes through at most ncol - 1 additions"""
    d = mc.friction_case(name)
    ncol = d["rho_d"].shape[1] * d["rho_d"].shape[2]
    fields = (d["uvel"][0], d["vvel"][0], d["rho_d"][0] + d["rho_v"][0])
    for slot, serial, exact, f in zip(mc.slot_means(d), mc.serial_means(d), mc.exact_means(d), fields):
        bound = (ncol + 1) * mc.U * np.abs(f).reshape(ncol, -1).astype(LD).sum(axis=0) / ncol
        assert np.all(np.abs(slot.astype(LD) - exact) <= bound)
        assert np.all(np.abs(np.asarray(serial).astype(LD) - exact) <= bound)
    # and ref.level0_means_slot is tests/msa_ref.py's level_mean on level 0
    import msa_ref
    nens = d["rho_d"].shape[-1]
    assert mc.same_bits(msa_ref.level_mean(d["uvel"][:1].reshape(1, ncol, nens))[0], mc.slot_means(d)[0])


@pytest.mark.parametrize("name", mc.SMALL_FRICTION_IDS + ["module_" + i for i in mc.MODULE_FRICTION_IDS])
def test_the_emulation_is_the_restatement_bit_for_bit_on_friction(name):
    d = mc.friction_case(name)
    fu, fv = mc.fluxes_f64(d)
    pu, pv = mc.fluxes_python(d)
    assert mc.same_bits(fu, pu) and mc.same_bits(fv, pv)
    assert mc.same_bits(mc.z0_f64(d), mc.z0_f64(d, python=True))


def test_the_emulated_z0_of_the_largest_case_is_the_restatement():
    d = mc.friction_case("capped_chunks")
    assert mc.same_bits(mc.z0_f64(d), mc.z0_f64(d, python=True))


@pytest.mark.parametrize("name", mc.ALL_FRICTION_STATES)
def test_the_restatement_is_within_E_of_the_longdouble_reference(name):
    """E_FLUX and E_Z0 are the worst errors of the float64 restatement, in units, at the same slot-order means, over every committed
    friction state.  Measured: fluxes 8.9 ragged, 6.2 few_columns, 3.5 one_member, 6.8 three_chunks, 7.4 uneven_chunks, 42.0
    capped_chunks, 43.5 / 4.4 / 2.7 / 15.6 for the four states of the module test (43.5: its calm cell with a positive buoyancy
    flux); z0 35.9 (ragged), 42.5 (capped_chunks), 31.2 (the module test's 70 members); nothing on the others above 10.3."""
    d = mc.friction_case(name)
    r = mc.case_reference(name)
    eu, ev = mc.flux_errors(*mc.fluxes_f64(d), r)
    raw, want = r["z0_raw"], r["z0"]
    ez = mc.z0_errors(mc.z0_f64(d), raw, want)
    print("%s: fluxes %.2f units at the worst (median %.2f, 99th percentile %.2f), z0 %.2f units"
          % (name, max(eu.max(), ev.max()), np.median(np.maximum(eu, ev)), np.percentile(np.maximum(eu, ev), 99), ez.max()))
    assert max(eu.max(), ev.max()) <= mc.E_FLUX and ez.max() <= mc.E_Z0
    assert mc.G_FLUX == 4 * mc.E_FLUX and mc.G_Z0 == 4 * mc.E_Z0
    mc.assert_fluxes_within(*mc.fluxes_f64(d), r)
    mc.assert_z0_within(mc.z0_f64(d), raw, want)


def _mp_cell(mp, args):
    """surface_friction_cell at 40 digits on the double inputs"""
    M = lambda x: mp.mpf(float(x))
    u, v, um, vm, rm, z, b, z0, r0, r1, r2, dz = (M(x) for x in args)
    vonk, eps, am, bm, pi = (M(x) for x in (ref.VONK, ref.EPS, ref.AM, ref.BM, ref.PI))
    c1 = pi / 2 - 3 * mp.log(2)
    wnd = max(mp.mpf(1), mp.sqrt(u * u + v * v))
    lnz = mp.log(z / z0)
    ustar = wnd * (vonk / lnz)
    if b != 0:
        for _ in range(8):
            zeta = min(mp.mpf(1), z * (-b * vonk / (ustar ** 3 + eps)))
            if zeta > 0:
                ustar = vonk * wnd / (lnz + am * zeta)
            else:
                x = mp.sqrt(mp.sqrt(1 - bm * zeta))
                ustar = wnd * vonk / (lnz - (2 * mp.log(1 + x) + mp.log(1 + x * x) - 2 * mp.atan(x) + c1))
    k = rm * ustar * ustar / wnd * (2 * ((r0 + r1) / 2) - (r1 + r2) / 2) / dz
    return -(u - um) * k, -(v - vm) * k


def _mpf_of(mp, x):
    """a longdouble as the exact mpf"""
    m, e = np.frexp(x)
    return mp.mpf(int(m * LD(2) ** 64)) * mp.mpf(2) ** (int(e) - 64)


def test_the_longdouble_reference_against_40_digits():
    """60 cells of every named case, drawn at random, against mpmath at 40 digits: agreement to 1e-3 of a unit.  The reference is
    evaluated in binary128 and rounded once to longdouble, which alone may cost 2^-11 = 4.9e-4 of a unit.  (np.longdouble throughout
    does not get there: its 64 bits are 11 more than a double's and the same operations amplify its roundings as they amplify the
    restatement's, which leaves 5.1e-3 of a unit on these 360 cells: test_the_longdouble_restatement_is_the_reference_to_its_64_bits.)"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    rng = np.random.default_rng(1)
    worst = 0.0
    for name in mc.FRICTION_IDS:
        d = mc.friction_case(name)
        r = mc.case_reference(name)
        args = [a.ravel() for a in mc.cell_inputs(d)]
        flat = {k: v.ravel() for k, v in r.items()}
        for i in rng.choice(args[0].size, min(60, args[0].size), replace=False):
            want = _mp_cell(mp, [a[i] for a in args])
            for got, w, unit in ((flat["fu"][i], want[0], flat["unit_u"][i]), (flat["fv"][i], want[1], flat["unit_v"][i])):
                if unit > 0:
                    worst = max(worst, float(abs(_mpf_of(mp, got) - w) / mp.mpf(float(unit))))
                else:
                    assert got == 0 and w == 0
    print("flux reference against mpmath: %.3g of a unit at the worst" % worst)
    assert worst <= 1e-3


@pytest.mark.parametrize("name", mc.ALL_FRICTION_STATES)
def test_the_longdouble_restatement_is_the_reference_to_its_64_bits(name):
    """surface_friction.h restated twice, in np.longdouble (numpy, vectorised) and in binary128 (C): every cell of every committed
    state agrees to what 64 bits can give -- 2^-11 of the float64 restatement's error, doubled: 2^-10 E_FLUX = 0.043 of a unit
    (measured 0.031 at the worst, in capped_chunks) -- and the units agree to the last place"""
    d = mc.friction_case(name)
    r, l = mc.case_reference(name), mc.friction_reference_ld(d)
    eu, ev = mc.flux_errors(l["fu"], l["fv"], r)
    print("%s: longdouble against binary128 %.4f of a unit at the worst" % (name, max(eu.max(), ev.max())))
    assert max(eu.max(), ev.max()) <= 2.0 ** -10 * mc.E_FLUX
    for k in ("unit_u", "unit_v"):
        assert np.all(np.abs(l[k] - r[k]) <= 4 * np.spacing(r[k]))
    raw, z0 = mc.z0_reference_ld(d)
    ez = float(mc.z0_errors(z0, r["z0_raw"], r["z0"]).max())
    print("%s: longdouble z0 against binary128 %.4f of a unit at the worst" % (name, ez))
    assert ez <= 2.0 ** -10 * mc.E_Z0                    # likewise: 0.042 of a unit
    pinned = (r["z0_raw"] < LD(0.00001)) | (r["z0_raw"] > LD(1))
    assert np.array_equal(z0[pinned], r["z0"][pinned])


def test_the_longdouble_z0_against_40_digits():
    """z0 of every member of every named case at 40 digits, after the clamps as the gate uses it: agreement to 1e-3 of a unit, as for
    the fluxes.  The reference is evaluated in binary128 and rounded once to longdouble (at most 2^-11 = 4.9e-4 of a unit);
    np.longdouble throughout leaves 9.9e-3 (test_the_longdouble_restatement_is_the_reference_to_its_64_bits)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    M = lambda x: mp.mpf(float(x))
    vonk, eps, am, bm, pi = (M(x) for x in (ref.VONK, ref.EPS, ref.AM, ref.BM, ref.PI))
    c1 = pi / 2 - 3 * mp.log(2)
    worst = 0.0
    for name in mc.FRICTION_IDS:
        d = mc.friction_case(name)
        clamped = mc.case_reference(name)["z0"]
        (rm,) = ref.level0_means_slot([d["rho_d"][0] + d["rho_v"][0]], d["tau"].size)
        for e in range(d["tau"].size):
            z, b, gu, gv, tau, rho = (M(x) for x in (d["zmid"][0, e], d["bflx"][e], d["gcm_uvel"][0, e], d["gcm_vvel"][0, e], d["tau"][e], rm[e]))
            wnd = max(mp.mpf(1), mp.sqrt(gu * gu + gv * gv))
            ustar = mp.sqrt(tau / rho)
            zeta = min(mp.mpf(1), z * (-b * vonk / (ustar ** 3 + eps)))
            if zeta >= 0:
                psi1 = -am * zeta
            else:
                x = mp.sqrt(mp.sqrt(1 - bm * zeta))
                psi1 = 2 * mp.log(1 + x) + mp.log(1 + x * x) - 2 * mp.atan(x) + c1
            want = z * mp.exp(-max(mp.mpf(0), vonk * wnd / (ustar + eps) + psi1))
            want = max(M(0.00001), min(mp.mpf(1), want))
            worst = max(worst, float(abs(_mpf_of(mp, clamped[e]) - want) / (mp.mpf(mc.U) * want)))
    print("longdouble z0 against mpmath: %.3g of a unit at the worst" % worst)
    assert worst <= 1e-3


FRICTION_OLD_GATE_ACCEPTS = {"serial_means": mc.FRICTION_IDS, "last_member_z0": ["ragged"], "last_chunk_zero_umean": ["capped_chunks"]}
FRICTION_MUST_REJECT = {"last_member_z0": "ragged", "last_chunk_zero_umean": "capped_chunks", "zeta_ge": "ragged"}


@pytest.mark.parametrize("mutant", ref.FRICTION_MUTANTS)
def test_the_cell_gate_rejects_every_friction_mutant(mutant):
    """one deliberate error at a time.  A mutant of the cell's own arithmetic runs through the scalar Python restatement on the small
    cases; one that changes what a cell is handed (the means, z0, dz) through the emulation on every case.  Where the old gate is said
    to accept a mutant, it is the placement of the small scales that hides it: the last member of ragged is uniform but for 1e-11, u
    has no mean in capped_chunks and its last chunk is calm.  zeta_ge differs from the reference only where zeta is exactly zero
    inside the loop: member 7 of ragged, whose denormal buoyancy flux times 0.4 rounds to -0.0."""
    names = mc.SMALL_FRICTION_IDS if mutant in mc.BODY_MUTANTS else mc.FRICTION_IDS
    rejected, old = [], {}
    for name in names:
        d = mc.friction_case(name)
        got = mc.fluxes_f64(d, mutant=mutant)
        try:
            mc.assert_fluxes_within(*got, mc.case_reference(name))
        except AssertionError:
            rejected.append(name)
        old[name] = mc.old_flux_gate_accepts(*got, *mc.fluxes_f64(d))
    print("%s: rejected on %s; the old gate accepts it on %s" % (mutant, rejected, [n for n, ok in old.items() if ok]))
    assert rejected, mutant
    if mutant in FRICTION_MUST_REJECT:
        assert FRICTION_MUST_REJECT[mutant] in rejected
    for name in FRICTION_OLD_GATE_ACCEPTS.get(mutant, []):
        assert old[name], (mutant, name)
    if mutant not in FRICTION_OLD_GATE_ACCEPTS:
        assert not all(old.values()), mutant


def test_the_z0_gate_holds_a_small_member_to_its_own_size():
    """the old gate let z0 = 3e-4 move by 1e-12 (the clamp puts the largest at 1.0): 3e-9 relative.  The member gate does not, and a
    member the clamps pin must hold the literal."""
    d = mc.friction_case("ragged")
    raw, want = mc.case_reference("ragged")["z0_raw"], mc.case_reference("ragged")["z0"]
    z0 = mc.z0_f64(d)
    inner = np.flatnonzero((raw > 1e-5) & (raw < 1e-3))
    assert inner.size and (raw < 1e-5).any() and (raw > 1).any()
    assert np.all(np.abs(z0 - want.astype(np.float64)) <= mc.OLD_GATE)
    for i, value in ((inner[0], z0[inner[0]] + 5e-13), (int(np.argmin(raw)), np.nextafter(1e-5, 1.0)), (int(np.argmax(raw)), np.nextafter(1.0, 0.0))):
        got = z0.copy()
        got[i] = value
        assert abs(got[i] - z0[i]) <= mc.OLD_GATE                             # the old gate accepts
        with pytest.raises(AssertionError):
            mc.assert_z0_within(got, raw, want)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU

def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def gpu_adjust(d):
    """pam_amd_saturation_adjustment through the C ABI on a copy of the case: (rho_v, rho_c, temp) and every other array after"""
    import torch
    c = d["case"]
    nens, nx, ny, nz = c.shape
    before = d["before"]
    own = {id(before[k]): _dev(before[k]) for k in mc.ADJUSTED}
    rho_d = _dev(d["rho_d"])
    massy = [own[id(m)] if id(m) in own else _dev(m) for m in d["massy"]]
    table = (C.c_void_p * len(massy))(*[t.data_ptr() for t in massy]) if massy else None
    rv, rc, t = (own[id(before[k])] for k in mc.ADJUSTED)
    capi.check(capi.load().pam_amd_saturation_adjustment(nens, nx, ny, nz, rho_d.data_ptr(), rv.data_ptr(), rc.data_ptr(), t.data_ptr(),
                                                         len(massy), table, mc.R_V, mc.CP_D, mc.CP_V, ref.CP_L, None))
    torch.cuda.synchronize()
    got = dict(zip(mc.ADJUSTED, (rv.cpu().numpy(), rc.cpu().numpy(), t.cpu().numpy())))
    others = [(m, x.cpu().numpy()) for m, x in zip(d["massy"], massy) if id(m) not in own] + [(d["rho_d"], rho_d.cpu().numpy())]
    return got, others


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.CAPI_IDS)
def test_gpu_saturation_adjustment_c_abi_equals_the_restatement_bit_for_bit(name):
    """specials (NaN, -0.0, negative densities, brackets at the tolerance, absurd and infinite densities among ordinary cells) and the
    lists of 0, 1 and 55 tracers that add mass: every bit of rho_v, rho_c and temp, no cell exempt, nothing else written, and a second
    call gives the first one's bits"""
    d = mc.saturation_case(name)
    got, others = gpu_adjust(d)
    exempt = mc.assert_adjusted_bits(got, d["want"], d["info"], d["before"])
    print("%s: %d of %d cells adjusted, %d exempt" % (name, int((d["info"]["branch"] > 0).sum()), d["info"]["branch"].size, exempt))
    assert exempt == 0
    for k in mc.ADJUSTED:
        assert mc.same_bits(got[k], d["want"][k]), k                       # the capped cells and every NaN too
    for host, after in others:
        assert mc.same_bits(after, host)
    again, _ = gpu_adjust(d)
    for k in mc.ADJUSTED:
        assert mc.same_bits(again[k], got[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.ORDER_IDS)
def test_gpu_saturation_adjustment_module_sums_the_tracers_in_registration_order(name):
    """modules.saturation_adjustment on the two states in which the order of rho = rho_d + tracers shows in the bits of temp (the
    restatement with the list reversed fails this gate: test_the_bit_gate_rejects_every_saturation_mutant).  The three shapes of the
    module test, where no order shows, are in tests/test_moist_surface_modules.py."""
    import torch
    import test_moist_surface_modules as tms
    from pam_amd import modules
    d = mc.saturation_case(name)
    c = tms._coupler(d["tracers"], d["fields"], d["case"].micro)
    c.run_module("saturation_adjustment", modules.saturation_adjustment)
    torch.cuda.synchronize()
    dump = tms._dump(c, list(d["fields"]))
    got = {"rho_v": dump["water_vapor"], "rho_c": dump[mc.CONDENSATE[d["case"].micro]], "temp": dump["temp"]}
    assert mc.assert_adjusted_bits(got, d["want"], d["info"], d["before"]) == 0


def gpu_friction(d, members=None):
    """both entry points through the C ABI, compute with the case's own z0 and bflx as inputs: dict(z0, sfc_bflx, zeroed (the fluxes
    after the init), fu, fv, kept (no input was written)).  members: a slice of the ensemble."""
    import torch
    sl = slice(None) if members is None else members
    h = {k: np.ascontiguousarray(v[..., sl]) for k, v in d.items()}
    nz, ny, nx, nens = h["rho_d"].shape
    t = {k: _dev(v) for k, v in h.items()}
    out = {k: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
           for k, shape in (("z0", (nens,)), ("sfc_bflx", (nens,)), ("iu", (ny, nx, nens)), ("iv", (ny, nx, nens)), ("fu", (ny, nx, nens)),
                            ("fv", (ny, nx, nens)))}
    lib = capi.load()
    p = lambda x: x.data_ptr()
    capi.check(lib.pam_amd_surface_friction_init(nens, nx, ny, nz, p(t["rho_d"]), p(t["rho_v"]), p(t["zmid"]), p(t["gcm_uvel"]), p(t["gcm_vvel"]),
                                                 p(t["tau"]), p(t["bflx"]), p(out["z0"]), p(out["sfc_bflx"]), p(out["iu"]), p(out["iv"]), None))
    capi.check(lib.pam_amd_surface_friction_compute(nens, nx, ny, nz, p(t["rho_d"]), p(t["rho_v"]), p(t["uvel"]), p(t["vvel"]), p(t["zmid"]),
                                                    p(t["zint"]), p(t["z0"]), p(t["bflx"]), p(out["fu"]), p(out["fv"]), None))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["zeroed"] = not res.pop("iu").any() and not res.pop("iv").any()
    res["kept"] = all(mc.same_bits(t[k].cpu().numpy(), h[k]) for k in h)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.FRICTION_IDS)
def test_gpu_surface_friction_c_abi_within_the_cell_and_member_gates(name):
    """compute_surface_friction with z0 and sfc_bflx as inputs: every cell of both fluxes within G_FLUX units of the longdouble
    reference at the slot-order means.  surface_friction_init: every member's z0 within G_Z0 units, the pinned ones exact; sfc_bflx
    the input's bits (the denormal among them); the fluxes zeroed.  A second call gives the first one's bits."""
    d = mc.friction_case(name)
    got = gpu_friction(d)
    r = mc.case_reference(name)
    worst = mc.assert_fluxes_within(got["fu"], got["fv"], r)
    raw, want = r["z0_raw"], r["z0"]
    worst_z0 = mc.assert_z0_within(got["z0"], raw, want)
    print("%s: fluxes %.2f units at the worst (gate %g), z0 %.2f units (gate %g)" % (name, worst, mc.G_FLUX, worst_z0, mc.G_Z0))
    assert mc.same_bits(got["sfc_bflx"], d["bflx"]) and got["zeroed"] and got["kept"]
    again = gpu_friction(d)
    for k in ("z0", "fu", "fv"):
        assert mc.same_bits(again[k], got[k]), k


@pytest.mark.gpu
def test_gpu_surface_friction_member_shards_give_the_bits_of_the_whole():
    """ragged: 70 members as 33 + 31 + 6, the last shard the ragged block's members with the smallest scales"""
    d = mc.friction_case("ragged")
    whole = gpu_friction(d)
    parts = [gpu_friction(d, sl) for sl in (slice(0, 33), slice(33, 64), slice(64, 70))]
    for k in ("z0", "fu", "fv"):
        assert mc.same_bits(np.concatenate([x[k] for x in parts], axis=-1), whole[k]), k
