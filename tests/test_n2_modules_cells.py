"""sponge_layer, perturb_temperature and broadcast_initial_gcm_column[_dry_density] cell by cell (tests/n2_modules_ref.py has the
longdouble restatements and the derivation of the per-cell gates, tests/n2_modules_cases.py the states, the named cases and the mutants).

Without a GPU: what the named states reach (census), the generator's known answers and that restatement, numpy generator and oracle
draw the same integers, the oracle and a numpy-double emulation of the device's summation order inside the per-cell gate on every named
case, every mutant of the restatement caught by the gate on every case meant to catch it, and the record of the gap: mutants that the
state and the max-norm of tests/test_modules.py let through.

On the GPU (-m gpu): every named case through PamCoupler.run_module (or the C entry point where the case says so), read back and
gated per cell, untouched levels compared bit for bit; on one ragged case of sponge and perturb: two runs give the same bits, member
shards give the whole call's bits, the dirty flags are those tests/test_modules.py asserts.

Each test prints its worst err/tol (pytest -s shows them; DESIGN.md section 8 has the record)."""
import copy
import ctypes as C

import numpy as np
import pytest

import n2_modules_cases as nc
import n2_modules_ref as nr

LD = nr.LD


def _sponge_gate(got, ref, what):
    """got (nf, nz, ny, nx, nens) double against a sponge_reference: bits below the sponge, tol inside.  Returns worst err/tol."""
    X, sp = ref["X"], ref["ref"]["sponge"]
    assert got.shape == X.shape and np.isfinite(got).all(), what
    assert np.array_equal(nr.bits(got[:, :sp.start]), nr.bits(X[:, :sp.start])), (what, "a level below the sponge changed")
    worst, where = nr.worst_ratio(got, ref["ref"])
    print("sponge %-34s %-9s worst err/tol %.3f at (field, k, j, i, e) = %s" % (ref["case"].name, what, worst, where))
    assert worst < 1.0, (what, worst, where)
    return worst


def _perturb_gate(got, ref, what):
    nl = ref["ref"]["nl"]
    assert got.shape == ref["T"].shape and np.isfinite(got).all(), what
    assert np.array_equal(nr.bits(got[nl:]), nr.bits(ref["T"][nl:])), (what, "a level at or above nz/4 changed")
    worst, where = nr.worst_ratio(got[:nl], dict(r=ref["ref"]["r"][:nl], tol=ref["ref"]["tol"][:nl])) if nl else (0.0, ())
    print("perturb %-33s %-9s worst err/tol %.3f at (k, j, i, e) = %s" % (ref["case"].name, what, worst, where))
    assert worst < 1.0, (what, worst, where)
    return worst


# ---- without a GPU: the generator ---------------------------------------------------------------------------------------------------

def test_splitmix64_known_answers():
    """the published first output of state 0, and of state 1234567"""
    assert nr.splitmix64_next(0)[1] == 0xE220A8397B1DCDAF
    assert nr.splitmix64_next(1234567)[1] == 6457827717110365317
    s, a = nr.splitmix64_next(0)
    assert nr.splitmix64_next(s)[1] == 0x6E789E6AA1B965F4          # the second output of state 0
    got = nr.splitmix64_ints(np.array([0, 1234567, -1], dtype=np.int64))
    assert [int(x) for x in got] == [0xE220A8397B1DCDAF, 6457827717110365317, nr.splitmix64_next(2 ** 64 - 1)[1]]


def test_restatement_numpy_generator_and_oracle_draw_the_same_integers():
    from oracle import awfl_oracle as ao
    from pam_amd import idealized as idz
    seeds = np.concatenate([np.arange(-5, 300, dtype=np.int64), np.array([2 ** 31 - 1, 2 ** 31, (2 ** 31 - 1) * 160 + 159,
                                                                          -(2 ** 31) * 160, 2 ** 62 + 12345], dtype=np.int64)])
    ints = nr.unit_ints(seeds)
    assert [int(x) for x in ints[5:8]] == [nr.splitmix64_next(s)[1] >> 11 for s in (0, 1, 2)]
    with np.errstate(over="ignore"):
        unit = idz._splitmix64(seeds.astype(np.uint64))
    assert np.array_equal(unit * 2.0 ** 53, ints.astype(np.float64)) and ints.max() < 2 ** 53        # 53 bits: the conversion is exact
    # the oracle's generator is not exported.  On a level of zeros but for one cell, with magnitude 1 and one perturbed level (scaling
    # 1), the perturbed cell IS the random number, a multiple of 2^-52 that holds all 53 bits of the integer; the rescale multiplies
    # every cell of a (level, member) by the same two doubles.  The serial double emulation, which draws from the restatement's
    # integers, must give the oracle's bits -- for every member id, negative and beyond 32 bits included.
    nens, nx, ny, nz = 8, 7, 3, 4
    ids = np.array([0, 1, 1, -3, 2 ** 31 - 1, -(2 ** 31), 77, 2 ** 31 - 2], dtype=np.int32)
    T = np.zeros((nz, ny, nx, nens))
    T[:, 0, 0, :] = 1.0
    want = nr.perturb_serial_emulation(T, ids, 1.0)
    got = T.copy()
    ao.perturb_temperature(got, ids, 1.0)
    assert np.array_equal(nr.bits(got), nr.bits(want))
    assert len(np.unique(got[0])) == 7 * ny * nx          # two of the eight members share an id, and so a level
    # ... and on the named states
    for name in nc.PERTURB_IDS:
        ref = nc.perturb_reference(name)
        assert np.array_equal(nr.bits(ref["oracle"]), nr.bits(ref["emulation"])), name
    # the generator of the benchmark's inputs (ids id0, id0 + 1, ...; numpy's pairwise means) inside the gate of the restatement
    T = nc.perturb_state(5, 4, 3, 9)
    ref = nr.perturb(T, np.arange(5) + 7, 30.0)
    worst, where = nr.worst_ratio(idz.perturb_temperature(T.copy(), 30.0, id0=7)[:2], dict(r=ref["r"][:2], tol=ref["tol"][:2]))
    assert worst < 1.0, (worst, where)


# ---- without a GPU: sponge_layer ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", nc.SPONGE_IDS)
def test_sponge_census_state_reaches_what_it_declares(name):
    ref = nc.sponge_reference(name)
    c, X, r = ref["case"], ref["X"], ref["ref"]
    nf, nz, ny, nx, nens = X.shape
    assert nens * nx * ny * nz <= 25000 and nf == 5 + c.ntr <= 55
    sp = r["sponge"]
    S = X[:, sp]
    ncol = nx * ny
    h = S.mean(axis=(2, 3))                                                   # (nf, levels, nens)
    if ncol > 1:
        assert (S.max(axis=(2, 3)) > S.min(axis=(2, 3))).all()                # every field varies on every sponge level of every member
        for t in range(5, nf):
            assert ((S[t] > 0).any(axis=(1, 2)) & (S[t] == 0).any(axis=(1, 2))).all(), t
        sd = S.std(axis=(2, 3))
        for f in (1, 2):
            assert (S[f].min(axis=(1, 2)) < 0).all() and (S[f].max(axis=(1, 2)) > 0).all()
        if ncol >= 15:
            assert (np.abs(h[[1, 2]]).mean() < 0.5 * sd[[1, 2]].mean()) and (np.abs(h[[0, 4]]) > 20 * sd[[0, 4]]).all()
    assert (np.abs(X[3, sp].mean(axis=(1, 2))) > 0.5).all() if ncol >= 5 else True      # a w whose mean matters
    if nens > 1:
        for f in range(nf if ncol > 1 else 5):                                # member-dependent means
            assert (np.abs(h[f, :, 0] - h[f, :, 1]) > 0).all(), f
    if c.ntr >= 4:
        mags = np.array([X[5 + t].max() for t in range(c.ntr)])
        assert mags.max() / mags.min() >= 1e3
    F = r["F"].astype(np.float64)
    tf = c.dt / ref["time_scale"]
    assert (F[:sp.start] == 0).all() and (F[sp] >= 0).all() and F[nz - 1].max() <= tf
    assert (F[sp.start] < 1e-30 * tf).all()                                   # rel_dist = 1 on the bottom sponge level: F vanishes
    if ref["num_layers"] >= 2:
        assert (F[nz - 1] > 0.5 * tf).all()
        if nens > 1:                                                          # the factor is the member's own
            a, b = F[sp.start + 1:, 0], F[sp.start + 1:, 1]
            assert (np.abs(a - b) > 1e-3 * np.maximum(a, b)).all(), (a, b)
    if "factor_above_1" in name:
        assert F.max() > 1.0


def test_sponge_census_named_cases_cover_the_edges():
    cs = nc.SPONGE
    assert {c.nx * c.ny for c in cs} >= {1, 5, 15, 16, 17, 33}
    assert {c.nens for c in cs} >= {1, 3, 64, 65, 130}
    assert {c.ntr + 5 for c in cs} >= {5, 6, 9, 55}
    assert any(c.num_layers == 1 for c in cs) and any(c.num_layers == 2 for c in cs) and any(c.num_layers == c.nz for c in cs)
    assert any(c.num_layers is None and c.nz > 5 for c in cs)
    assert any(c.dt > c.time_scale for c in cs if c.time_scale)
    assert {c.via for c in cs if c.ntr in (0, 50)} >= {"capi"} and all(c.via == "capi" for c in cs if c.ntr == 0)
    assert nc.SPONGE_BY_NAME[nc.SPONGE_RAGGED].nens % 64 not in (0, 1)


@pytest.mark.parametrize("name", nc.SPONGE_IDS)
def test_sponge_oracle_and_slot_order_emulation_are_inside_the_gate(name):
    ref = nc.sponge_reference(name)
    _sponge_gate(ref["oracle"], ref, "oracle")
    _sponge_gate(ref["emulation"], ref, "emulation")
    if ref["num_layers"] == 1:      # F = 0 on the only level: the input, within tol
        worst, _ = nr.worst_ratio(ref["X"], ref["ref"])
        assert worst < 1.0


@pytest.mark.parametrize("mutant", list(nc.SPONGE_MUTANTS))
def test_sponge_gate_catches_every_mutant_of_the_restatement(mutant):
    meant = [c for c in nc.SPONGE if nc.SPONGE_MUTANTS[mutant](c)]
    assert len(meant) >= 2
    for c in meant:
        ref = nc.sponge_reference(c.name)
        L, ts = nc.layers_and_scale(c)
        bad = nr.sponge(ref["X"], ref["zint"], ref["zmid"], c.dt, L, ts, mutant=mutant)["r"].astype(np.float64)
        worst, where = nr.worst_ratio(bad, ref["ref"])
        print("sponge mutant %-26s on %-34s err/tol %.3g" % (mutant, c.name, worst))
        assert worst > 1.0, (mutant, c.name, worst)


def _present_state():
    """the state and the call of tests/test_modules.py::test_gpu_sponge_layer_matches_oracle, at the size the measurements of
    DESIGN.md section 8 were taken"""
    import test_modules as tm
    from oracle import awfl_oracle as ao
    zint, zi, zm, f = tm._case(nens=3, nx=5, ny=4, nz=12)
    X = nr.stack(f)
    g = copy.deepcopy(f)
    ao.sponge_layer(g, zi, zm, 2.0, num_layers=4, time_scale=30.0)
    return X, np.ascontiguousarray(zi), np.ascontiguousarray(zm), nr.stack(g)


def _passes_present_max_norm(got, oracle):
    return all(np.abs(got[f] - oracle[f]).max() <= 1e-14 * max(np.abs(oracle[f]).max(), 1e-300) for f in range(len(oracle)))


def test_present_state_and_max_norm_let_mutants_through():
    """The record of the gap.  On the state every other sponge test shares the oracle's sponge changes wvel and nothing else, and under
    the max-norm of tests/test_modules.py (1e-14 max|field|)
      * a sponge that reads member 0's heights for every member, one that skips the last tracer and one that takes its means from
        member (e + 64) % nens pass in every field;
      * a sponge with the factor of the level above, with half the factor, or with w relaxed to its mean is wrong in wvel alone: eight
        of the nine fields cannot tell;
      * a cell of the smallest sponge level (water vapour at the top, 6e-4 of the field's maximum) may be off by 1e-11 of itself,
        1e4 times the per-cell gate on that very state.  (Off by 1e-9 of itself it is 6e-13 of the maximum, which the max-norm does
        see: measured, the level would have to be another two decades below the maximum.)
    All of these fail the per-cell gate on the named cases (test_sponge_gate_catches_every_mutant_of_the_restatement)."""
    X, zi, zm, oracle = _present_state()
    changed = [f for f in range(len(X)) if not np.array_equal(X[f], oracle[f])]
    assert changed == [nr.WFLD]
    true = nr.sponge(X, zi, zm, 2.0, 4, 30.0)
    assert _passes_present_max_norm(true["r"].astype(np.float64), oracle)

    def wrong_fields(bad):
        return [f for f in range(len(X)) if np.abs(bad[f] - oracle[f]).max() > 1e-14 * max(np.abs(oracle[f]).max(), 1e-300)]
    for mutant in ("member0_heights", "last_tracer_skipped", "mean_from_member_plus_64"):
        bad = nr.sponge(X, zi, zm, 2.0, 4, 30.0, mutant=mutant)["r"].astype(np.float64)
        assert wrong_fields(bad) == [], mutant
    for mutant in ("factor_from_level_above", "factor_halved", "w_to_its_mean"):
        bad = nr.sponge(X, zi, zm, 2.0, 4, 30.0, mutant=mutant)["r"].astype(np.float64)
        assert wrong_fields(bad) == [nr.WFLD], mutant
    one = nr.sponge(X, zi, zm, 2.0, 4, 30.0, mutant="one_cell_1e-9")
    cell = tuple(int(x) for x in one["cell"])
    assert wrong_fields(one["r"].astype(np.float64)) == [cell[0]] and cell[0] == 5 and cell[1] == X.shape[1] - 1
    assert abs(oracle[cell]) < 1e-3 * np.abs(oracle[cell[0]]).max()
    bad = oracle.copy()
    bad[cell] *= 1 + 1e-11
    assert wrong_fields(bad) == []
    worst, where = nr.worst_ratio(bad, true)
    assert where == cell and worst > 1e3, (worst, where)


# ---- without a GPU: perturb_temperature ---------------------------------------------------------------------------------------------

def test_perturb_census_named_cases_cover_the_edges():
    cs = nc.PERTURB
    assert {c.nz for c in cs} >= {3, 4, 7, 8, 17}
    assert {c.nx * c.ny for c in cs} >= {1, 2, 15, 40}
    assert {c.nens for c in cs} >= {1, 3, 33, 64, 65, 70}
    assert any(c.nens == 33 and c.nz // 4 == 2 for c in cs)
    assert {c.magnitude for c in cs} == {0.25, 30.0}
    kinds = dict(zero=False, dup=False, neg=False, wide=False)
    for c in cs:
        ids = nc.perturb_ids(c.ids, c.nens).astype(np.int64)
        assert c.nens * c.nx * c.ny * c.nz <= 25000
        nl = c.nz // 4
        kinds["zero"] |= bool((ids == 0).any())
        kinds["dup"] |= len(np.unique(ids)) < len(ids)
        kinds["neg"] |= bool((ids < 0).any())
        kinds["wide"] |= bool((ids == 2 ** 31 - 1).any()) and (2 ** 31 - 1) * nl * c.nx * c.ny >= 2 ** 32
        T = nc.perturb_reference(c.name)["T"]
        assert T.min() > 200.0                                         # positive: the gate's premise
        if c.nx * c.ny >= 15:
            assert ((T.max(axis=(1, 2)) - T.min(axis=(1, 2))) > 25.0).all()
        if c.nens > 1:
            assert (np.abs(T.mean(axis=(1, 2))[:, 0] - T.mean(axis=(1, 2))[:, 1]) > 0).all()
    assert all(kinds.values()), kinds
    # hmean1 / hmean2 clearly leaves 1 at magnitude 30
    ref = nc.perturb_reference("n33_2x1x8_duplicate_ids")
    T, r = ref["T"], ref["ref"]["r"].astype(np.float64)
    assert np.abs(r[:2].mean(axis=(1, 2)) / T[:2].mean(axis=(1, 2)) - 1).max() < 1e-14          # the mean is restored ...
    assert np.abs(r[:2] - T[:2]).max() > 5.0                                                    # ... by cells that moved by kelvins
    assert np.median(np.abs(ref["ref"]["ratio"] - 1)) > 1e-3                                    # ... and a rescale that is not the identity


@pytest.mark.parametrize("name", nc.PERTURB_IDS)
def test_perturb_oracle_and_serial_emulation_are_inside_the_gate(name):
    ref = nc.perturb_reference(name)
    _perturb_gate(ref["oracle"], ref, "oracle")
    _perturb_gate(ref["emulation"], ref, "emulation")
    c = ref["case"]
    if c.nz // 4 == 0:
        assert np.array_equal(nr.bits(ref["oracle"]), nr.bits(ref["T"]))
    if c.nx * c.ny == 1:      # the rescale restores the only cell of the level
        assert np.array_equal(ref["ref"]["r"], ref["T"].astype(LD))


@pytest.mark.parametrize("mutant", list(nc.PERTURB_MUTANTS))
def test_perturb_gate_catches_every_mutant_of_the_restatement(mutant):
    meant = [c for c in nc.PERTURB if nc.PERTURB_MUTANTS[mutant](c)]
    assert len(meant) >= 2
    for c in meant:
        ref = nc.perturb_reference(c.name)
        bad = nr.perturb(ref["T"], ref["ids"], c.magnitude, mutant=mutant)["r"].astype(np.float64)
        worst, where = nr.worst_ratio(bad, ref["ref"])
        print("perturb mutant %-24s on %-30s err/tol %.3g" % (mutant, c.name, worst))
        assert worst > 1.0, (mutant, c.name, worst)


# ---- without a GPU: broadcast -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", nc.BROADCAST, ids=nc.BROADCAST_IDS)
def test_broadcast_oracle_copies_bits_and_the_dry_density_variant_one_field(shape):
    from oracle import awfl_oracle as ao
    nens, nx, ny, nz = shape
    ncell = nens * nx * ny * nz
    assert ncell <= 25000
    crm, gcm = nc.broadcast_state(*shape)
    gb = [nr.bits(g) for g in gcm]
    assert set(int(s) for s in nc.SPECIALS) <= set(int(b) for g in gb for b in g.reshape(-1))
    for n in (1, 6):
        got = dict(zip(ao.BROADCAST_CRM, (c.copy() for c in crm)))
        ao.broadcast_initial_gcm_column(got, dict(zip(ao.BROADCAST_GCM, gcm)), dry_density_only=n == 1)
        want = nr.broadcast([nr.bits(c) for c in crm], gb, n)
        for f, name in enumerate(ao.BROADCAST_CRM):
            assert np.array_equal(nr.bits(got[name]), want[f]), (n, name)
            assert np.array_equal(want[f], nr.bits(crm[f])) == (f >= n)


def test_broadcast_census_cell_counts_around_the_workgroup_size():
    cells = {s[0]: set() for s in nc.BROADCAST}
    for nens, nx, ny, nz in nc.BROADCAST:
        n = nens * nx * ny * nz
        cells[nens].add("below" if n < 256 else "multiple" if n % 256 == 0 else "past" if n % 256 <= 16 else "other")
    assert cells == {1: {"below", "multiple", "past"}, 70: {"below", "multiple", "past"}}


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------

def _tracer_names(ntr):
    return ["water_vapor"] + ["tracer%02d" % t for t in range(1, ntr)]


def _device_sponge(c, X, zi, zm, check_dirty=False):
    """the case's call on (a member shard of) its state: the fields afterwards, stacked"""
    import torch
    from pam_amd import PamCoupler, capi, modules
    X, zi, zm = np.array(X), np.array(zi), np.array(zm)      # (the references are read-only; torch wants writable arrays)
    nf, nz, ny, nx, nens = X.shape
    if c.via == "capi":
        L, ts = nc.layers_and_scale(c)
        dev = torch.device("cuda:0")
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in X]
        zi_d, zm_d = torch.from_numpy(zi).to(dev), torch.from_numpy(zm).to(dev)
        ptrs = (C.c_void_p * nf)(*[x.data_ptr() for x in t])
        with torch.cuda.device(dev):
            capi.check(capi.load().pam_amd_sponge_layer(nens, nx, ny, nz, nf, ptrs, zi_d.data_ptr(), zm_d.data_ptr(), float(c.dt), int(L),
                                                        float(ts), None, torch.cuda.current_stream(dev).cuda_stream))
            torch.cuda.synchronize()
        return np.stack([x.cpu().numpy() for x in t])
    coupler = PamCoupler("cuda:0")
    coupler.set_option("crm_dt", c.dt)
    if c.num_layers is not None:
        coupler.set_option("sponge_num_layers", c.num_layers)
        coupler.set_option("sponge_time_scale", c.time_scale)
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(nx * 500.0, ny * 500.0, zi)
    for n in _tracer_names(c.ntr):
        coupler.add_tracer(n, "", True, True)
    dm = coupler.get_data_manager_device_readwrite()
    assert np.array_equal(dm.get("vertical_midpoint_height", readonly=True).cpu().numpy(), zm)
    coupler.load_fields(nr.unstack(X))
    dirty = coupler.run_module("sponge_layer", modules.sponge_layer)
    torch.cuda.synchronize()
    if check_dirty:
        assert "temp" in dirty and "water_vapor" in dirty
        assert sorted(dirty) == sorted(["density_dry", "uvel", "vvel", "wvel", "temp"] + _tracer_names(c.ntr))
    return nr.stack(coupler.dump_fields())


@pytest.mark.gpu
@pytest.mark.parametrize("name", nc.SPONGE_IDS)
def test_gpu_sponge_named_case_is_inside_the_gate_in_every_cell(name):
    ref = nc.sponge_reference(name)
    got = _device_sponge(ref["case"], ref["X"], ref["zint"], ref["zmid"], check_dirty=ref["case"].via == "coupler")
    _sponge_gate(got, ref, "device")


def _shard(a, lo, hi):
    return np.ascontiguousarray(a[..., lo:hi])


@pytest.mark.gpu
def test_gpu_sponge_is_deterministic_and_member_shards_equal_the_whole_call():
    """on a state where every field's mean is a relaxation target (the shard test of tests/test_modules.py only ever sees w move)"""
    ref = nc.sponge_reference(nc.SPONGE_RAGGED)
    c, X, zi, zm = ref["case"], ref["X"], ref["zint"], ref["zmid"]
    whole = _device_sponge(c, X, zi, zm, check_dirty=True)
    _sponge_gate(whole, ref, "device")
    assert np.array_equal(nr.bits(_device_sponge(c, X, zi, zm)), nr.bits(whole))
    for lo, hi in ((0, 5), (5, c.nens), (40, 41)):
        part = _device_sponge(c, _shard(X, lo, hi), _shard(zi, lo, hi), _shard(zm, lo, hi))
        assert np.array_equal(nr.bits(part), nr.bits(_shard(whole, lo, hi))), (lo, hi)


def _device_perturb(T, ids, magnitude, check_dirty=False):
    import torch
    from pam_amd import PamCoupler, modules
    T, ids = np.array(T), np.array(ids)
    nz, ny, nx, nens = T.shape
    coupler = PamCoupler("cuda:0")
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(nx * 500.0, ny * 500.0, np.linspace(0, 12000.0, nz + 1))
    coupler.add_tracer("water_vapor", "", True, True)
    dm = coupler.get_data_manager_device_readwrite()
    dm.get("temp").copy_(torch.from_numpy(T))
    keep = []
    dirty = coupler.run_module("perturb_temperature", lambda cp: keep.append(modules.perturb_temperature(cp, ids, magnitude)))
    torch.cuda.synchronize()
    if check_dirty:
        assert sorted(dirty) == ["temp"]
    return dm.get("temp", readonly=True).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", nc.PERTURB_IDS)
def test_gpu_perturb_named_case_is_inside_the_gate_in_every_cell(name):
    ref = nc.perturb_reference(name)
    got = _device_perturb(ref["T"], ref["ids"], ref["case"].magnitude, check_dirty=True)
    _perturb_gate(got, ref, "device")
    if ref["case"].nz // 4 and ref["case"].nx * ref["case"].ny > 1:
        assert np.abs(got - ref["T"]).max() > 0.1 * ref["case"].magnitude


@pytest.mark.gpu
def test_gpu_perturb_is_deterministic_and_member_shards_equal_the_whole_call():
    ref = nc.perturb_reference(nc.PERTURB_RAGGED)
    c, T, ids = ref["case"], ref["T"], ref["ids"]
    whole = _device_perturb(T, ids, c.magnitude, check_dirty=True)
    _perturb_gate(whole, ref, "device")
    assert np.array_equal(nr.bits(_device_perturb(T, ids, c.magnitude)), nr.bits(whole))
    for lo, hi in ((0, 5), (5, c.nens), (40, 41)):
        part = _device_perturb(_shard(T, lo, hi), np.ascontiguousarray(ids[lo:hi]), c.magnitude)
        assert np.array_equal(nr.bits(part), nr.bits(_shard(whole, lo, hi))), (lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", nc.BROADCAST, ids=nc.BROADCAST_IDS)
def test_gpu_broadcast_copies_bits_and_the_dry_density_variant_one_field(shape):
    import torch
    from oracle import awfl_oracle as ao
    from pam_amd import PamCoupler, modules
    nens, nx, ny, nz = shape
    crm, gcm = nc.broadcast_state(*shape)
    coupler = PamCoupler("cuda:0")
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(nx * 500.0, ny * 500.0, np.linspace(0, 12000.0, nz + 1))
    coupler.add_tracer("water_vapor", "", True, True)
    dm = coupler.get_data_manager_device_readwrite()
    for n, a in list(zip(ao.BROADCAST_GCM, gcm)) + list(zip(ao.BROADCAST_CRM, crm)):
        dm.get(n).copy_(torch.from_numpy(a))
    cb, gb = [nr.bits(c) for c in crm], [nr.bits(g) for g in gcm]

    def read():
        torch.cuda.synchronize()
        return [nr.bits(dm.get(n, readonly=True).cpu().numpy()) for n in ao.BROADCAST_CRM]
    for f, b in enumerate(read()):          # the upload itself keeps every bit, canaries and special values
        assert np.array_equal(b, cb[f])
    dirty = coupler.run_module("broadcast", modules.broadcast_initial_gcm_column_dry_density)
    assert "density_dry" in dirty and "temp" not in dirty and sorted(dirty) == ["density_dry"]
    for f, (g, w) in enumerate(zip(read(), nr.broadcast(cb, gb, 1))):
        assert np.array_equal(g, w), ("dry density", ao.BROADCAST_CRM[f])
    dirty = coupler.run_module("broadcast", modules.broadcast_initial_gcm_column)
    assert sorted(dirty) == sorted(ao.BROADCAST_CRM)
    for f, (g, w) in enumerate(zip(read(), nr.broadcast(cb, gb, 6))):
        assert np.array_equal(g, w), ("all six", ao.BROADCAST_CRM[f])
    for n, g in zip(ao.BROADCAST_GCM, gb):  # the columns are read, never written
        assert np.array_equal(nr.bits(dm.get(n, readonly=True).cpu().numpy()), g), n
