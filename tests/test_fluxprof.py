"""The CRM flux profiles, everything that needs no GPU: the numpy restatement of the contract (tests/fluxprof_ref.py) against a scalar loop
of its sentences and against an exact value; the device bodies under g++ (tests/emu/fluxprof_emu.cpp) against the restatement bit for bit
on every shape and named case under every mapping of threads to work; members split over calls; the census of the branches the named cases
reach; the mutants; the C ABI's refusals; the boundary of the C++ header and the host program built from it."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fluxprof_ref as ref
import test_boundary_surface as tb
from fluxprof_emu_harness import KERNEL, ONE_WALKER, REVERSED, EmuBackend
from pam_amd import capi
from tools import native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
HEADER = os.path.join(HOST, "modules", "flux_profiles.h")
ALL_CONFIGS = ref.CONFIGS + ref.SLOT_CONFIGS


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement itself

def _scalar_case(case):
    """the contract's sentences, one float64 at a time"""
    f64 = np.float64
    qc = f64(case["qc"])
    out = {x: (None if a is None else a.copy()) for x, a in case["out0"].items()}
    with np.errstate(all="ignore"):
        for f, factor in case["steps"]:
            nz, ny, nx, nens = f["rho_d"].shape
            c, i = f.get("rho_c"), f.get("rho_i")
            ncol = ny * nx
            r = f64(1.0) / f64(ncol)
            for k in range(nz):
                for e in range(nens):
                    def cell(cc):
                        jy, ix = divmod(cc, nx)
                        at = lambda n: f64(f[n][k, jy, ix, e])
                        rho = at("rho_d") + at("rho_v")
                        w = at("wvel")
                        wat = at("rho_v")
                        if c is not None:
                            wat = wat + at("rho_c")
                        if i is not None:
                            wat = wat + at("rho_i")
                        cloudy = False
                        if c is not None or i is not None:
                            cond = at("rho_c") + at("rho_i") if (c is not None and i is not None) else (at("rho_c") if c is not None else at("rho_i"))
                            cloudy = bool(cond > qc * rho)
                        return dict(m=rho * w, temp=at("temp"), q=wat / rho, uvel=at("uvel"), vvel=at("vvel"), wvel=w), cloudy, bool(w > 0)
                    names = ["mcup", "mcdn", "mcuup", "mcudn", "cld"] + ["A_" + n for n in ("m", "temp", "q", "uvel", "vvel", "wvel")] + \
                            ["Bm_" + n for n in ("temp", "q", "uvel", "vvel")] + ["B_" + n for n in ("uvel", "vvel", "wvel")]
                    assert len(names) == 18
                    slots = {n: [f64(0.0)] * 16 for n in names}
                    shift, _, _ = cell(0)
                    for cc in range(ncol):
                        x, cloudy, up = cell(cc)
                        s = cc % 16

                        def add(n, v):
                            slots[n][s] = slots[n][s] + v * r
                        add(("mcup" if up else "mcdn") if cloudy else ("mcuup" if up else "mcudn"), x["m"])
                        if cloudy:
                            add("cld", f64(1.0))
                        d = {n: x[n] - shift[n] for n in x}
                        for n in d:
                            add("A_" + n, d[n])
                        for n in ("temp", "q", "uvel", "vvel"):
                            add("Bm_" + n, d["m"] * d[n])
                        for n in ("uvel", "vvel", "wvel"):
                            add("B_" + n, d[n] * d[n])
                    tot = {}
                    for n in names:
                        a = f64(0.0)
                        for s in range(16):
                            a = a + slots[n][s]
                        tot[n] = a
                    val = {n: tot[n] for n in ("mcup", "mcdn", "mcuup", "mcudn", "cld")}
                    for name, n in zip(ref.FLUXES, ("temp", "q", "uvel", "vvel")):
                        val[name] = tot["Bm_" + n] - tot["A_m"] * tot["A_" + n]
                    var = []
                    for n in ("uvel", "vvel", "wvel"):
                        v = tot["B_" + n] - tot["A_" + n] * tot["A_" + n]
                        var.append(f64(0.0) if v < 0 else v)
                    val["tke"] = f64(0.5) * ((var[0] + var[1]) + var[2])
                    for n in ref.OUT:
                        if out[n] is not None:
                            out[n][k, e] = f64(out[n][k, e]) + val[n] * f64(factor)
    return out


@pytest.mark.parametrize("config", [c for c in ref.CONFIGS if c[3] <= 3], ids=ref.config_id)
def test_restatement_is_the_scalar_loop(config):
    for name in ref.CASE_NAMES:
        assert ref.results_differ(_scalar_case(ref.cases(config)[name]), ref.reference(config, name)) == [], name


def test_order_of_the_sums_is_neither_pairwise_nor_two_pass():
    """the tests below pin the order of the sums, not just their value: numpy's pairwise sum over the cells gives other bits of a mass
    flux, and a two-pass (mean first) covariance other bits of a flux, while both agree to 1e-12 relative"""
    config = (5, 3, 7, 3)
    f = ref.cases(config)["base"]["steps"][0][0]
    for k in range(config[0]):
        val = ref.level_values(f, k, ref.QC)
        x, cloudy, up = ref.cell_values(f, k, ref.QC)
        total = ((val["mcup"] + val["mcdn"]) + val["mcuup"]) + val["mcudn"]
        pairwise = (x["m"] * (1.0 / 21)).sum(axis=0)
        assert not ref.same_bits(ref.level_mean(x["m"]), pairwise)
        assert np.allclose(total, pairwise, rtol=1e-12, atol=0) and np.allclose(ref.level_mean(x["m"]), pairwise, rtol=1e-12, atol=0)
        for name, n in zip(ref.FLUXES, ("temp", "q", "uvel", "vvel")):
            two_pass = ((x["m"] - x["m"].mean(axis=0)) * (x[n] - x[n].mean(axis=0))).mean(axis=0)
            assert not ref.same_bits(val[name], two_pass), name
            assert np.allclose(val[name], two_pass, rtol=1e-12, atol=0), name


@pytest.mark.parametrize("ncol", [5, 17, 64, 333, 1024])
def test_one_pass_form_against_an_exact_value(ncol):
    """the fluxes and the variances of the restatement against np.longdouble, two-pass, from the per-cell float64 m and q as the contract
    rounds them.  The gate is the bound of the summation tree (ceil(ncol / 16) adds in a slot, 16 over the slots) plus the roundings of
    d, d d, (d d) r, A A and the final subtraction (6): gamma (mean|d_m d_x| + mean|d_m| mean|d_x|)"""
    config = (2, 1, ncol, 3)
    f = ref.base_fields(config, np.random.default_rng(ncol))
    gamma = (math.ceil(ncol / 16) + 16 + 6) * 2.0 ** -52
    L = np.longdouble
    worst = 0.0
    for k in range(2):
        val = ref.level_values(f, k, ref.QC)
        x, _, _ = ref.cell_values(f, k, ref.QC)
        d = {n: a.astype(L) - a[0].astype(L) for n, a in x.items()}
        pairs = [(name, "m", n) for name, n in zip(ref.FLUXES, ("temp", "q", "uvel", "vvel"))] + [(None, n, n) for n in ("uvel", "vvel", "wvel")]
        var = {}
        for name, a, b in pairs:
            exact = ((x[a].astype(L) - x[a].astype(L).mean(axis=0)) * (x[b].astype(L) - x[b].astype(L).mean(axis=0))).mean(axis=0)
            gate = gamma * (np.abs(d[a] * d[b]).mean(axis=0) + np.abs(d[a]).mean(axis=0) * np.abs(d[b]).mean(axis=0))
            if name is None:
                var[b] = (exact, gate)
                continue
            err = np.abs(val[name].astype(L) - exact)
            worst = max(worst, float((err / gate).max()))
            assert (err <= gate).all(), (name, k, err, gate)
        exact = L(0.5) * (var["uvel"][0] + var["vvel"][0] + var["wvel"][0])
        gate = L(0.5) * (var["uvel"][1] + var["vvel"][1] + var["wvel"][1]) + 3 * 2.0 ** -53 * exact
        err = np.abs(val["tke"].astype(L) - exact)
        worst = max(worst, float((err / gate).max()))
        assert (err <= gate).all(), ("tke", k, err, gate)
    print("ncol %d: largest error / gate %.3f" % (ncol, worst))


# ------------------------------------------------------------------------------------------------------------------------------
# the device bodies under g++ against the restatement

def _mappings(nens):
    """the kernel's own (16 slot walkers per member in blocks of min(nens, 64)), its threads in reversed order, one walker doing all 16
    slots, and 1 and 7 members per block"""
    return [(KERNEL, None), (REVERSED, None), (ONE_WALKER, None), (KERNEL, 1), (REVERSED, 7)]


@pytest.mark.parametrize("config", ALL_CONFIGS, ids=ref.config_id)
def test_emulation_matches_restatement_bit_for_bit(config):
    for name in ref.CASE_NAMES:
        want = ref.reference(config, name)
        for mapping, me in _mappings(config[3]):
            got = ref.run_case(EmuBackend(mapping, me), ref.cases(config)[name])
            assert ref.results_differ(got, want) == [], (name, mapping, me)


@pytest.mark.parametrize("config", [c for c in ref.CONFIGS if c[3] == 65], ids=ref.config_id)
def test_member_chunks_equal_the_whole_ensemble(config):
    """members in chunks of 1, 63 and 1 as separate calls: the whole ensemble's bits, in the restatement and in the emulation"""
    cuts = (slice(0, 1), slice(1, 64), slice(64, 65))
    for backend in (ref.RefBackend(), EmuBackend(KERNEL), EmuBackend(ONE_WALKER)):
        for name in ref.CASE_NAMES:
            got = ref.join([ref.run_case(backend, ref.members(ref.cases(config)[name], sl)) for sl in cuts])
            assert ref.results_differ(got, ref.reference(config, name)) == [], name


# ------------------------------------------------------------------------------------------------------------------------------
# the named cases reach every branch

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_census_of_the_named_cases():
    seen = dict.fromkeys(["at_threshold_is_clear", "ulp_above_is_cloudy", "zero_w_is_not_up", "nan_w_is_not_up", "nan_condensate_is_clear",
                          "nan_temp_reaches_flux_t_alone", "constant_level_gives_plus_zero", "variance_rounds_negative",
                          "neg_zero_gives_plus_zero", "two_weights"] + ["absent_" + x for x in ref.SAMPLED], 0)
    slot_counts, cells_per_slot = set(), set()
    for config in ALL_CONFIGS:
        nz, ny, nx, nens = config
        ncol = ny * nx
        slot_counts.add(min(ncol, 16))
        cells_per_slot |= {len(range(s, ncol, 16)) for s in range(16)}
        cs = ref.cases(config)
        k, j, i, e = ref.special(config)
        base = ref.reference(config, "base")
        f = cs["base"]["steps"][0][0]
        if ncol >= 16:                                       # each of the four classes is non-empty in at least half of the (k,e) pairs
            count = dict.fromkeys(("cu", "cd", "nu", "nd"), 0)
            for kk in range(nz):
                _, cloudy, up = ref.cell_values(f, kk, ref.QC)
                for n, mask in (("cu", cloudy & up), ("cd", cloudy & ~up), ("nu", ~cloudy & up), ("nd", ~cloudy & ~up)):
                    count[n] += int(mask.any(axis=0).sum())
            assert all(2 * v >= nz * nens for v in count.values()), (config, count)
        # all clear / all cloudy: the sampled sums of the other side are exactly 0.0, the cloud fraction 0 and (within the sum's rounding) 1
        clear, cloudy = ref.reference(config, "all_clear"), ref.reference(config, "all_cloudy")
        assert all((clear[x] == 0).all() for x in ref.SAMPLED) and (cloudy["mcuup"] == 0).all() and (cloudy["mcudn"] == 0).all()
        assert np.allclose(cloudy["cld"], ref.FACTOR, rtol=1e-14, atol=0)
        assert ref.same_bits(clear["flux_t"], base["flux_t"]) and ref.same_bits(clear["tke"], base["tke"])
        # exactly at the threshold: the level is clear; one ulp above: every cell of it is cloudy
        at, above = ref.reference(config, "at_threshold"), ref.reference(config, "ulp_above_threshold")
        assert at["cld"][k, e] == 0.0 and at["mcup"][k, e] == 0.0 and at["mcdn"][k, e] == 0.0
        seen["at_threshold_is_clear"] += 1
        assert np.isclose(above["cld"][k, e], ref.FACTOR, rtol=1e-14, atol=0) and above["mcuup"][k, e] == 0.0 and above["mcudn"][k, e] == 0.0
        seen["ulp_above_is_cloudy"] += 1
        # w = +-0.0: nothing is up -- the NaN of the special cell's m is in a not-up sum, the up sums are exactly 0.0
        wz = ref.reference(config, "w_zero")
        assert wz["mcup"][k, e] == 0.0 and wz["mcuup"][k, e] == 0.0 and (np.isnan(wz["mcdn"][k, e]) or np.isnan(wz["mcudn"][k, e]))
        seen["zero_w_is_not_up"] += 1
        nw = ref.reference(config, "nan_w")
        assert np.isfinite(nw["mcup"]).all() and np.isfinite(nw["mcuup"]).all() and np.isfinite(nw["cld"]).all()
        assert np.isnan(nw["mcdn"][k, e]) != np.isnan(nw["mcudn"][k, e]) and np.isnan(nw["tke"][k, e]) and np.isnan(nw["flux_t"][k, e])
        assert sum(int(np.isnan(nw[x]).sum()) for x in ref.OUT) == 6          # one sampled sum, the four fluxes and tke, at (k, e) alone
        seen["nan_w_is_not_up"] += 1
        nc = ref.reference(config, "nan_rho_c")
        assert all(np.isfinite(nc[x]).all() for x in ref.OUT if x != "flux_qt") and np.argwhere(np.isnan(nc["flux_qt"])).tolist() == [[k, e]]
        assert np.isfinite(nc["mcup"]).all() and ref.same_bits(nc["flux_t"], base["flux_t"])
        seen["nan_condensate_is_clear"] += 1
        nt = ref.reference(config, "nan_temp")
        assert all(np.isfinite(nt[x]).all() for x in ref.OUT if x != "flux_t") and np.argwhere(np.isnan(nt["flux_t"])).tolist() == [[k, e]]
        seen["nan_temp_reaches_flux_t_alone"] += 1
        cl = ref.reference(config, "constant_level")
        assert all((_bits(cl[x]) == 0).all() for x in ref.FLUXES + ("tke",))
        assert (cl["cld"] != 0).any() or nz * nens == 1
        seen["constant_level_gives_plus_zero"] += 1
        # B - A A < 0 before the clamp, found by the search of fluxprof_ref on every shape of at least five columns
        if ncol >= 5 and config in ref.CONFIGS:
            assert ref.NEGATIVE_FOUND[config], config
        if ref.NEGATIVE_FOUND[config]:
            g = cs["var_rounds_negative"]["steps"][0][0]
            pre = [dict() for _ in range(nz)]
            for kk in range(nz):
                ref.level_values(g, kk, ref.QC, preclamp=pre[kk])
            assert any((p["uvel"] < 0).any() for p in pre)
            assert (ref.reference(config, "var_rounds_negative")["tke"] >= 0).all()
            seen["variance_rounds_negative"] += 1
        # absent species
        for has_c, has_i in ref.CONDENSATE:
            got = ref.reference(config, "c%d_i%d" % (int(has_c), int(has_i)))
            gone = {x for x in ref.OUT if got[x] is None}
            assert gone == (set() if (has_c or has_i) else set(ref.SAMPLED))
            for x in gone:
                seen["absent_" + x] += 1
            assert ref.same_bits(got["flux_t"], base["flux_t"]) and ref.same_bits(got["tke"], base["tke"])
        assert ref.results_differ(ref.reference(config, "c1_i1"), base) == []
        nzr = ref.reference(config, "neg_zero")
        assert all((_bits(cs["neg_zero"]["out0"][x]) == 0x8000000000000000).all() and (_bits(nzr[x]) == 0).all() for x in ref.OUT)
        seen["neg_zero_gives_plus_zero"] += 1
        assert [round(fac / ref.FACTOR) for _, fac in cs["two_steps"]["steps"]] == [3, 1]
        seen["two_weights"] += 1
    assert all(v >= 1 for v in seen.values()), seen
    assert slot_counts == set(range(1, 17)), slot_counts             # every number of occupied slots
    assert {0, 1, 2, 4} <= cells_per_slot, cells_per_slot            # empty slots, one cell, a ragged last round, full rounds


# ------------------------------------------------------------------------------------------------------------------------------
# mutants of the restatement: each is caught by a named case

MUTANT_CONFIG = (5, 3, 7, 65)    # 21 columns: 1/21 is not exact and the slots hold one or two cells
CAUGHT_BY = {"ge_threshold": ("at_threshold", "cld"), "w_ge_zero": ("w_zero", "mcuup"), "shift_from_mean": ("base", "flux_t"),
             "q_over_rho_d": ("base", "flux_qt"), "no_clamp": ("var_rounds_negative", "tke"), "all_classes_add": ("base", "mcup"),
             "slots_reversed": ("base", "mcudn")}


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_caught(mutant):
    name, expect = CAUGHT_BY[mutant]
    got = ref.run_case(ref.RefBackend(mutant), ref.cases(MUTANT_CONFIG)[name])
    bad = ref.results_differ(got, ref.reference(MUTANT_CONFIG, name))
    assert expect in bad, (mutant, bad)


def test_no_mutant_is_the_restatement():
    for name in ref.CASE_NAMES:
        assert ref.results_differ(ref.run_case(ref.RefBackend(None), ref.cases(MUTANT_CONFIG)[name]), ref.reference(MUTANT_CONFIG, name)) == []
    assert set(CAUGHT_BY) == set(ref.MUTANTS)


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI: the symbol; refusals before any device is asked for

def test_entry_point_is_exported_and_declared_and_the_abi_stays_5():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    name = "pam_amd_flux_profiles"
    assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared
    assert lib.pam_amd_awfl_abi_version() == 5


def _table(*ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


A = [(i + 1) << 32 for i in range(40)]      # invented addresses 2^32 bytes apart, far more than any array of these sizes; never dereferenced
GOOD = dict(nens=4, nx=4, ny=4, nz=4, fields=A[0:8], qc=1.0e-5, out=A[8:18], factor=0.1)


def _call(lib, **kw):
    a = dict(GOOD, **kw)
    tab = lambda v: None if v is None else _table(*v)
    return lib.pam_amd_flux_profiles(a["nens"], a["nx"], a["ny"], a["nz"], tab(a["fields"]), a["qc"], tab(a["out"]), a["factor"], None)


def _but(table, **kw):
    vals = list(table)
    for i, v in kw.items():
        vals[int(i[1:])] = v
    return vals


def test_entry_point_rejects_bad_arguments_before_touching_a_device():
    lib = capi.load()
    cells, F, O = 4 * 4 * 4 * 4 * 8, GOOD["fields"], GOOD["out"]
    bad = [dict(nens=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=1 << 16, ny=1 << 15), dict(nz=65536),
           dict(fields=None), dict(out=None),
           dict(fields=_but(F, f0=None)), dict(fields=_but(F, f1=None)), dict(fields=_but(F, f4=None)), dict(fields=_but(F, f5=None)),
           dict(fields=_but(F, f6=None)), dict(fields=_but(F, f7=None)),
           dict(out=_but(O, o0=None)), dict(out=_but(O, o1=None)), dict(out=_but(O, o4=None)),     # a sampled output missing with condensate there
           dict(fields=_but(F, f3=None), out=_but(O, o0=None, o1=None, o4=None)),                  # cloud alone is a condensate
           dict(fields=_but(F, f2=None), out=_but(O, o4=None)),
           dict(fields=_but(F, f2=None, f3=None)),                                                 # sampled outputs given with no condensate
           dict(fields=_but(F, f2=None, f3=None), out=_but(O, o0=None, o1=None)),
           dict(fields=_but(F, f2=None, f3=None), out=_but(O, o0=None, o4=None)),
           dict(out=_but(O, o2=None)), dict(out=_but(O, o3=None)), dict(out=_but(O, o5=None)), dict(out=_but(O, o6=None)),
           dict(out=_but(O, o7=None)), dict(out=_but(O, o8=None)), dict(out=_but(O, o9=None)),
           dict(qc=-1e-9), dict(qc=math.nan), dict(qc=math.inf), dict(factor=math.nan), dict(factor=math.inf), dict(factor=-math.inf),
           dict(out=_but(O, o9=A[0])),                                 # an output on an input
           dict(out=_but(O, o9=A[7] + cells - 8)),                     # on its last element
           dict(out=_but(O, o0=A[2] + 8)),                             # inside the cloud field
           dict(out=_but(O, o5=A[8] + 8)),                             # two outputs one element apart
           dict(out=_but(O, o5=A[9] + 8 * 15))]                        # on the last element of another output
    for n, kw in enumerate(bad):
        assert _call(lib, **kw) == -1, (n, kw)                         # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert b"flux_profiles" in lib.pam_amd_awfl_last_error(), (n, kw)


def test_valid_arguments_get_past_validation():
    """the same tables unchanged, at the limits, and with the absent parts NULL: whatever comes back, it is not EINVAL (without a device
    PAM_AMD_ENOGPU; the launch itself is the GPU tests' business and is not made here where a device exists)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: a launch on invented addresses is not to be made")
    lib = capi.load()
    F, O = GOOD["fields"], GOOD["out"]
    assert _call(lib) == -2
    assert _call(lib, qc=0.0, factor=0.0) == -2
    assert _call(lib, nens=1, nx=1, ny=1, nz=1) == -2
    assert _call(lib, fields=_but(F, f2=None, f3=None), out=_but(O, o0=None, o1=None, o4=None)) == -2
    assert _call(lib, fields=_but(F, f3=None)) == -2
    assert _call(lib, fields=_but(F, f2=None)) == -2
    assert _call(lib, out=_but(O, o5=A[8] + 8 * 16)) == -2             # two outputs back to back


# ------------------------------------------------------------------------------------------------------------------------------
# the boundary of the C++ header, and the host program built from it

def test_header_calls_only_members_the_reference_has():
    coupler, dm = tb._used_members(open(HEADER).read())
    assert {"get_option", "option_exists", "set_option"} <= coupler and {"get", "register_and_allocate", "entry_exists", "get_shape"} <= dm, (coupler, dm)
    assert coupler <= tb.REF_COUPLER, sorted(coupler - tb.REF_COUPLER)
    assert dm <= tb.REF_DM, sorted(dm - tb.REF_DM)
    ours = tb._declared(os.path.join(HOST, "pam_coupler.h"))
    assert (coupler | dm) <= ours, sorted((coupler | dm) - ours)


def test_driver_still_calls_only_members_the_reference_has():
    text = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    coupler, dm = tb._used_members(text)
    assert coupler <= tb.REF_COUPLER and dm <= tb.REF_DM
    assert "[--column-diag PATH] [--flux-profiles PATH]" in text and "modules::flux_profiles_init" in text


def test_header_names_the_entries_options_and_signatures_of_the_contract():
    text = tb._strip_comments(open(HEADER).read())
    for s in ['"prof_%s"' % x for x in ref.OUT] + ['"crm_prof_qc_threshold"', '"crm_dt"', '"gcm_physics_dt"', '"micro"', '"cloud_liquid"',
                                                   '"cloud_water"', '"ice"', '"density_dry"', '"water_vapor"', '"temp"', '"uvel"', '"vvel"',
                                                   '"wvel"']:
        assert s in text, s
    n = tb._norm(text)
    assert "inlinevoidflux_profiles_init(PamCoupler&coupler){" in n
    assert "inlinevoidflux_profiles(PamCoupler&coupler,realweight=1){" in n
    assert "realfactor=crm_dt/gcm_dt*weight;" in n                       # time_average_accumulate's convention
    assert '"crm_prof_qc_threshold",1.e-5' in n


def test_python_layer_has_the_signatures_of_the_contract():
    import inspect
    from pam_amd import modules
    assert inspect.signature(modules.flux_profiles).parameters["weight"].default == 1
    assert list(inspect.signature(modules.flux_profiles).parameters) == ["coupler", "weight"]
    assert list(inspect.signature(modules.flux_profiles_init).parameters) == ["coupler"]
    assert modules.FLUX_PROFILES == tuple("prof_" + x for x in ref.OUT)
    assert modules.FLUX_PROFILES_DEFAULTS == (("crm_prof_qc_threshold", 1.0e-5),)


def cxx_program():
    """tests/cxx/flux_profiles, built the way the examples' driver is built (no device is needed to build it)"""
    return native_build.cxx_program("flux_profiles")


def test_header_compiles_into_a_host_program():
    """the program builds against the header and the library and, given no arguments, leaves with its usage status before any HIP call"""
    r = subprocess.run([cxx_program()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
