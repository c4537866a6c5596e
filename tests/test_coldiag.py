"""The CRM column diagnostics, everything that needs no GPU: the numpy restatement of the contract (tests/coldiag_ref.py) against a scalar
loop of its sentences; the device bodies under g++ (tests/emu/coldiag_emu.cpp) against the restatement bit for bit on every shape and named
case under every mapping of threads to work; members split over calls; the census of the branches the named cases reach; the mutants; the
C ABI's refusals; the boundary of the C++ header and the host program built from it."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import coldiag_ref as ref
import test_boundary_surface as tb
from coldiag_emu_harness import ASCENDING, BLOCK_SLOTS, FOUR_WALKERS, REVERSED, ROLLED, THREAD_SLOTS, EmuBackend
from pam_amd import capi
from tools import native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
HEADER = os.path.join(HOST, "modules", "column_diagnostics.h")
ALL_CONFIGS = ref.CONFIGS + ref.SLOT_CONFIGS


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement itself

def _scalar_case(case):
    """the contract's sentences, one float64 at a time"""
    f64 = np.float64
    P = {k: f64(v) for k, v in case["params"].items()}
    zint = case["zint"]
    out = {x: (None if a is None else a.copy()) for x, a in case["out0"].items()}
    with np.errstate(invalid="ignore", over="ignore"):
        for f, precip, factor in case["steps"]:
            nz, ny, nx, nens = f["rho_v"].shape
            c, i, frac = f.get("rho_c"), f.get("rho_i"), f.get("cldfrac")
            cloudy = c is not None or i is not None
            col = {x: np.zeros((ny * nx, nens)) for x in ref.OUT}
            for e in range(nens):
                for cc in range(ny * nx):
                    jy, ix = divmod(cc, nx)
                    pw, lwp, iwp = f64(0.0), f64(0.0), f64(0.0)
                    cwp, cf = [f64(0.0)] * 4, [f64(0.0)] * 4
                    for k in range(nz - 1, -1, -1):
                        dz = f64(zint[k + 1, e]) - f64(zint[k, e])
                        pw = pw + f64(f["rho_v"][k, jy, ix, e]) * dz
                        if not cloudy:
                            continue
                        terms = []
                        if c is not None:
                            w = f64(c[k, jy, ix, e]) * dz
                            lwp = lwp + w
                            terms.append(w)
                        if i is not None:
                            w = f64(i[k, jy, ix, e]) * dz
                            iwp = iwp + w
                            terms.append(w)
                        cw = terms[0] + terms[1] if len(terms) == 2 else terms[0]
                        if frac is not None:
                            cld = f64(frac[k, jy, ix, e])
                        else:
                            dens = [f64(a[k, jy, ix, e]) for a in (c, i) if a is not None]
                            cld = f64(1.0) if (dens[0] + dens[1] if len(dens) == 2 else dens[0]) > 0 else f64(0.0)
                        T, rd, rv = (f64(f[n][k, jy, ix, e]) for n in ("temp", "rho_d", "rho_v"))
                        p = (rd * P["R_d"]) * T + (rv * P["R_v"]) * T
                        cls = ref.LOW if p >= P["p_low"] else (ref.HGH if p < P["p_high"] else ref.MED)
                        for x in (0, cls):
                            cwp[x] = cwp[x] + cw
                            if cld > cf[x]:
                                cf[x] = cld
                    for x, name in enumerate(ref.COVERS):
                        col[name][cc, e] = cf[x] if cwp[x] > P["cwp_threshold"] else 0.0
                    col["lwp"][cc, e], col["iwp"][cc, e], col["pw"][cc, e] = lwp, iwp, pw
                    for n in ref.PRECIP:
                        if precip is not None and precip.get(n) is not None:
                            col[n][cc, e] = precip[n][jy, ix, e]
            r = f64(1.0) / f64(ny * nx)
            for x in ref.OUT:
                if out[x] is None:
                    continue
                for e in range(nens):
                    slots = [f64(0.0)] * 16
                    for cc in range(ny * nx):
                        slots[cc % 16] = slots[cc % 16] + f64(col[x][cc, e]) * r
                    tot = f64(0.0)
                    for s in range(16):
                        tot = tot + slots[s]
                    out[x][e] = f64(out[x][e]) + tot * f64(factor)
    return out


SCALAR_CASES = ("base", "low_high", "at_threshold", "ulp_above_threshold", "cldfrac", "c1_i0_liq", "c0_i1_no_table", "c0_i0_neither", "nan_temp",
                "nan_rho_c", "nan_cldfrac", "neg_zero", "factor_third", "two_steps")


@pytest.mark.parametrize("config", [c for c in ref.CONFIGS if c[3] <= 3], ids=ref.config_id)
def test_restatement_is_the_scalar_loop(config):
    for name in SCALAR_CASES:
        assert ref.results_differ(_scalar_case(ref.cases(config)[name]), ref.reference(config, name)) == [], name


def test_order_of_the_sums_is_neither_reversed_nor_pairwise():
    """the tests below pin the order of the two sums, not just their value: the column's walk bottom-up gives other bits of pw, and so does
    numpy's pairwise sum over the columns"""
    config = (5, 3, 7, 3)
    f, zint = ref.cases(config)["base"]["steps"][0][0], ref.cases(config)["base"]["zint"]
    down, _ = ref.column_values(f, zint, ref.PARAMS)
    up, _ = ref.column_values(f, zint, ref.PARAMS, "bottom_up")
    assert not ref.same_bits(down["pw"], up["pw"]) and np.allclose(down["pw"], up["pw"], rtol=1e-14, atol=0)
    slots = ref.column_mean(down["pw"])
    pairwise = (down["pw"].reshape(21, 3) * (1.0 / 21)).sum(axis=0)
    assert not ref.same_bits(slots, pairwise) and np.allclose(slots, pairwise, rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------------------------------------------
# the device bodies under g++ against the restatement

def _mappings(nens):
    """the kernel's own (ascending threads, 16 slot walkers per member in the kernel's member blocks or one walker per member), the scan in
    reversed thread order and with its levels one by one, and every mean mapping at two other block widths"""
    return [(ASCENDING, BLOCK_SLOTS, None), (ASCENDING, THREAD_SLOTS, None), (REVERSED, BLOCK_SLOTS, min(nens, 37)), (REVERSED, THREAD_SLOTS, None),
            (ROLLED, BLOCK_SLOTS, 1), (ROLLED, FOUR_WALKERS, None)]


@pytest.mark.parametrize("config", ALL_CONFIGS, ids=ref.config_id)
def test_emulation_matches_restatement_bit_for_bit(config):
    for name in ref.CASE_NAMES:
        want = ref.reference(config, name)
        for order, mapping, me in _mappings(config[3]):
            got = ref.run_case(EmuBackend(order, mapping, me), ref.cases(config)[name])
            assert ref.results_differ(got, want) == [], (name, order, mapping, me)


@pytest.mark.parametrize("config", [c for c in ref.CONFIGS if c[3] == 65], ids=ref.config_id)
def test_member_chunks_equal_the_whole_ensemble(config):
    """members in chunks of 1, 63 and 1 as separate calls: the whole ensemble's bits, in the restatement and in the emulation"""
    cuts = (slice(0, 1), slice(1, 64), slice(64, 65))
    for backend in (ref.RefBackend(), EmuBackend(ASCENDING, BLOCK_SLOTS), EmuBackend(REVERSED, THREAD_SLOTS)):
        for name in ref.CASE_NAMES:
            got = ref.join([ref.run_case(backend, ref.members(ref.cases(config)[name], sl)) for sl in cuts])
            assert ref.results_differ(got, ref.reference(config, name)) == [], name


# ------------------------------------------------------------------------------------------------------------------------------
# the named cases reach every branch

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_census_of_the_named_cases():
    seen = dict.fromkeys(["cloud_in_%s" % x for x in ref.COVERS] + ["clear_in_%s" % x for x in ref.COVERS] +
                         ["above_threshold", "below_threshold", "at_threshold", "nan_path", "nan_pressure_is_middle", "nan_cld_ignored",
                          "neg_zero_gives_plus_zero", "two_weights"] + ["absent_" + x for x in ref.OUT if x != "pw"], 0)
    slot_counts, cells_per_slot = set(), set()
    thr = ref.PARAMS["cwp_threshold"]
    for config in ALL_CONFIGS:
        nz, ny, nx, nens = config
        ncol = ny * nx
        slot_counts.add(min(ncol, 16))
        cells_per_slot |= {len(range(s, ncol, 16)) for s in range(16)}
        cs = ref.cases(config)
        for name in ["base"] + list(ref.CLASS_SETS):
            f = cs[name]["steps"][0][0]
            vals, cwp = ref.column_values(f, cs[name]["zint"], ref.PARAMS)
            for x, cover in enumerate(ref.COVERS):
                seen["cloud_in_" + cover] += int((vals[cover] > 0).sum())
                seen["clear_in_" + cover] += int((vals[cover] == 0).sum())
                seen["above_threshold"] += int((cwp[x] > thr).sum())
                seen["below_threshold"] += int(((cwp[x] < thr) & (cwp[x] > 0)).sum())
            if name in ref.CLASS_SETS:                         # condensate in exactly these classes
                for x, cover in enumerate(ref.COVERS[1:], start=1):
                    if x not in ref.CLASS_SETS[name]:
                        assert (cwp[x] == 0).all() and (vals[cover] == 0).all(), (name, cover)
        # exactly at the threshold: clear; one ulp above: the flag's 1.0
        for name, cover in (("at_threshold", 0.0), ("ulp_above_threshold", 1.0)):
            vals, cwp = ref.column_values(cs[name]["steps"][0][0], cs[name]["zint"], ref.PARAMS)
            assert cwp[0][0, 0, 0] == (thr if name == "at_threshold" else np.nextafter(thr, np.inf)) and vals["cldtot"][0, 0, 0] == cover, name
            assert vals["lwp"][0, 0, 0] == cwp[0][0, 0, 0]
        seen["at_threshold"] += 1
        # absent parts
        for has_c, has_i in ref.CONDENSATE:
            for form in ref.PRECIP_FORMS:
                name = "c%d_i%d_%s" % (int(has_c), int(has_i), form)
                if name not in cs:
                    continue
                got, base = ref.reference(config, name), ref.reference(config, "base")
                gone = {x for x in ref.OUT if got[x] is None}
                want = set() if (has_c or has_i) else set(ref.COVERS)
                want |= (set() if has_c else {"lwp"}) | (set() if has_i else {"iwp"})
                want |= {"both": set(), "liq": {"precip_ice"}, "ice": {"precip_liq"}, "neither": set(ref.PRECIP), "no_table": set(ref.PRECIP)}[form]
                assert gone == want, name
                for x in gone:
                    seen["absent_" + x] += 1
                assert ref.same_bits(got["pw"], base["pw"])
                if has_c:
                    assert ref.same_bits(got["lwp"], base["lwp"])
        # NaNs: a NaN temperature makes the level middle and reaches nothing else; a NaN in rho_c reaches lwp alone (its column's covers
        # are 0.0); a NaN cloud fraction is ignored
        k, j, i, e = ref.special_cell(config)
        nt, nc, nf, base = (ref.reference(config, n) for n in ("nan_temp", "nan_rho_c", "nan_cldfrac", "base"))
        assert all(np.isfinite(nt[x]).all() for x in ref.OUT)
        vals, _ = ref.column_values(cs["nan_temp"]["steps"][0][0], cs["nan_temp"]["zint"], ref.PARAMS)
        if nz == 1:
            assert vals["cldmed"][j, i, e] == 1.0 and vals["cldlow"][j, i, e] == 0.0 and vals["cldhgh"][j, i, e] == 0.0
            seen["nan_pressure_is_middle"] += 1
        assert np.argwhere(np.isnan(nc["lwp"])).tolist() == [[e]] and all(np.isfinite(nc[x]).all() for x in ref.OUT if x != "lwp")
        vals, _ = ref.column_values(cs["nan_rho_c"]["steps"][0][0], cs["nan_rho_c"]["zint"], ref.PARAMS)
        assert vals["cldtot"][j, i, e] == 0.0
        seen["nan_path"] += 1
        assert all(np.isfinite(nf[x]).all() for x in ref.OUT)
        seen["nan_cld_ignored"] += 1
        nzr = ref.reference(config, "neg_zero")
        assert all((_bits(cs["neg_zero"]["out0"][x]) == 0x8000000000000000).all() and (_bits(nzr[x]) == 0).all() for x in ref.OUT)
        seen["neg_zero_gives_plus_zero"] += 1
        fz = ref.reference(config, "factor_zero")
        assert all(ref.same_bits(fz[x], cs["factor_zero"]["out0"][x] + 0.0) for x in ref.OUT)
        assert [round(fac / ref.FACTOR) for _, _, fac in cs["two_steps"]["steps"]] == [3, 1]
        seen["two_weights"] += 1
    assert all(v >= 1 for v in seen.values()), seen
    assert slot_counts == set(range(1, 17)), slot_counts             # every number of occupied slots
    assert {0, 1, 2, 4} <= cells_per_slot, cells_per_slot            # empty slots, one cell, a ragged last round, full rounds


# ------------------------------------------------------------------------------------------------------------------------------
# mutants of the restatement: each is caught by a named case

MUTANT_CONFIG = (5, 3, 7, 65)    # 21 columns: 1/21 is not exact, so WHERE the scaling happens shows; five levels, so the walk's direction does
CAUGHT_BY = {"bottom_up": ("base", "pw"), "ge_threshold": ("at_threshold", "cldtot"), "classes_swapped": ("base", "cldlow"),
             "scale_after_sum": ("base", "pw"), "fma": ("factor_third", "pw")}


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_caught(mutant):
    name, expect = CAUGHT_BY[mutant]
    got = ref.run_case(ref.RefBackend(mutant), ref.cases(MUTANT_CONFIG)[name])
    bad = ref.results_differ(got, ref.reference(MUTANT_CONFIG, name))
    assert expect in bad, (mutant, bad)


def test_no_mutant_is_the_restatement():
    assert ref.results_differ(ref.run_case(ref.RefBackend(None), ref.cases(MUTANT_CONFIG)["base"]), ref.reference(MUTANT_CONFIG, "base")) == []
    assert set(CAUGHT_BY) == set(ref.MUTANTS)


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI: the symbols; refusals before any device is asked for

NEW_SYMBOLS = ("pam_amd_column_diagnostics", "pam_amd_column_diagnostics_debug_mapping")


def test_entry_points_are_exported_and_declared_and_the_abi_stays_5():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    assert lib.pam_amd_awfl_abi_version() == 5


def _table(*ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


A = [(i + 1) << 32 for i in range(40)]      # invented addresses 2^32 bytes apart, far more than any array of these sizes; never dereferenced
GOOD = dict(nens=4, nx=4, ny=4, nz=4, fields=A[0:6], zint=A[6], precip=A[7:9], R_d=287.0, R_v=461.0, p_low=70000.0, p_high=40000.0, thr=1e-3,
            out=A[9:18], factor=0.1)


def _call(lib, **kw):
    a = dict(GOOD, **kw)
    tab = lambda v: None if v is None else _table(*v)
    return lib.pam_amd_column_diagnostics(a["nens"], a["nx"], a["ny"], a["nz"], tab(a["fields"]), a["zint"], tab(a["precip"]), a["R_d"], a["R_v"],
                                          a["p_low"], a["p_high"], a["thr"], tab(a["out"]), a["factor"], None)


def _but(table, **kw):
    vals = list(table)
    for i, v in kw.items():
        vals[int(i[1:])] = v
    return vals


def test_entry_point_rejects_bad_arguments_before_touching_a_device():
    lib = capi.load()
    cells, F, O, PR = 4 * 4 * 4 * 4 * 8, GOOD["fields"], GOOD["out"], GOOD["precip"]
    bad = [dict(nens=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=1 << 16, ny=1 << 15), dict(nz=65536),
           dict(fields=None), dict(out=None), dict(zint=None),
           dict(fields=_but(F, f0=None)), dict(fields=_but(F, f1=None)), dict(fields=_but(F, f2=None)),
           dict(fields=_but(F, f3=None)),                              # lwp without rho_c
           dict(out=_but(O, o4=None)),                                 # rho_c without lwp
           dict(fields=_but(F, f4=None)), dict(out=_but(O, o5=None)),
           dict(precip=_but(PR, p0=None)), dict(out=_but(O, o7=None)), dict(precip=_but(PR, p1=None)), dict(out=_but(O, o8=None)),
           dict(precip=None),                                          # a NULL table: both absent, their outputs are not
           dict(precip=None, out=_but(O, o7=None)),
           dict(out=_but(O, o0=None)), dict(out=_but(O, o2=None)), dict(out=_but(O, o3=None)),      # a cover missing with condensate there
           dict(fields=_but(F, f3=None, f4=None), out=_but(O, o4=None, o5=None)),                   # covers given with no condensate
           dict(fields=_but(F, f3=None, f4=None), out=_but(O, o0=None, o1=None, o2=None, o4=None, o5=None)),
           dict(out=_but(O, o6=None)),
           dict(R_d=math.nan), dict(R_v=math.inf), dict(p_low=math.nan), dict(p_high=-math.inf), dict(factor=math.nan), dict(factor=math.inf),
           dict(p_low=40000.0, p_high=40000.5),
           dict(thr=-1e-9), dict(thr=math.nan),
           dict(out=_but(O, o6=A[0])),                                 # an output on an input
           dict(out=_but(O, o6=A[0] + cells - 8)),                     # on its last element
           dict(out=_but(O, o0=A[6] + 8 * 19)),                        # on the last element of zint
           dict(out=_but(O, o7=A[8] + 8)),                             # inside a precipitation array
           dict(out=_but(O, o1=A[9] + 8))]                             # two outputs one element apart
    for i, kw in enumerate(bad):
        assert _call(lib, **kw) == -1, (i, kw)                         # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert b"column_diagnostics" in lib.pam_amd_awfl_last_error(), (i, kw)
    for mapping in (-1, 3):
        assert lib.pam_amd_column_diagnostics_debug_mapping(mapping) == -1
        assert b"column_diagnostics" in lib.pam_amd_awfl_last_error()


def test_valid_arguments_get_past_validation():
    """the same tables unchanged, at the limits, and with the absent parts NULL: whatever comes back, it is not EINVAL (without a device
    PAM_AMD_ENOGPU; the launch itself is the GPU tests' business and is not made here where a device exists)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: a launch on invented addresses is not to be made")
    lib = capi.load()
    F, O = GOOD["fields"], GOOD["out"]
    assert _call(lib) == -2
    assert _call(lib, p_low=40000.0, p_high=40000.0, thr=0.0, factor=0.0) == -2
    assert _call(lib, fields=_but(F, f3=None, f4=None, f5=None), precip=None, out=[None] * 6 + [O[6], None, None]) == -2
    assert _call(lib, fields=_but(F, f4=None), precip=_but(GOOD["precip"], p1=None), out=_but(O, o5=None, o8=None)) == -2


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
    assert "[--column-diag PATH]" in text and "modules::column_diagnostics_init" in text


def test_header_names_the_entries_options_and_signatures_of_the_contract():
    text = tb._strip_comments(open(HEADER).read())
    for s in ['"diag_%s"' % x for x in ref.OUT] + ['"crm_diag_p_low"', '"crm_diag_p_high"', '"crm_diag_cwp_threshold"', '"R_d"', '"R_v"', '"cldfrac"',
                                                   '"cloud_liquid"', '"cloud_water"', '"ice"', '"density_dry"', '"water_vapor"', '"precl"',
                                                   '"precip_liq_surf_out"', '"precip_ice_surf_out"', '"vertical_interface_height"']:
        assert s in text, s
    n = tb._norm(text)
    assert "inlinevoidcolumn_diagnostics_init(PamCoupler&coupler){" in n
    assert "inlinevoidcolumn_diagnostics(PamCoupler&coupler,realweight=1){" in n
    assert "realfactor=crm_dt/gcm_dt*weight;" in n                       # time_average_accumulate's convention
    assert '"crm_diag_p_low",70000.' in n and '"crm_diag_p_high",40000.' in n and '"crm_diag_cwp_threshold",1.e-3' in n


def test_python_layer_has_the_signatures_of_the_contract():
    import inspect
    from pam_amd import modules
    assert inspect.signature(modules.column_diagnostics).parameters["weight"].default == 1
    assert list(inspect.signature(modules.column_diagnostics_init).parameters) == ["coupler"]
    assert modules.COLUMN_DIAGNOSTICS == tuple("diag_" + x for x in ref.OUT)
    assert dict(modules.COLUMN_DIAGNOSTICS_DEFAULTS) == {"crm_diag_p_low": 70000.0, "crm_diag_p_high": 40000.0, "crm_diag_cwp_threshold": 1.0e-3}


def cxx_program():
    """tests/cxx/column_diag, built the way the examples' driver is built (no device is needed to build it)"""
    return native_build.cxx_program("column_diag")


def test_header_compiles_into_a_host_program():
    """the program builds against the header and the library and, given no arguments, leaves with its usage status before any HIP call"""
    r = subprocess.run([cxx_program()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
