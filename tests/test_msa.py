"""CRM mean-state acceleration, everything that needs no GPU: the numpy restatement of the contract (tests/msa_ref.py) against a
scalar loop; the order of its sums pinned against the serial and the pairwise order; the device bodies under g++
(tests/emu/msa_emu.cpp) against the restatement bit for bit on every shape and named case; the census of the branches the named
cases reach; the mutants; conservation within its derived bound; the step clock; the C ABI's refusals; the adaptor's boundary."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import msa_ref as ref
import test_boundary_surface as tb
from msa_emu_harness import EmuBackend
from pam_amd import capi
from pam_amd.capi import PamAmdError
from pam_amd.modules import MsaClock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement itself

def _scalar_level_mean(f, scale):
    """the contract's sentence, one Python float at a time"""
    nz, ncol, nens = f.shape
    r = 1.0 / ncol
    out = np.empty((nz, nens))
    for k in range(nz):
        for e in range(nens):
            slots = [0.0] * 16
            for c in range(ncol):
                v = float(f[k, c, e])
                slots[c % 16] = slots[c % 16] + (v * r if scale else v)
            tot = 0.0
            for s in range(16):
                tot = tot + slots[s]
            out[k, e] = tot
    return out


@pytest.mark.parametrize("shape", [((4, 1, 5), 3), ((5, 1, 17), 3), ((3, 4, 5), 1), ((6, 8, 8), 3)], ids=ref.shape_id)
def test_restatement_is_the_scalar_loop(shape):
    st = ref.cases(shape)["base"]["after"]
    for name in ("temp", "uvel", "water_vapor"):
        assert ref.same_bits(ref.level_mean(st[name]), _scalar_level_mean(st[name], True)), name
        assert ref.same_bits(ref.level_sum(st[name]), _scalar_level_mean(st[name], False)), name


def test_restatement_apply_is_the_scalar_loop():
    shape = ((5, 1, 17), 3)
    case = ref.cases(shape)["base"]
    got = ref.reference(shape, "base")
    st, tend, a = case["after"], got["tend"], case["a"]
    nz, ncol, nens = st["temp"].shape
    modes = set()
    for k in range(nz):
        for e in range(nens):
            d_t, d_q = a * float(tend["t"][k, e]), a * float(tend["q"][k, e])
            vp = [float(st["water_vapor"][k, c, e]) + d_q for c in range(ncol)]
            pos, neg = [0.0] * 16, [0.0] * 16
            for c in range(ncol):
                pos[c % 16] = pos[c % 16] + (vp[c] if vp[c] > 0 else 0.0)
                neg[c % 16] = neg[c % 16] + (vp[c] if vp[c] < 0 else 0.0)
            P = N = 0.0
            for s in range(16):
                P, N = P + pos[s], N + neg[s]
            for c in range(ncol):
                if not N < 0:
                    want, mode = vp[c], 0
                elif P + N > 0:
                    want, mode = (vp[c] if vp[c] > 0 else 0.0) * (1.0 + N / P), 1
                else:
                    want, mode = 0.0, 2
                modes.add(mode)
                assert got["fields"]["water_vapor"][k, c, e] == want
                assert got["fields"]["temp"][k, c, e] == float(st["temp"][k, c, e]) + d_t
    assert modes == {0, 1, 2}


@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[0][1] * s[0][2] >= 17 and s[1] == 3], ids=ref.shape_id)
def test_slot_order_is_neither_the_serial_nor_the_pairwise_order(shape):
    """on the mixed-sign winds the contract's order gives other bits than a serial walk and than numpy's pairwise sum: the tests
    below pin the order, not just the value"""
    u = ref.cases(shape)["base"]["after"]["uvel"]
    r = 1.0 / u.shape[1]
    slots = ref.level_mean(u)
    serial = np.zeros_like(slots)
    for c in range(u.shape[1]):
        serial = serial + u[:, c, :] * r
    pairwise = np.sum(u * r, axis=1)
    assert not ref.same_bits(slots, serial)
    assert not ref.same_bits(slots, pairwise)
    assert np.allclose(slots, serial, rtol=0, atol=1e-12 * np.abs(u).max())


# ------------------------------------------------------------------------------------------------------------------------------
# the device bodies under g++ against the restatement

@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape):
    """every named case; the kernel's member blocks (min(nens, 64)) and two other widths: the bits do not depend on the mapping"""
    nens = shape[1]
    for name in ref.CASE_NAMES:
        want = ref.reference(shape, name)
        for me in sorted({min(nens, 64), min(nens, 37), 1}):
            got = ref.run_case(EmuBackend(me), ref.cases(shape)[name])
            assert ref.results_differ(got, want) == [], (name, me)


# ------------------------------------------------------------------------------------------------------------------------------
# the named cases reach every branch

def test_census_of_the_named_cases():
    seen = dict.fromkeys(("clean", "filled", "zeroed", "equal_no_cease", "ulp_above_ceases", "nan_ceases", "no_cloud", "no_ice",
                          "vapour_only", "uv_untouched", "flag_set_writes_nothing", "a_zero_writes_nothing"), 0)
    for shape in ref.SHAPES:
        cs = ref.cases(shape)
        r = ref.reference(shape, "base")
        assert r["cease"] == 0
        vp = cs["base"]["after"]["water_vapor"] + (cs["base"]["a"] * r["tend"]["q"])[:, None, :]
        _, _, mode = ref.vapor_levels(vp)
        seen["clean"] += int((mode == 0).sum())
        seen["filled"] += int((mode == 1).sum())
        seen["zeroed"] += int((mode == 2).sum())
        wv = r["fields"]["water_vapor"]
        assert (wv >= 0).all() and (wv[np.broadcast_to((mode == 2)[:, None, :], wv.shape)] == 0).all()

        eq = ref.reference(shape, "ttend_equal")
        assert (np.abs(eq["tend"]["t"]) == cs["ttend_equal"]["max_ttend"]).sum() >= 1
        seen["equal_no_cease"] += eq["cease"] == 0
        up = ref.reference(shape, "ttend_one_ulp_above")
        top = np.abs(up["tend"]["t"]).max()
        assert np.nextafter(cs["ttend_one_ulp_above"]["max_ttend"], np.inf) == top
        seen["ulp_above_ceases"] += up["cease"] == 1
        nan = ref.reference(shape, "nan_in_temp")
        assert np.isnan(nan["tend"]["t"]).sum() == 1
        seen["nan_ceases"] += nan["cease"] == 1
        for name in ("ttend_one_ulp_above", "nan_in_temp", "flag_already_set", "accel_factor_zero"):      # nothing is written
            assert ref.results_differ(dict(ref.reference(shape, name), fields=cs[name]["after"]), ref.reference(shape, name)) == [], name
        seen["flag_set_writes_nothing"] += ref.reference(shape, "flag_already_set")["cease"] == 1
        seen["a_zero_writes_nothing"] += ref.reference(shape, "accel_factor_zero")["cease"] == 0
        for name, gone in (("no_cloud", ("cloud",)), ("no_ice", ("ice",)), ("vapour_only", ("cloud", "ice"))):
            got = ref.reference(shape, name)
            assert all(got["fields"][g] is None for g in gone)
            assert not ref.same_bits(got["tend"]["q"], r["tend"]["q"]), name       # the absent species is really left out
            seen[name] += 1
        off = ref.reference(shape, "accel_uv_off")
        assert ref.same_bits(off["fields"]["uvel"], cs["base"]["after"]["uvel"]) and ref.same_bits(off["fields"]["vvel"], cs["base"]["after"]["vvel"])
        assert not ref.same_bits(r["fields"]["uvel"], cs["base"]["after"]["uvel"])
        assert ref.same_bits(off["fields"]["temp"], r["fields"]["temp"])
        seen["uv_untouched"] += 1
        for f in ("cloud", "ice"):                                                 # never written
            assert ref.same_bits(r["fields"][f], cs["base"]["after"][f])
    assert all(v >= 1 for v in seen.values()), seen
    n = len(ref.SHAPES)
    assert all(seen[k] == n for k in ("equal_no_cease", "ulp_above_ceases", "nan_ceases", "flag_set_writes_nothing", "a_zero_writes_nothing")), seen


# ------------------------------------------------------------------------------------------------------------------------------
# mutants of the restatement: each is caught by a named case

CAUGHT_BY = {"slots_descending": "base", "scale_after_sum": "base", "cease_ge": "ttend_equal", "cloud_incremented": "base",
             "factor_minus": "base"}


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_caught(mutant):
    shape = ((5, 1, 17), 3)          # ncol no power of two: 1/ncol is not exact, so WHERE the scaling happens shows
    name = CAUGHT_BY[mutant]
    got = ref.run_case(ref.RefBackend(mutant), ref.cases(shape)[name])
    bad = ref.results_differ(got, ref.reference(shape, name))
    assert bad, mutant
    expect = {"slots_descending": "save_u", "scale_after_sum": "save_t", "cease_ge": "cease", "cloud_incremented": "cloud",
              "factor_minus": "water_vapor"}[mutant]
    assert expect in bad, (mutant, bad)


def test_no_mutant_is_the_restatement():
    shape = ((5, 1, 17), 3)
    assert ref.results_differ(ref.run_case(ref.RefBackend(None), ref.cases(shape)["base"]), ref.reference(shape, "base")) == []
    assert set(CAUGHT_BY) == set(ref.MUTANTS)


# ------------------------------------------------------------------------------------------------------------------------------
# conservation: a derived bound

@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_level_means_move_by_the_increment_within_the_rounding_bound(shape):
    """On levels that keep or fill their vapour, the level mean after the apply is the level mean before it plus the increment:
    |M(T_out) - (M(T) + d_T)| <= 2 (ncol + 3) u M(|T_out|).  Every one of the ncol products and adds of a mean rounds once (relative
    u each, at most ncol + 1 roundings along any path through slot and fold), on both sides, plus the roundings of d, of T + d and
    of the right-hand side's add: 2 (ncol + 3) u covers them to first order.  The same for the vapour against M(v')."""
    case = ref.cases(shape)["base"]
    r = ref.reference(shape, "base")
    st, a = case["after"], case["a"]
    ncol = st["temp"].shape[1]
    bound = 2 * (ncol + 3) * U
    d_t, d_q = a * r["tend"]["t"], a * r["tend"]["q"]
    t_out = r["fields"]["temp"]
    err = np.abs(ref.level_mean(t_out) - (ref.level_mean(st["temp"]) + d_t))
    lim = bound * ref.level_mean(np.abs(t_out))
    print("temp: worst fraction of the bound %.3f" % (err / lim).max())
    assert (err <= lim).all()
    vp = st["water_vapor"] + d_q[:, None, :]
    _, _, mode = ref.vapor_levels(vp)
    keep = mode != 2
    v_out = r["fields"]["water_vapor"]
    err = np.abs(ref.level_mean(v_out) - ref.level_mean(vp))
    lim = bound * ref.level_mean(np.abs(v_out))
    print("vapour: worst fraction of the bound %.3f" % (err[keep] / lim[keep]).max())
    assert keep.any() and (err[keep] <= lim[keep]).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the step clock

def _run_clock(nstop, a, cease_at=None):
    """-> weights of the steps; cease_at: the (1-based) step whose accelerate raises the flag"""
    clock, weights = MsaClock(nstop, a), []
    while not clock.done():
        step = len(weights) + 1
        cease = clock.accelerating() and step == cease_at
        weights.append(clock.advance(cease))
        assert clock.count == sum(weights) <= nstop
        assert len(weights) <= nstop
    return weights


def test_clock_without_cease_takes_a_third_of_the_steps():
    assert _run_clock(12, 2) == [3, 3, 3, 3]
    assert _run_clock(12, 0) == [1] * 12
    assert _run_clock(12, 1) == [2] * 6
    assert _run_clock(12, 11) == [12]


@pytest.mark.parametrize("i", [1, 2, 3, 4])
def test_clock_cease_at_step_i(i):
    """steps before i count 3, step i and every later one count 1: (i - 1) + 12 - 3 (i - 1) steps in all, weights summing to nstop"""
    w = _run_clock(12, 2, cease_at=i)
    assert w == [3] * (i - 1) + [1] * (12 - 3 * (i - 1))
    assert len(w) == (i - 1) + 12 - 3 * (i - 1) and sum(w) == 12


def test_clock_never_accelerates_again_after_a_cease():
    clock = MsaClock(12, 2)
    assert clock.accelerating() and clock.advance(True) == 1
    while not clock.done():
        assert not clock.accelerating()
        assert clock.advance(False) == 1
    assert clock.count == 12


@pytest.mark.parametrize("nstop, a", [(10, 2), (12, 0.5), (12, -1), (12, math.nan), (12, math.inf), (0, 2), (2, 2)])
def test_clock_refuses_what_does_not_divide(nstop, a):
    with pytest.raises(PamAmdError):
        MsaClock(nstop, a)


def test_cpp_clock_is_the_python_clock():
    """the C++ twin, line by line: the same refusals, the same rule for the weight"""
    text = tb._strip_comments(open(os.path.join(HOST, "modules", "mean_state_acceleration.h")).read())
    body = text[text.index("class MsaClock"):text.index("struct MsaArrays_")]
    n = re.sub(r"\s+", "", body)
    assert "if(steps!=std::floor(steps)||steps>nstop||nstop%(int)steps!=0)endrun(" in n
    assert "if(cease)ceased_=true;intweight=accelerating()?per_step_:1;count_+=weight;returnweight;" in n
    assert "boolaccelerating()const{return!ceased_&&per_step_>1;}" in n
    assert "booldone()const{returncount_>=nstop_;}" in n


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI: refusals before any device is asked for; the symbols

NEW_SYMBOLS = ("pam_amd_msa_diagnose", "pam_amd_msa_tendencies", "pam_amd_msa_apply")


def test_entry_points_are_exported_and_declared_and_the_abi_stays_5():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    assert lib.pam_amd_awfl_abi_version() == 5


def test_entry_points_reject_bad_arguments_before_touching_a_device():
    lib = capi.load()
    F6 = (C.c_void_p * 6)(64, 64, None, None, 64, 64)          # never dereferenced: validation fails first
    F6null = (C.c_void_p * 6)()
    F6no_uv = (C.c_void_p * 6)(64, 64, None, None, None, None)
    P4 = (C.c_void_p * 4)(64, 64, 64, 64)
    P4null = (C.c_void_p * 4)(64, 64, None, 64)
    flag = C.c_int(0)
    dia, ten, app = lib.pam_amd_msa_diagnose, lib.pam_amd_msa_tendencies, lib.pam_amd_msa_apply
    cases = [
        ("msa_diagnose", lambda: dia(0, 4, 4, 4, F6, P4, None)),
        ("msa_diagnose", lambda: dia(4, 0, 4, 4, F6, P4, None)),
        ("msa_diagnose", lambda: dia(4, 4, 0, 4, F6, P4, None)),
        ("msa_diagnose", lambda: dia(4, 4, 4, 0, F6, P4, None)),
        ("msa_diagnose", lambda: dia(4, 4, 4, 4, None, P4, None)),
        ("msa_diagnose", lambda: dia(4, 4, 4, 4, F6, None, None)),
        ("msa_diagnose", lambda: dia(4, 4, 4, 4, F6null, P4, None)),
        ("msa_diagnose", lambda: dia(4, 4, 4, 4, F6no_uv, P4, None)),
        ("msa_diagnose", lambda: dia(4, 4, 4, 4, F6, P4null, None)),
        ("msa_tendencies", lambda: ten(4, 4, 4, 0, F6, P4, P4, 5.0, 64, None, None)),
        ("msa_tendencies", lambda: ten(4, 4, 4, 4, None, P4, P4, 5.0, 64, None, None)),
        ("msa_tendencies", lambda: ten(4, 4, 4, 4, F6, None, P4, 5.0, 64, None, None)),
        ("msa_tendencies", lambda: ten(4, 4, 4, 4, F6, P4, None, 5.0, 64, None, None)),
        ("msa_tendencies", lambda: ten(4, 4, 4, 4, F6, P4null, P4, 5.0, 64, None, None)),
        ("msa_tendencies", lambda: ten(4, 4, 4, 4, F6, P4, P4, 0.0, 64, None, None)),
        ("msa_tendencies", lambda: ten(4, 4, 4, 4, F6, P4, P4, -1.0, 64, None, None)),
        ("msa_tendencies", lambda: ten(4, 4, 4, 4, F6, P4, P4, math.nan, 64, None, None)),
        ("msa_tendencies", lambda: ten(4, 4, 4, 4, F6, P4, P4, 5.0, None, C.byref(flag), None)),
        ("msa_apply", lambda: app(0, 4, 4, 4, F6, P4, 2.0, 1, None, None)),
        ("msa_apply", lambda: app(4, 4, 4, 4, None, P4, 2.0, 1, None, None)),
        ("msa_apply", lambda: app(4, 4, 4, 4, F6, None, 2.0, 1, None, None)),
        ("msa_apply", lambda: app(4, 4, 4, 4, F6, P4null, 2.0, 1, None, None)),
        ("msa_apply", lambda: app(4, 4, 4, 4, F6no_uv, P4, 2.0, 1, None, None)),
        ("msa_apply", lambda: app(4, 4, 4, 4, F6, P4, -1.0, 1, None, None)),
        ("msa_apply", lambda: app(4, 4, 4, 4, F6, P4, math.nan, 1, None, None)),
        ("msa_apply", lambda: app(4, 4, 4, 4, F6, P4, math.inf, 1, None, None)),
    ]
    for i, (who, call) in enumerate(cases):
        assert call() == -1, (i, who)                              # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert who.encode() in lib.pam_amd_awfl_last_error(), (i, who)
    assert flag.value == 0
    # a == 0 makes no launch: valid arguments return 0 with or without a device, and without accel_uv the winds may be absent
    assert app(4, 4, 4, 4, F6, P4, 0.0, 1, None, None) == 0
    assert app(4, 4, 4, 4, F6no_uv, P4, 0.0, 0, None, None) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# the boundary of the C++ adaptor; the statistics weight

ADAPTOR = os.path.join(HOST, "modules", "mean_state_acceleration.h")


def test_adaptor_calls_only_members_the_reference_has():
    coupler, dm = tb._used_members(open(ADAPTOR).read())
    assert {"get_option", "set_option", "option_exists"} <= coupler and {"get", "register_and_allocate", "entry_exists"} <= dm, (coupler, dm)
    assert coupler <= tb.REF_COUPLER, sorted(coupler - tb.REF_COUPLER)
    assert dm <= tb.REF_DM, sorted(dm - tb.REF_DM)
    ours = tb._declared(os.path.join(HOST, "pam_coupler.h"))
    assert (coupler | dm) <= ours, sorted((coupler | dm) - ours)


def test_driver_still_calls_only_members_the_reference_has():
    coupler, dm = tb._used_members(open(os.path.join(ROOT, "examples", "driver.cpp")).read())
    assert coupler <= tb.REF_COUPLER and dm <= tb.REF_DM


def test_adaptor_names_the_entries_and_options_of_the_contract():
    text = open(ADAPTOR).read()
    for s in ('"accel_save_"', '"accel_tend_"', '"crm_accel_ceaseflag"', '"crm_accel_factor"', '"crm_accel_uv"', '"crm_accel_max_ttend"',
              '"cloud_liquid"', '"cloud_water"', '"ice"'):
        assert s in text, s
    n = tb._norm(tb._strip_comments(open(os.path.join(HOST, "modules", "time_average.h")).read()))
    assert "voidtime_average_accumulate(PamCoupler&coupler,std::vector<std::string>var_names,realweight){" in n
    assert "voidtime_average_accumulate(PamCoupler&coupler,std::vector<std::string>var_names){time_average_accumulate(coupler,var_names,1);}" in n
    assert "realfactor=crm_dt/gcm_dt*weight;" in n


def test_python_time_average_weight_defaults_to_one():
    import inspect
    from pam_amd import modules
    assert inspect.signature(modules.time_average_accumulate).parameters["weight"].default == 1
    assert (20.0 / 900.0) * float(1) == 20.0 / 900.0
