"""CRM variance transport, everything that needs no GPU: the numpy restatement of the contract (tests/vt_ref.py) against a scalar loop;
the device bodies under g++ (tests/emu/vt_emu.cpp) against the restatement bit for bit on every shape and named case; the census of the
branches the named cases reach; the mutants; the one-pass variance against a two-pass np.longdouble variance within the bound of its
summation tree; what the apply does to mean and variance within a derived bound; the C ABI's refusals; the adaptor's boundary."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import vt_ref as ref
import test_boundary_surface as tb
from vt_emu_harness import EmuBackend
from pam_amd import capi
from tools import native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
U = 2.0 ** -53
LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement itself

def _scalar_stats(x):
    """the contract's sentences, one Python float at a time"""
    nz, ncol, nens = x.shape
    r = 1.0 / ncol
    mean, var = np.empty((nz, nens)), np.empty((nz, nens))
    for k in range(nz):
        for e in range(nens):
            c = float(x[k, 0, e])
            sa, sb = [0.0] * 16, [0.0] * 16
            for i in range(ncol):
                d = float(x[k, i, e]) - c
                sa[i % 16] = sa[i % 16] + d * r
                dd = d * d
                sb[i % 16] = sb[i % 16] + dd * r
            A = B = 0.0
            for s in range(16):
                A, B = A + sa[s], B + sb[s]
            aa = A * A
            v = B - aa
            mean[k, e], var[k, e] = c + A, (0.0 if v < 0 else v)
    return mean, var


@pytest.mark.parametrize("shape", [((4, 1, 5), 3), ((5, 1, 17), 3), ((3, 4, 5), 1), ((6, 8, 8), 3), ((2, 1, 1), 3)], ids=ref.shape_id)
def test_restatement_is_the_scalar_loop(shape):
    st = ref.cases(shape)["base"]["now"]
    for x in ref.QUANTITIES:
        got, want = ref.level_stats(ref.quantity(st, x)), _scalar_stats(ref.quantity(st, x))
        assert ref.same_bits(got[0], want[0]) and ref.same_bits(got[1], want[1]), x


def test_restatement_scale_and_apply_are_the_scalar_loop():
    shape = ((5, 1, 17), 3)
    for name in ("base", "dry_cells", "clamp_low", "tend_inf"):
        case, got = ref.cases(shape)[name], ref.reference(shape, name)
        st = case["now"]
        nz, ncol, nens = st["temp"].shape
        for k in range(nz):
            for e in range(nens):
                s = {}
                for x in ref.QUANTITIES:
                    var, tend = float(got["var"][x][k, e]), float(case["tend"][x][k, e])
                    ratio = 1.0 + (case["dt"] * tend) / var if var > 0 else math.nan
                    if not var > 0 or ratio != ratio:
                        s[x] = 1.0
                    else:
                        s[x] = min(max(math.sqrt(max(ratio, 0.0)), 1.0 - case["lim"]), 1.0 + case["lim"])
                    assert got["scale"][x][k, e] == s[x], (name, x)
                g, m = {x: s[x] - 1.0 for x in s}, {x: float(got["mean"][x][k, e]) for x in s}
                q = [(float(st["water_vapor"][k, i, e]) + float(st["cloud"][k, i, e])) + float(st["ice"][k, i, e]) for i in range(ncol)]
                vp = [float(st["water_vapor"][k, i, e]) + g["q"] * (q[i] - m["q"]) for i in range(ncol)]
                pos, neg = [0.0] * 16, [0.0] * 16
                for i in range(ncol):
                    pos[i % 16] = pos[i % 16] + (vp[i] if vp[i] > 0 else 0.0)
                    neg[i % 16] = neg[i % 16] + (vp[i] if vp[i] < 0 else 0.0)
                P = N = 0.0
                for sl in range(16):
                    P, N = P + pos[sl], N + neg[sl]
                for i in range(ncol):
                    t = float(st["temp"][k, i, e])
                    assert got["fields"]["temp"][k, i, e] == (t + g["t"] * (t - m["t"]) if g["t"] != 0 else t)
                    if g["q"] == 0:
                        want = float(st["water_vapor"][k, i, e])
                    elif not N < 0:
                        want = vp[i]
                    elif P + N > 0:
                        want = (vp[i] if vp[i] > 0 else 0.0) * (1.0 + N / P)
                    else:
                        want = 0.0
                    assert got["fields"]["water_vapor"][k, i, e] == want, name
                for x in ref.QUANTITIES:
                    assert got["feedback"][x][k, e] == (float(got["end_var"][x][k, e]) - float(got["var_start"][x][k, e])) / case["gcm_dt"]


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

def _scale_branches(case, r):
    """how many (k,e,quantity) take each branch of the scale"""
    n = dict.fromkeys(("one_by_zero_variance", "one_by_nan", "low_clamp", "high_clamp", "interior", "negative_ratio"), 0)
    lo, hi = 1.0 - case["lim"], 1.0 + case["lim"]
    for x in r["var"]:
        var, s = r["var"][x], r["scale"][x]
        with np.errstate(all="ignore"):
            ratio = 1.0 + (case["dt"] * case["tend"][x]) / var
        live = (var > 0) & ~np.isnan(ratio)
        n["one_by_zero_variance"] += int(((var == 0) & (s == 1.0)).sum())
        n["one_by_nan"] += int(((np.isnan(var) | ((var > 0) & np.isnan(ratio))) & (s == 1.0)).sum())
        n["low_clamp"] += int((live & (s == lo) & (ratio < lo * lo)).sum())
        n["high_clamp"] += int((live & (s == hi) & (ratio > hi * hi)).sum())
        n["interior"] += int((live & (s > lo) & (s < hi) & (s != 1.0)).sum())
        n["negative_ratio"] += int((live & (ratio < 0) & (s == lo)).sum())
    return n


def _vapor_modes(case, r):
    g = r["scale"]["q"] - 1.0
    with np.errstate(all="ignore"):
        vp = case["now"]["water_vapor"] + g[:, None, :] * (ref.quantity(case["now"], "q") - r["mean"]["q"][:, None, :])
        _, _, mode = ref.vapor_levels(vp, g != 0)
    return mode, g != 0


def test_census_of_the_named_cases():
    """every case reaches the branch it is named after, on every shape where the shape allows it; a case that reaches none of its
    branches fails here rather than passing empty"""
    total = dict.fromkeys(("one_by_zero_variance", "one_by_nan", "low_clamp", "high_clamp", "interior", "negative_ratio", "clean", "filled",
                           "zeroed"), 0)
    for shape in ref.SHAPES:
        (nz, ny, nx), nens = shape
        ncol, cs = ny * nx, ref.cases(shape)
        count = {name: _scale_branches(cs[name], ref.reference(shape, name)) for name in ref.CASE_NAMES}
        for name in ref.CASE_NAMES:
            for b, v in count[name].items():
                total[b] += v
        nq = 3 * nz * nens
        if ncol == 1:                                  # a single column has no variance: every scale is 1, nothing is written
            for name in ref.CASE_NAMES:
                if name != "nan_in_temp":
                    assert count[name]["one_by_zero_variance"] == (2 if name == "use_u_off" else 3) * nz * nens, name
                r = ref.reference(shape, name)
                assert ref.results_differ(dict(r, fields=cs[name]["now"]), r, tables=()) == [], name
            continue
        base = ref.reference(shape, "base")
        assert count["base"]["interior"] == nq                                    # strictly inside the clamp, both signs
        assert all((base["scale"][x] > 1).any() and (base["scale"][x] < 1).any() for x in ref.QUANTITIES) or nz * nens < 4
        assert count["clamp_low"]["low_clamp"] == nq and count["clamp_high"]["high_clamp"] == nq
        assert count["ratio_negative"]["negative_ratio"] == nq
        zero = ref.reference(shape, "tend_zero")
        assert all((zero["scale"][x] == 1.0).all() for x in ref.QUANTITIES)
        assert ref.results_differ(dict(zero, fields=cs["tend_zero"]["now"]), zero, tables=()) == []          # nothing is written
        assert count["tend_nan"]["one_by_nan"] == 3 and count["tend_nan"]["interior"] == nq - 3
        inf = ref.reference(shape, "tend_inf")
        assert all(inf["scale"][x][0, 0] == 1.0 + ref.LIMIT and inf["scale"][x][-1, -1] == 1.0 - ref.LIMIT for x in ref.QUANTITIES)
        assert count["zero_variance_level"]["one_by_zero_variance"] == nens
        zv = ref.reference(shape, "zero_variance_level")
        assert (zv["var"]["t"][0] == 0.0).all() and ref.same_bits(zv["fields"]["temp"][0], cs["zero_variance_level"]["now"]["temp"][0])
        nan = ref.reference(shape, "nan_in_temp")
        kk, ee = nz // 2, nens // 2
        assert np.isnan(nan["var"]["t"]).sum() == 1 and np.isnan(nan["var"]["t"][kk, ee]) and nan["scale"]["t"][kk, ee] == 1.0
        assert ref.same_bits(nan["fields"]["temp"][kk, :, ee], cs["nan_in_temp"]["now"]["temp"][kk, :, ee])    # that (k,e) keeps its bits
        assert count["nan_in_temp"]["one_by_nan"] == 1 and count["nan_in_temp"]["interior"] == nq - 1          # the others proceed
        assert not ref.same_bits(nan["fields"]["water_vapor"][kk, :, ee], cs["nan_in_temp"]["now"]["water_vapor"][kk, :, ee])
        far = cs["outlier_cell0"]["now"]["temp"]
        assert (np.abs(far[:, 0, :] - far[:, 1:, :].mean(axis=1)) > 9.99 * far[:, 1:, :].std(axis=1)).all()
        mode, on = _vapor_modes(cs["dry_cells"], ref.reference(shape, "dry_cells"))
        assert on.all()
        for m, kind in enumerate(("clean", "filled", "zeroed")):
            total[kind] += int((mode == m).sum())
        kind = (np.arange(nz)[:, None] + np.arange(nens)[None, :]) % 3
        assert ((mode == 1) == (kind == 0)).all() and ((mode == 2) == (kind == 1)).all()
        wv = ref.reference(shape, "dry_cells")["fields"]["water_vapor"]
        assert (wv >= 0).all() and (wv[np.broadcast_to((mode == 2)[:, None, :], wv.shape)] == 0).all()
        mode, _ = _vapor_modes(cs["base"], base)
        assert (mode == 0).all()                                                    # the base case's vapour stays clean
        for name, gone in (("no_cloud", ("cloud",)), ("no_ice", ("ice",)), ("vapour_only", ("cloud", "ice"))):
            got = ref.reference(shape, name)
            assert all(got["fields"][g] is None for g in gone)
            assert not ref.same_bits(got["var"]["q"], base["var"]["q"]), name         # the absent species is really left out
        off = ref.reference(shape, "use_u_off")
        assert off["fields"]["uvel"] is None and set(off["scale"]) == {"t", "q"}
        assert ref.same_bits(off["fields"]["temp"], base["fields"]["temp"])
        assert not ref.same_bits(base["fields"]["uvel"], cs["base"]["now"]["uvel"])
        for f in ("cloud", "ice"):                                                  # never written
            assert ref.same_bits(base["fields"][f], cs["base"]["now"][f])
    assert all(v >= 1 for v in total.values()), total


# ------------------------------------------------------------------------------------------------------------------------------
# mutants of the restatement: each is caught by a named case

CAUGHT_BY = {"slots_descending": ("base", "mean_u"), "unshifted": ("base", "var_t"), "var_fma": ("base", "var_u"),
             "mean_form": ("base", "temp"), "clamp_before_root": ("clamp_low", "scale_t"), "cloud_incremented": ("base", "cloud"),
             "feedback_reciprocal": ("base", "feedback_t")}


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_caught(mutant):
    shape = ((6, 8, 8), 3)
    name, expect = CAUGHT_BY[mutant]
    got = ref.run_case(ref.RefBackend(mutant), ref.cases(shape)[name])
    bad = ref.results_differ(got, ref.reference(shape, name))
    assert expect in bad, (mutant, bad)


def test_no_mutant_is_the_restatement():
    shape = ((6, 8, 8), 3)
    assert ref.results_differ(ref.run_case(ref.RefBackend(None), ref.cases(shape)["base"]), ref.reference(shape, "base")) == []
    assert set(CAUGHT_BY) == set(ref.MUTANTS)


# ------------------------------------------------------------------------------------------------------------------------------
# the one-pass variance against two passes in extended precision

def _moments(x):
    """M(d^2) and M(|d|), d = x - x(cell 0), in np.longdouble"""
    d = x.astype(LD) - x[:, :1, :].astype(LD)
    return (d * d).mean(axis=1), np.abs(d).mean(axis=1)


def _gamma(ncol, more=0):
    return (math.ceil(ncol / 16) + 22 + more) * U


def _var_bound(x):
    m2, m1 = _moments(x)
    return _gamma(x.shape[1]) * (m2 + 2 * m1 * m1)


def _mean_bound(x, mean):
    """|mean - true mean| <= (n_s + 18) u M(|d|) + u |mean|: the terms of A carry the rounding of d, of r, of d r, at most n_s adds in
    the slot and 15 in the fold; the add c + A rounds once"""
    _, m1 = _moments(x)
    return (math.ceil(x.shape[1] / 16) + 18) * U * m1 + U * np.abs(mean)


@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[1] in (3, 65)], ids=ref.shape_id)
def test_variance_is_within_the_bound_of_its_summation_tree(shape):
    """|var - Var| <= gamma (M(d^2) + 2 M(|d|)^2), gamma = (n_s + 22) u, n_s = ceil(ncol / 16), u = 2^-53, Var the two-pass variance in
    np.longdouble.  To first order: every term of B = M(d^2) carries the rounding of d twice (d^2), of r, of d d, of (d d) r, at most n_s
    adds in its slot and 15 in the fold: (n_s + 20) u M(d^2), the terms being of one sign.  Every term of A = M(d) carries the rounding of
    d, of r, of d r, n_s and 15 adds: |dA| <= (n_s + 18) u M(|d|), so A A is off by 2 |A| |dA| + u A^2 <= (2 n_s + 37) u M(|d|)^2.  The
    subtraction rounds once: u M(d^2).  In all (n_s + 21) u M(d^2) + (2 n_s + 37) u M(|d|)^2 <= gamma (M(d^2) + 2 M(|d|)^2).  The variance
    is invariant under the shift, so Var(d) = Var(x) exactly; a result clamped to 0.0 moves towards Var >= 0."""
    worst = 0.0
    for name in ("base", "outlier_cell0", "dry_cells"):
        st = ref.cases(shape)[name]["now"]
        got = ref.reference(shape, name)
        for x in ref.QUANTITIES:
            f = ref.quantity(st, x)
            two_pass = ((f.astype(LD) - f.astype(LD).mean(axis=1, keepdims=True)) ** 2).mean(axis=1)
            err, lim = np.abs(got["var"][x].astype(LD) - two_pass), _var_bound(f)
            assert (err <= lim).all(), (name, x)
            if shape[0][1] * shape[0][2] > 1:
                worst = max(worst, float((err / lim).max()))
                assert (np.abs(got["mean"][x].astype(LD) - f.astype(LD).mean(axis=1)) <= _mean_bound(f, got["mean"][x])).all(), (name, x)
    print("worst fraction of the bound %.3f" % worst)


@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[1] in (3, 65) and s[0][1] * s[0][2] > 1], ids=ref.shape_id)
def test_apply_scales_the_variance_by_s_squared_and_keeps_the_mean(shape):
    """The base case: nothing clamps, the vapour stays clean.  With m and s the computed mean and scale, the exact result of the apply is
    y = x + g (x - m) = m + s (x - m), whose variance is s^2 Var(x) exactly and whose mean is m + s (mu - m), mu the true mean of x.
    The computed cell differs from y by at most delta = u |y| + 2 u |g| |x - m| (the add rounds once; x - m and the product round
    once each, both times |g| |x - m| large).  For total water, whose anomaly goes through the vapour, x is the computed q, and the
    re-diagnosed q' = (v' + cloud) + ice adds two roundings of size u |q'| and the old sum's two of size u |q|, with u |v'| for the add.
      variance: |var' - s^2 var| <= E_var(x') + 2 M(|x' - mean'| delta) + 4 M(delta^2) + s^2 E_var(x): the statistics bound on both
      sides, and a perturbation e of the cells, |e| <= delta, moves the variance by 2 M((y - mean) e) + M((e - M(e))^2).
      mean: |mean' - mean| <= E_mean(x') + M(delta) + (1 + |g|) E_mean(x): the true mean moves by g (mu - m) only.
    E_var and E_mean are the bounds of the test above."""
    case, r = ref.cases(shape)["base"], ref.reference(shape, "base")
    worst_v = worst_m = 0.0
    for x in ref.QUANTITIES:
        old, new = ref.quantity(case["now"], x).astype(LD), ref.quantity(r["fields"], x).astype(LD)
        s, m = r["scale"][x].astype(LD), r["mean"][x].astype(LD)
        g = np.abs(s - 1)[:, None, :]
        delta = U * np.abs(new) + 2 * U * g * np.abs(old - m[:, None, :])
        if x == "q":
            delta = U * np.abs(r["fields"]["water_vapor"].astype(LD)) + 2 * U * np.abs(new) + 2 * U * np.abs(old) + 2 * U * g * np.abs(old - m[:, None, :])
        f_old, f_new = ref.quantity(case["now"], x), ref.quantity(r["fields"], x)
        dev = np.abs(new - r["end_mean"][x].astype(LD)[:, None, :])
        lim_v = _var_bound(f_new) + 2 * (dev * delta).mean(axis=1) + 4 * (delta * delta).mean(axis=1) + s * s * _var_bound(f_old)
        err_v = np.abs(r["end_var"][x].astype(LD) - s * s * r["var"][x].astype(LD))
        assert (err_v <= lim_v).all(), x
        lim_m = _mean_bound(f_new, r["end_mean"][x]) + delta.mean(axis=1) + (1 + np.abs(s - 1)) * _mean_bound(f_old, r["mean"][x])
        err_m = np.abs(r["end_mean"][x].astype(LD) - m)
        assert (err_m <= lim_m).all(), x
        worst_v, worst_m = max(worst_v, float((err_v / lim_v).max())), max(worst_m, float((err_m / lim_m).max()))
        assert (r["scale"][x] != 1.0).all() and not ref.same_bits(f_new, f_old)
    print("worst fraction of the bound: variance %.3f, mean %.3f" % (worst_v, worst_m))


@pytest.mark.parametrize("shape", [((5, 1, 17), 3), ((6, 8, 8), 65)], ids=ref.shape_id)
def test_a_gain_of_zero_keeps_the_bits(shape):
    """scale == 1 in one quantity at one (k,e) and everywhere: those fields keep their bits there, negative vapour included"""
    case = ref.cases(shape)["dry_cells"]
    r = ref.reference(shape, "dry_cells")
    for be in (ref.RefBackend(), EmuBackend()):
        for x, f in (("t", "temp"), ("q", "water_vapor"), ("u", "uvel")):
            scale = {y: v.copy() for y, v in r["scale"].items()}
            scale[x][1, 2] = 1.0
            out = be.apply(case["now"], True, r["mean"], scale)
            assert ref.same_bits(out[f][1, :, 2], case["now"][f][1, :, 2]), (x, type(be).__name__)
            assert not ref.same_bits(out[f][1, :, 1], case["now"][f][1, :, 1])
        ones = {y: np.ones_like(v) for y, v in r["scale"].items()}
        out = be.apply(case["now"], True, r["mean"], ones)
        assert all(ref.same_bits(out[f], case["now"][f]) for f in ref.FIELDS)
        assert (out["water_vapor"] < 0).any()


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI: refusals before any device is asked for; the symbols

NEW_SYMBOLS = ("pam_amd_vt_diagnose", "pam_amd_vt_forcing", "pam_amd_vt_apply", "pam_amd_vt_feedback")


def test_entry_points_are_exported_and_declared_and_the_abi_stays_5():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    assert lib.pam_amd_awfl_abi_version() == 5


def test_entry_points_reject_bad_arguments_and_leave_their_outputs_untouched():
    """the pointers are host arrays here: a refusal comes before the first HIP call, so nothing dereferences them, and afterwards every
    array still holds the pattern it was filled with"""
    lib = capi.load()
    arrays = [np.full(64, 7.25) for _ in range(17)]
    ptr = [a.ctypes.data for a in arrays]
    F = (C.c_void_p * 5)(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4])
    Fnull = (C.c_void_p * 5)()
    Fno_vapor = (C.c_void_p * 5)(ptr[0], None, ptr[2], ptr[3], ptr[4])
    Fno_temp = (C.c_void_p * 5)(None, ptr[1], ptr[2], ptr[3], ptr[4])
    Fno_u = (C.c_void_p * 5)(ptr[0], ptr[1], None, None, None)
    T = [(C.c_void_p * 3)(*ptr[5 + 3 * i:8 + 3 * i]) for i in range(4)]
    Thole = (C.c_void_p * 3)(ptr[5], None, ptr[7])
    Tno_u = (C.c_void_p * 3)(ptr[5], ptr[6], None)
    dia, frc, app, fb = lib.pam_amd_vt_diagnose, lib.pam_amd_vt_forcing, lib.pam_amd_vt_apply, lib.pam_amd_vt_feedback
    big = 65536                                                    # ny nx = 2^32 > 2^31 - 1
    cases = [
        ("vt_diagnose", lambda: dia(0, 4, 4, 4, F, 1, T[0], T[1], None)),
        ("vt_diagnose", lambda: dia(4, 0, 4, 4, F, 1, T[0], T[1], None)),
        ("vt_diagnose", lambda: dia(4, 4, 0, 4, F, 1, T[0], T[1], None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 0, F, 1, T[0], T[1], None)),
        ("vt_diagnose", lambda: dia(4, big, big, 4, F, 1, T[0], T[1], None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 4, None, 1, T[0], T[1], None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 4, F, 1, None, T[1], None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 4, F, 1, T[0], None, None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 4, Fnull, 1, T[0], T[1], None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 4, Fno_temp, 1, T[0], T[1], None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 4, Fno_vapor, 1, T[0], T[1], None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 4, Fno_u, 1, T[0], T[1], None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 4, F, 1, Thole, T[1], None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 4, F, 1, T[0], Tno_u, None)),
        ("vt_diagnose", lambda: dia(4, 4, 4, 4, F, 0, T[0], Thole, None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 0, F, 1, T[0], 20.0, 0.05, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, None, 1, T[0], 20.0, 0.05, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, None, 20.0, 0.05, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], 20.0, 0.05, None, T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], 20.0, 0.05, T[1], None, T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], 20.0, 0.05, T[1], T[2], None, None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], 20.0, 0.05, T[1], T[2], Tno_u, None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, Fno_u, 1, T[0], 20.0, 0.05, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], 0.0, 0.05, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], -1.0, 0.05, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], math.nan, 0.05, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], math.inf, 0.05, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], 20.0, 0.0, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], 20.0, 1.0, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], 20.0, -0.1, T[1], T[2], T[3], None)),
        ("vt_forcing", lambda: frc(4, 4, 4, 4, F, 1, T[0], 20.0, math.nan, T[1], T[2], T[3], None)),
        ("vt_apply", lambda: app(0, 4, 4, 4, F, 1, T[0], T[1], None)),
        ("vt_apply", lambda: app(4, 4, 4, 4, None, 1, T[0], T[1], None)),
        ("vt_apply", lambda: app(4, 4, 4, 4, F, 1, None, T[1], None)),
        ("vt_apply", lambda: app(4, 4, 4, 4, F, 1, T[0], None, None)),
        ("vt_apply", lambda: app(4, 4, 4, 4, F, 1, T[0], Thole, None)),
        ("vt_apply", lambda: app(4, 4, 4, 4, Fno_u, 1, T[0], T[1], None)),
        ("vt_apply", lambda: app(4, 4, 4, 4, Fno_vapor, 0, T[0], T[1], None)),
        ("vt_feedback", lambda: fb(4, 4, 4, 0, F, 1, T[0], 240.0, T[1], T[2], T[3], None)),
        ("vt_feedback", lambda: fb(4, 4, 4, 4, None, 1, T[0], 240.0, T[1], T[2], T[3], None)),
        ("vt_feedback", lambda: fb(4, 4, 4, 4, F, 1, None, 240.0, T[1], T[2], T[3], None)),
        ("vt_feedback", lambda: fb(4, 4, 4, 4, F, 1, T[0], 240.0, T[1], T[2], None, None)),
        ("vt_feedback", lambda: fb(4, 4, 4, 4, F, 1, Thole, 240.0, T[1], T[2], T[3], None)),
        ("vt_feedback", lambda: fb(4, 4, 4, 4, Fno_u, 1, T[0], 240.0, T[1], T[2], T[3], None)),
        ("vt_feedback", lambda: fb(4, 4, 4, 4, F, 1, T[0], 0.0, T[1], T[2], T[3], None)),
        ("vt_feedback", lambda: fb(4, 4, 4, 4, F, 1, T[0], -240.0, T[1], T[2], T[3], None)),
        ("vt_feedback", lambda: fb(4, 4, 4, 4, F, 1, T[0], math.nan, T[1], T[2], T[3], None)),
        ("vt_feedback", lambda: fb(4, 4, 4, 4, F, 1, T[0], math.inf, T[1], T[2], T[3], None)),
    ]
    for i, (who, call) in enumerate(cases):
        assert call() == -1, (i, who)                              # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert who.encode() in lib.pam_amd_awfl_last_error(), (i, who)
        assert all((a == 7.25).all() for a in arrays), (i, who)


# ------------------------------------------------------------------------------------------------------------------------------
# the boundary of the C++ adaptor, the driver, the build

ADAPTOR = os.path.join(HOST, "modules", "variance_transport.h")


def test_adaptor_calls_only_members_the_reference_has():
    coupler, dm = tb._used_members(open(ADAPTOR).read())
    assert {"get_option", "set_option", "option_exists"} <= coupler and {"get", "register_and_allocate", "entry_exists"} <= dm, (coupler, dm)
    assert coupler <= tb.REF_COUPLER, sorted(coupler - tb.REF_COUPLER)
    assert dm <= tb.REF_DM, sorted(dm - tb.REF_DM)
    ours = tb._declared(os.path.join(HOST, "pam_coupler.h"))
    assert (coupler | dm) <= ours, sorted((coupler | dm) - ours)
    coupler, dm = tb._used_members(open(os.path.join(ROOT, "examples", "driver.cpp")).read())
    assert coupler <= tb.REF_COUPLER and dm <= tb.REF_DM


def test_adaptor_and_python_mirror_name_the_same_entries_and_options():
    import inspect
    from pam_amd import modules
    text, py = open(ADAPTOR).read(), inspect.getsource(modules)
    for s in ('"vt_mean_"', '"vt_var_"', '"vt_var_start_"', '"vt_scale_"', '"vt_tend_"', '"vt_feedback_"', '"crm_vt_u"', '"crm_vt_scale_limit"',
              '"crm_dt"', '"gcm_physics_dt"', '"cloud_liquid"', '"cloud_water"', '"ice"'):
        assert s in text, s
    for s in ('"crm_vt_u"', '"crm_vt_scale_limit"', '"crm_dt"', '"gcm_physics_dt"', "vt_%s_%s"):
        assert s in py, s
    assert [n for n, _ in modules.VT_ENTRIES] == ["mean", "var", "var_start", "scale", "tend", "feedback"]
    n = tb._norm(tb._strip_comments(text))
    for f in ("inlinevoidvt_init(PamCoupler&coupler){", "inlinevoidvt_apply_forcing(PamCoupler&coupler,realdt){",
              "inlinevoidvt_apply_forcing(PamCoupler&coupler){vt_apply_forcing(coupler,coupler.get_option<real>(\"crm_dt\"));}",
              "inlinevoidvt_compute_feedback(PamCoupler&coupler){"):
        assert f in n, f
    for f in ("vt_init", "vt_apply_forcing", "vt_compute_feedback"):
        assert callable(getattr(modules, f))
    assert inspect.signature(modules.vt_apply_forcing).parameters["dt"].default is None


def test_build_depends_on_the_device_header():
    deps = native_build.dependencies(native_build.LIB_SOURCES)
    assert os.path.join(native_build.CSRC, "vt_device.h") in deps and os.path.join(HOST, "modules", "variance_transport.h") in deps
    assert '#include "vt_device.h"' in open(os.path.join(ROOT, "pam_amd", "csrc", "modules_kernels.hip")).read()
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert '"--vt"' in drv and '"--vt-u"' in drv and '"--vt-limit"' in drv
