"""Large-scale forcing, everything that needs no GPU: the device bodies under g++ (tests/emu/lsforcing_emu.cpp) against the numpy
restatement (tests/lsforcing_ref.py) bit for bit on every shape and named case, narrow and wide; the census of what the named cases
reach, on the restatement alone; the properties of the scheme on the restatement and on the emulation; the mutants of the restatement;
the C ABI's symbols, refusals and answer without a device; the wrappers' refusals; the C++ module, the driver, the tool and the
documents."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lsforcing_ref as ref
import lsforcing_cases as lc
from lsforcing_harness import EmuBackend
from pam_amd import capi
from tools.native_build import cxx_program, syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
LD = np.longdouble
U = 2.0 ** -53
BACKENDS = (("restatement", ref.RefBackend), ("emulation", EmuBackend))
_EMU = {}


def emu(shape, name, wide=False):
    """the emulation's outputs of a named case, computed once"""
    if (shape, name, wide) not in _EMU:
        _EMU[shape, name, wide] = EmuBackend(wide).run(lc.cases(shape)[name])
    return _EMU[shape, name, wide]


def inputs(case):
    return {n: case["fields"][n] for n in ref.STATE + tuple(case["tracers"])}


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the device bodies under g++

@pytest.mark.parametrize("wide", (False, True), ids=("narrow", "wide"))
@pytest.mark.parametrize("shape", lc.SHAPES, ids=ref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape, wide):
    for name in lc.CASE_NAMES:
        assert ref.results_differ(emu(shape, name, wide), lc.reference(shape, name), nan_by_place=True) == [], name


@pytest.mark.parametrize("shape", lc.SHAPES, ids=ref.shape_id)
def test_emulated_increments_match_and_absent_ones_are_not_written(shape):
    for name in ("all_on", "no_target_q", "no_target_u", "nan_cell"):
        case = lc.cases(shape)[name]
        _, inc = EmuBackend().run(case, with_inc=True)
        want = ref.nudging(case)
        for x in ref.QUANTITIES:
            assert (inc[x] is None) == (want[x] is None), (name, x)
            if want[x] is not None:
                assert ref.same_bits(inc[x], want[x], nan_by_place=True), (name, x)


@pytest.mark.parametrize("shape", [s for s in lc.SHAPES if s[3] >= 64], ids=ref.shape_id)
def test_members_split_over_calls_equal_the_whole(shape):
    """three calls with the matching slices of zmid, fcor and every profile, on the restatement and on the emulation"""
    nens = shape[3]
    for name in ("all_on", "nan_w", "nan_cell", "clamp"):
        case, want = lc.cases(shape)[name], lc.reference(shape, name)
        for label, backend in BACKENDS:
            parts = [backend().run(ref.members(case, slice(lo, hi))) for lo, hi in ((0, 1), (1, 37), (37, nens))]
            got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
            assert ref.results_differ(got, want, nan_by_place=True) == [], (name, label)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the census, on the restatement and the cases alone

def test_census_of_the_named_cases():
    """over the case set as a whole: levels with w > 0, w < 0 and w == 0 that take a term; both closed ends with the wind blowing into them
    (w > 0 at the ground, w < 0 at the lid); a sign change of wsub inside a column; different signs in neighbouring members of one
    wavefront; the positive clamp acting and not acting; the vapour first, last and in the middle of the table; 0, 1 and 7 tracers; each
    optional input absent on its own; the NaNs where they belong"""
    n = dict(up=0, down=0, rest=0, ground=0, lid=0, turn=0, neighbours=0)
    for shape in lc.SHAPES:
        nz, ny, nx, nens = shape
        w = lc.cases(shape)["all_on"]["wsub"]
        k = np.arange(nz)[:, None]
        n["up"] += int(((w > 0) & (k > 0)).sum())
        n["down"] += int(((w < 0) & (k < nz - 1)).sum())
        n["rest"] += int((w == 0).sum())
        n["ground"] += int((w[0] > 0).sum())
        n["lid"] += int((w[nz - 1] < 0).sum())
        n["turn"] += int(((w > 0).any(axis=0) & (w < 0).any(axis=0)).sum())
        e = np.arange(nens - 1)
        same_wave = (e // 64) == ((e + 1) // 64)
        n["neighbours"] += int(((w[:, :-1] * w[:, 1:] < 0) & same_wave[None, :]).sum())
    print("census:", n)
    assert all(v > 0 for v in n.values()), n
    for shape in lc.SHAPES[2:]:                                   # every shape with a wavefront of members has all three
        w = lc.cases(shape)["all_on"]["wsub"]
        assert (w > 0).any() and (w < 0).any() and (w == 0).any(), shape
    # the clamp
    assert sum(lc.clamped(s, "clamp") for s in lc.SHAPES) > 0
    for shape in lc.SHAPES[1:]:
        assert lc.clamped(shape, "clamp") > 0, shape
        v = lc.reference(shape, "clamp")[ref.VAPOUR]
        assert (v > 0).any() and (v == 0).any() and not (v < 0).any()
        assert lc.clamped(shape, "all_on") == 0 and (lc.reference(shape, "all_on")[ref.VAPOUR] > 0).all()
    # the table
    shape = lc.SHAPES[-1]
    cs = lc.cases(shape)
    assert cs["vapour_first"]["tracers"].index(ref.VAPOUR) == 0 and cs["vapour_last"]["tracers"].index(ref.VAPOUR) == 6
    assert cs["all_on"]["tracers"].index(ref.VAPOUR) == 3
    assert [len(cs[c]["tracers"]) for c in ("no_tracers", "one_tracer", "all_on")] == [0, 1, 7]
    assert cs["all_on"]["positive"] == (True, True, True, True, True, False, True)
    assert (cs["all_on"]["fields"][lc.UNFLAGGED] < 0).any()
    # each optional input absent on its own
    optional = lambda c: dict(wsub=c["wsub"], temp_tend=c["temp_tend"], qv_tend=c["qv_tend"], coriolis=c["fcor"],
                              **{"target_" + x: (c["target"] or {}).get(x) for x in ref.QUANTITIES})
    assert all(v is not None for v in optional(cs["all_on"]).values())
    for name in lc.ABSENT:
        absent = sorted(k for k, v in optional(cs[name]).items() if v is None)
        assert absent == [name[3:]], (name, absent)
        assert (cs[name]["ug"] is None) == (cs[name]["vg"] is None) == (cs[name]["fcor"] is None)
    # the NaNs: a NaN w makes its level of its member a NaN and nothing else; a NaN cell stays in its column
    for shape in lc.SHAPES:
        nz, ny, nx, nens = shape
        (kw, ew), (kt, jt, it, et), (kq, jq, iq, eq) = lc.nan_places(shape)
        got = lc.reference(shape, "nan_w")
        for name in ref.STATE + tuple(lc.cases(shape)["nan_w"]["tracers"]):
            want = np.zeros(shape, dtype=bool)
            want[kw, :, :, ew] = True
            assert np.array_equal(np.isnan(got[name]), want), (shape, name)
        got = lc.reference(shape, "nan_cell")
        column = np.zeros(shape, dtype=bool)
        column[:, jt, it, et] = True
        assert np.isnan(got["temp"][kt, jt, it, et]) and not np.isnan(got["temp"][~column]).any()
        column = np.zeros(shape, dtype=bool)
        column[:, jq, iq, eq] = True
        assert np.isnan(got[ref.VAPOUR][kq, jq, iq, eq])
        for name in lc.cases(shape)["nan_cell"]["tracers"]:       # rho of that cell is a NaN, and with it every ratio formed there
            assert not np.isnan(got[name][~column]).any(), name
        assert not np.isnan(got["uvel"]).any() and not np.isnan(got["vvel"]).any()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. properties, on the restatement and on the emulation

@pytest.mark.parametrize("label,backend", BACKENDS, ids=[b[0] for b in BACKENDS])
@pytest.mark.parametrize("shape", lc.SHAPES, ids=ref.shape_id)
def test_a_zero_or_absent_forcing_keeps_every_bit(shape, label, backend):
    case = lc.cases(shape)["zero_forcing"]
    assert ref.results_differ(backend().run(case), inputs(case)) == []
    nothing = dict(case, wsub=None, temp_tend=None, qv_tend=None, ug=None, vg=None, fcor=None, target=None)
    assert ref.results_differ(backend().run(nothing), inputs(nothing)) == []


@pytest.mark.parametrize("label,backend", BACKENDS, ids=[b[0] for b in BACKENDS])
def test_one_column_nudged_at_dt_rate_one_lands_on_the_target(label, backend):
    """ny nx == 1: the level mean is the cell.  dt rate == 1.0 exactly (8 x 0.125).  x' = x + 1.0 (target - x): the difference and the
    sum round once each, so x' is within 2 ulp of the larger of |x| and |target|; the vapour goes through rho_v' = rho_v + rho inc and
    is read back as rho_v' / rho, three more roundings: 5 ulp of the target"""
    shape = (4, 1, 1, 3)
    rng = np.random.default_rng(5)
    zmid, _ = lc.grid(4, 3)
    rho = 1.0 + 0.1 * rng.random(shape)
    qv = 0.01 * (1.0 + rng.random(shape))
    fields = dict(uvel=rng.random(shape) - 0.5, vvel=rng.random(shape) - 0.5, temp=290.0 + 10.0 * rng.random(shape), density_dry=rho * (1.0 - qv))
    fields[ref.VAPOUR] = rho * qv
    prof = lambda lo, hi: lo + (hi - lo) * rng.random((4, 3))
    one = np.full((4, 3), 0.125)
    target = dict(t=prof(285.0, 305.0), q=prof(0.005, 0.03), u=prof(-5.0, 5.0), v=prof(-5.0, 5.0))
    case = dict(fields=fields, tracers=(ref.VAPOUR,), positive=(True,), zmid=zmid, wsub=None, temp_tend=None, qv_tend=None, ug=None, vg=None,
                fcor=None, target=target, rate={x: one for x in ref.QUANTITIES}, dt=8.0, grav=9.80616, cp_d=1004.64)
    got = backend().run(case)
    col = lambda a: a[:, None, None, :]
    for n, x in (("temp", "t"), ("uvel", "u"), ("vvel", "v")):
        bound = 2.0 * np.spacing(np.maximum(np.abs(fields[n]), np.abs(col(target[x]))))
        assert (np.abs(got[n] - col(target[x])) <= bound).all(), n
    q_new = got[ref.VAPOUR] / (fields["density_dry"] + fields[ref.VAPOUR])
    assert (np.abs(q_new - col(target["q"])) <= 5.0 * np.spacing(col(target["q"]))).all()
    assert not ref.same_bits(got[ref.VAPOUR], fields[ref.VAPOUR])


@pytest.mark.parametrize("label,backend", BACKENDS, ids=[b[0] for b in BACKENDS])
@pytest.mark.parametrize("shape", lc.SHAPES[1:], ids=ref.shape_id)
def test_a_profile_constant_in_z_is_left_alone_by_any_wsub(shape, label, backend):
    """winds constant along every column, and tracers whose ratio to rho is a power of two (so that rho_x / rho is that number exactly at
    every level): exactly unchanged.  temp on an adiabat T0 - gc z: g = temp + gc z is T0 within an ulp of T0 at every level, the
    difference of two such is at most 2 ulp, and with a Courant number below 1 the increment is below that: 2 ulp of T0"""
    nz, ny, nx, nens = shape
    base = lc.cases(shape)["subsidence_only"]
    rng = np.random.default_rng(11)
    flat = (1, ny, nx, nens)
    # rho with 29 low bits clear: rho 2^-p, rho - rho 2^-p and their sum are then exact, and so is every ratio
    rho = (base["fields"]["density_dry"] + base["fields"][ref.VAPOUR]).astype(np.float32).astype(np.float64)
    gc = base["grav"] / base["cp_d"]
    T0 = 295.0 + 10.0 * rng.random(flat)
    f = dict(uvel=np.broadcast_to(16.0 * rng.random(flat) - 8.0, shape).copy(), vvel=np.broadcast_to(rng.random(flat), shape).copy(),
             temp=T0 - gc * base["zmid"][:, None, None, :])
    for i, n in enumerate(base["tracers"]):
        if n != ref.VAPOUR:
            f[n] = np.broadcast_to(2.0 ** -rng.integers(1, 12, flat), shape) * rho * (-1.0 if n == lc.UNFLAGGED else 1.0)
    q = np.broadcast_to(2.0 ** -rng.integers(5, 9, flat), shape)
    f[ref.VAPOUR] = q * rho
    f["density_dry"] = rho - f[ref.VAPOUR]
    assert np.array_equal(f["density_dry"] + f[ref.VAPOUR], rho) and np.array_equal(f[ref.VAPOUR] / rho, q)
    case = dict(base, fields=dict(base["fields"], **f))
    got = backend().run(case)
    for n in ("uvel", "vvel") + tuple(case["tracers"]):
        assert ref.same_bits(got[n], case["fields"][n]), n
    assert (np.abs(got["temp"] - f["temp"]) <= 2.0 * np.spacing(T0)).all()


@pytest.mark.parametrize("label,backend", BACKENDS, ids=[b[0] for b in BACKENDS])
@pytest.mark.parametrize("shape", lc.SHAPES, ids=ref.shape_id)
def test_subsidence_alone_never_overshoots(shape, label, backend):
    """within the wrappers' limit (every case has Courant numbers within 0.9) each new g(k) lies between the two old values it was formed
    from: exactly for the winds, whose g is the field; for temp and the tracers g is read back as temp' + gc z and rho_x' / rho, which
    round again: 4 ulp of the larger of the two old values"""
    case = lc.cases(shape)["subsidence_only"]
    got = backend().run(case)
    F, nz = case["fields"], shape[0]
    w = case["wsub"][:, None, None, :]
    k = np.arange(nz)[:, None, None, None]
    rho = F["density_dry"] + F[ref.VAPOUR]
    gz = (case["grav"] / case["cp_d"]) * case["zmid"][:, None, None, :]
    below = lambda a: np.concatenate([a[:1], a[:-1]])
    above = lambda a: np.concatenate([a[1:], a[-1:]])
    for n in ref.STATE + tuple(case["tracers"]):
        slack = 4.0
        if n == "temp":
            old, new = F[n] + gz, got[n] + gz
        elif n in ("uvel", "vvel"):
            old, new, slack = F[n], got[n], 0.0
        else:
            old, new = F[n] / rho, got[n] / rho
        other = np.where((w > 0) & (k > 0), below(old), np.where((w < 0) & (k < nz - 1), above(old), old))
        lo, hi = np.minimum(old, other), np.maximum(old, other)
        tol = slack * np.spacing(np.maximum(np.abs(lo), np.abs(hi)))
        assert ((new >= lo - tol) & (new <= hi + tol)).all(), n
        moved = (other != old) & (w != 0)
        if moved.any():
            assert (new[np.broadcast_to(moved, new.shape)] != old[np.broadcast_to(moved, old.shape)]).mean() > 0.9, n
    assert ref.same_bits(got["temp"], lc.reference(shape, "subsidence_only")["temp"])


def coriolis_case(shape, fdt):
    """the winds, a geostrophic wind and nothing else; f dt = fdt in every member, of either sign"""
    nz, ny, nx, nens = shape
    base = lc.cases(shape)["all_on"]
    sign = np.where(np.arange(nens) % 3 == 2, -1.0, 1.0)
    return dict(base, wsub=None, temp_tend=None, qv_tend=None, target=None, fcor=sign * (fdt / base["dt"]))


def coriolis_gate(case, u, v):
    """S = (u - ug)^2 + (v - vg)^2 before the step, in np.longdouble, and the per-cell rounding bound E of S after it, from the
    np.longdouble evaluation of the step's own formulas.  The rotation itself keeps S.  Each new component carries the rounding of the
    last sum, U |u'|, and of the six operations and three coefficients behind the quotient, 7 U r with r = sqrt(S); S moves by at most
    2 r times the two components' errors: E = 2 r U (|u'| + |v'| + 14 r).  The gate is G = 4 E"""
    col = lambda a: np.asarray(a)[:, None, None, :].astype(LD)
    ug, vg = col(case["ug"]), col(case["vg"])
    a = LD(0.5) * (np.asarray(case["fcor"]).astype(LD) * LD(case["dt"]))
    du, dv = u.astype(LD) - ug, v.astype(LD) - vg
    un = ug + ((1 - a * a) * du + (2 * a) * dv) / (1 + a * a)
    vn = vg + ((1 - a * a) * dv - (2 * a) * du) / (1 + a * a)
    S = du * du + dv * dv
    r = np.sqrt(S)
    return S, 2 * r * LD(U) * (np.abs(un) + np.abs(vn) + 14 * r)


def ageostrophic(case, u, v):
    col = lambda a: np.asarray(a)[:, None, None, :].astype(LD)
    du, dv = u.astype(LD) - col(case["ug"]), v.astype(LD) - col(case["vg"])
    return du * du + dv * dv


@pytest.mark.parametrize("label,backend", BACKENDS, ids=[b[0] for b in BACKENDS])
@pytest.mark.parametrize("shape", lc.SHAPES, ids=ref.shape_id)
def test_the_coriolis_step_keeps_the_ageostrophic_speed(shape, label, backend):
    worst = 0.0
    for fdt in (1.0e-3, 0.3, 2.5):
        case = coriolis_case(shape, fdt)
        S, E = coriolis_gate(case, case["fields"]["uvel"], case["fields"]["vvel"])
        got = backend().run(case)
        err = np.abs(ageostrophic(case, got["uvel"], got["vvel"]) - S)
        assert (err <= 4 * E).all(), fdt
        worst = max(worst, float((err / (4 * E)).max()))
        assert not ref.same_bits(got["uvel"], case["fields"]["uvel"])
        assert ref.same_bits(got["temp"], case["fields"]["temp"])
    print("worst fraction of the gate %.3f" % worst)


@pytest.mark.parametrize("label,backend", BACKENDS, ids=[b[0] for b in BACKENDS])
def test_fifty_coriolis_steps_do_not_grow_the_inertial_oscillation(label, backend):
    """f dt = 0.3, N = 50: |S_N - S_0| stays within the gates of the N steps added together, while the forward-Euler mutant has multiplied
    S by (1 + 0.09)^50"""
    shape = (5, 1, 17, 65)
    case = coriolis_case(shape, 0.3)
    u, v = case["fields"]["uvel"], case["fields"]["vvel"]
    S0, total = ageostrophic(case, u, v), 0
    for _ in range(50):
        _, E = coriolis_gate(case, u, v)
        total = total + 4 * E
        got = backend().run(dict(case, fields=dict(case["fields"], uvel=u, vvel=v)))
        u, v = got["uvel"], got["vvel"]
    err = np.abs(ageostrophic(case, u, v) - S0)
    print("worst fraction of the accumulated gate %.3f" % float((err / total).max()))
    assert (err <= total).all()
    mu, mv = case["fields"]["uvel"], case["fields"]["vvel"]
    for _ in range(50):
        m = ref.ls_forcing(dict(case, fields=dict(case["fields"], uvel=mu, vvel=mv)), mutant="euler_coriolis")
        mu, mv = m["uvel"], m["vvel"]
    assert (ageostrophic(case, mu, mv) > 50 * S0).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the mutants of the restatement

@pytest.mark.parametrize("mutant,name,fields,only", (
    ("downwind", "subsidence_only", ("uvel", "vvel", "temp", ref.VAPOUR, "tracer_a", lc.UNFLAGGED), False),
    ("wrong_dz_upper", "subsidence_only", ("uvel", "vvel", "temp", ref.VAPOUR, "tracer_a", lc.UNFLAGGED), False),
    ("temp_without_adiabat", "subsidence_only", ("temp",), True),
    ("nudge_cells", "no_wsub", ("uvel", "vvel", "temp", ref.VAPOUR), True),
    ("euler_coriolis", "all_on", ("uvel", "vvel"), True),
    ("clamp_unflagged", "subsidence_only", (lc.UNFLAGGED,), True)))
def test_mutants_of_the_restatement_are_caught(mutant, name, fields, only):
    """every mutant changes the fields it should on every shape that can show it (more than one level, for one-level columns take no
    subsidence), and, where it is a mutant of one term, no other field of that case"""
    assert mutant in ref.MUTANTS
    for shape in lc.SHAPES[1:]:
        case, want = lc.cases(shape)[name], lc.reference(shape, name)
        differ = ref.results_differ(ref.ls_forcing(case, mutant=mutant), want, nan_by_place=True)
        assert set(fields) <= set(differ), (shape, differ)
        assert not only or differ == sorted(fields), (shape, differ)


def test_the_properties_reject_the_mutants_too():
    """the mutants that break a property, on the property's own terms: downwind overshoots; without the adiabat term an adiabat is not
    left alone; nudging of cells damps the turbulence: the variance about the level mean shrinks, where nudging the mean keeps every
    deviation within rounding"""
    shape = (5, 1, 17, 65)
    case = lc.cases(shape)["subsidence_only"]
    F = case["fields"]
    got = ref.ls_forcing(case, mutant="downwind")
    lo = np.minimum(np.minimum(F["uvel"], np.concatenate([F["uvel"][:1], F["uvel"][:-1]])), np.concatenate([F["uvel"][1:], F["uvel"][-1:]]))
    assert (got["uvel"] < lo).any()
    gc = case["grav"] / case["cp_d"]
    adiabat = dict(case, fields=dict(F, temp=300.0 - gc * np.broadcast_to(case["zmid"][:, None, None, :], shape)))
    moved = np.abs(ref.ls_forcing(adiabat, mutant="temp_without_adiabat")["temp"] - adiabat["fields"]["temp"])
    assert moved.max() > 1.0e-3 and np.abs(ref.ls_forcing(adiabat)["temp"] - adiabat["fields"]["temp"]).max() < 1.0e-12
    nudge = dict(lc.cases(shape)["no_wsub"], fcor=None, ug=None, vg=None)
    dev = lambda a: a - a.mean(axis=(1, 2), keepdims=True)
    before = dev(nudge["fields"]["uvel"])
    honest = dev(ref.ls_forcing(nudge)["uvel"])
    cells = dev(ref.ls_forcing(nudge, mutant="nudge_cells")["uvel"])
    assert np.abs(honest - before).max() < 1.0e-13
    rated = nudge["rate"]["u"][:, None, None, :] > 0.01
    assert (np.abs(cells) < np.abs(before))[np.broadcast_to(rated, before.shape)].all()


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the C ABI: its symbols; refusals before any device is asked for; the answer without a device

def test_capi_symbols():
    lib = capi.load()
    for s in ("pam_amd_ls_nudging", "pam_amd_ls_forcing", "pam_amd_ls_forcing_debug_wide_index"):
        assert s in capi.MODULE_SYMBOLS and getattr(lib, s) is not None
    header = open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read()
    assert "int pam_amd_ls_forcing(int nens, int nx, int ny, int nz, double *uvel, double *vvel, double *temp, int num_tracers," in header
    assert "int pam_amd_ls_nudging(int nens, int nx, int ny, int nz, const double *const *fields, const double *const *target," in header
    assert "int pam_amd_ls_forcing_debug_wide_index(int on);" in header
    assert len(capi.MODULE_SYMBOLS["pam_amd_ls_forcing"][1]) == 24 and len(capi.MODULE_SYMBOLS["pam_amd_ls_nudging"][1]) == 10
    assert lib.pam_amd_ls_forcing_debug_wide_index(1) == 0 and lib.pam_amd_ls_forcing_debug_wide_index(0) == 0


NENS, NX, NY, NZ = 4, 3, 2, 4
CELLS, ROWS = NENS * NX * NY * NZ, NZ * NENS


def _abi():
    """host arrays filled with a pattern, and the two calls over them with keyword overrides"""
    lib = capi.load()
    names = ("u", "v", "temp", "rd", "rv", "tr0", "tr1", "zmid", "wsub", "tt", "qt", "fcor", "ug", "vg", "tgt_t", "tgt_q", "tgt_u", "tgt_v",
             "rate_t", "rate_q", "rate_uv", "inc_t", "inc_q", "inc_u", "inc_v", "spare")
    arrays = [np.full(CELLS + 16, 7.25) for _ in names]
    P = dict(zip(names, [a.ctypes.data for a in arrays]))
    tab = lambda ps: (C.c_void_p * len(ps))(*ps)
    good = dict(nens=NENS, nx=NX, ny=NY, nz=NZ, dt=10.0, grav=9.80616, cp_d=1004.64, ntr=3, tracers=["tr0", "rv", "tr1"], positive=[1, 1, 0],
                inc=["inc_t", "inc_q", "inc_u", "inc_v"], target=["tgt_t", "tgt_q", "tgt_u", "tgt_v"], rate=["rate_t", "rate_q", "rate_uv", "rate_uv"],
                fields=["temp", "rd", "rv", "u", "v"], **{n: n for n in names})

    def args(kw):
        a = dict(good)
        a.update(kw)
        ptr = lambda key: None if a[key] is None else (P[a[key]] if isinstance(a[key], str) else a[key])
        table = lambda key: None if a[key] is None else tab([None if x is None else (P[x] if isinstance(x, str) else x) for x in a[key]])
        return a, ptr, table

    def forcing(**kw):
        a, ptr, table = args(kw)
        flags = None if a["positive"] is None else (C.c_ubyte * max(len(a["positive"]), 1))(*a["positive"])
        return lib.pam_amd_ls_forcing(a["nens"], a["nx"], a["ny"], a["nz"], ptr("u"), ptr("v"), ptr("temp"), a["ntr"], table("tracers"), flags,
                                      ptr("rd"), ptr("rv"), ptr("zmid"), ptr("wsub"), ptr("tt"), ptr("qt"), table("inc"), ptr("fcor"), ptr("ug"),
                                      ptr("vg"), a["dt"], a["grav"], a["cp_d"], None)

    def nudging(**kw):
        a, ptr, table = args(kw)
        return lib.pam_amd_ls_nudging(a["nens"], a["nx"], a["ny"], a["nz"], table("fields"), table("target"), table("rate"), a["dt"],
                                      table("inc"), None)
    return lib, arrays, P, forcing, nudging


def test_entry_points_reject_bad_arguments_and_leave_the_arrays_untouched():
    """the pointers are host arrays here: a refusal comes before the first HIP call, so nothing dereferences them, and afterwards every
    array still holds the pattern it was filled with"""
    lib, arrays, P, forcing, nudging = _abi()
    bad = (0.0, -1.0, math.nan, math.inf)
    calls = [dict(nens=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=70000, ny=70000)]
    calls += [{n: None} for n in ("u", "v", "temp", "rd", "rv", "zmid")]
    calls += [dict(ntr=-1), dict(ntr=65), dict(tracers=None), dict(positive=None), dict(tracers=["tr0", None, "tr1"])]
    calls += [dict(ug=None), dict(vg=None), dict(fcor=None), dict(ug=None, vg=None)]
    calls += [{n: b} for n in ("dt", "grav", "cp_d") for b in bad]
    calls += [dict(tracers=["tr0", "tr1", "spare"]), dict(ntr=0, tracers=None, positive=None),           # the vapour's increments without the vapour
              dict(tracers=["tr0", "tr1", "spare"], inc=None)]
    # an output that overlaps a read-only input or another output: whole arrays, and one element at either end
    last = 8 * CELLS - 8
    calls += [dict(u="v"), dict(temp="u"), dict(u="rd"), dict(v=P["rd"] + last), dict(temp=P["zmid"] + 8 * ROWS - 8), dict(wsub="temp"),
              dict(tt=P["u"] + last), dict(fcor=P["v"] + last), dict(ug=P["tr0"] + last), dict(inc=["inc_t", "inc_q", "inc_u", "tr1"]),
              dict(tracers=["tr0", "rv", "tr0"]), dict(tracers=["tr0", "rv", "rv"]), dict(tracers=["tr0", "rv", "u"]),
              dict(tracers=["tr0", "rv", P["rd"] + last]), dict(tracers=["rd", "rv", "tr1"]), dict(rd=P["rv"] + last), dict(zmid=P["rv"] + last)]
    for i, kw in enumerate(calls):
        assert forcing(**kw) == -1, (i, kw)                        # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert lib.pam_amd_awfl_last_error().startswith(b"ls_forcing: "), i
        assert all((a == 7.25).all() for a in arrays), i
    calls = [dict(nens=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=70000, ny=70000), dict(nz=65536)]
    calls += [dict(fields=None), dict(target=None), dict(rate=None), dict(inc=None)]
    calls += [dict(dt=b) for b in bad]
    calls += [dict(rate=["rate_t", None, "rate_uv", "rate_uv"]), dict(inc=["inc_t", "inc_q", None, "inc_v"]),
              dict(target=["tgt_t", None, "tgt_u", "tgt_v"]),                                            # an inc without its target
              dict(fields=[None, "rd", "rv", "u", "v"]), dict(fields=["temp", None, "rv", "u", "v"]), dict(fields=["temp", "rd", None, "u", "v"]),
              dict(fields=["temp", "rd", "rv", None, "v"]), dict(fields=["temp", "rd", "rv", "u", None]),
              dict(inc=["inc_t", "inc_t", "inc_u", "inc_v"]), dict(inc=["inc_t", "inc_q", "inc_u", P["inc_u"] + 8 * ROWS - 8]),
              dict(inc=["tgt_t", "inc_q", "inc_u", "inc_v"]), dict(inc=["inc_t", "rate_uv", "inc_u", "inc_v"]),
              dict(inc=["inc_t", "inc_q", "inc_u", P["v"] + last]), dict(inc=["inc_t", "inc_q", P["rd"], "inc_v"])]
    for i, kw in enumerate(calls):
        assert nudging(**kw) == -1, (i, kw)
        assert lib.pam_amd_awfl_last_error().startswith(b"ls_nudging: "), i
        assert all((a == 7.25).all() for a in arrays), i


def test_entry_points_name_themselves_when_there_is_no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    lib, arrays, P, forcing, nudging = _abi()
    none4 = [None] * 4
    for kw in (dict(), dict(wsub=None), dict(tt=None), dict(qt=None), dict(inc=None), dict(fcor=None, ug=None, vg=None),
               dict(ntr=0, tracers=None, positive=None, qt=None, inc=["inc_t", None, "inc_u", "inc_v"]), dict(nz=1), dict(ntr=1, tracers=["rv"]),
               dict(wsub=None, tt=None, qt=None, inc=None), dict(wsub=None, tt=None, qt=None, fcor=None, ug=None, vg=None),
               dict(fcor=P["v"] + 8 * CELLS)):
        assert forcing(**kw) == -2, kw
        assert lib.pam_amd_awfl_last_error() == b"ls_forcing: no HIP device available (this library has no CPU path)"
    for kw in (dict(), dict(target=["tgt_t", None, None, None], rate=["rate_t", None, None, None], inc=["inc_t", None, None, None],
                            fields=["temp", None, None, None, None]),
               dict(target=[None, "tgt_q", None, None], rate=none4[:1] + ["rate_q", None, None], inc=[None, "inc_q", None, None],
                    fields=[None, "rd", "rv", None, None]), dict(nz=1)):
        assert nudging(**kw) == -2, kw
        assert lib.pam_amd_awfl_last_error() == b"ls_nudging: no HIP device available (this library has no CPU path)"
    # nothing to do is no error and asks for no device
    assert nudging(target=none4, rate=none4, inc=none4) == 0
    assert forcing(wsub=None, tt=None, qt=None, inc=None, fcor=None, ug=None, vg=None) == 0
    assert all((a == 7.25).all() for a in arrays)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the layers above: the Python functions on a host coupler, the C++ module, the driver, the tool, the documents

def _host_coupler(nz=4, ny=2, nx=3, nens=5):
    from pam_amd import PamCoupler
    coupler = PamCoupler("cpu")
    coupler.set_option("crm_dt", 10.0)
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    zint = ((np.arange(nz + 1) / nz) ** 1.5 * 9000.0)[:, None] * (1.0 + 0.05 * np.arange(nens))[None, :]
    coupler.set_grid(1000.0 * nx, 1000.0 * ny, zint)
    zmid = 0.5 * (zint[:-1] + zint[1:])
    return coupler, zmid


def test_init_registers_what_is_given_and_nothing_else():
    from pam_amd import modules
    coupler, zmid = _host_coupler()
    dm = coupler.get_data_manager_device_readwrite()
    w = np.array([-0.01, -0.02, 0.03, 0.0])
    rate = np.full((4, 5), 1.0e-3) * (1.0 + np.arange(5))
    modules.ls_forcing_init(coupler, wsub=w, nudge_temp=np.full(4, 300.0), nudge_rate_temp=rate, ug=np.full(4, 5.0), vg=np.zeros(4), fcor=1.0e-4)
    want = {"ls_wsub", "ls_nudge_temp", "ls_nudge_rate_temp", "ls_ug", "ls_vg", "ls_fcor", "ls_inc_temp"}
    every = {n for n, _ in modules.LS_PROFILES} | set(modules.LS_INCREMENTS) | {"ls_fcor"}
    assert {n for n in every if dm.entry_exists(n)} == want
    assert tuple(dm.get("ls_wsub").shape) == (4, 5) and tuple(dm.get("ls_fcor").shape) == (5,)
    assert (dm.get("ls_wsub").numpy() == w[:, None]).all() and (dm.get("ls_fcor").numpy() == 1.0e-4).all()
    assert ref.same_bits(dm.get("ls_nudge_rate_temp").numpy(), rate)
    dz = (zmid[1:] - zmid[:-1]).min(axis=0)
    assert coupler.get_option("ls_courant_rate") == float((0.03 / dz).max()) and coupler.get_option("ls_nudge_rate_max") == 5.0e-3
    assert len(modules.LS_PROFILES) == 12 and len(set(modules.LS_RATES)) == 3


def test_the_wrappers_refuse_a_step_that_is_too_long_and_an_incomplete_set():
    from pam_amd import modules
    from pam_amd.capi import PamAmdError
    coupler, zmid = _host_coupler()
    with pytest.raises(PamAmdError, match="call ls_forcing_init first"):
        modules.ls_forcing(coupler)
    dzmin = float((zmid[1:] - zmid[:-1]).min())
    modules.ls_forcing_init(coupler, wsub=np.array([0.0, -0.11 * dzmin, 0.0, 0.0]))
    with pytest.raises(PamAmdError, match="exceeds the thinnest layer"):
        modules.ls_forcing(coupler)                                  # crm_dt 10: a Courant number of 1.1
    with pytest.raises(PamAmdError, match="exceeds the thinnest layer"):
        modules.ls_forcing(coupler, dt=9.5)
    coupler, _ = _host_coupler()
    modules.ls_forcing_init(coupler, nudge_u=np.zeros(4), nudge_rate_uv=np.array([0.0, 0.05, 0.1001, 0.0]))
    with pytest.raises(PamAmdError, match="nudging rate exceeds 1"):
        modules.ls_forcing(coupler)
    for kw in (dict(ug=np.zeros(4)), dict(ug=np.zeros(4), vg=np.zeros(4)), dict(fcor=1.0e-4), dict(nudge_temp=np.zeros(4)),
               dict(nudge_v=np.zeros(4)), dict(wsub=np.zeros(3)), dict(wsub=np.zeros((4, 4))), dict(ug=np.zeros(4), vg=np.zeros(4), fcor=np.zeros(3))):
        coupler, _ = _host_coupler()
        with pytest.raises(PamAmdError, match="ls_forcing_init"):
            modules.ls_forcing_init(coupler, **kw)


def test_cxx_module_compiles(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "modules/large_scale_forcing.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  modules::LsProfiles p;\n  p.wsub = {0.0, 0.0};\n"
                   "  modules::ls_forcing_init(coupler, p);\n  modules::ls_forcing(coupler);\n  modules::ls_forcing(coupler, 5.0);\n  return 0;\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cxx_program_builds_and_the_entry_points_answer_without_a_device():
    """tests/cxx/ls_forcing.cpp builds against the header and the library; without a file it hands both entry points host arrays that pass
    every check, so where there is no device both return PAM_AMD_ENOGPU.  (The coupler of the C++ layer allocates on the device, so its
    entries are registered, and the module run against the restatement, in tests/test_lsforcing_gpu.py.)"""
    import torch
    r = subprocess.run([cxx_program("ls_forcing")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-500:])
    if not torch.cuda.is_available():
        assert r.stdout.strip() == "### rc -2 -2"
    r = subprocess.run([cxx_program("ls_forcing"), "one"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2


def test_cxx_module_and_python_functions_name_the_same_entries_and_options():
    import inspect
    from pam_amd import modules
    text = open(os.path.join(HOST, "modules", "large_scale_forcing.h")).read()
    py = inspect.getsource(modules)
    for n, desc in modules.LS_PROFILES:
        assert '"%s"' % n in text and desc in text, n
    for s in ('"ls_fcor"', '"ls_inc_temp"', '"ls_inc_qv"', '"ls_inc_u"', '"ls_inc_v"', '"ls_courant_rate"', '"ls_nudge_rate_max"',
              '"vertical_midpoint_height"', "pam_amd_ls_nudging(", "pam_amd_ls_forcing("):
        assert s in text and s in py, s


def test_driver_bench_tool_and_documents_know_the_forcing():
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert drv.count('"--ls-forcing"') == 1 and drv.count('"--coriolis"') == 1 and drv.count("[--ls-forcing PATH [--coriolis F]]") >= 2
    assert "ls forcing: etime" in drv
    assert drv.index("modules::sponge_layer);") < drv.index("modules::ls_forcing(c)") < drv.index("modules::compute_surface_fluxes(c)")
    tool = open(os.path.join(ROOT, "tools", "bench_modules.py")).read()
    assert '"lsforcing"' in tool and "pam_amd_ls_forcing" in tool and "pam_amd_ls_nudging" in tool
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ls_forcing" in open(os.path.join(ROOT, doc)).read(), doc
