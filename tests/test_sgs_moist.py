"""The moist branch of the Smagorinsky SGS closure and the surface fluxes of heat and vapour in its solve, everything that needs no GPU:
the numpy restatement (tests/sgs_moist_ref.py) against its scalar-loop twin; the device bodies under g++ (tests/emu/sgs_moist_emu.cpp)
against the restatement bit for bit on every shape, named case and placement of c', and at strides that need 64-bit offsets; the census
of what the named cases reach; exp_c against math.exp; the equivalences with the dry entry points; the physics of the two frequencies; the
column sums the fluxes change; the mutants; the C ABI's refusals; the C++ plug-in class and its Python mirror."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import sgs_ref as ref
import sgs_moist_ref as mref
from sgs_emu_harness import EmuBackend as DryEmuBackend
from sgs_moist_emu_harness import PATHS, EmuBackend, exp_c as emu_exp_c, load
from pam_amd import capi
from tools.native_build import syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
U = 2.0 ** -53
LD = np.longdouble
COEF_CASES = ("kessler_set", "p3_set", "cloud_only", "threshold_positive")      # cases with a cloud table and finite fields


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the restatement itself, and the device bodies under g++

@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_restatement_is_the_scalar_loop(shape):
    """the vectorised form against one Python float at a time; the larger shapes on a selection of members (members are independent)"""
    idx = list(range(shape[3])) if np.prod(shape) < 500 else [0, 1, 63, shape[3] - 1]
    for name in ("p3_set", "precip_only", "empty_tables", "threshold_positive", "nan_cell", "vapour_last_with_lhf", "downward_lhf"):
        case = mref.cases(shape)[name]
        want = {n: np.ascontiguousarray(a[..., idx]) for n, a in mref.reference(shape, name).items()}
        sub = mref.members(case, idx)
        assert mref.results_differ(mref.run_case(mref.ScalarBackend(), sub), want) == [], name


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape):
    """every named case with c' in LDS rows of 64 lanes, in LDS rows of 5 lanes and in the workspace; the solve in place, the vapour
    aliased into the tracer table and the latent flux at the vapour's index, as the entry point has them"""
    for name in mref.CASE_NAMES:
        want = mref.reference(shape, name)
        for path in PATHS:
            got = mref.run_case(EmuBackend(path), mref.cases(shape)[name])
            assert mref.results_differ(got, want) == [], (name, path)


def _sparse(nbytes):
    """address space without memory behind it: only the pages a test touches are ever committed"""
    import mmap
    noreserve = getattr(mmap, "MAP_NORESERVE", 0x4000)
    m = mmap.mmap(-1, nbytes, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | noreserve)
    return m, C.addressof(C.c_char.from_buffer(m))


def _cell(addr, offset):
    return C.c_double.from_address(addr + 8 * offset)


def test_emulation_at_strides_that_need_64_bit_offsets():
    """one column of three levels whose levels lie 2^31 + 5 elements apart at a flat index inside the level beyond 2^31: the solve with
    both fluxes (the fluxes at that flat index too, the vapour beyond the fields kept in registers), then the moist coefficient walk with
    two cloud species and one precipitating.  A 32-bit product anywhere in the new code reads or writes another cell, or none."""
    lib = load()
    shape = (3, 1, 2, 65)
    case = mref.cases(shape)["vapour_last_with_lhf"]
    want = mref.reference(shape, "vapour_last_with_lhf")
    k1, k2 = mref.coefficients(case)
    e, i = 3, 1
    level, off = 2 ** 31 + 5, 2 ** 31 + 64
    names = ("uvel", "vvel", "wvel", "temp", "density_dry") + case["tracers"]          # the vapour is the last of them
    m, addr = _sparse(8 * (4 * level + off))
    base = {n: 32 * a for a, n in enumerate(names + ("tk", "tkh", "cp", "zint", "zmid", "shf", "lhf"))}
    for n in names:
        for k in range(3):
            _cell(addr, base[n] + off + k * level).value = case["fields"][n][k, 0, i, e]
    for k in range(3):
        _cell(addr, base["tk"] + off + k * level).value = k1[k, 0, i, e]
        _cell(addr, base["tkh"] + off + k * level).value = k2[k, 0, i, e]
        _cell(addr, base["zmid"] + k * level).value = case["zmid"][k, e]
    for k in range(4):
        _cell(addr, base["zint"] + k * level).value = case["zint"][k, e]
    _cell(addr, base["shf"] + off).value = case["sfc_shf"][0, i, e]
    _cell(addr, base["lhf"] + off).value = case["sfc_lhf"][0, i, e]
    at = lambda n: addr + 8 * base[n]
    gc = case["grav"] / case["cp_d"]
    tr = case["tracers"]
    for cls, fields, sfc, K, scale in ((0, ref.WINDS, (None, None, None), "tk", 0.0), (1, ("temp",), ("shf",), "tkh", case["cp_d"]),
                                       (2, tr, tuple("lhf" if n == "water_vapor" else None for n in tr), "tkh", case["latvap"])):
        table = (C.c_void_p * len(fields))(*[at(n) for n in fields])
        stab = (C.c_void_p * len(fields))(*[None if s is None else at(s) for s in sfc])
        lib.emu_sgs_flux_solve_at(cls, table, len(fields), stab, off, at("density_dry"), at("water_vapor"), at(K), at("zint"), at("zmid"), level,
                                  level, 3, case["dt"], gc, at("cp"), level, scale)
    assert off + 2 * level > 2 ** 32 and tr.index("water_vapor") >= 4
    for n in ("wvel", "temp") + tr:
        got = np.array([_cell(addr, base[n] + off + k * level).value for k in range(3)])
        assert mref.same_bits(got, want[n][:, 0, i, e]), n
    del m
    # the coefficient walk: levels 2^31 + 5 apart, two cells along x, one member
    sub = mref.members(case, [e])
    wtk, wtkh = mref.coefficients(sub)
    m, addr = _sparse(8 * (4 * level + 1024))
    fields = ref.WINDS + ("temp", "density_dry", "water_vapor") + case["cloud"] + case["precip"]
    base = {n: 16 * a for a, n in enumerate(fields + ("tk", "tkh", "zint", "zmid"))}
    for n in fields:
        for k in range(3):
            for x in range(2):
                _cell(addr, base[n] + k * level + x).value = sub["fields"][n][k, 0, x, 0]
    for k in range(4):
        _cell(addr, base["zint"] + k).value = sub["zint"][k, 0]
    for k in range(3):
        _cell(addr, base["zmid"] + k).value = sub["zmid"][k, 0]
    at = lambda n: addr + 8 * base[n]
    table = (C.c_void_p * 6)(*[at(n) for n in fields[:6]])
    cloud = (C.c_void_p * 4)(*[at(n) for n in case["cloud"]])
    precip = (C.c_void_p * 8)(*[at(n) for n in case["precip"]])
    for x in range(2):
        lib.emu_sgs_moist_coef_at(table, len(case["cloud"]), cloud, len(case["precip"]), precip, at("zint"), at("zmid"), level, 1, 2, 1, 3, 0, x, 0,
                                  case["dx"], case["dy"], case["grav"], case["cp_d"], case["R_d"], case["R_v"], case["cloud_threshold"], case["cs"],
                                  case["prandtl"], at("tk"), at("tkh"))
    got = np.array([[_cell(addr, base["tk"] + k * level + x).value for x in range(2)] for k in range(3)])
    got2 = np.array([[_cell(addr, base["tkh"] + k * level + x).value for x in range(2)] for k in range(3)])
    assert len(case["cloud"]) == 2 and mref.same_bits(got, wtk[:, 0, :, 0]) and mref.same_bits(got2, wtkh[:, 0, :, 0])
    del m


# ------------------------------------------------------------------------------------------------------------------------------
# 2. what the named cases reach

@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[0] >= 3], ids=ref.shape_id)
def test_census_of_the_named_cases(shape):
    """per case with a cloud table: saturated and unsaturated cells; the clamp arg < 0 reached and not reached in each branch; both
    branches together in at least half of the (level, 64-lane) groups where a level holds 64 lanes or more; every output finite.  The
    two-level shape is left out: its one column is cloudy at both ends by construction"""
    nz = shape[0]
    for name in COEF_CASES:
        case = mref.cases(shape)[name]
        sat = mref.stability(case)[3]
        tk, tkh, arg = mref.coefficients(case, with_arg=True)
        assert sat.any() and not sat.all(), name
        for branch in (sat, ~sat):
            assert (arg[branch] < 0).any() and (arg[branch] >= 0).any(), name
        lev = sat.reshape(nz, -1)
        groups = [lev[k, g:g + 64] for k in range(nz) for g in range(0, lev.shape[1] - 63, 64)]
        assert groups and np.mean([g.any() and not g.all() for g in groups]) >= 0.5, name
        print("%s %s: saturated %.2f, clamped in cloud %.2f, outside %.2f, %d groups" % (ref.shape_id(shape), name, sat.mean(),
                                                                                         (arg[sat] < 0).mean(), (arg[~sat] < 0).mean(), len(groups)))
    for name in mref.CASE_NAMES:
        out = mref.reference(shape, name)
        if name == "nan_cell":
            assert np.isnan(out["tk"]).any() and not np.isnan(out["tk"]).all() and np.isnan(out["temp"]).any()
        else:
            assert all(np.isfinite(a).all() for a in out.values()), name


def test_named_cases_hold_what_they_are_named_for():
    shape = (7, 3, 5, 130)
    nz, ny, nx, nens = shape
    cs = mref.cases(shape)
    F = cs["kessler_set"]["fields"]
    assert 180 < F["temp"].min() < 210 and 300 < F["temp"].max() < 306          # "about 190 to 305 K": what the exponential must span
    for n in ("cloud_liquid", "cloud_water", "ice"):
        c = F[n]
        assert 0.2 < (c == 0).mean() < 0.8 and c[0, 0, 0, 0] > 0 and c[-1, -1, -1, -1] > 0, n
        for axis in (0, 1, 2, 3):                      # cloudy beside clear along every direction
            a, b = np.swapaxes(c, 0, axis)[:-1] > 0, np.swapaxes(c, 0, axis)[1:] > 0
            assert (a != b).mean() > 0.2, (n, axis)
    assert ((F["cloud_water"] == 0) & (F["ice"] > 0)).any() and ((F["cloud_water"] > 0) & (F["ice"] > 0)).any()
    assert [len(cs[n]["cloud"]) for n in ("kessler_set", "p3_set", "cloud_only", "precip_only", "empty_tables")] == [1, 2, 1, 0, 0]
    assert [len(cs[n]["precip"]) for n in ("kessler_set", "p3_set", "cloud_only", "precip_only", "empty_tables")] == [1, 1, 0, 1, 0]
    # the threshold: one cell holds exactly threshold rho and is unsaturated; cloud below it exists, and so does cloud above it
    t = cs["threshold_positive"]
    at = (0, ny // 2, nx // 2, nens // 3)
    c = t["fields"]["cloud_water"] + t["fields"]["ice"]
    rho = t["fields"]["density_dry"] + t["fields"]["water_vapor"]
    sat = mref.stability(t)[3]
    assert t["cloud_threshold"] > 0 and c[at] == t["cloud_threshold"] * rho[at] and c[at] > 0 and not sat[at]
    assert ((c > 0) & ~sat).sum() > 1 and sat.any()
    assert mref.stability(dict(t, cloud_threshold=np.nextafter(t["cloud_threshold"], 0.0)))[3][at]
    # a NaN cloud cell is unsaturated (the comparison is false), a NaN temperature goes where the restatement puts it
    n = cs["nan_cell"]
    assert np.isnan(n["fields"]["cloud_liquid"]).sum() == 1 and not mref.stability(n)[3][nz - 1, 0, 0, 0]
    assert cs["shf_only"]["sfc_lhf"] is None and cs["lhf_only"]["sfc_shf"] is None and cs["fluxes_both"]["sfc_shf"] is not None
    assert (cs["fluxes_both"]["sfc_shf"] < 0).any() and (cs["fluxes_both"]["sfc_shf"] > 0).any()
    assert cs["vapour_last_with_lhf"]["tracers"].index("water_vapor") == 6
    down = mref.reference(shape, "downward_lhf")["water_vapor"]
    assert (cs["downward_lhf"]["sfc_lhf"] < 0).all() and (down < 0).any() and (down[0] > 0).any() and np.isfinite(down).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the exponential

def test_exp_c_against_math_exp():
    """100 000 arguments of the saturation pressure from 150 K to 350 K (x from -18.1 to +4.2): at most 2 ulp from math.exp, which is
    within 1 ulp of the true value itself.  Deterministic CPU arithmetic: measured 1 ulp.  The emulated device body gives the same bits"""
    temp = np.linspace(150.0, 350.0, 100000)
    tc = temp - 273.15
    x = (17.625 * tc) / (243.04 + tc)
    assert x.min() < -18.0 and x.max() > 4.1
    y = mref.exp_c(x)
    want = np.array([math.exp(v) for v in x])
    ulps = np.abs(y - want) / np.spacing(want)
    print("exp_c: at most %.1f ulp from math.exp over [%.2f, %.2f]" % (ulps.max(), x.min(), x.max()))
    assert ulps.max() <= 2.0
    assert mref.same_bits(emu_exp_c(x), y)
    assert mref.same_bits(np.array([mref.scalar_exp_c(float(v)) for v in x[::97]]), y[::97])
    wide = np.linspace(-700.0, 700.0, 20001)
    assert mref.same_bits(emu_exp_c(wide), mref.exp_c(wide))


def test_exp_c_special_arguments():
    x = np.array([np.nan, -700.5, -1.0e300, -np.inf, 700.5, 1.0e300, np.inf, 0.0, -700.0, 700.0])
    for y in (mref.exp_c(x), emu_exp_c(x), np.array([mref.scalar_exp_c(float(v)) for v in x])):
        assert np.isnan(y[0]) and (y[1:4] == 0.0).all() and not np.signbit(y[1:4]).any() and (y[4:7] == np.inf).all() and y[7] == 1.0
        assert 0.0 < y[8] < 1.0e-303 and 1.0e303 < y[9] < np.inf
    assert mref.same_bits(mref.exp_c(x), emu_exp_c(x))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the equivalences with the dry entry points

@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_empty_tables_and_null_fluxes_give_the_dry_bits(shape):
    """the moist coefficients with both tables empty are sgs_ref.coefficients, and the flux solve with both fluxes NULL is
    sgs_ref.diffuse: in the restatement, and in the emulated device bodies on every placement of c' (against the dry bodies too)"""
    case = mref.cases(shape)["empty_tables"]
    assert case["sfc_shf"] is None and case["sfc_lhf"] is None and case["sfc_flx_u"] is not None
    tk, tkh = ref.coefficients(case)
    want = dict(ref.diffuse(case, tk, tkh), tk=tk, tkh=tkh)
    assert mref.results_differ(mref.reference(shape, "empty_tables"), want) == []
    for path in PATHS:
        assert mref.results_differ(mref.run_case(EmuBackend(path), case), want) == [], path
        dry = DryEmuBackend(path)
        got = dict(dry.diffuse(case, tk, tkh))
        got["tk"], got["tkh"] = dry.coefficients(case)
        assert mref.results_differ(got, want) == [], path
    # a nonzero threshold and the gas constants change nothing without a cloud table
    assert mref.results_differ(mref.run_case(EmuBackend(), dict(case, cloud_threshold=0.5, R_d=1.0, R_v=2.0)), want) == []


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the physics of the two frequencies

def _column(t0, p0, gamma, nz=5, dz=100.0, cloud=1.0e-4, rain=0.0):
    """a hydrostatic-looking saturated column: temp = t0 - gamma z, the vapour at saturation, dry density from p0 at the ground"""
    zint = np.arange(nz + 1)[:, None] * dz + np.zeros((nz + 1, 1))
    zmid = 0.5 * (zint[:-1] + zint[1:])
    shape = (nz, 1, 1, 1)
    z = zmid[:, None, None, :] + np.zeros(shape)
    temp = t0 - gamma * z
    p = p0 * np.exp(-ref.GRAV * z / (mref.R_D * t0))
    tc = temp - 273.15
    es = 610.94 * np.exp(17.625 * tc / (243.04 + tc))
    rho_v = es / (mref.R_V * temp)
    rho_d = (p - es) / (mref.R_D * temp)
    zero = np.zeros(shape)
    fields = dict(uvel=zero, vvel=zero, wvel=zero, temp=temp, density_dry=rho_d, water_vapor=rho_v, cloud_liquid=np.full(shape, cloud),
                  precip_liquid=np.full(shape, rain))
    return dict(fields=fields, tracers=(), cloud=("cloud_liquid",), precip=("precip_liquid",), zint=zint, zmid=zmid, dx=ref.DX, dy=ref.DY,
                grav=ref.GRAV, cp_d=ref.CP_D, cs=ref.CS, prandtl=ref.PRANDTL, dt=ref.DT, R_d=mref.R_D, R_v=mref.R_V, latvap=mref.LATVAP,
                cloud_threshold=0.0)


def test_saturated_and_unsaturated_frequency_on_hand_made_columns():
    """290 K, 900 hPa, 6.5 K/km: steeper than the moist adiabat (about 4.6 K/km there), less steep than the dry one: the saturated N2 is
    negative and the unsaturated one positive (the prototype: -5.9e-5 and +1.1e-4 / s2).  At 230 K there is hardly any vapour left to
    condense, so the two agree in sign and the saturated one is the smaller"""
    warm = _column(290.0, 90000.0, 0.0065)
    n2, unsat, satn2, sat = mref.stability(warm)
    print("290 K: saturated N2 %.3e, unsaturated N2 %.3e" % (satn2[2, 0, 0, 0], unsat[2, 0, 0, 0]))
    assert sat.all() and (satn2 < 0).all() and (unsat > 0).all() and mref.same_bits(n2, satn2)
    assert -1.0e-4 < satn2[2, 0, 0, 0] < -3.0e-5 and 0.8e-4 < unsat[2, 0, 0, 0] < 1.4e-4
    tk_moist = mref.coefficients(warm)[0]
    tk_dry = mref.coefficients(dict(warm, cloud=(), precip=()))[0]
    assert (tk_moist > 0).all() and (tk_dry == 0).all()                  # the dry closure switches the mixing off inside this cloud
    cold = _column(230.0, 40000.0, 0.0065)
    n2, unsat, satn2, sat = mref.stability(cold)
    print("230 K: saturated N2 %.3e, unsaturated N2 %.3e" % (satn2[2, 0, 0, 0], unsat[2, 0, 0, 0]))
    assert sat.all() and (satn2 > 0).all() and (unsat > 0).all() and (satn2 < unsat).all()


def test_precipitation_lowers_trho_by_temp_times_its_mixing_ratio():
    """precip_only: never saturated, and Trho = temp ((1 + 0.608 qv) - ql) lies below the dry Tv = temp (1 + 0.608 qv) by temp ql up to
    the roundings of f - ql and of the two products: 3 u Tv"""
    for shape in ref.SHAPES:
        case = mref.cases(shape)["precip_only"]
        F = case["fields"]
        trho, qt, c, rho = mref.thermo(case, F)
        assert c is None and mref.stability(case)[3] is None
        tv = ref.virtual_temp(F["temp"], F["density_dry"], F["water_vapor"])
        ql = F["precip_liquid"].astype(LD) / rho.astype(LD)
        err = np.abs((tv.astype(LD) - trho.astype(LD)) - F["temp"].astype(LD) * ql)
        assert (err <= 3 * U * np.abs(tv)).all() and (trho[F["precip_liquid"] > 0] < tv[F["precip_liquid"] > 0]).all()
        assert mref.same_bits(trho[F["precip_liquid"] == 0], tv[F["precip_liquid"] == 0])


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the column sums the fluxes change

@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_the_fluxes_add_what_they_carry_to_the_column_sums(shape):
    """S rho dz temp over a column grows by dt sfc_shf / cp_d and S dz rho_v by dt sfc_lhf / latvap.  The solve keeps w^T x = w^T r to the
    bound of tests/test_sgs_smag.py (18 u of the magnitudes of the rows, plus the right-hand side of temp and the sums' own error in
    np.longdouble); here r holds the flux term, whose own formation adds 4 roundings of the term: 4 u w(0) |term|.  Measured against the
    flux itself in np.longdouble"""
    case = mref.cases(shape)["fluxes_both"]
    got = mref.reference(shape, "fluxes_both")
    F = case["fields"]
    nz = shape[0]
    k1, k2 = mref.coefficients(case)
    rho = F["density_dry"] + F["water_vapor"]
    dz = (case["zint"][1:] - case["zint"][:-1])[:, None, None, :]
    gc = case["grav"] / case["cp_d"]
    dt = LD(case["dt"])
    worst = 0.0
    for n, cls, flux in (("temp", "heat", case["sfc_shf"].astype(LD) / LD(case["cp_d"])), ("water_vapor", "tracer", case["sfc_lhf"].astype(LD) / LD(case["latvap"]))):
        lower, diag, upper, dzf_m, dzf_p, _ = ref.rows(cls, rho, k2, case["zint"], case["zmid"], case["dt"])
        w = (dz + 0 * rho if cls == "tracer" else rho * dz).astype(LD)
        x, r = got[n].astype(LD), F[n].astype(LD)
        xm, xp = np.concatenate([x[:1], x[:-1]]), np.concatenate([x[1:], x[-1:]])
        lim = 18 * U * (w * (np.abs(lower * xm) + np.abs(diag * x) + np.abs(upper * xp))).sum(axis=0)
        if cls == "heat":
            lim = lim + U * (w * (4 * gc * (np.abs(upper * dzf_p) + np.abs(lower * dzf_m)) + np.abs(r) + gc * 1.0e4)).sum(axis=0)
        lim = lim + 2 * nz * LD(2.0) ** -64 * (w * (np.abs(x) + np.abs(r))).sum(axis=0) + 4 * U * np.abs(dt * flux)
        gain = (w * x).sum(axis=0) - (w * r).sum(axis=0)
        err = np.abs(gain - dt * flux)
        assert (err <= lim).all(), (n, float((err / lim).max()))
        assert (np.abs(gain) > 100 * lim).mean() > 0.9, n                 # the gain itself is far above the bound: the test sees it
        worst = max(worst, float((err / lim).max()))
    print("worst fraction of the bound %.3f" % worst)
    # every other field is the solve without the two fluxes
    plain = mref.run_case(mref.RefBackend(), dict(case, sfc_shf=None, sfc_lhf=None))
    assert sorted(mref.results_differ(got, plain)) == ["temp", "water_vapor"]


# ------------------------------------------------------------------------------------------------------------------------------
# 7. the mutants of the restatement

CAUGHT_BY = dict(branch_ge=("threshold_positive", "tk"), qs_without_rho=("kessler_set", "tk"), loading_dropped=("precip_only", "tk"),
                 dqt_dropped=("kessler_set", "tk"), second_cloud_ignored_in_sat=("p3_set", "tk"), branch_on_upper_neighbour=("threshold_positive", "tk"),
                 exp_degree_12=("p3_set", "tk"), shf_without_rho=("shf_only", "temp"), lhf_divided_by_rho=("lhf_only", "water_vapor"),
                 flux_at_top=("fluxes_both", "temp"))
# what the one column of two cloudy cells cannot show: a cell with cloud in the second species alone, and one of the few arguments at
# which the last term of the exponential changes the rounding
NOT_AT_TWO_CELLS = ("second_cloud_ignored_in_sat", "exp_degree_12")


@pytest.mark.parametrize("mutant", mref.MUTANTS)
def test_every_mutant_is_caught_by_a_named_case(mutant):
    """each wrong line changes the bits of its named case on every shape; a mutant of the solve leaves the coefficients alone and one of
    the coefficients leaves the solve alone (the solve is judged on the restatement's coefficients)"""
    assert set(CAUGHT_BY) == set(mref.MUTANTS)
    name, field = CAUGHT_BY[mutant]
    for shape in ref.SHAPES:
        if shape == (2, 1, 1, 1) and mutant in NOT_AT_TWO_CELLS:
            continue
        got = mref.run_case(mref.RefBackend(mutant), mref.cases(shape)[name])
        diff = mref.results_differ(got, mref.reference(shape, name))
        assert field in diff, (shape, diff)
        assert set(diff) <= ({"tk", "tkh"} if field == "tk" else {"temp", "water_vapor"}), (shape, diff)


# ------------------------------------------------------------------------------------------------------------------------------
# 8. the C ABI: refusals before any device is asked for; the symbols

NEW_SYMBOLS = ("pam_amd_sgs_smag_coefficients_moist", "pam_amd_sgs_smag_diffuse_fluxes")


def test_entry_points_are_exported_and_declared_and_the_abi_stays_5():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    assert lib.pam_amd_awfl_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read()
    assert "a moist N2 is left for later" not in header and "pam_amd_sgs_smag_coefficients_moist (below)" in header


def test_entry_points_reject_bad_arguments_and_leave_the_arrays_untouched():
    """the pointers are host arrays here: a refusal comes before the first HIP call, so nothing dereferences them, and afterwards every
    array still holds the pattern it was filled with"""
    lib = capi.load()
    n = 4 * 2 * 3 * 4                                              # nens 4, nx 3, ny 2, nz 4
    arrays = [np.full(n + 16, 7.25) for _ in range(20)]
    p = [a.ctypes.data for a in arrays]
    u, v, w, t, rd, rv, zi, zm, tk, tkh, su, sv, q1, q2, c1, c2, r1, shf, lhf = p[:19]
    tab = lambda size, *ptrs: (C.c_void_p * size)(*ptrs)
    C2, P1 = tab(4, c1, c2), tab(8, r1)
    T3 = tab(3, q1, rv, q2)                                        # the vapour itself in the table
    T2 = tab(2, q1, q2)                                            # and a table without it
    good = dict(dx=500.0, dy=500.0, grav=9.8, cp_d=1004.0, R_d=287.0, R_v=461.0, thr=0.0, cs=0.2, prandtl=0.33)

    def coef(nens=4, nx=3, ny=2, nz=4, ptrs=None, nc=2, cloud=C2, npr=1, precip=P1, out=None, **kw):
        a = dict(good)
        a.update(kw)
        ptrs = ptrs or [u, v, w, t, rd, rv]
        out = out or [tk, tkh]
        return lib.pam_amd_sgs_smag_coefficients_moist(nens, nx, ny, nz, *ptrs, nc, cloud, npr, precip, zi, zm, a["dx"], a["dy"], a["grav"], a["cp_d"],
                                                       a["R_d"], a["R_v"], a["thr"], a["cs"], a["prandtl"], *out, None)

    def dif(nens=4, nx=3, ny=2, nz=4, nt=3, table=T3, sfc=(su, sv), dt=10.0, grav=9.8, cp_d=1004.0, fl=(shf, lhf), latvap=2.5e6, temp=t):
        return lib.pam_amd_sgs_smag_diffuse_fluxes(nens, nx, ny, nz, u, v, w, temp, nt, table, rd, rv, tk, tkh, zi, zm, *sfc, dt, grav, cp_d, *fl, latvap,
                                                   None)

    calls = [lambda: coef(nc=-1), lambda: coef(nc=5), lambda: coef(npr=-1), lambda: coef(npr=9), lambda: coef(cloud=None), lambda: coef(precip=None),
             lambda: coef(cloud=tab(4, c1, None)), lambda: coef(precip=tab(8, None)), lambda: coef(nc=3, cloud=tab(4, c1, c2, None)),
             lambda: coef(out=[c1, tkh]), lambda: coef(out=[tk, r1 + 8]), lambda: coef(out=[tk, c2 + 8 * n - 8]), lambda: coef(thr=-1.0e-9),
             lambda: coef(thr=math.nan), lambda: coef(thr=math.inf), lambda: coef(nz=1), lambda: coef(nens=0),
             lambda: coef(ptrs=[u, v, w, None, rd, rv]), lambda: coef(out=[tk, None]), lambda: coef(out=[tk, tk])]
    for name in ("R_d", "R_v", "dx", "cp_d", "prandtl"):
        calls += [lambda name=name, bad=bad: coef(**{name: bad}) for bad in (0.0, -1.0, math.nan, math.inf)]
    calls += [lambda bad=bad: dif(latvap=bad) for bad in (0.0, -1.0, math.nan, math.inf)]
    calls += [lambda: dif(nt=2, table=T2), lambda: dif(nt=0, table=None), lambda: dif(fl=(t, lhf)), lambda: dif(fl=(shf, q1)),
              lambda: dif(fl=(u + 8, None)), lambda: dif(nz=1), lambda: dif(nt=-1), lambda: dif(temp=None), lambda: dif(dt=0.0),
              lambda: dif(nt=2, table=T2, fl=(None, lhf))]
    for i, call in enumerate(calls):
        assert call() == -1, i                                     # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert all((a == 7.25).all() for a in arrays), i
    assert b"sgs_smag_diffuse_fluxes" in lib.pam_amd_awfl_last_error()
    assert coef(nc=5) == -1 and b"sgs_smag_coefficients_moist" in lib.pam_amd_awfl_last_error()
    # what is allowed gets past the argument checks.  Without a device the call then ends in PAM_AMD_ENOGPU and names itself; with one,
    # the host arrays here must not reach a kernel, so it is not made
    import torch
    if not torch.cuda.is_available():
        ok = [(lambda: coef(), b"sgs_smag_coefficients_moist"), (lambda: coef(nc=0, cloud=None, npr=0, precip=None), b"sgs_smag_coefficients_moist"),
              (lambda: coef(nc=0, cloud=None), b"sgs_smag_coefficients_moist"), (lambda: coef(thr=0.25), b"sgs_smag_coefficients_moist"),
              (lambda: dif(), b"sgs_smag_diffuse_fluxes"), (lambda: dif(fl=(None, None)), b"sgs_smag_diffuse_fluxes"),
              (lambda: dif(nt=2, table=T2, fl=(shf, None)), b"sgs_smag_diffuse_fluxes"), (lambda: dif(fl=(None, lhf), sfc=(None, None)), b"sgs_smag_diffuse_fluxes")]
        for call, who in ok:
            assert call() not in (0, -1)
            assert lib.pam_amd_awfl_last_error().startswith(who + b":"), lib.pam_amd_awfl_last_error()
            assert all((a == 7.25).all() for a in arrays)


# ------------------------------------------------------------------------------------------------------------------------------
# 9. the C++ plug-in class, its Python mirror, the driver, the tools

SGS_H = os.path.join(HOST, "physics", "sgs", "smag_amd", "SGS.h")


def test_cxx_class_compiles_in_one_translation_unit_with_the_moist_options(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "physics/micro/none/Microphysics.h"\n#include "physics/sgs/smag_amd/SGS.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  Microphysics micro;\n  SGS sgs;\n  micro.init(coupler);\n"
                   '  coupler.set_option<bool>("sgs_smag_moist", true);\n  coupler.set_option<bool>("sgs_smag_surface_fluxes", true);\n'
                   '  coupler.set_option<real>("sgs_smag_cloud_threshold", 1.0e-6);\n'
                   "  sgs.init(coupler);\n  sgs.timeStep(coupler);\n  sgs.finalize(coupler);\n  return (int)sgs.sgs_name().size();\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cxx_class_and_python_class_name_the_same_new_fields_and_options():
    from pam_amd import physics
    text, py = open(SGS_H).read(), inspect.getsource(physics.SGSSmagorinsky)
    names = ('"sgs_smag_moist"', '"sgs_smag_surface_fluxes"', '"sgs_smag_cloud_threshold"', '"sfc_shf"', '"sfc_lhf"', '"micro"', '"kessler"', '"p3"',
             '"cloud_liquid"', '"precip_liquid"', '"cloud_water"', '"ice"', '"rain"', '"R_d"', '"R_v"', '"latvap"', "2501000.0",
             "input surface sensible heat flux [W/m2]", "input surface latent heat flux [W/m2]", "pam_amd_sgs_smag_coefficients_moist",
             "pam_amd_sgs_smag_diffuse_fluxes", "pam_amd_sgs_smag_coefficients(", "pam_amd_sgs_smag_diffuse(")
    for s in names:
        assert s in text and s in py, s
    sig = inspect.signature(physics.SGSSmagorinsky.__init__).parameters
    assert list(sig)[1:] == ["cs", "prandtl", "moist", "surface_fluxes", "cloud_threshold"]
    assert sig["moist"].default is False and sig["surface_fluxes"].default is False and sig["cloud_threshold"].default == 0.0
    assert physics.SGSSmagorinsky.CONDENSATE == {"kessler": (("cloud_liquid",), ("precip_liquid",)), "p3": (("cloud_water", "ice"), ("rain",)),
                                                 "none": ((), ())}


def test_driver_bench_tool_and_documents_know_the_new_entry_points():
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert drv.count('"--sgs-smag"') == 1 and '"--sgs-moist"' in drv and '"--sfc-fluxes"' in drv
    assert drv.count("[--sgs-moist] [--sfc-fluxes SHF LHF]") >= 2
    tool = open(os.path.join(ROOT, "tools", "bench_modules.py")).read()
    assert '"sgs_coefficients_moist"' in tool and '"sgs_diffuse_fluxes"' in tool
    kern = open(os.path.join(ROOT, "pam_amd", "csrc", "modules_kernels.hip")).read()
    assert "sgs_coef_moist_kernel" in kern and "sgs_solve_flux_kernel" in kern
    table = open(os.path.join(ROOT, "profiles", "r15_sgs_moist_kernel_resources.txt")).read()
    rows = {l.split()[0]: l.split()[1:] for l in table.split("\n") if l.startswith("sgs_")}
    assert set(rows) == {"sgs_coef_kernel", "sgs_coef_moist_kernel", "sgs_solve_kernel<true>", "sgs_solve_kernel<false>", "sgs_solve_flux_kernel<true>",
                         "sgs_solve_flux_kernel<false>"}
    assert all(r[3] == "0" for r in rows.values())                 # no scratch in any of them
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "pam_amd_sgs_smag_coefficients_moist" in text and "pam_amd_sgs_smag_diffuse_fluxes" in text, doc
