"""The native Smagorinsky SGS closure, everything that needs no GPU: the numpy restatement of the contract (tests/sgs_ref.py) against its
scalar-loop twin; the device bodies under g++ (tests/emu/sgs_emu.cpp) against the restatement bit for bit on every shape, named case and
placement of c', and at strides that need 64-bit offsets; known answers of the coefficients and of the solve within measured bounds; the
conserved column sums within derived bounds; the mutants; the C ABI's refusals; the C++ plug-in class and its Python mirror."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import sgs_ref as ref
from sgs_emu_harness import PATHS, EmuBackend, load
from pam_amd import capi
from tools import native_build
from tools.native_build import syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
U = 2.0 ** -53
LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the restatement itself, and the device bodies under g++

@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_restatement_is_the_scalar_loop(shape):
    """the vectorised form against one Python float at a time; the two larger shapes on a slice of members (members are independent)"""
    for name in ("base", "vapour_last", "no_surface_flux", "zero_k_faces"):
        case = ref.cases(shape)[name]
        want = ref.reference(shape, name)
        members = list(range(shape[3])) if shape[3] <= 65 and np.prod(shape) < 3000 else [0, 1, 63, shape[3] - 1]
        sub = dict(case, fields={n: np.ascontiguousarray(a[..., members]) for n, a in case["fields"].items()},
                   zint=np.ascontiguousarray(case["zint"][:, members]), zmid=np.ascontiguousarray(case["zmid"][:, members]))
        for n in ("sfc_flx_u", "sfc_flx_v", "tk", "tkh"):
            if case.get(n) is not None:
                sub[n] = np.ascontiguousarray(case[n][..., members])
        got = ref.run_case(ref.ScalarBackend(), sub)
        assert ref.results_differ(got, {n: np.ascontiguousarray(a[..., members]) for n, a in want.items()}) == [], name


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape):
    """every named case with c' in LDS rows of 64 lanes, in LDS rows of 5 lanes and in the workspace; the solve in place, the vapour
    aliased into the tracer table as a caller of the C ABI has it"""
    for name in ref.CASE_NAMES:
        want = ref.reference(shape, name)
        for path in PATHS:
            got = ref.run_case(EmuBackend(path), ref.cases(shape)[name])
            assert ref.results_differ(got, want) == [], (name, path)


def test_named_cases_hold_what_they_are_named_for():
    """stable, neutral-to-unstable and calm levels in one column; per-member grids; the vapour first, in the middle and last, beyond the
    fields a thread keeps in registers; surface fluxes present and absent; a NaN cell"""
    shape = (7, 3, 5, 130)
    cs = ref.cases(shape)
    tk = ref.reference(shape, "base")["tk"]
    col = tk[:, 1, 2, 7]
    assert (col == 0).any() and (col > 0).any() and (tk == 0).mean() > 0.1 and (tk > 0).mean() > 0.1
    assert not np.array_equal(cs["base"]["zint"][:, 0], cs["base"]["zint"][:, 1])
    assert [c["tracers"].index("water_vapor") for c in (cs["base"], cs["vapour_middle"], cs["vapour_last"])] == [0, 2, 5]
    assert cs["no_surface_flux"]["sfc_flx_u"] is None and cs["base"]["sfc_flx_u"] is not None and cs["no_tracers"]["tracers"] == ()
    assert np.isnan(cs["nan_cell"]["fields"]["temp"]).sum() == 1
    nan = ref.reference(shape, "nan_cell")
    assert np.isnan(nan["tk"]).any() and not np.isnan(nan["tk"]).all() and np.isnan(nan["temp"][:, 1, 2, 65]).all()
    assert not np.isnan(nan["temp"][:, 0, 0, 0]).any()


def _sparse(nbytes):
    """address space without memory behind it: only the pages a test touches are ever committed"""
    import mmap
    noreserve = getattr(mmap, "MAP_NORESERVE", 0x4000)      # Linux's value where this Python does not name it
    m = mmap.mmap(-1, nbytes, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | noreserve)
    return m, C.addressof(C.c_char.from_buffer(m))


def _cell(addr, offset):
    return C.c_double.from_address(addr + 8 * offset)


def test_emulation_at_strides_that_need_64_bit_offsets():
    """one column of three levels whose levels lie 2^31 + 5 elements apart, at a flat index inside the level beyond 2^31, and whose c' rows
    lie as far apart: a 32-bit product anywhere in sgs_device.h reads or writes another cell, or none.  The arrays are interleaved in one
    sparse mapping (array a at element a), and what comes back is held to the restatement on the dense column."""
    lib = load()
    shape = (3, 1, 2, 65)
    case = ref.cases(shape)["vapour_last"]
    want = ref.reference(shape, "vapour_last")
    k1, k2 = ref.coefficients(case)
    e, i = 3, 1
    level, off = 2 ** 31 + 5, 2 ** 31 + 64
    names = ("uvel", "vvel", "wvel", "temp", "density_dry") + case["tracers"]          # the vapour is the last of them
    m, addr = _sparse(8 * (4 * level + off))
    base = {n: 16 * a for a, n in enumerate(names + ("tk", "tkh", "cp", "zint", "zmid", "sfc_u", "sfc_v"))}
    for n in names:
        for k in range(3):
            _cell(addr, base[n] + off + k * level).value = case["fields"][n][k, 0, i, e]
    for k in range(3):
        _cell(addr, base["tk"] + off + k * level).value = k1[k, 0, i, e]
        _cell(addr, base["tkh"] + off + k * level).value = k2[k, 0, i, e]
        _cell(addr, base["zmid"] + k * level).value = case["zmid"][k, e]
    for k in range(4):
        _cell(addr, base["zint"] + k * level).value = case["zint"][k, e]
    _cell(addr, base["sfc_u"] + off).value = case["sfc_flx_u"][0, i, e]
    _cell(addr, base["sfc_v"] + off).value = case["sfc_flx_v"][0, i, e]
    at = lambda n: addr + 8 * base[n]
    gc = case["grav"] / case["cp_d"]
    for cls, fields, sfc, K in ((0, ref.WINDS, ("sfc_u", "sfc_v", None), "tk"), (1, ("temp",), None, "tkh"), (2, case["tracers"], None, "tkh")):
        table = (C.c_void_p * len(fields))(*[at(n) for n in fields])
        stab = None if sfc is None else (C.c_void_p * 3)(*[None if s is None else at(s) for s in sfc])
        lib.emu_sgs_solve_at(cls, table, len(fields), stab, off, at("density_dry"), at("water_vapor"), at(K), at("zint"), at("zmid"), level, level,
                             3, case["dt"], gc, at("cp"), level)
    assert off + 2 * level > 2 ** 32 and len(case["tracers"]) > 4
    for n in ref.WINDS + ("temp",) + case["tracers"]:
        got = np.array([_cell(addr, base[n] + off + k * level).value for k in range(3)])
        assert ref.same_bits(got, want[n][:, 0, i, e]), n
    del m
    # the coefficient walk: levels 2^31 + 5 apart, two cells along x, one member
    sub = dict(case, fields={n: np.ascontiguousarray(a[..., e:e + 1]) for n, a in case["fields"].items()}, zint=case["zint"][:, e:e + 1],
               zmid=case["zmid"][:, e:e + 1])
    wtk, wtkh = ref.coefficients(sub)
    m, addr = _sparse(8 * (4 * level + 1024))
    six = ref.WINDS + ("temp", "density_dry", "water_vapor")
    base = {n: 16 * a for a, n in enumerate(six + ("tk", "tkh", "zint", "zmid"))}
    for n in six:
        for k in range(3):
            for x in range(2):
                _cell(addr, base[n] + k * level + x).value = sub["fields"][n][k, 0, x, 0]
    for k in range(4):
        _cell(addr, base["zint"] + k).value = sub["zint"][k, 0]
    for k in range(3):
        _cell(addr, base["zmid"] + k).value = sub["zmid"][k, 0]
    table = (C.c_void_p * 6)(*[addr + 8 * base[n] for n in six])
    for x in range(2):
        lib.emu_sgs_coef_at(table, addr + 8 * base["zint"], addr + 8 * base["zmid"], level, 1, 2, 1, 3, 0, x, 0, case["dx"], case["dy"], case["grav"],
                            case["cp_d"], case["cs"], case["prandtl"], addr + 8 * base["tk"], addr + 8 * base["tkh"])
    got = np.array([[_cell(addr, base["tk"] + k * level + x).value for x in range(2)] for k in range(3)])
    got2 = np.array([[_cell(addr, base["tkh"] + k * level + x).value for x in range(2)] for k in range(3)])
    assert ref.same_bits(got, wtk[:, 0, :, 0]) and ref.same_bits(got2, wtkh[:, 0, :, 0])
    del m


# ------------------------------------------------------------------------------------------------------------------------------
# 2. known answers of the coefficients.  Tolerances are measured, not picked: the same restatement in np.longdouble on the same float64
# inputs gives the float64 restatement's own rounding error d on the case; the gate is 4 d plus a floor for what the rounding of the INPUTS
# does to the analytic value (a few ulps of the largest term, carried through the formula), which d cannot see.

def _uniform_case(nz, ny, nx, nens, dz=256.0, temp=None, **kw):
    zint = np.arange(nz + 1)[:, None] * dz + np.zeros((nz + 1, nens))
    zmid = 0.5 * (zint[:-1] + zint[1:])
    shape = (nz, ny, nx, nens)
    z = zmid[:, None, None, :] + np.zeros(shape)
    gc = ref.GRAV / ref.CP_D
    fields = dict(uvel=np.zeros(shape), vvel=np.zeros(shape), wvel=np.zeros(shape), temp=300.0 - gc * z if temp is None else temp(z),
                  density_dry=np.full(shape, 1.0), water_vapor=np.zeros(shape))
    c = dict(fields=fields, tracers=(), zint=zint, zmid=zmid, dx=ref.DX, dy=ref.DY, grav=ref.GRAV, cp_d=ref.CP_D, cs=ref.CS, prandtl=ref.PRANDTL,
             dt=ref.DT, sfc_flx_u=None, sfc_flx_v=None)
    c.update(kw)
    return c, z


def _measured(case, analytic, floor, what):
    tk = ref.coefficients(case)[0]
    d = float(np.abs(tk.astype(LD) - ref.coefficients(case, dtype=LD)[0]).max())
    err = float(np.abs(tk.astype(LD) - analytic).max())
    print("%s: distance of the float64 restatement from np.longdouble %.3e, from the analytic value %.3e, gate %.3e" % (what, d, err, 4 * d + floor))
    assert err <= 4 * d + floor, (what, err, d, floor)
    return tk


def test_uniform_wind_and_a_strongly_stable_column_give_exactly_zero():
    """a uniform wind has Def2 == 0.0 exactly (every difference is x - x); an isothermal column has N2 = g^2 / (cp T) > 0, so the argument
    is negative and tk is exactly 0.0; and a shear of 0.01 / s is still below N2 / prandtl = 9.6e-4 / s^2"""
    case, z = _uniform_case(5, 3, 4, 3, temp=lambda z: 280.0 + 0.0 * z)
    case["fields"].update(uvel=np.full(z.shape, 7.5), vvel=np.full(z.shape, -3.25), wvel=np.full(z.shape, 0.125))
    for be in (ref.RefBackend(), EmuBackend()):
        tk, tkh = be.coefficients(case)
        assert (tk == 0.0).all() and (tkh == 0.0).all() and not np.signbit(tk).any()
    case["fields"]["uvel"] = 0.01 * z
    tk, tkh = ref.coefficients(case)
    assert (tk == 0.0).all() and (tkh == 0.0).all()


def test_linear_shear_over_a_neutral_column_gives_cs_dz_squared_times_the_shear():
    """u = S z with S = 2^-6 / s on a grid of 256 m is exact in float64, so uz = S exactly at every level, the one-sided ends included;
    temp = T0 - (g/cp) z without vapour is neutral up to the rounding of temp: 300 K carries u 300 per sample, which the difference over one
    span of 256 m or two turns into at most 4 u 300 / 256 of dTv/dz, times (g / T) / prandtl in the argument, times tk / (2 arg) in tk: the
    floor.  Measured: distance from np.longdouble 5.8e-15, from the analytic value 1.2e-13, gate 4.5e-12 (tk = 40.96)."""
    S = 2.0 ** -6
    case, z = _uniform_case(6, 1, 2, 3)
    case["fields"]["uvel"] = S * z
    exact = (LD(ref.CS) * 256) ** 2 * S
    floor = float(exact) / (2 * S * S) * (ref.GRAV / 290.0) / ref.PRANDTL * 4 * U * 300.0 / 256.0
    tk = _measured(case, exact, floor, "linear shear")
    assert (np.abs(tk - float(exact)) < 1e-9).all()


def test_a_sine_in_x_gives_the_centred_difference_value():
    """u = A sin(kx i + 0.3) over the neutral column: ux = A sin(kx) cos(kx i + 0.3) / dx, Def2 = 2 ux^2.  The samples carry u A each, so
    ux carries 2 u A / (2 dx) and tk = l^2 sqrt(2) |ux| carries l^2 sqrt(2) u A / dx; the neutral column's noise enters as above.
    Measured: distance from np.longdouble 1.1e-14, from the analytic value 3.1e-13, gate 3.8e-11."""
    A, nx = 10.0, 8
    case, z = _uniform_case(4, 1, nx, 2)
    i = np.arange(nx, dtype=LD)[None, None, :, None]
    kx = 2 * LD(np.pi) / nx
    case["fields"]["uvel"] = (A * np.sin(kx * i + LD(0.3)) + np.zeros(z.shape, dtype=LD)).astype(np.float64)
    ux = A * np.sin(kx) * np.cos(kx * i + LD(0.3)) / LD(ref.DX) + np.zeros(z.shape, dtype=LD)
    l2 = (LD(ref.CS) * 256) ** 2
    exact = l2 * np.sqrt(LD(2.0)) * np.abs(ux)
    arg_min = float(2 * (ux * ux).min())
    floor = float(l2) * math.sqrt(2.0) * 4 * U * A / ref.DX + float(exact.max()) / (2 * arg_min) * (ref.GRAV / 290.0) / ref.PRANDTL * 4 * U * 300.0 / 256.0
    _measured(case, exact, floor, "sine in x")


def test_ny_of_one_equals_a_field_that_is_constant_along_y():
    shape = (5, 1, 4, 130)
    case = ref.cases(shape)["base"]
    wide = dict(case, fields={n: np.ascontiguousarray(np.repeat(a, 3, axis=1)) for n, a in case["fields"].items()})
    for be in (ref.RefBackend(), EmuBackend()):
        tk1, tkh1 = be.coefficients(case)
        tk3, tkh3 = be.coefficients(wide)
        for j in range(3):
            assert ref.same_bits(tk3[:, j:j + 1], tk1) and ref.same_bits(tkh3[:, j:j + 1], tkh1)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the solve with hand-set coefficients

def _solve_case(nz, nens=3, K=25.0, dz=200.0, rho=1.1):
    case, z = _uniform_case(nz, 1, 2, nens, dz=dz)
    shape = z.shape
    case["fields"]["density_dry"] = np.full(shape, rho)
    case["tk"], case["tkh"] = np.full(shape, K), np.full(shape, K / ref.PRANDTL)
    return case, z


def _ld_distance(case, got):
    want = ref.diffuse(case, case["tk"], case["tkh"], dtype=LD)
    return {n: float(np.abs(got[n].astype(LD) - want[n]).max()) for n in got}


@pytest.mark.parametrize("nz", [2, 5, 16])
def test_a_cosine_eigenmode_decays_by_its_factor(nz):
    """f(k) = A cos(pi m (k + 1/2) / nz) is an eigenvector of the discrete Neumann operator on a uniform grid with uniform density and K:
    backward Euler divides it by 1 + 4 dt K / dz^2 sin^2(pi m / (2 nz)).  A wind with K = tk and a tracer with K = tkh.  The samples carry
    u A each and the solve is a contraction in the maximum norm: a floor of 4 u A.  Measured: the worst distance from the analytic value
    is 1.2e-15, 1.6e-15 and 4.2e-15 at nz = 2, 5 and 16 (A = 7.3; the gate is 6.5e-15 and more)."""
    A = 7.3
    case, z = _solve_case(nz)
    k = np.arange(nz, dtype=LD)[:, None, None, None]
    worst = 0.0
    for m in sorted({1, nz // 2, nz - 1}):
        mode = A * np.cos(LD(np.pi) * m * (k + LD(0.5)) / nz) + np.zeros(z.shape, dtype=LD)
        case["fields"]["wvel"] = mode.astype(np.float64)
        case["fields"]["tracer_a"] = (mode + A).astype(np.float64)
        case["tracers"] = ("tracer_a",)
        got = ref.diffuse(case, case["tk"], case["tkh"])
        d = _ld_distance(case, got)
        s2 = np.sin(LD(np.pi) * m / (2 * nz)) ** 2
        for n, K, shift in (("wvel", LD(25.0), 0.0), ("tracer_a", LD(25.0) / LD(ref.PRANDTL), A)):
            lam = 1 / (1 + 4 * LD(ref.DT) * K / LD(200.0) ** 2 * s2)
            err = float(np.abs(got[n].astype(LD) - (lam * mode + shift)).max())
            gate = 4 * d[n] + 4 * U * 2 * A
            assert err <= gate, (n, m, err, gate)
            worst = max(worst, err)
            assert 0 < float(lam) < 1
    print("nz %d: worst distance from the analytic value %.3e" % (nz, worst))


def test_the_neutral_temperature_profile_is_a_fixed_point():
    """temp = T0 - (g/cp) zmid: temp + (g/cp) zmid is constant, so nothing is diffused.  The samples of temp carry u 300 each and the solve is
    a contraction: a floor of 4 u 300.  Measured: distance from np.longdouble 5.7e-14, from the profile 5.7e-14 (one ulp of 300)."""
    case, z = _solve_case(9)
    got = ref.diffuse(case, case["tk"], case["tkh"])
    d = _ld_distance(case, got)["temp"]
    err = float(np.abs(got["temp"] - case["fields"]["temp"]).max())
    print("neutral profile: distance from np.longdouble %.3e, from the profile %.3e" % (d, err))
    assert err <= 4 * d + 4 * U * 300.0
    emu = EmuBackend().diffuse(case, case["tk"], case["tkh"])
    assert ref.same_bits(emu["temp"], got["temp"])


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_the_three_column_sums_are_kept_within_the_roundings(shape):
    """Without surface flux the weighted column sums S rho dz f (winds, temp) and S dz rho_x (tracers) are kept: with the weights w the
    rows satisfy w^T A = w^T in exact arithmetic (the g of a face enters the two rows it joins with opposite signs), and for temp
    S w (upper dzf_above - lower dzf_below) = S (g dzf - g dzf) = 0 as well.  What remains is rounding, bounded as test_hd.py bounds its
    level sums, by the magnitudes the roundings act on:
      the computed lower, diag, upper carry at most 4 roundings each on the way from g and rho dz: 5 u |entry| with the rounding of g;
      the Thomas algorithm on a diagonally dominant tridiagonal matrix solves (A + E) x = r with |E| <= 3 f(u) |A|, f(u) = 4 u + O(u^2)
      (Higham, Accuracy and Stability of Numerical Algorithms, section 9.6): 13 u |entry|;
    so |w^T x - w^T r| <= 18 u S_k w_k (|lower x(k-1)| + |diag x(k)| + |upper x(k+1)|), and for temp the right-hand side adds
    4 u w_k (g/cp)(|upper dzf_above| + |lower dzf_below|) + u w_k |r|.  The sums of the test itself are taken in np.longdouble, whose own
    error is at most 2 nz 2^-64 times the sum of the magnitudes."""
    case = ref.cases(shape)["no_surface_flux"]
    got = ref.reference(shape, "no_surface_flux")
    F = case["fields"]
    nz = shape[0]
    rho = F["density_dry"] + F["water_vapor"]
    dz = (case["zint"][1:] - case["zint"][:-1])[:, None, None, :]
    gc = case["grav"] / case["cp_d"]
    worst = 0.0
    for n in ref.WINDS + ("temp",) + case["tracers"]:
        cls = "momentum" if n in ref.WINDS else ("heat" if n == "temp" else "tracer")
        K = got["tk"] if cls == "momentum" else got["tkh"]
        lower, diag, upper, dzf_m, dzf_p, _ = ref.rows(cls, rho, K, case["zint"], case["zmid"], case["dt"])
        w = (dz + 0 * rho if cls == "tracer" else rho * dz).astype(LD)
        x, r = got[n].astype(LD), F[n].astype(LD)
        xm, xp = np.concatenate([x[:1], x[:-1]]), np.concatenate([x[1:], x[-1:]])
        mags = np.abs(lower * xm) + np.abs(diag * x) + np.abs(upper * xp)
        lim = 18 * U * (w * mags).sum(axis=0)
        if cls == "heat":
            lim = lim + U * (w * (4 * gc * (np.abs(upper * dzf_p) + np.abs(lower * dzf_m)) + np.abs(r) + gc * 1.0e4)).sum(axis=0)
        lim = lim + 2 * nz * LD(2.0) ** -64 * (w * (np.abs(x) + np.abs(r))).sum(axis=0)
        err = np.abs((w * x).sum(axis=0) - (w * r).sum(axis=0))
        assert (err <= lim).all(), (n, float((err / lim).max()))
        worst = max(worst, float((err / np.where(lim > 0, lim, 1)).max()))
    print("worst fraction of the bound %.3f" % worst)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_tracers_stay_non_negative_zero_k_levels_keep_their_bits_and_the_vapour_may_stand_anywhere(shape):
    nz = shape[0]
    for name in ("base", "vapour_middle", "vapour_last", "zero_k_faces"):
        case, got = ref.cases(shape)[name], ref.reference(shape, name)
        for n in case["tracers"]:
            assert (case["fields"][n] >= 0).all() and (got[n] >= 0).all(), (name, n)
    # levels 0 .. 2 have K == 0: the faces 1/2 and 3/2 vanish, so level 1 keeps its bits in every class (at nz == 2 the one face there is)
    case, got = ref.cases(shape)["zero_k_faces"], ref.reference(shape, "zero_k_faces")
    for be_got in (got, ref.run_case(EmuBackend("workspace"), case)):
        for n in ref.WINDS + ("temp",) + case["tracers"]:
            assert ref.same_bits(be_got[n][1], case["fields"][n][1]), n
            if nz > 3:
                assert not ref.same_bits(be_got[n][3:], case["fields"][n][3:]), n
    # every field of the call comes out with the same bits wherever the vapour stands, and whatever else is in the table
    a, b, c = (ref.reference(shape, n) for n in ("base", "vapour_middle", "vapour_last"))
    assert ref.results_differ(b, c) == []
    assert ref.results_differ(a, {n: b[n] for n in a}) == []


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the mutants of the restatement

@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_caught_by_a_named_case(mutant):
    """a swapped pair of face weights, rho(k) in place of rho(k-1) and rho(k+1) in the tracer row, a dropped g/cp in N2 and in the heat
    row, the one-sided derivative in the wrong place: each changes the bits of a named case on every shape"""
    assert set(ref.MUTANTS) == {"face_swapped", "tracer_rho_k", "n2_no_lapse", "heat_no_lapse", "one_sided_wrong_place"}
    where = dict(face_swapped=("uvel", "temp", "rain"), tracer_rho_k=("rain",), n2_no_lapse=("tk",), heat_no_lapse=("temp",),
                 one_sided_wrong_place=("tk",))[mutant]
    for shape in ref.SHAPES:
        got = ref.run_case(ref.RefBackend(mutant), ref.cases(shape)["base"])
        diff = ref.results_differ(got, ref.reference(shape, "base"))
        assert set(where) <= set(diff), (shape, diff)
        if mutant == "tracer_rho_k":
            assert not {"uvel", "temp", "tk"} & set(diff)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the C ABI: refusals before any device is asked for; the symbols

NEW_SYMBOLS = ("pam_amd_sgs_smag_coefficients", "pam_amd_sgs_smag_diffuse", "pam_amd_sgs_smag_debug_path")


def test_entry_points_are_exported_and_declared_and_the_abi_stays_5():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    assert lib.pam_amd_awfl_abi_version() == 5


def test_entry_points_reject_bad_arguments_and_leave_the_arrays_untouched():
    """the pointers are host arrays here: a refusal comes before the first HIP call, so nothing dereferences them, and afterwards every
    array still holds the pattern it was filled with"""
    lib = capi.load()
    n = 4 * 2 * 3 * 4                                              # nens 4, nx 3, ny 2, nz 4
    arrays = [np.full(n + 16, 7.25) for _ in range(16)]
    p = [a.ctypes.data for a in arrays]
    u, v, w, t, rd, rv, zi, zm, tk, tkh, su, sv, q1, q2 = p[:14]
    T2 = (C.c_void_p * 2)(q1, q2)
    Tv = (C.c_void_p * 3)(q1, rv, q2)                              # the vapour itself in the table: allowed
    Tvv = (C.c_void_p * 3)(rv, q1, rv)                             # twice: two outputs overlap
    Thole = (C.c_void_p * 2)(q1, None)
    Tdup = (C.c_void_p * 2)(q1, q1)
    Ttemp = (C.c_void_p * 2)(q1, t)
    Ttk = (C.c_void_p * 2)(q1, tkh + 8)
    T65 = (C.c_void_p * 65)(*([q1] * 65))
    big = 65536                                                    # ny nx = 2^32 > 2^31 - 1
    good = dict(dx=500.0, dy=500.0, grav=9.8, cp_d=1004.0, cs=0.2, prandtl=0.33)

    def coef(nens=4, nx=3, ny=2, nz=4, ptrs=None, **kw):
        a = dict(good)
        a.update(kw)
        ptrs = ptrs or [u, v, w, t, rd, rv, zi, zm]
        out = [a.pop("tk", tk), a.pop("tkh", tkh)]
        return lib.pam_amd_sgs_smag_coefficients(nens, nx, ny, nz, *ptrs, a["dx"], a["dy"], a["grav"], a["cp_d"], a["cs"], a["prandtl"], *out, None)

    def dif(nens=4, nx=3, ny=2, nz=4, fields=None, nt=2, table=T2, ro=None, sfc=(su, sv), dt=10.0, grav=9.8, cp_d=1004.0):
        fields = fields or [u, v, w, t]
        ro = ro or [rd, rv, tk, tkh, zi, zm]
        return lib.pam_amd_sgs_smag_diffuse(nens, nx, ny, nz, *fields, nt, table, *ro, *sfc, dt, grav, cp_d, None)

    calls = [lambda i=i: coef(ptrs=[None if j == i else x for j, x in enumerate([u, v, w, t, rd, rv, zi, zm])]) for i in range(8)]
    calls += [lambda: coef(tk=None), lambda: coef(tkh=None), lambda: coef(nens=0), lambda: coef(nx=0), lambda: coef(ny=0), lambda: coef(nz=1),
              lambda: coef(nz=0), lambda: coef(nx=big, ny=big), lambda: coef(tk=u), lambda: coef(tkh=zi), lambda: coef(tk=tkh), lambda: coef(tkh=tk + 8 * n - 8)]
    for name in good:
        calls += [lambda name=name, bad=bad: coef(**{name: bad}) for bad in (0.0, -1.0, math.nan, math.inf)]
    calls += [lambda i=i: dif(fields=[None if j == i else x for j, x in enumerate([u, v, w, t])]) for i in range(4)]
    calls += [lambda i=i: dif(ro=[None if j == i else x for j, x in enumerate([rd, rv, tk, tkh, zi, zm])]) for i in range(6)]
    calls += [lambda: dif(table=None), lambda: dif(table=Thole), lambda: dif(nt=-1), lambda: dif(nt=65, table=T65), lambda: dif(nens=0),
              lambda: dif(nx=0), lambda: dif(ny=0), lambda: dif(nz=1), lambda: dif(nx=big, ny=big), lambda: dif(table=Tdup), lambda: dif(table=Ttemp),
              lambda: dif(table=Ttk), lambda: dif(nt=3, table=Tvv), lambda: dif(fields=[u, u, w, t]), lambda: dif(fields=[u, v, w, rd]),
              lambda: dif(fields=[u, v, w, rv]), lambda: dif(fields=[tk, v, w, t]), lambda: dif(sfc=(u, sv)), lambda: dif(sfc=(su, q2)),
              lambda: dif(fields=[zm, v, w, t])]
    for name in ("dt", "grav", "cp_d"):
        calls += [lambda name=name, bad=bad: dif(**{name: bad}) for bad in (0.0, -1.0, math.nan, math.inf)]
    calls += [lambda: lib.pam_amd_sgs_smag_debug_path(-1), lambda: lib.pam_amd_sgs_smag_debug_path(3)]
    for i, call in enumerate(calls):
        assert call() == -1, i                                     # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert b"sgs" in lib.pam_amd_awfl_last_error(), i
        assert all((a == 7.25).all() for a in arrays), i
    for path in (1, 2, 0):
        assert lib.pam_amd_sgs_smag_debug_path(path) == 0
    # what is allowed gets past the argument checks: the vapour once in the table, either flux absent, no tracers at all.  Without a
    # device the call then ends in PAM_AMD_ENOGPU; with one, the host arrays here must not reach a kernel, so it is not made
    import torch
    if not torch.cuda.is_available():
        for call in (lambda: dif(nt=3, table=Tv), lambda: dif(sfc=(None, None)), lambda: dif(nt=0, table=None)):
            assert call() not in (0, -1)
            assert all((a == 7.25).all() for a in arrays)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. the C++ plug-in class, its Python mirror, the driver, the build

SGS_H = os.path.join(HOST, "physics", "sgs", "smag_amd", "SGS.h")


def test_cxx_class_compiles_in_one_translation_unit_with_micro_none_and_a_radiation_class(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "physics/micro/none/Microphysics.h"\n#include "physics/radiation/forced_amd/radiation.h"\n'
                   '#include "physics/sgs/smag_amd/SGS.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  Microphysics micro;\n  SGS sgs;\n  Radiation rad;\n  micro.init(coupler);\n"
                   "  sgs.init(coupler);\n  rad.init(coupler);\n  rad.timeStep(coupler);\n  sgs.timeStep(coupler);\n  micro.timeStep(coupler);\n"
                   "  static_assert(SGS::get_num_tracers() == 0, \"\");\n  sgs.finalize(coupler);\n  return (int)sgs.sgs_name().size();\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cxx_class_and_python_class_name_the_same_fields_and_options():
    import pam_amd
    from pam_amd import physics
    text, py = open(SGS_H).read(), inspect.getsource(physics.SGSSmagorinsky)
    names = ('"tk"', '"tkh"', '"sfc_mom_flx_u"', '"sfc_mom_flx_v"', '"sgs"', '"smagorinsky"', '"sgs_smag_cs"', '"sgs_smag_prandtl"', '"crm_dt"',
             '"grav"', '"cp_d"', '"uvel"', '"vvel"', '"wvel"', '"temp"', '"density_dry"', '"water_vapor"', '"vertical_interface_height"',
             '"vertical_midpoint_height"')
    for s in names:
        assert s in text and s in py, s
    assert "get_tracer_names" in text and "get_tracer_names" in py and "get_dx" in text and "get_dx" in py
    assert pam_amd.SGSSmagorinsky is physics.SGSSmagorinsky
    sig = inspect.signature(physics.SGSSmagorinsky.__init__).parameters
    assert sig["cs"].default == 0.2 and sig["prandtl"].default == 1.0 / 3.0
    assert physics.SGSSmagorinsky.get_num_tracers() == 0 and physics.SGSSmagorinsky.sgs_name() == "smagorinsky"
    assert "sgs_smag_cs\", 0.2" in text and "sgs_smag_prandtl\", 1.0 / 3.0" in text
    for member in ("static int constexpr get_num_tracers()", "void init(pam::PamCoupler &coupler)", "void timeStep(pam::PamCoupler &coupler)",
                   "void finalize(pam::PamCoupler &coupler)", "std::string sgs_name() const"):
        assert member in text, member


def test_build_depends_on_the_new_headers_and_the_driver_has_the_option():
    deps = native_build.dependencies(native_build.LIB_SOURCES)
    assert os.path.join(native_build.CSRC, "sgs_device.h") in deps and SGS_H in deps
    assert '#include "sgs_device.h"' in open(os.path.join(ROOT, "pam_amd", "csrc", "modules_kernels.hip")).read()
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert drv.count('"--sgs-smag"') == 1 and drv.count("[--sgs-smag CS PRANDTL]") >= 2 and '#include "physics/sgs/smag_amd/SGS.h"' in drv
    assert "no SGS scheme is ported here" not in open(os.path.join(HOST, "modules", "surface_friction.h")).read()
