"""The prognostic-TKE closure of the native SGS plug-in, everything that needs no GPU: the numpy restatement of the contract
(tests/sgs_tke_ref.py) against its scalar-loop twin; the device bodies under g++ (tests/emu/sgs_tke_emu.cpp) against the restatement bit
for bit on every shape and named case; the census of the branches the base case takes; the mutants; the properties of the step
(positivity, dt = 0, the neutral fixed point, decay in a stable layer); the restatement's own rounding error; the host constants; the C
ABI's refusals; the C++ plug-in class and its Python mirror."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import sgs_tke_ref as tref
from sgs_tke_harness import EmuBackend, constants as emu_constants, step as emu_step
from pam_amd import capi
from tools import native_build
from tools.native_build import syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
SGS_H = os.path.join(HOST, "physics", "sgs", "tke_amd", "SGS.h")
LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the restatement itself, and the device bodies under g++

@pytest.mark.parametrize("shape", tref.SHAPES, ids=tref.shape_id)
def test_restatement_is_the_scalar_loop(shape):
    """the vectorised form against one Python float at a time; the larger shapes on a slice of members (members are independent)"""
    for name in ("base", "negative_tke", "nan_tke_cell", "neutral_exact", "p3_set"):
        case, want = tref.cases(shape)[name], tref.reference(shape, name)
        idx = list(range(shape[3])) if np.prod(shape) < 500 else [0, 1, shape[3] // 2, shape[3] - 1]
        got = tref.run_case(tref.ScalarBackend(), tref.members(case, idx))
        assert tref.results_differ(got, {n: np.ascontiguousarray(a[..., idx]) for n, a in want.items()}) == [], name


@pytest.mark.parametrize("shape", tref.SHAPES, ids=tref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape):
    """every named case through the dry or the moist instance of the walk, tke updated in place"""
    be = EmuBackend()
    for name in tref.CASE_NAMES:
        got = tref.run_case(be, tref.cases(shape)[name])
        assert tref.results_differ(got, tref.reference(shape, name)) == [], name


@pytest.mark.parametrize("shape", [s for s in tref.SHAPES if np.prod(s) >= 64], ids=tref.shape_id)
def test_census_of_the_base_case(shape):
    """every branch of the step is taken in `base`: N2 <= 0; the floor, the range between and the cap of the length; e1 clipped and not;
    tke keeping its bits and not"""
    case = tref.cases(shape)["base"]
    out, tk, tkh, p = tref.coefficients(case, parts=True)
    st = p["stable"]
    census = {"N2 <= 0": (p["N2"] <= 0), "floor": st & (p["ls"] < p["lo"]), "between": st & (p["ls"] >= p["lo"]) & (p["ls"] <= p["delta"]),
              "cap": st & (p["ls"] > p["delta"]), "e1 clipped": p["e1u"] < 0, "e1 not clipped": p["e1u"] >= 0, "kept": p["keep"],
              "replaced": ~p["keep"]}
    print({n: int(m.sum()) for n, m in census.items()})
    for n, m in census.items():
        assert m.any(), n


def test_named_cases_hold_what_they_are_named_for():
    shape = (7, 3, 5, 130)
    cs = tref.cases(shape)
    assert (cs["zero_tke"]["fields"]["tke"] == 0).all() and (tref.reference(shape, "zero_tke")["tke"] > 0).any()
    assert (cs["negative_tke"]["fields"]["tke"] < 0).mean() > 0.1
    assert cs["dt_zero"]["dt"] == 0.0 and cs["seed_zero"]["seed"] == 0.0
    nan = tref.reference(shape, "nan_tke_cell")
    assert np.isnan(cs["nan_tke_cell"]["fields"]["tke"]).sum() == 1
    assert all(np.isnan(nan[n]).sum() == 1 for n in ("tke", "tk", "tkh"))            # a NaN in tke stays in its cell
    nan = tref.reference(shape, "nan_wind_cell")
    assert 1 < np.isnan(nan["tk"]).sum() <= 7 and not np.isnan(nan["tk"][3, 1, 2, 65])   # its neighbours' differences read it, not its own
    _, _, _, p = tref.coefficients(cs["stable_floor"], parts=True)
    assert (p["stable"] & (p["ls"] < p["lo"])).all()
    _, _, _, p = tref.coefficients(cs["unstable"], parts=True)
    assert (p["N2"] < 0).all()
    _, _, _, p = tref.coefficients(cs["neutral_exact"], parts=True)
    assert (p["N2"] == 0).all() and ((cs["neutral_exact"]["fields"]["tke"] == 0).mean() > 0.3)
    z = tref.reference(shape, "seed_zero")
    assert (z["tke"][cs["seed_zero"]["fields"]["tke"] == 0] == 0).all()                # without a seed nothing grows from zero
    assert tref.results_differ(tref.reference(shape, "empty_tables"), tref.reference(shape, "base")) == []
    for n in ("kessler_set", "p3_set", "ice1m_set"):
        assert "tk" in tref.results_differ(tref.reference(shape, n), tref.reference(shape, "base")), n
    assert cs["fluxes_both"]["sfc_shf"] is not None and cs["fluxes_both"]["sfc_lhf"] is not None


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the mutants

CAUGHT_BY = dict(diss_at_e1="base", length_no_floor="stable_floor", length_no_cap="base", branch_ge="neutral_exact", buoy_sign="unstable",
                 seed_dropped="zero_tke", pr_fixed_3="stable_floor", clip_dropped="base", tke_without_rho="base", keep_bits_dropped="dt_zero",
                 tkh_from_e0="base")


@pytest.mark.parametrize("mutant", tref.MUTANTS)
def test_every_mutant_is_caught_by_a_named_case(mutant):
    """each one-line change of the restatement changes the bits of its named case on every shape of 64 cells or more (the census's
    rule: two cells cannot hold every branch)"""
    assert set(CAUGHT_BY) == set(tref.MUTANTS)
    name = CAUGHT_BY[mutant]
    for shape in [s for s in tref.SHAPES if np.prod(s) >= 64]:
        got = tref.run_case(tref.RefBackend(mutant), tref.cases(shape)[name])
        assert tref.results_differ(got, tref.reference(shape, name), nan_by_place=True) != [], (shape, name)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. properties of the restatement

@pytest.mark.parametrize("shape", tref.SHAPES, ids=tref.shape_id)
def test_tke_stays_non_negative_and_dt_zero_keeps_the_bits(shape):
    for name in tref.CASE_NAMES:
        if name == "nan_wind_cell":
            continue
        tin, tout = tref.cases(shape)[name]["fields"]["tke"], tref.reference(shape, name)["tke"]
        ok = ~np.isnan(tin)
        assert (tout[ok] >= 0).all(), name
    tin, tout = tref.cases(shape)["nan_wind_cell"]["fields"]["tke"], tref.reference(shape, "nan_wind_cell")["tke"]
    assert (tout[~np.isnan(tout)] >= 0).all()
    tin, tout = tref.cases(shape)["dt_zero"]["fields"]["tke"], tref.reference(shape, "dt_zero")["tke"]
    assert (tin >= 0).all() and tref.same_bits(tin, tout)


def _iterate(e, D, N2, dt, seed, steps, mutant=None, cs=0.2, ck=0.1, delta=100.0):
    ce, ce1, ce2 = tref.constants(cs, ck)
    one, hist = np.float64(1.0), [float(e)]
    e = np.float64(e)
    for _ in range(steps):
        e, tk, tkh = tref.tke_step(e, one, np.float64(D), np.float64(N2), np.float64(delta), dt, ck, ce1, ce2, seed, mutant)
        hist.append(float(e))
    return hist, float(tk)


@pytest.mark.parametrize("D", [1e-4, 1e-2])
@pytest.mark.parametrize("e_start", [1e-6, 1e-3, 10.0])
def test_the_neutral_fixed_point_is_smagorinskys_whatever_dt_is(D, e_start):
    """cs = 0.2, ck = 0.1, delta = 100, N2 = 0, seed = 0, dt = 600: after 64 steps tk = (cs delta)^2 sqrt(Def2) within 1e-12 relative, and
    from below the approach is monotone.  The variant with sqrt(e1) in the dissipation (mutant diss_at_e1) settles elsewhere"""
    want = (0.2 * 100.0) ** 2 * math.sqrt(D)
    hist, tk = _iterate(e_start, D, 0.0, 600.0, 0.0, 64)
    print("Def2 %g, start %g: tk %.17g, wanted %.17g, relative %.3e" % (D, e_start, tk, want, abs(tk - want) / want))
    assert abs(tk - want) <= 1e-12 * want
    e_fix = (want / (0.1 * 100.0)) ** 2
    if e_start < e_fix:
        assert all(b >= a for a, b in zip(hist, hist[1:]))
    _, tk_mutant = _iterate(e_start, D, 0.0, 600.0, 0.0, 64, mutant="diss_at_e1")
    assert abs(tk_mutant - want) > 1e-3 * want


def test_tke_decays_in_a_stable_layer_at_richardson_one():
    """Def2 = N2 = 1e-4, dt = 10, seed = 1e-3, from e = 1: e never increases and is at most 1e-12 after 5000 steps (0.0 was observed)"""
    hist, _ = _iterate(1.0, 1e-4, 1e-4, 10.0, 1e-3, 5000)
    print("e after 5000 steps: %.3e" % hist[-1])
    assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] <= 1e-12


def test_one_cell_under_gxx_is_the_restatement_on_hand_picked_values():
    ce, ce1, ce2 = tref.constants(0.2, 0.1)
    for tke, rho, D, N2 in ((0.0, 1.1, 1e-5, -1e-4), (0.3, 0.7, 1e-4, 2e-4), (-0.2, 1.0, 1e-5, 1e-6), (50.0, 1.2, 0.0, 1e-9), (0.0, 1.0, 1e-6, 0.0),
                            (math.nan, 1.0, 1e-6, 1e-4), (1.0, 1.0, math.nan, 1e-4), (1.0, 1.0, 1e-5, math.nan), (1e-9, 1.0, 0.0, 3e-4)):
        a = emu_step(tke, rho, D, N2, 250.0, 10.0, 0.1, ce1, ce2, 1e-3)
        b = tref.tke_step(np.float64(tke), np.float64(rho), np.float64(D), np.float64(N2), np.float64(250.0), 10.0, 0.1, ce1, ce2, 1e-3)
        assert tref.same_bits(np.array(a), np.array([float(x) for x in b]), nan_by_place=True), (tke, rho, D, N2)


def test_rounding_error_of_the_float64_restatement_is_measured():
    """the same restatement in np.longdouble on the same float64 inputs: the float64 restatement's own rounding error on `base`.  It gates
    nothing (the device is held to the bits); the figure stands in DESIGN.md section 8.  Only cells whose branches agree in both
    precisions are compared: at a threshold a last-place difference picks the other arm"""
    shape = (7, 3, 5, 130)
    case = tref.cases(shape)["base"]
    a, b = tref.coefficients(case, parts=True), tref.coefficients(case, dtype=LD, parts=True)
    same = np.ones(shape, dtype=bool)
    for n in ("stable", "keep"):
        same &= a[3][n] == b[3][n]
    same &= ((a[3]["ls"] < a[3]["lo"]) == (b[3]["ls"] < b[3]["lo"])) & ((a[3]["ls"] > a[3]["delta"]) == (b[3]["ls"] > b[3]["delta"]))
    same &= (a[3]["e1u"] < 0) == (b[3]["e1u"] < 0)
    worst = {}
    for q, n in enumerate(("tke", "tk", "tkh")):
        scale = np.maximum(np.abs(b[q]), LD(np.abs(a[q]).max()) * LD(1e-6))
        worst[n] = float((np.abs(a[q].astype(LD) - b[q]) / scale)[same].max())
    print("cells compared %d of %d; worst relative distance from np.longdouble: %s" % (same.sum(), same.size, worst))
    assert same.mean() > 0.9 and all(np.isfinite(v) for v in worst.values())


def test_host_constants_are_the_same_bits_in_python_and_cxx():
    from pam_amd import physics
    want = (0.6249999999999999, 0.16964285714285712, 0.45535714285714285)
    assert tref.constants(0.2, 0.1) == want
    assert physics.SGSTke.constants(0.2, 0.1) == want
    assert emu_constants(0.2, 0.1) == want
    for cs, ck in ((0.17, 0.1), (0.2, 0.09), (0.23, 0.12)):
        assert emu_constants(cs, ck) == physics.SGSTke.constants(cs, ck) == tref.constants(cs, ck)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the C ABI: refusals before any device is asked for; the symbols

NEW_SYMBOLS = ("pam_amd_sgs_tke_coefficients", "pam_amd_sgs_tke_coefficients_moist")


def test_entry_points_are_exported_and_declared_and_the_abi_stays_5():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    assert lib.pam_amd_awfl_abi_version() == 5


def refusals(lib, p):
    """the calls that must return PAM_AMD_EINVAL, as closures over 16 arrays' addresses p (host or device: nothing dereferences them)"""
    u, v, w, t, rd, rv, tke, zi, zm, tk, tkh, q1, q2, q3 = p[:14]
    n = 4 * 2 * 3 * 4                                              # nens 4, nx 3, ny 2, nz 4
    big = 65536
    good = dict(dx=500.0, dy=500.0, dt=10.0, grav=9.8, cp_d=1004.0, ck=0.1, ce1=0.17, ce2=0.45, seed=1e-3)
    goodm = dict(good, R_d=287.0, R_v=461.0, cloud_threshold=0.0)
    T1, T2 = (C.c_void_p * 4)(q1), (C.c_void_p * 8)(q2, q3)
    Thole = (C.c_void_p * 8)(q2, None)
    Ttke = (C.c_void_p * 4)(tke)

    def dry(nens=4, nx=3, ny=2, nz=4, ptrs=None, **kw):
        a = dict(good)
        a.update(kw)
        ptrs = ptrs or [u, v, w, t, rd, rv, tke, zi, zm]
        out = [a.pop("tk", tk), a.pop("tkh", tkh)]
        return lib.pam_amd_sgs_tke_coefficients(nens, nx, ny, nz, *ptrs, a["dx"], a["dy"], a["dt"], a["grav"], a["cp_d"], a["ck"], a["ce1"],
                                                a["ce2"], a["seed"], *out, None)

    def moist(nens=4, nx=3, ny=2, nz=4, ptrs=None, nc=1, cloud=T1, npr=2, precip=T2, z=None, **kw):
        a = dict(goodm)
        a.update(kw)
        ptrs = ptrs or [u, v, w, t, rd, rv, tke]
        z = z or [zi, zm]
        out = [a.pop("tk", tk), a.pop("tkh", tkh)]
        return lib.pam_amd_sgs_tke_coefficients_moist(nens, nx, ny, nz, *ptrs, nc, cloud, npr, precip, *z, a["dx"], a["dy"], a["dt"], a["grav"],
                                                      a["cp_d"], a["R_d"], a["R_v"], a["cloud_threshold"], a["ck"], a["ce1"], a["ce2"], a["seed"],
                                                      *out, None)

    nine = [u, v, w, t, rd, rv, tke, zi, zm]
    calls = [lambda i=i: dry(ptrs=[None if j == i else x for j, x in enumerate(nine)]) for i in range(9)]
    calls += [lambda i=i: moist(ptrs=[None if j == i else x for j, x in enumerate(nine[:7])]) for i in range(7)]
    calls += [lambda: moist(z=[None, zm]), lambda: moist(z=[zi, None])]
    for f in (dry, moist):
        calls += [lambda f=f: f(tk=None), lambda f=f: f(tkh=None), lambda f=f: f(nens=0), lambda f=f: f(nx=0), lambda f=f: f(ny=0),
                  lambda f=f: f(nz=1), lambda f=f: f(nz=0), lambda f=f: f(nx=big, ny=big), lambda f=f: f(tk=u), lambda f=f: f(tkh=zi),
                  lambda f=f: f(tk=tkh), lambda f=f: f(tkh=tk + 8 * n - 8),
                  lambda f=f: f(tk=tke), lambda f=f: f(tkh=tke + 8)]                                  # tke overlapping an output
        for name in ("dx", "dy", "grav", "cp_d", "ck", "ce1"):
            calls += [lambda f=f, name=name, bad=bad: f(**{name: bad}) for bad in (0.0, -1.0, math.nan, math.inf)]
        for name in ("ce2", "seed", "dt"):
            calls += [lambda f=f, name=name, bad=bad: f(**{name: bad}) for bad in (-1.0, math.nan, math.inf)]
    for i in range(6):                                                                                # tke overlapping an input
        calls.append(lambda i=i: dry(ptrs=[nine[i] + 8 if j == 6 else x for j, x in enumerate(nine)]))
        calls.append(lambda i=i: moist(ptrs=[nine[i] if j == 6 else x for j, x in enumerate(nine[:7])]))
    calls += [lambda: dry(ptrs=nine[:6] + [zi, zi, zm]), lambda: dry(ptrs=nine[:6] + [zm, zi, zm]), lambda: moist(cloud=Ttke),
              lambda: moist(nc=-1), lambda: moist(nc=5), lambda: moist(npr=-1), lambda: moist(npr=9), lambda: moist(cloud=None),
              lambda: moist(precip=None), lambda: moist(precip=Thole), lambda: moist(tk=q1), lambda: moist(tkh=q3)]
    for name in ("R_d", "R_v"):
        calls += [lambda name=name, bad=bad: moist(**{name: bad}) for bad in (0.0, -1.0, math.nan, math.inf)]
    calls += [lambda bad=bad: moist(cloud_threshold=bad) for bad in (-1.0, math.nan, math.inf)]
    allowed = [lambda: dry(dt=0.0), lambda: dry(seed=0.0, ce2=0.0), lambda: moist(nc=0, cloud=None, npr=0, precip=None)]
    return calls, allowed


def test_entry_points_reject_bad_arguments_and_leave_the_arrays_untouched():
    """the pointers are host arrays here: a refusal comes before the first HIP call, so nothing dereferences them, and afterwards every
    array still holds the pattern it was filled with"""
    lib = capi.load()
    arrays = [np.full(4 * 2 * 3 * 4 + 16, 7.25) for _ in range(16)]
    calls, allowed = refusals(lib, [a.ctypes.data for a in arrays])
    for i, call in enumerate(calls):
        assert call() == -1, i                                     # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert b"sgs_tke" in lib.pam_amd_awfl_last_error(), i
        assert all((a == 7.25).all() for a in arrays), i
    # what is allowed gets past the argument checks; without a device the call then ends in PAM_AMD_ENOGPU; with one, the host arrays
    # here must not reach a kernel, so it is not made
    import torch
    if not torch.cuda.is_available():
        for call in allowed:
            assert call() not in (0, -1)
            assert all((a == 7.25).all() for a in arrays)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the C++ plug-in class, its Python mirror, the driver, the build

def test_cxx_class_compiles_in_one_translation_unit_with_micro_none_and_a_radiation_class(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "physics/micro/none/Microphysics.h"\n#include "physics/radiation/forced_amd/radiation.h"\n'
                   '#include "physics/sgs/tke_amd/SGS.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  Microphysics micro;\n  SGS sgs;\n  Radiation rad;\n  micro.init(coupler);\n"
                   "  sgs.init(coupler);\n  rad.init(coupler);\n  rad.timeStep(coupler);\n  sgs.timeStep(coupler);\n  micro.timeStep(coupler);\n"
                   "  static_assert(SGS::get_num_tracers() == 1, \"\");\n  sgs.finalize(coupler);\n  return (int)sgs.sgs_name().size();\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cxx_class_and_python_class_name_the_same_fields_and_options():
    import pam_amd
    from pam_amd import physics
    text, py = open(SGS_H).read(), inspect.getsource(physics.SGSTke)
    names = ('"tke"', '"Turbulent Kinetic Energy (m^2/s^2)"', '"tk"', '"tkh"', '"sfc_mom_flx_u"', '"sfc_mom_flx_v"', '"sfc_shf"', '"sfc_lhf"', '"sgs"',
             '"sgs_tke_cs"', '"sgs_tke_ck"', '"sgs_tke_seed"', '"sgs_tke_moist"', '"sgs_tke_surface_fluxes"', '"sgs_tke_cloud_threshold"', '"crm_dt"',
             '"grav"', '"cp_d"', '"uvel"', '"vvel"', '"wvel"', '"temp"', '"density_dry"', '"water_vapor"', '"vertical_interface_height"',
             '"vertical_midpoint_height"', '"micro"', '"R_d"', '"R_v"', '"latvap"')
    for s in names:
        assert s in text and s in py, s
    assert "get_tracer_names" in text and "get_tracer_names" in py and "get_dx" in text and "get_dx" in py
    assert pam_amd.SGSTke is physics.SGSTke
    sig = inspect.signature(physics.SGSTke.__init__).parameters
    assert [sig[n].default for n in ("cs", "ck", "seed", "moist", "surface_fluxes", "cloud_threshold")] == [0.2, 0.1, 1e-3, False, False, 0.0]
    assert physics.SGSTke.get_num_tracers() == 1 and physics.SGSTke.sgs_name() == "tke"
    for member in ("static int constexpr get_num_tracers()", "void init(pam::PamCoupler &coupler)", "void timeStep(pam::PamCoupler &coupler)",
                   "void finalize(pam::PamCoupler &coupler)", "std::string sgs_name() const"):
        assert member in text, member
    assert "SGS.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read() and "tke_amd" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_build_depends_on_the_new_header_and_the_driver_has_the_option():
    deps = native_build.dependencies(native_build.LIB_SOURCES)
    assert SGS_H in deps
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert drv.count('"--sgs-tke"') == 1 and "[--sgs-tke CS CK]" in drv and '#include "physics/sgs/tke_amd/SGS.h"' in drv
