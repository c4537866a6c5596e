"""The native grey two-stream longwave radiation scheme, everything that needs no GPU: the device bodies under g++
(tests/emu/grayrad_emu.cpp) against the numpy restatement (tests/grayrad_ref.py) bit for bit on every shape and named case, with each
member's own grid and with identical columns; the census of what the named cases reach; the energy closure of every column; the physics
of the cloud case; the mutants; members split over calls; the wide-index instance; the C ABI's refusals and its answer without a device;
the C++ plug-in class and its Python mirror."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import grayrad_ref as ref
import grayrad_cases as gc
from grayrad_emu_harness import EmuBackend
from pam_amd import capi
from tools.native_build import syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
U = 2.0 ** -53
FINITE_CASES = tuple(n for n in gc.CASE_NAMES if n != "nan_cell")
DEEP = [s for s in gc.SHAPES if s[0] >= 5]          # shapes whose cloud layer lies inside the column


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the device bodies under g++

@pytest.mark.parametrize("per_member", [True, False], ids=["own_grid", "identical_columns"])
@pytest.mark.parametrize("shape", gc.SHAPES, ids=ref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape, per_member):
    """every named case; the first shape has one level, so both boundaries fall in one cell"""
    for name in gc.CASE_NAMES:
        want = gc.outputs(gc.reference(shape, name, per_member))
        got = EmuBackend().run(gc.cases(shape, per_member)[name])
        assert ref.results_differ(got, want, nan_by_place=True) == [], name


@pytest.mark.parametrize("shape", gc.SHAPES, ids=ref.shape_id)
def test_wide_index_instance_equals_the_narrow_one(shape):
    for name in ("two_and_two", "thick_cloud", "nan_cell"):
        case = gc.cases(shape)[name]
        assert ref.results_differ(EmuBackend(wide=True).run(case), EmuBackend().run(case), nan_by_place=True) == [], name


@pytest.mark.parametrize("shape", [s for s in gc.SHAPES if s[3] >= 64], ids=ref.shape_id)
def test_members_split_over_calls_equal_the_whole(shape):
    """three calls with the matching slices of zint and of sfc_temp"""
    nens = shape[3]
    for name in ("two_and_two", "p3_set", "nan_cell"):
        case, want = gc.cases(shape)[name], gc.outputs(gc.reference(shape, name))
        parts = [EmuBackend().run(gc.members(case, slice(lo, hi))) for lo, hi in ((0, 1), (1, 37), (37, nens))]
        got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
        assert ref.results_differ(got, want, nan_by_place=True) == [], name


# ------------------------------------------------------------------------------------------------------------------------------
# 2. what the named cases are named for

@pytest.mark.parametrize("shape", gc.SHAPES, ids=ref.shape_id)
def test_census_of_the_named_cases(shape):
    """per case which of t == 0, t == 1 and 0 < t < 1 it reaches; together they reach all three"""
    reached = [False, False, False]
    for name in gc.CASE_NAMES:
        t = gc.reference(shape, name)["t"]
        found = (bool((t == 0).any()), bool((t == 1).any()), bool(((t > 0) & (t < 1)).any()))
        for have, want in zip(found, gc.CENSUS[name]):
            assert have == ((np.prod(shape) > 1) if want is None else want), (name, found)
        reached = [a or b for a, b in zip(reached, found)]
    assert all(reached)
    cloud = gc.reference(shape, "thick_cloud")["t"]
    cols = gc.cloudy_columns(shape)
    for k in range(shape[0]):
        assert ((cloud[k] == 0) == (cols if k in gc.cloud_levels(shape[0]) else np.zeros_like(cols))).all(), k


@pytest.mark.parametrize("shape", gc.SHAPES, ids=ref.shape_id)
def test_named_cases_hold_what_they_are_named_for(shape):
    cs = gc.cases(shape)
    counts = {(len(c["liquid"]), len(c["ice"])) for c in cs.values()}
    assert {n for n, _ in counts} == {0, 1, 2} and {n for _, n in counts} == {0, 1, 2}
    assert any(c["sfc_temp"] is not None for c in cs.values()) and any(c["sfc_temp"] is None for c in cs.values())
    assert cs["p3_set"]["lw_down_top"] > 0
    # all four coefficients zero: no heating at all, to the bit, and the surface emission leaves the top unchanged
    z = gc.reference(shape, "k_zero")
    assert (z["rad_heating"] == 0.0).all() and not np.signbit(z["rad_heating"]).any()
    assert ref.same_bits(z["rad_olr"], z["rad_lw_up_sfc"]) and ref.same_bits(z["temp"], cs["k_zero"]["fields"]["temp"])
    # dt = 0 diagnoses only
    d = gc.reference(shape, "dt_zero")
    assert ref.same_bits(d["temp"], cs["dt_zero"]["fields"]["temp"]) and (d["rad_heating"] != 0).any()
    assert ref.same_bits(EmuBackend().run(cs["dt_zero"])["temp"], cs["dt_zero"]["fields"]["temp"])
    # one NaN in temp: exactly that (column, member) is affected, in every output, and nothing else differs from the same case without it
    k, j, i, e = gc.nan_place(shape)
    bad = gc.reference(shape, "nan_cell")
    clean = ref.radiation(dict(cs["nan_cell"], fields=dict(cs["nan_cell"]["fields"], temp=cs["clear_sky"]["fields"]["temp"])))
    hit = np.zeros(shape[1:], dtype=bool)
    hit[j, i, e] = True
    for n in ref.OUTPUTS:
        nan = np.isnan(bad[n])
        if n == "rad_lw_up_sfc" and k > 0:      # the surface emission lies below the NaN, and the upward sweep carries it up only
            assert not nan.any()
        else:                                   # every level of the column: down from the NaN by D, up from it by U
            assert ((nan.all(axis=0) if nan.ndim == 4 else nan) == hit).all() and ((nan.any(axis=0) if nan.ndim == 4 else nan) == hit).all(), n
        assert ref.same_bits(np.where(hit, 0.0, bad[n]), np.where(hit, 0.0, clean[n])), n


@pytest.mark.parametrize("shape", gc.SHAPES, ids=ref.shape_id)
def test_energy_closure_of_every_column(shape):
    """S_k cap_k heating_k = (U[0] - D[0]) - (U[nz] - D[nz]), cap = (cp_d (rho_d + rho_v)) dz, on the emulation's outputs.
    The bound.  With u = 2^-53, a_k = D[k+1] - D[k] and b_k = U[k] - U[k+1] in exact arithmetic over the stored D and U, the k-th term
    fl(cap_k fl(fl(fl(a_k) + fl(b_k)) / cap_k)) carries five roundings: one on each difference (u |a_k|, u |b_k|), one on their sum, one
    on the quotient and one on the product (3 u |a_k + b_k|), so it is within 4 u (|a_k| + |b_k|) of a_k + b_k to first order.  The
    exact sum of a_k + b_k telescopes to the right-hand side.  The terms are added here with math.fsum, which adds no error, and the
    right-hand side is formed with three roundings, each below u (|U[0]| + |D[0]| + |U[nz]| + |D[nz]|).  With S = sum_k (|a_k| + |b_k|)
    + |U[0]| + |D[0]| + |U[nz]| + |D[nz]| the whole error is below 4 u S, hence below 4 nz u S: the multiple is 4."""
    nz = shape[0]
    for name in FINITE_CASES:
        case, r = gc.cases(shape)[name], gc.reference(shape, name)
        got = EmuBackend().run(case)
        D, Uf, cap = r["D"], r["U"], r["cap"]
        terms = cap * got["rad_heating"]
        mags = np.abs(D[1:] - D[:-1]) + np.abs(Uf[:-1] - Uf[1:])
        rhs = (Uf[0] - D[0]) - (Uf[nz] - D[nz])
        for idx in np.ndindex(*shape[1:]):
            lhs = math.fsum(terms[(slice(None),) + idx])
            S = math.fsum(mags[(slice(None),) + idx]) + abs(Uf[0][idx]) + abs(D[0][idx]) + abs(Uf[nz][idx]) + abs(D[nz][idx])
            assert abs(lhs - rhs[idx]) <= 4 * nz * U * S, (name, idx, lhs, rhs[idx])


@pytest.mark.parametrize("shape", DEEP, ids=ref.shape_id)
def test_physics_of_the_cloud_case(shape):
    """against numpy only: a cloudy column cools most at the cloud's top level, and the surface under the cloud receives more than
    under a clear sky; the clear columns of the cloud case have the bits of the clear-sky case"""
    cloud, clear = gc.reference(shape, "thick_cloud"), gc.reference(shape, "clear_sky")
    cols, top = gc.cloudy_columns(shape), max(gc.cloud_levels(shape[0]))
    assert (np.argmin(cloud["rad_heating"], axis=0)[cols] == top).all() and (cloud["rad_heating"][top][cols] < 0).all()
    assert (cloud["rad_lw_down_sfc"][cols] > clear["rad_lw_down_sfc"][cols]).all()
    for n in ref.OUTPUTS:
        assert ref.same_bits(cloud[n][..., ~cols], clear[n][..., ~cols]), n


CAUGHT_BY = dict(sweeps_swapped="p3_set", one_minus_t_dropped="clear_sky", rho_d_alone="clear_sky", surface_at_level_1="clear_sky")


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_caught_by_the_emulation_comparison(mutant):
    assert set(CAUGHT_BY) == set(ref.MUTANTS)
    for shape in ((2, 1, 3, 3), (7, 3, 2, 65)):
        case = gc.cases(shape)[CAUGHT_BY[mutant]]
        assert ref.results_differ(EmuBackend().run(case), gc.outputs(ref.radiation(case, mutant))) != [], shape


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the C ABI: refusals before any device is asked for; the answer without a device

def _abi_call(lib):
    n = 4 * 2 * 3 * 4                                              # nens 4, nx 3, ny 2, nz 4
    arrays = [np.full(n + 16, 7.25) for _ in range(14)]
    p = [a.ctypes.data for a in arrays]
    names = ("temp", "rd", "rv", "l1", "l2", "i1", "i2", "zint", "sfc", "heat", "olr", "down", "up", "spare")
    P = dict(zip(names, p))
    tab = lambda *ptrs: (C.c_void_p * 2)(*ptrs)
    good = dict(nens=4, nx=3, ny=2, nz=4, nl=2, liquid=tab(P["l1"], P["l2"]), ni=1, ice=tab(P["i1"]), k_d=1e-4, k_v=0.1, k_l=85.0, k_i=40.0,
                sigma=ref.SIGMA, cp_d=1004.0, top=0.0, dt=10.0, **P)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.pam_amd_radiation_gray(a["nens"], a["nx"], a["ny"], a["nz"], a["temp"], a["rd"], a["rv"], a["nl"], a["liquid"], a["ni"], a["ice"],
                                          a["zint"], a["sfc"], a["k_d"], a["k_v"], a["k_l"], a["k_i"], a["sigma"], a["cp_d"], a["top"], a["dt"],
                                          a["heat"], a["olr"], a["down"], a["up"], None)
    return arrays, P, tab, n, call


def test_entry_point_rejects_bad_arguments_and_leaves_the_arrays_untouched():
    """the pointers are host arrays here: a refusal comes before the first HIP call, so nothing dereferences them, and afterwards every
    array still holds the pattern it was filled with"""
    lib = capi.load()
    arrays, P, tab, n, call = _abi_call(lib)
    calls = [dict(nens=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=70000, ny=70000), dict(nl=-1), dict(nl=3), dict(ni=-1), dict(ni=3),
             dict(liquid=None), dict(ice=None), dict(liquid=tab(P["l1"], None)), dict(ice=tab(None)), dict(cp_d=0.0), dict(cp_d=-1.0),
             dict(cp_d=math.nan), dict(cp_d=math.inf)]
    calls += [{name: None} for name in ("temp", "rd", "rv", "zint", "heat", "olr", "down", "up")]
    calls += [{name: bad} for name in ("k_d", "k_v", "k_l", "k_i", "sigma", "top", "dt") for bad in (-1.0e-9, math.nan, math.inf)]
    # an output that overlaps an input or another output: whole arrays, and one element at either end
    calls += [dict(heat=P["temp"]), dict(heat=P["rd"]), dict(temp=P["rv"]), dict(olr=P["down"]), dict(up=P["sfc"]), dict(down=P["zint"]),
              dict(heat=P["l2"] + 8 * n - 8), dict(temp=P["i1"] + 8), dict(olr=P["heat"] + 8 * n - 8), dict(up=P["temp"]),
              dict(olr=P["zint"] + 8 * 19), dict(sfc=P["olr"])]
    for i, kw in enumerate(calls):
        assert call(**kw) == -1, (i, kw)                           # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert lib.pam_amd_awfl_last_error().startswith(b"radiation_gray: "), i
        assert all((a == 7.25).all() for a in arrays), i


def test_entry_point_names_itself_when_there_is_no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    lib = capi.load()
    arrays, P, tab, n, call = _abi_call(lib)
    for kw in (dict(), dict(sfc=None), dict(nl=0, liquid=None, ni=0, ice=None), dict(dt=0.0), dict(olr=P["zint"] + 8 * 20)):
        assert call(**kw) == -2, kw
        assert lib.pam_amd_awfl_last_error() == b"radiation_gray: no HIP device available (this library has no CPU path)"
        assert all((a == 7.25).all() for a in arrays)
    assert lib.pam_amd_radiation_gray_debug_wide_index(1) == 0 and call() == -2 and lib.pam_amd_radiation_gray_debug_wide_index(0) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the C++ plug-in class, its Python mirror, the driver, the tools

RAD_H = os.path.join(HOST, "physics", "radiation", "gray_amd", "radiation.h")


def test_cxx_class_compiles_in_one_translation_unit(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "physics/micro/none/Microphysics.h"\n#include "physics/radiation/gray_amd/radiation.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  Microphysics micro;\n  Radiation rad;\n  micro.init(coupler);\n"
                   '  coupler.set_option<int>("rad_gray_every", 3);\n'
                   "  rad.init(coupler);\n  rad.timeStep(coupler);\n  rad.finalize(coupler);\n  return (int)rad.radiation_name().size();\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cxx_class_and_python_class_name_the_same_fields_and_options():
    import pam_amd
    from pam_amd import physics
    assert pam_amd.RadiationGray is physics.RadiationGray and physics.RadiationGray.radiation_name() == "gray"
    text, py = open(RAD_H).read(), inspect.getsource(physics.RadiationGray)
    names = ('"radiation"', '"gray"', '"rad_gray_k_d"', '"rad_gray_k_v"', '"rad_gray_k_l"', '"rad_gray_k_i"', '"rad_gray_lw_down_top"',
             '"rad_gray_every"', '"rad_heating"', '"rad_olr"', '"rad_lw_down_sfc"', '"rad_lw_up_sfc"', '"sfc_temp"', '"sigma"', "5.670374419e-8",
             '"micro"', '"kessler"', '"p3"', '"cloud_liquid"', '"cloud_water"', '"ice"', '"crm_dt"', '"cp_d"', "pam_amd_radiation_gray(",
             "pam_amd_radiation_forced(", "untuned")
    for s in names:
        assert s in text and s in py, s
    sig = inspect.signature(physics.RadiationGray.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("k_d", 1e-4), ("k_v", 0.1), ("k_l", 85.0), ("k_i", 40.0), ("lw_down_top", 0.0),
                                                                   ("every", 1)]
    assert physics.RadiationGray.CONDENSATE == {"kessler": (("cloud_liquid",), ()), "p3": (("cloud_water",), ("ice",)), "none": ((), ())}


def test_driver_bench_tool_and_documents_know_the_scheme():
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert drv.count('"--radiation-gray"') == 1 and drv.count("[--radiation-gray [EVERY]]") >= 2 and "radiation gray:" in drv
    tool = open(os.path.join(ROOT, "tools", "bench_modules.py")).read()
    assert '"grayrad"' in tool and "pam_amd_radiation_gray" in tool
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "radiation_gray" in open(os.path.join(ROOT, doc)).read() or "gray_amd/radiation.h" in open(os.path.join(ROOT, doc)).read(), doc
    assert "untuned" in open(os.path.join(ROOT, "DESIGN.md")).read()
