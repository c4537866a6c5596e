"""The native grey two-stream shortwave radiation scheme, everything that needs no GPU: the device bodies under g++
(tests/emu/grayrad_sw_emu.cpp) against the numpy restatement (tests/grayrad_sw_ref.py) bit for bit on every shape and named case; the
census of what the named cases reach; the mutants; the energy closure of every column and the conservative-scattering property within
bounds counted from the roundings; Beer's law; the all-zero case; the physics of the cloud case; night; the day members of a mixed
wavefront alone; members split over calls; the wide-index instance; the C ABI's refusals and its answer without a device; the C++ plug-in
class and its Python mirror."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import grayrad_sw_ref as ref
import grayrad_sw_cases as sc
from grayrad_sw_emu_harness import EmuBackend, POISON
from pam_amd import capi
from tools import native_build
from tools.native_build import syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
U = 2.0 ** -53
FINITE_CASES = tuple(n for n in sc.CASE_NAMES if n not in ("nan_cell", "nan_coszen"))
DEEP = [s for s in sc.SHAPES if s[0] >= 5]          # shapes whose cloud layer lies inside the column
_EMU = {}


def emu(shape, name):
    """the emulation's outputs of a named case, computed once"""
    if (shape, name) not in _EMU:
        _EMU[shape, name] = EmuBackend().run(sc.cases(shape)[name])
    return _EMU[shape, name]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the device bodies under g++

@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape):
    """every named case; the first shape has one level, so both boundaries fall in one cell"""
    for name in sc.CASE_NAMES:
        assert ref.results_differ(emu(shape, name), sc.outputs(sc.reference(shape, name)), nan_by_place=True) == [], name


@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_wide_index_instance_equals_the_narrow_one(shape):
    for name in ("two_and_two", "mixed_night", "nan_cell"):
        assert ref.results_differ(EmuBackend(wide=True).run(sc.cases(shape)[name]), emu(shape, name), nan_by_place=True) == [], name


@pytest.mark.parametrize("shape", [s for s in sc.SHAPES if s[3] >= 64], ids=ref.shape_id)
def test_members_split_over_calls_equal_the_whole(shape):
    """three calls with the matching slices of zint, coszen and sfc_albedo"""
    nens = shape[3]
    for name in ("two_and_two", "mixed_night", "nan_coszen", "nan_cell"):
        case, want = sc.cases(shape)[name], sc.outputs(sc.reference(shape, name))
        parts = [EmuBackend().run(sc.members(case, slice(lo, hi))) for lo, hi in ((0, 1), (1, 37), (37, nens))]
        got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
        assert ref.results_differ(got, want, nan_by_place=True) == [], name


@pytest.mark.parametrize("shape", [s for s in sc.SHAPES if s[3] > 1], ids=ref.shape_id)
def test_day_members_of_a_mixed_wavefront_equal_the_same_members_alone(shape):
    case = sc.cases(shape)["mixed_night"]
    day = np.flatnonzero(~(case["coszen"] <= 0))
    assert 0 < day.size < shape[3]
    alone, whole = EmuBackend().run(sc.members(case, day)), emu(shape, "mixed_night")
    assert ref.results_differ(alone, {n: whole[n][..., day] for n in ref.OUTPUTS}) == []


# ------------------------------------------------------------------------------------------------------------------------------
# 2. what the named cases are named for

@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_census_of_the_named_cases(shape):
    """per case which of ta == 0, ta == 1, 0 < ta < 1, b == 0, b > 0 its day members reach and whether night and day share a group of 64
    lanes; together the cases reach all of them wherever the shape has a second member"""
    reached = [False] * 6
    for name in sc.CASE_NAMES:
        found = sc.census(shape, sc.reference(shape, name), sc.cases(shape)[name])
        assert found == sc.expected(shape, name), (name, found)
        reached = [a or b for a, b in zip(reached, found)]
    assert all(reached[:5]) and reached[5] == (shape[3] > 1)
    black, cols = sc.reference(shape, "black_absorber")["ta"], sc.cloudy_columns(shape)
    for k in range(shape[0]):
        assert ((black[k] == 0) == (cols if k in sc.cloud_levels(shape[0]) else np.zeros_like(cols))).all(), k


@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_named_cases_hold_what_they_are_named_for(shape):
    cs = sc.cases(shape)
    counts = {(len(c["liquid"]), len(c["ice"])) for c in cs.values()}
    assert {n for n, _ in counts} == {0, 1, 2} and {n for _, n in counts} == {0, 1, 2}
    assert any(c["sfc_albedo"] is not None for c in cs.values()) and any(c["sfc_albedo"] is None for c in cs.values())
    assert cs["beer"]["albedo"] == 0.0 and cs["albedo_one"]["albedo"] == 1.0 and (cs["grazing"]["coszen"] == 1.0e-3).all()
    mixed = cs["mixed_night"]["coszen"]
    if shape[3] >= 7:
        assert (mixed == 0).any() and np.signbit(mixed[mixed == 0]).any() and (mixed < 0).any() and (mixed > 0).any()
    # dt = 0 diagnoses only
    d = emu(shape, "dt_zero")
    assert ref.same_bits(d["temp"], cs["dt_zero"]["fields"]["temp"]) and (d["rad_sw_heating"] != 0).any()
    # one NaN in the vapour: exactly that (column, member) is affected, in every output and at every level, and nothing else differs from
    # the same case without it
    k, j, i, e = sc.nan_place(shape)
    bad = emu(shape, "nan_cell")
    clean = ref.radiation(dict(cs["nan_cell"], fields=dict(cs["nan_cell"]["fields"], water_vapor=cs["clear_sky"]["fields"]["water_vapor"])))
    hit = np.zeros(shape[1:], dtype=bool)
    hit[j, i, e] = True
    for n in ref.OUTPUTS:
        nan = np.isnan(bad[n])
        assert ((nan.all(axis=0) if nan.ndim == 4 else nan) == hit).all() and ((nan.any(axis=0) if nan.ndim == 4 else nan) == hit).all(), n
        assert ref.same_bits(np.where(hit, 0.0, bad[n]), np.where(hit, 0.0, clean[n])), n
    # one NaN coszen: it is day, fills the columns of its own member with NaN, and no other member sees it
    bad, m = emu(shape, "nan_coszen"), shape[3] // 2
    clean = sc.reference(shape, "cloud")
    others = np.arange(shape[3]) != m
    for n in ref.OUTPUTS:
        assert np.isnan(bad[n][..., m]).all(), n
        assert ref.same_bits(bad[n][..., others], clean[n][..., others]), n


@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_night_outputs_are_exact_zeros_and_temp_keeps_its_bits(shape):
    """mu0 <= 0, 0.0 and -0.0 included: +0.0 over the poison in the heating and in the three fluxes, temp untouched; an all-night call
    too"""
    case = sc.cases(shape)["mixed_night"]
    for c in (case, dict(case, coszen=np.where(np.arange(shape[3]) % 2 == 0, -0.0, -1.0))):
        night = c["coszen"] <= 0
        got = emu(shape, "mixed_night") if c is case else EmuBackend().run(c)
        assert night.all() or c is case
        for n in ref.OUTPUTS[1:]:
            z = got[n][..., night]
            assert (z == 0.0).all() and not np.signbit(z).any(), n
            assert not (got[n][..., ~night] == POISON).any(), n
        assert ref.same_bits(got["temp"][..., night], c["fields"]["temp"][..., night])
        if (~night).any():
            assert not ref.same_bits(got["temp"][..., ~night], c["fields"]["temp"][..., ~night])


@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_energy_closure_of_every_column(shape):
    """S_k cap_k heating_k = (Fd[nz] - Fu[nz]) - (Fd[0] - Fu[0]), cap = (cp_d (rho_d + rho_v)) dz, on the emulation's outputs, for every
    day member of every finite case.
    The bound, counted as tests/test_grayrad.py counts the longwave one.  With u = 2^-53, a_k = Fd[k+1] - Fd[k] and b_k = Fu[k] - Fu[k+1]
    in exact arithmetic over the stored fluxes, the k-th term fl(cap_k fl(fl(fl(a_k) + fl(b_k)) / cap_k)) carries five roundings: one on
    each difference (u |a_k|, u |b_k|), one on their sum, one on the quotient and one on the product (3 u |a_k + b_k|), so it is within
    4 u (|a_k| + |b_k|) of a_k + b_k to first order.  The exact sum of a_k + b_k telescopes to the right-hand side.  The terms are added
    with math.fsum, which adds no error, and the right-hand side is formed with three roundings, each below u (|Fd[0]| + |Fu[0]| +
    |Fd[nz]| + |Fu[nz]|).  With S = sum_k (|a_k| + |b_k|) + |Fd[0]| + |Fu[0]| + |Fd[nz]| + |Fu[nz]| the whole error is below 4 u S,
    hence below 4 nz u S: the multiple is 4.  (Fluxes that underflow, under the grazing sun, err by 2^-1075 each, far below u Fd[nz].)"""
    nz = shape[0]
    for name in FINITE_CASES:
        r, got = sc.reference(shape, name), emu(shape, name)
        Fd, Fu, cap = r["Fd"], r["Fu"], r["cap"]
        assert ref.same_bits(got["rad_sw_down_sfc"][..., ~r["night"]], Fd[0][..., ~r["night"]])
        with np.errstate(all="ignore"):
            terms = cap * got["rad_sw_heating"]
            mags = np.abs(Fd[1:] - Fd[:-1]) + np.abs(Fu[:-1] - Fu[1:])
            rhs = (Fd[nz] - Fu[nz]) - (Fd[0] - Fu[0])
        for idx in np.ndindex(*shape[1:]):
            if r["night"][idx[2]]:
                continue
            lhs = math.fsum(terms[(slice(None),) + idx])
            S = math.fsum(mags[(slice(None),) + idx]) + abs(Fd[0][idx]) + abs(Fu[0][idx]) + abs(Fd[nz][idx]) + abs(Fu[nz][idx])
            assert abs(lhs - rhs[idx]) <= 4 * nz * U * S, (name, idx, lhs, rhs[idx])


@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_conservative_scattering_carries_the_net_flux_through(shape):
    """all four a_* zero: ta = 1.0, so T = tr and R = fl(1 - tr).  The net flux N[k] = Fd[k] - Fu[k] is the same at every interface to
    rounding, and the heating is that rounding.
    The bound, to first order in u = 2^-53, every quantity below being the stored one of level k (Rb, R, T, q <= 1, 1 / q >= 1).
    In exact arithmetic over the stored R, T and Rb[k], with R + T = 1 + d (|d| <= u, the rounding of r), the adding step gives
    1 - Rb*[k+1] = T (1 - Rb[k]) / q - d (T Rb[k] / q + 1), Rb* being the unrounded Rb[k+1], and T Fd[k+1] / q is the unrounded Fd[k].
    So N[k+1] - N[k], both taken as Fd (1 - Rb), is made of: the rounding of Fd[k], three operations on a q that itself carries two
    absolute roundings below u, |eF| <= (3 + 2 / q) u Fd[k] <= 5 u Fd[k] / q; the one of Rb[k+1], |eR| <= (4 + 2 / q) u <= 6 u / q (two
    products, q, the quotient, the sum), times Fd[k+1]; and d (T Rb / q + 1) Fd[k+1] <= 2 u Fd[k+1] / q.  Fu = fl(Rb Fd) adds u Fd[k] and
    u Fd[k+1].  Together |N[k+1] - N[k]| <= u (6 Fd[k] + 9 Fd[k+1]) / q =: B_k over the stored fluxes, and forming the two N here adds
    u (Fd[k] + Fd[k+1]).  cap_k heating_k is that difference formed with the five roundings of the energy-closure test, within
    4 u (|a_k| + |b_k|) of it."""
    r, got = sc.reference(shape, "conservative"), emu(shape, "conservative")
    Fd, Fu, q, cap = r["Fd"], r["Fu"], r["q"], r["cap"]
    assert (r["ta"] == 1.0).all() and not r["night"].any()
    N = Fd - Fu
    B = U * (6 * Fd[:-1] + 9 * Fd[1:]) / q
    assert (np.abs(N[1:] - N[:-1]) <= B + U * (Fd[:-1] + Fd[1:])).all()
    mags = np.abs(Fd[1:] - Fd[:-1]) + np.abs(Fu[:-1] - Fu[1:])
    assert (np.abs(cap * got["rad_sw_heating"]) <= B + 4 * U * mags).all()
    # and it is rounding noise beside the same clouds when they absorb: the largest heating is a 10^-9 of theirs
    assert np.abs(got["rad_sw_heating"]).max() < 1e-9 * np.abs(emu(shape, "two_and_two")["rad_sw_heating"]).max()


@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_beers_law_without_scattering_over_a_black_surface(shape):
    """s_l = s_i = 0 and albedo 0: every Fu is 0.0, Fd[0] is the product of the ta down the column to the bit, and it is
    solar_constant mu0 exp(-m S_k a_k dz_k).  The tolerance of the last: every factor ta_k carries the relative error of da_k, six
    roundings, which the exponential turns into 6 u da_k, that of exp_c (a degree-13 Taylor series on |r| <= ln 2 / 2: truncation below
    10^-17, and some 2 u of Horner rounding beside the reduction's), and one rounding of the product: below (8 nz + 8 S da) u"""
    case, r, got = sc.cases(shape)["beer"], sc.reference(shape, "beer"), emu(shape, "beer")
    assert (got["rad_sw_up_sfc"] == 0.0).all() and (got["rad_sw_up_top"] == 0.0).all() and (r["Fu"] == 0.0).all()
    Fd = np.broadcast_to(case["solar_constant"] * case["coszen"], shape[1:]).copy()
    for k in range(shape[0] - 1, -1, -1):
        Fd = r["ta"][k] * Fd
    assert ref.same_bits(got["rad_sw_down_sfc"], Fd)
    tau = r["da"].astype(np.longdouble).sum(axis=0)
    want = (case["solar_constant"] * case["coszen"]).astype(np.longdouble) * np.exp(-tau)
    assert (np.abs(got["rad_sw_down_sfc"] - want) <= (8 * shape[0] + 8 * tau) * U * want).all()
    assert (got["rad_sw_heating"] > 0).all()


@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_all_zero_coefficients_are_exact(shape):
    """every coefficient zero: Fu[k] = albedo Fd[nz] at every k, so both upward outputs have those bits, the sun reaches the ground
    whole, and the heating is +0.0 exactly"""
    case, got = sc.cases(shape)["all_zero"], emu(shape, "all_zero")
    top = np.broadcast_to(case["solar_constant"] * case["coszen"], shape[1:])
    assert ref.same_bits(got["rad_sw_down_sfc"], top)
    assert ref.same_bits(got["rad_sw_up_sfc"], case["albedo"] * top) and ref.same_bits(got["rad_sw_up_top"], case["albedo"] * top)
    assert (got["rad_sw_heating"] == 0.0).all() and not np.signbit(got["rad_sw_heating"]).any()
    assert ref.same_bits(got["temp"], case["fields"]["temp"])
    r = sc.reference(shape, "all_zero")
    assert ref.same_bits(r["Fu"], np.broadcast_to(case["albedo"] * top, r["Fu"].shape))


@pytest.mark.parametrize("shape", DEEP, ids=ref.shape_id)
def test_physics_of_the_cloud_case(shape):
    """a cloudy column reflects more to the top and passes less to the surface than the same column without its cloud, and heats most
    in the cloud; the clear columns of the cloud case have the bits of the clear-sky case; over a white surface nothing is absorbed
    there, so more leaves the top"""
    cloud, clear = emu(shape, "cloud"), emu(shape, "clear_sky")
    cols, levels = sc.cloudy_columns(shape), sc.cloud_levels(shape[0])
    assert (cloud["rad_sw_up_top"][cols] > clear["rad_sw_up_top"][cols]).all()
    assert (cloud["rad_sw_down_sfc"][cols] < clear["rad_sw_down_sfc"][cols]).all()
    assert np.isin(np.argmax(cloud["rad_sw_heating"], axis=0)[cols], levels).all() and (cloud["rad_sw_heating"] > 0).all()
    for n in ref.OUTPUTS:
        assert ref.same_bits(cloud[n][..., ~cols], clear[n][..., ~cols]), n
    assert (emu(shape, "albedo_one")["rad_sw_up_top"] > cloud["rad_sw_up_top"]).all()


CAUGHT_BY = dict(r_from_b="two_and_two", trt_other_way="cloud", m_before_dz="clear_sky", night_not_positive="nan_coszen",
                 fu_from_rb_above="clear_sky")


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_caught_by_the_emulation_comparison(mutant):
    assert set(CAUGHT_BY) == set(ref.MUTANTS)
    for shape in ((5, 1, 4, 64), (7, 3, 2, 65)):
        case = sc.cases(shape)[CAUGHT_BY[mutant]]
        assert ref.results_differ(emu(shape, CAUGHT_BY[mutant]), sc.outputs(ref.radiation(case, mutant)), nan_by_place=True) != [], shape


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the C ABI: its symbols; refusals before any device is asked for; the answer without a device

def test_capi_symbols():
    lib = capi.load()
    for name in ("pam_amd_radiation_gray_sw", "pam_amd_radiation_gray_sw_debug_wide_index"):
        assert name in capi.MODULE_SYMBOLS and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read()
    assert "int pam_amd_radiation_gray_sw(int nens" in header and "int pam_amd_radiation_gray_sw_debug_wide_index(int on);" in header
    assert len(capi.MODULE_SYMBOLS["pam_amd_radiation_gray_sw"][1]) == 29


def _abi_call(lib):
    n = 4 * 2 * 3 * 4                                              # nens 4, nx 3, ny 2, nz 4
    names = ("temp", "rd", "rv", "l1", "l2", "i1", "i2", "zint", "coszen", "alb", "heat", "down", "up", "top", "spare")
    arrays = [np.full(n + 16, 7.25) for _ in names]
    P = dict(zip(names, [a.ctypes.data for a in arrays]))
    tab = lambda *ptrs: (C.c_void_p * 2)(*ptrs)
    good = dict(nens=4, nx=3, ny=2, nz=4, nl=2, liquid=tab(P["l1"], P["l2"]), ni=1, ice=tab(P["i1"]), solar=1361.0, a_d=1e-6, a_v=2e-3, a_l=0.1,
                a_i=0.1, s_l=11.0, s_i=5.0, albedo=0.07, cp_d=1004.0, dt=10.0, **P)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.pam_amd_radiation_gray_sw(a["nens"], a["nx"], a["ny"], a["nz"], a["temp"], a["rd"], a["rv"], a["nl"], a["liquid"], a["ni"],
                                             a["ice"], a["zint"], a["coszen"], a["alb"], a["solar"], a["a_d"], a["a_v"], a["a_l"], a["a_i"],
                                             a["s_l"], a["s_i"], a["albedo"], a["cp_d"], a["dt"], a["heat"], a["down"], a["up"], a["top"], None)
    return arrays, P, tab, n, call


def test_entry_point_rejects_bad_arguments_and_leaves_the_arrays_untouched():
    """the pointers are host arrays here: a refusal comes before the first HIP call, so nothing dereferences them, and afterwards every
    array still holds the pattern it was filled with"""
    lib = capi.load()
    arrays, P, tab, n, call = _abi_call(lib)
    calls = [dict(nens=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=70000, ny=70000), dict(nl=-1), dict(nl=3), dict(ni=-1), dict(ni=3),
             dict(liquid=None), dict(ice=None), dict(liquid=tab(P["l1"], None)), dict(ice=tab(None)), dict(cp_d=0.0), dict(cp_d=-1.0),
             dict(cp_d=math.nan), dict(cp_d=math.inf), dict(albedo=-1.0e-9), dict(albedo=1.0 + 1.0e-9), dict(albedo=math.nan),
             dict(albedo=math.inf)]
    calls += [{name: None} for name in ("temp", "rd", "rv", "zint", "coszen", "heat", "down", "up", "top")]
    calls += [{name: bad} for name in ("solar", "a_d", "a_v", "a_l", "a_i", "s_l", "s_i", "dt") for bad in (-1.0e-9, math.nan, math.inf)]
    # an output that overlaps an input or another output: whole arrays, and one element at either end
    calls += [dict(heat=P["temp"]), dict(heat=P["rd"]), dict(temp=P["rv"]), dict(top=P["down"]), dict(up=P["alb"]), dict(down=P["zint"]),
              dict(heat=P["l2"] + 8 * n - 8), dict(temp=P["i1"] + 8), dict(top=P["heat"] + 8 * n - 8), dict(up=P["temp"]),
              dict(top=P["zint"] + 8 * 19), dict(alb=P["top"]), dict(down=P["coszen"] + 8 * 3), dict(coszen=P["heat"])]
    for i, kw in enumerate(calls):
        assert call(**kw) == -1, (i, kw)                           # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert lib.pam_amd_awfl_last_error().startswith(b"radiation_gray_sw: "), i
        assert all((a == 7.25).all() for a in arrays), i


def test_entry_point_names_itself_when_there_is_no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    lib = capi.load()
    arrays, P, tab, n, call = _abi_call(lib)
    for kw in (dict(), dict(alb=None), dict(nl=0, liquid=None, ni=0, ice=None), dict(dt=0.0), dict(albedo=0.0), dict(albedo=1.0),
               dict(top=P["zint"] + 8 * 20), dict(down=P["coszen"] + 8 * 4)):
        assert call(**kw) == -2, kw
        assert lib.pam_amd_awfl_last_error() == b"radiation_gray_sw: no HIP device available (this library has no CPU path)"
        assert all((a == 7.25).all() for a in arrays)
    assert lib.pam_amd_radiation_gray_sw_debug_wide_index(1) == 0 and call() == -2 and lib.pam_amd_radiation_gray_sw_debug_wide_index(0) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the C++ plug-in class, its Python mirror, the driver, the tools

RAD_H = os.path.join(HOST, "physics", "radiation", "gray_amd", "radiation.h")


def test_cxx_class_compiles_with_the_sun_on(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "physics/micro/none/Microphysics.h"\n#include "physics/radiation/gray_amd/radiation.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  Microphysics micro;\n  Radiation rad;\n  micro.init(coupler);\n"
                   '  coupler.set_option<bool>("rad_gray_shortwave", true);\n  coupler.set_option<real>("rad_gray_sw_coszen", 0.5);\n'
                   "  rad.init(coupler);\n  rad.timeStep(coupler);\n  rad.finalize(coupler);\n  return (int)rad.radiation_name().size();\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cxx_class_and_python_class_name_the_same_fields_and_options():
    from pam_amd import physics
    text, py = open(RAD_H).read(), inspect.getsource(physics.RadiationGray)
    names = ['"rad_gray_shortwave"', '"rad_sw_heating"', '"rad_sw_down_sfc"', '"rad_sw_up_sfc"', '"rad_sw_up_top"', '"rad_coszen"', '"sfc_albedo"',
             "pam_amd_radiation_gray_sw(", "untuned starting points"]
    names += ['"rad_gray_sw_%s"' % n for n in ("solar_constant", "albedo", "a_d", "a_v", "a_l", "a_i", "s_l", "s_i")]
    for s in names:
        assert s in text and s in py, s
    assert text.count("pam_amd_radiation_forced(") >= 2 and py.count("pam_amd_radiation_forced(") >= 2
    sig = inspect.signature(physics.RadiationGray.shortwave).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("shortwave", True), ("solar_constant", 1361.0), ("coszen", 1.0), ("albedo", 0.07),
                                                                   ("a_d", 1e-6), ("a_v", 2e-3), ("a_l", 0.1), ("a_i", 0.1), ("s_l", 11.0), ("s_i", 5.0)]
    for n, v in (("solar_constant", "1361.0"), ("albedo", "0.07"), ("a_d", "1.0e-6"), ("a_v", "2.0e-3"), ("a_l", "0.1"), ("a_i", "0.1"), ("s_l", "11.0"),
                 ("s_i", "5.0")):
        assert 'dflt(coupler, "rad_gray_sw_%s", %s);' % (n, v) in text, n
    rad = physics.RadiationGray(every=2)
    assert rad.sun is False and rad.shortwave(coszen=0.5) is rad and rad.sun is True and rad.coszen == 0.5
    assert rad.sw_defaults == (1361.0, 0.07, 1e-6, 2e-3, 0.1, 0.1, 11.0, 5.0)


def test_driver_bench_tool_and_documents_know_the_shortwave():
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert drv.count('"--shortwave"') == 1 and drv.count("[--shortwave COSZEN [ALBEDO]]") >= 2 and "sw_down_sfc" in drv and "sw_up_top" in drv
    tool = open(os.path.join(ROOT, "tools", "bench_modules.py")).read()
    assert '"grayrad_sw"' in tool and "pam_amd_radiation_gray_sw" in tool
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "radiation_gray_sw" in open(os.path.join(ROOT, doc)).read() or "rad_gray_shortwave" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.join(native_build.CSRC, "grayrad_sw_device.h") in native_build.dependencies(native_build.LIB_SOURCES)
