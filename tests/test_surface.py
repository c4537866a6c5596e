"""Bulk surface fluxes over a slab ocean, everything that needs no GPU: the device body under g++ (tests/emu/surface_emu.cpp) against the
numpy restatement (tests/surface_ref.py) bit for bit on every shape and named case; the census of what the named cases reach; two sanity
anchors; the slab step; members split over calls; the C ABI's symbol, its refusals and its answer without a device; the host arithmetic
of surface_fluxes_init; the C++ module, the driver, the tool and the documents."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import surface_ref as ref
import surface_cases as sc
from surface_emu_harness import EmuBackend
from pam_amd import capi
from tools import native_build
from tools.native_build import syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
_EMU = {}


def emu(shape, name):
    """the emulation's outputs of a named case, computed once"""
    if (shape, name) not in _EMU:
        _EMU[shape, name] = EmuBackend().run(sc.cases(shape)[name])
    return _EMU[shape, name]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the device body under g++

@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape):
    for name in sc.CASE_NAMES:
        assert ref.results_differ(emu(shape, name), sc.outputs(sc.reference(shape, name)), nan_by_place=True) == [], name


@pytest.mark.parametrize("shape", [s for s in sc.SHAPES if s[3] >= 64], ids=ref.shape_id)
def test_members_split_over_calls_equal_the_whole(shape):
    """three calls with the matching slices of zmid, cn, cstar, sfc_temp and the radiation"""
    nens = shape[3]
    for name in ("mixed", "nan_cell", "lw_only"):
        case, want = sc.cases(shape)[name], sc.outputs(sc.reference(shape, name))
        parts = [EmuBackend().run(ref.members(case, slice(lo, hi))) for lo, hi in ((0, 1), (1, 37), (37, nens))]
        got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
        assert ref.results_differ(got, want, nan_by_place=True) == [], name


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the census, on the restatement alone

@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_census_of_the_named_cases(shape):
    """mixed: both branches of f in every group of 64 consecutive members of every column (with fewer than 64 members: over the whole
    shape; the shape of ONE element can hold one branch only, and there the census asks for exactly that); neutral: rib == 0 everywhere,
    so f == 1 and ch == cn in bits; dew: sfc_lhf < 0 somewhere; calm: only the gust term carries the exchange; the NaNs stay in place"""
    nz, ny, nx, nens = shape
    rib = sc.reference(shape, "mixed")["rib"]
    assert not np.isnan(rib).any()
    if nens >= 64:
        for j in range(ny):
            for i in range(nx):
                for lo in range(0, nens - 63):
                    g = rib[j, i, lo:lo + 64]
                    assert (g < 0).any() and (g >= 0).any(), (j, i, lo)
    elif rib.size > 1:
        assert (rib < 0).any() and (rib >= 0).any()
    else:
        assert ((rib < 0) | (rib >= 0)).all()
    sa, Ts = sc.reference(shape, "mixed")["sa"], sc.cases(shape)["mixed"]["sfc_temp"]
    if rib.size > 1:
        assert (Ts > sa).any() and (Ts < sa).any()
    neutral = sc.reference(shape, "neutral")
    assert (neutral["rib"] == 0.0).all() and (neutral["f"] == 1.0).all()
    assert ref.same_bits(neutral["tva"], neutral["tvs"])
    assert ref.same_bits(neutral["ch"], np.broadcast_to(sc.cases(shape)["neutral"]["cn"], (ny, nx, nens)))
    dew = sc.reference(shape, "dew")
    assert (dew["qv"] > dew["qs"]).all() and (dew["sfc_lhf"] < 0).any()
    calm = sc.reference(shape, "calm")
    assert (calm["w"] == sc.cases(shape)["calm"]["gust"]).all()
    assert (sc.reference(shape, "dry_surface")["qs"] == 0.0).all()
    (jt, it, et), (js, is_, es) = sc.nan_places(shape)
    nan = sc.reference(shape, "nan_cell")
    want = np.zeros((ny, nx, nens), dtype=bool)
    want[jt, it, et] = want[js, is_, es] = True
    for n in ref.OUTPUTS:
        assert np.array_equal(np.isnan(nan[n]), want), n


def _anchor(Ts, air, qv, wind):
    z, z0, rho = 50.0, 1.0e-4, 1.15
    cn, cstar = ref.transfer_parameters(np.array([z]), np.array([z0]))
    one = lambda x: np.full((1, 1, 1, 1), x)
    case = dict(sc.CONSTANTS, gust=1.0, fields=dict(temp=one(air), density_dry=one(rho * (1.0 - qv)), water_vapor=one(rho * qv), uvel=one(wind),
                                                    vvel=one(0.0)),
                zmid=np.array([[z]]), cn=cn, cstar=cstar, sfc_temp=np.full((1, 1, 1), Ts), lw_down=None, lw_up=None, sw_down=None, sw_up=None,
                slab_heat_capacity=0.0)
    r = ref.surface(case, internals=True)
    got = {k: float(r[k].ravel()[0]) for k in ("rib", "ch", "sfc_shf", "sfc_lhf")}
    # the same in the textbook's words, with libm: guards a sign or a unit slip, not the rounding
    C_ = sc.CONSTANTS
    es = 610.94 * math.exp(17.625 * (Ts - 273.15) / (243.04 + Ts - 273.15))
    qs = C_["wetness"] * es / (C_["R_v"] * Ts) / rho
    sa = air + C_["grav"] / C_["cp_d"] * z
    w = math.sqrt(wind * wind + 1.0)
    tva, tvs = sa * (1 + 0.608 * qv), Ts * (1 + 0.608 * qs)
    rib = C_["grav"] * z * (tva - tvs) / (tvs * w * w)
    cn_ = (0.4 / math.log(z / z0)) ** 2
    f = 1 - 9.4 * rib / (1 + 5.3 * 9.4 * cn_ * math.sqrt(z / z0) * math.sqrt(-rib)) if rib < 0 else 1 / (1 + 4.7 * rib) ** 2
    plain = dict(rib=rib, ch=cn_ * f, sfc_shf=rho * C_["cp_d"] * cn_ * f * w * (Ts - sa), sfc_lhf=rho * C_["latvap"] * cn_ * f * w * (qs - qv))
    for k in got:
        assert got[k] == pytest.approx(plain[k], rel=1e-9), k
    return got


def test_sanity_anchors():
    """z = 50 m, z0 = 1e-4 m, rho = 1.15, gust = 1: a warm ocean under a trade wind, and warm air over a cold surface.  The figures are what
    the restatement printed; each is held to 5 %"""
    warm = _anchor(300.0, 298.5, 0.015, 5.0)
    print("warm ocean:", warm)
    assert warm["sfc_shf"] == pytest.approx(6.0881165761, rel=0.05) and warm["sfc_lhf"] == pytest.approx(100.548795422, rel=0.05)
    assert warm["rib"] == pytest.approx(-0.139327706244, rel=0.05) and warm["ch"] == pytest.approx(1.02123602397e-3, rel=0.05)
    stable = _anchor(295.0, 299.0, 0.012, 3.0)
    print("stable:", stable)
    assert stable["rib"] == pytest.approx(0.615132890989, rel=0.05) and stable["ch"] == pytest.approx(6.13685115758e-5, rel=0.05)
    assert stable["sfc_shf"] == pytest.approx(-1.00626172005, rel=0.05)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_slab_step(shape):
    """slab_heat_capacity (sfc_temp_new - Ts) / dt equals net within the rounding of the three operations involved (the product with dt,
    the division, the sum with Ts): 4 ulp of max(|Ts| slab_heat_capacity / dt, |net|); without a slab, and with dt = 0, sfc_temp keeps
    its bits"""
    for name in ("mixed", "no_radiation", "lw_only", "dew", "calm"):
        case, r = sc.cases(shape)[name], sc.reference(shape, name)
        cap, dt, Ts = case["slab_heat_capacity"], case["dt"], case["sfc_temp"]
        got = cap * (emu(shape, name)["sfc_temp"] - Ts) / dt
        bound = 4.0 * np.spacing(np.maximum(np.abs(Ts) * cap / dt, np.abs(r["net"])))
        assert (np.abs(got - r["net"]) <= bound).all(), name
        assert not ref.same_bits(emu(shape, name)["sfc_temp"], Ts), name
    for name in ("slab_off", "dt_zero"):
        assert ref.same_bits(emu(shape, name)["sfc_temp"], sc.cases(shape)[name]["sfc_temp"]), name
        assert ref.results_differ({n: emu(shape, name)[n] for n in ("sfc_shf", "sfc_lhf")},
                                  {n: sc.reference(shape, "mixed")[n] for n in ("sfc_shf", "sfc_lhf")}) == [], name
    (js, is_, es) = sc.nan_places(shape)[1]
    for name in ("slab_off", "dt_zero"):                      # and a NaN sfc_temp keeps its bits too
        case = dict(sc.cases(shape)[name], sfc_temp=sc.cases(shape)["nan_cell"]["sfc_temp"])
        assert ref.same_bits(EmuBackend().run(case)["sfc_temp"], case["sfc_temp"]), name
    net = sc.reference(shape, "no_radiation")["net"]
    both = sc.reference(shape, "mixed")
    assert ref.same_bits(net, 0.0 - (both["sfc_shf"] + both["sfc_lhf"]))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the C ABI: its symbol; refusals before any device is asked for; the answer without a device

def test_capi_symbol():
    lib = capi.load()
    assert "pam_amd_surface_fluxes" in capi.MODULE_SYMBOLS and lib.pam_amd_surface_fluxes is not None
    header = open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read()
    assert "int pam_amd_surface_fluxes(int nens, int nx, int ny, int nz, const double *temp" in header
    assert "1000.0" in header and "4186.0" in header
    assert len(capi.MODULE_SYMBOLS["pam_amd_surface_fluxes"][1]) == 28


def _abi_call(lib):
    n = 4 * 2 * 3 * 4                                              # nens 4, nx 3, ny 2, nz 4
    names = ("temp", "rd", "rv", "u", "v", "zmid", "cn", "cstar", "ts", "lwd", "lwu", "swd", "swu", "shf", "lhf", "spare")
    arrays = [np.full(n + 16, 7.25) for _ in names]
    P = dict(zip(names, [a.ctypes.data for a in arrays]))
    good = dict(nens=4, nx=3, ny=2, nz=4, gust=1.0, wetness=0.98, grav=9.80616, cp_d=1004.64, R_v=461.505, latvap=2501000.0, cap=4186000.0,
                dt=10.0, **P)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.pam_amd_surface_fluxes(a["nens"], a["nx"], a["ny"], a["nz"], a["temp"], a["rd"], a["rv"], a["u"], a["v"], a["zmid"], a["cn"],
                                          a["cstar"], a["ts"], a["lwd"], a["lwu"], a["swd"], a["swu"], a["gust"], a["wetness"], a["grav"],
                                          a["cp_d"], a["R_v"], a["latvap"], a["cap"], a["dt"], a["shf"], a["lhf"], None)
    return arrays, P, n, call


def test_entry_point_rejects_bad_arguments_and_leaves_the_arrays_untouched():
    """the pointers are host arrays here: a refusal comes before the first HIP call, so nothing dereferences them, and afterwards every
    array still holds the pattern it was filled with"""
    lib = capi.load()
    arrays, P, n, call = _abi_call(lib)
    level = 4 * 3 * 2
    calls = [dict(nens=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=70000, ny=70000)]
    calls += [{name: None} for name in ("temp", "rd", "rv", "u", "v", "zmid", "cn", "cstar", "ts", "shf", "lhf")]
    calls += [{name: bad} for name in ("gust", "dt", "cap") for bad in (-1.0e-9, math.nan, math.inf, -math.inf)]
    calls += [dict(wetness=bad) for bad in (-1.0e-9, 1.0 + 1.0e-9, math.nan, math.inf)]
    calls += [{name: bad} for name in ("grav", "cp_d", "R_v", "latvap") for bad in (0.0, -1.0, math.nan, math.inf)]
    calls += [dict(lwd=None), dict(lwu=None), dict(swd=None), dict(swu=None), dict(lwd=None, swu=None)]
    # an output that overlaps an input or another output: whole arrays, and one element at either end; sfc_temp counts as both
    calls += [dict(shf=P["lhf"]), dict(shf=P["ts"]), dict(lhf=P["ts"]), dict(shf=P["temp"]), dict(lhf=P["rv"] + 8 * n - 8), dict(ts=P["temp"]),
              dict(ts=P["u"] + 8 * n - 8), dict(ts=P["zmid"] + 8 * 15), dict(ts=P["cn"] + 8 * 3), dict(cstar=P["ts"] + 8 * level - 8),
              dict(lwd=P["ts"]), dict(swu=P["shf"] + 8 * level - 8), dict(lhf=P["swd"] + 8), dict(shf=P["lhf"] + 8 * level - 8), dict(v=P["lhf"])]
    for i, kw in enumerate(calls):
        assert call(**kw) == -1, (i, kw)                           # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert lib.pam_amd_awfl_last_error().startswith(b"surface_fluxes: "), i
        assert all((a == 7.25).all() for a in arrays), i


def test_entry_point_names_itself_when_there_is_no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    lib = capi.load()
    arrays, P, n, call = _abi_call(lib)
    level = 4 * 3 * 2
    for kw in (dict(), dict(lwd=None, lwu=None), dict(swd=None, swu=None), dict(lwd=None, lwu=None, swd=None, swu=None), dict(dt=0.0), dict(cap=0.0),
               dict(gust=0.0), dict(wetness=0.0), dict(wetness=1.0), dict(shf=P["lhf"] + 8 * level), dict(ts=P["cn"] + 8 * 4), dict(nz=1)):
        assert call(**kw) == -2, kw
        assert lib.pam_amd_awfl_last_error() == b"surface_fluxes: no HIP device available (this library has no CPU path)"
        assert all((a == 7.25).all() for a in arrays)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the layers above: the host arithmetic of the init, the C++ module, the driver, the tool, the documents

def _host_coupler(nz=4, ny=2, nx=3, nens=5):
    from pam_amd import PamCoupler
    coupler = PamCoupler("cpu")
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    zint = ((np.arange(nz + 1) / nz) ** 1.5 * 9000.0)[:, None] * (1.0 + 0.05 * np.arange(nens))[None, :]
    coupler.set_grid(1000.0 * nx, 1000.0 * ny, zint)
    return coupler, 0.5 * (zint[0] + zint[1])


def test_init_forms_cn_and_cstar_on_the_host():
    """without a z0 entry: the argument (a float or nens values), else 1e-4 m; with one: the entry, whatever the argument says"""
    from pam_amd import modules
    for z0_arg, want_z0 in ((None, np.full(5, 1.0e-4)), (2.0e-3, np.full(5, 2.0e-3)), (1.0e-4 * (1.0 + np.arange(5)), 1.0e-4 * (1.0 + np.arange(5)))):
        coupler, zmid0 = _host_coupler()
        modules.surface_fluxes_init(coupler, sst=[299.0, 300.0, 301.0, 302.0, 303.0], z0=z0_arg, slab_depth=2.5)
        dm = coupler.get_data_manager_device_readwrite()
        assert ref.same_bits(dm.get("vertical_midpoint_height")[0].numpy(), zmid0)
        cn, cstar = ref.transfer_parameters(zmid0, want_z0)
        assert ref.same_bits(dm.get("sfc_cn").numpy(), cn) and ref.same_bits(dm.get("sfc_cstar").numpy(), cstar)
        lnz = np.log(zmid0 / want_z0)
        assert np.allclose(dm.get("sfc_cn").numpy(), 0.16 / lnz ** 2, rtol=1e-14)
        assert np.allclose(dm.get("sfc_cstar").numpy(), 5.3 * 9.4 * 0.16 / lnz ** 2 * np.sqrt(zmid0 / want_z0), rtol=1e-14)
        assert (dm.get("sfc_temp").numpy() == np.array([299.0, 300.0, 301.0, 302.0, 303.0])).all()
        assert tuple(dm.get("sfc_temp").shape) == (2, 3, 5) == tuple(dm.get("sfc_shf").shape) == tuple(dm.get("sfc_lhf").shape)
        assert (dm.get("sfc_shf").numpy() == 0).all() and (dm.get("sfc_lhf").numpy() == 0).all()
        assert [coupler.get_option(n) for n in ("sfc_slab_depth", "sfc_gust", "sfc_wetness")] == [2.5, 1.0, 0.98]
    coupler, zmid0 = _host_coupler()
    dm = coupler.get_data_manager_device_readwrite()
    dm.register_and_allocate("z0", "Momentum roughness height [m]", (5,), ("nens",))
    z0 = np.array([1.0e-4, 3.0e-4, 1.0e-3, 5.0e-2, 0.1])
    dm.get("z0").copy_(__import__("torch").as_tensor(z0))
    coupler.set_option("sfc_gust", 0.5)
    dm.register_and_allocate("sfc_temp", "surface temperature [K]", (2, 3, 5), ("y", "x", "nens"))
    dm.get("sfc_temp").fill_(288.0)
    modules.surface_fluxes_init(coupler, sst=300.0, z0=7.0)
    cn, cstar = ref.transfer_parameters(zmid0, z0)
    assert ref.same_bits(dm.get("sfc_cn").numpy(), cn) and ref.same_bits(dm.get("sfc_cstar").numpy(), cstar)
    assert (dm.get("sfc_temp").numpy() == 288.0).all()                                  # an existing entry keeps its values
    assert [coupler.get_option(n) for n in ("sfc_slab_depth", "sfc_gust", "sfc_wetness")] == [0.0, 0.5, 0.98]
    modules.surface_fluxes_init(coupler, sst=310.0, slab_depth=9.0, gust=3.0, wetness=0.5)    # a second init overwrites neither
    assert (dm.get("sfc_temp").numpy() == 288.0).all()
    assert [coupler.get_option(n) for n in ("sfc_slab_depth", "sfc_gust", "sfc_wetness")] == [0.0, 0.5, 0.98]


def test_python_and_sgs_name_the_flux_entries_alike():
    from pam_amd import modules, physics
    assert modules.SURFACE_FLUX_FIELDS == physics.SGSSmagorinsky.FLUX_FIELDS
    assert modules.SURFACE_LATVAP == physics.SGSSmagorinsky.LATVAP
    assert modules.SURFACE_RHO_W * modules.SURFACE_C_W == ref.RHO_W * ref.C_W == 4186000.0


def test_cxx_module_compiles(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "modules/surface_fluxes.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  modules::surface_fluxes_init(coupler, 300.0, 1.0);\n"
                   "  modules::compute_surface_fluxes(coupler);\n  modules::compute_surface_fluxes(coupler, 5.0);\n  return 0;\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cxx_module_and_python_functions_name_the_same_entries_and_options():
    import inspect
    from pam_amd import modules
    text = open(os.path.join(HOST, "modules", "surface_fluxes.h")).read()
    py = inspect.getsource(modules)
    for s in ('"sfc_temp"', '"sfc_cn"', '"sfc_cstar"', '"sfc_slab_depth"', '"sfc_gust"', '"sfc_wetness"', '"z0"', '"vertical_midpoint_height"',
              '"rad_lw_down_sfc"', '"rad_lw_up_sfc"', '"rad_sw_down_sfc"', '"rad_sw_up_sfc"', "pam_amd_surface_fluxes(", "1000.0", "4186.0",
              "input surface sensible heat flux [W/m2]", "input surface latent heat flux [W/m2]"):
        assert s in text and s in py, s


def test_driver_bench_tool_and_documents_know_the_surface():
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert drv.count('"--surface"') == 1 and drv.count("[--surface SST [DEPTH]]") >= 2 and "surface: etime" in drv
    assert drv.index("modules::sponge_layer);") < drv.index("modules::compute_surface_fluxes(c)") < drv.index('"surface_friction", modules::compute_surface_friction')
    tool = open(os.path.join(ROOT, "tools", "bench_modules.py")).read()
    assert '"surface"' in tool and "pam_amd_surface_fluxes" in tool
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "surface_fluxes" in open(os.path.join(ROOT, doc)).read(), doc
    deps = native_build.dependencies(native_build.LIB_SOURCES)
    assert os.path.join(native_build.CSRC, "surface_device.h") in deps and os.path.join(HOST, "modules", "surface_fluxes.h") in deps
