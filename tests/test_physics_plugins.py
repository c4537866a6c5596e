"""The forced radiation plug-in, the "none" plug-ins and PamCoupler::compute_pressure_array (physics/radiation/forced/radiation.h,
physics/{radiation,sgs,micro}/none, pam_core/pam_coupler.h:360-393): the CPU restatement (tests/plugins_ref.py) against hand-computed
values and against the reference's own outputs (tests/golden/plugins_ref.npz), the host emulation of the device bodies
(pam_amd/csrc/plugins_device.h under g++) against the restatement bit for bit, the C ABI's argument checks, the plug-in headers'
boundary, and on the GPU the HIP path against the restatement bit for bit, the Python classes, a CRM loop with radiative forcing and
the driver's --radiation."""
import copy
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import plugins_ref as ref
import test_boundary_surface as tb
from pam_amd import capi
from tools.native_build import emu_library, syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plugins_ref.npz")
EXTRACT = os.path.join(ROOT, "tests", "golden", "plugins_extract.json")
DRIVER = os.path.join(ROOT, "examples", "driver")
CI_YAML = os.path.join(ROOT, "tests", "golden", "ci_input_pama.yaml")
REFERENCE = os.environ.get("PAM_REF", os.path.join(os.path.dirname(ROOT), "reference"))
_DP = C.POINTER(C.c_double)

NENS = [1, 3, 64, 65, 130]
GRIDS = [(32, 32), (1, 65), (6, 1)]            # (ny, nx)
GRID_IDS = ["32x32", "1x65", "6x1"]
NZ = 3
CP_D, CRM_DT, R_D, R_V = 1003.0, 20.0, 287.0, 461.0


def rad_grids(ny, nx):
    """every divisor pair of the grid, as (rad_ny, rad_nx)"""
    return [(ry, rx) for ry in ref.divisors(ny) for rx in ref.divisors(nx)]


def temperature(shape, seed):
    return np.random.default_rng(seed).uniform(190.0, 310.0, shape)


def tendency(shape, seed):
    """both signs over five decades, with subnormals, signed zeros, an infinity and NaNs among them"""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(shape) * 10.0 ** rng.uniform(-4, 1, shape)
    flat = q.reshape(-1)
    special = [4.9e-324, -4.9e-324, 2.0e-310, 0.0, -0.0, np.nan, np.inf, -np.nan]
    for n, v in enumerate(special):
        flat[(7 * n + 1) % flat.size] = v
    return q


def densities(shape, seed):
    rng = np.random.default_rng(seed)
    rho_v = rng.uniform(0.0, 0.02, shape)
    rho_v.reshape(-1)[::11] = 0.0
    rho_v.reshape(-1)[5 % rho_v.size] = np.nan
    return rng.uniform(0.05, 1.3, shape), rho_v


def same_bits(a, b):
    """NaN in the same places, every other element equal bit for bit (the signs of zeros included).  IEEE 754 leaves the sign and the
    payload of a NaN result to the implementation, so those are not compared"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(np.where(np.isnan(a), 0.0, a).view(np.uint64), np.where(np.isnan(b), 0.0, b).view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement

def test_restatement_radiation_by_hand():
    """nz 1, ny 2, nx 4, nens 2 on a 1 x 2 rad grid (fy 2, fx 2): T + q / cp_d * dt with values whose roundings are exact"""
    temp = np.arange(16, dtype=np.float64).reshape(1, 2, 4, 2) + 200.0
    tend = np.array([1.0, 2.0, 4.0, 8.0]).reshape(1, 1, 2, 2) * 0.5          # rad cell (0, ir), member e: 0.5 * 2^(2 ir + e)
    got = ref.radiation_forced(temp, tend, cp_d=0.25, dt=0.125)               # q / 0.25 * 0.125 = q / 2, exact
    for j in range(2):
        for i in range(4):
            for e in range(2):
                assert got[0, j, i, e] == temp[0, j, i, e] + 0.25 * 2.0 ** (2 * (i // 2) + e), (j, i, e)
    # the order: fl(fl(q / cp_d) * dt), not q * fl(dt / cp_d) and not fl(q * dt) / cp_d
    q, cp, dt, T = 0.1, 1003.0, 20.0, 250.0
    one = ref.radiation_forced(np.full((1, 1, 1, 1), T), np.full((1, 1, 1, 1), q), cp, dt)[0, 0, 0, 0]
    assert one == T + (q / cp) * dt
    qs = np.random.default_rng(0).standard_normal(4000)
    a = ref.radiation_forced(np.zeros((1, 1, 4000, 1)), qs.reshape(1, 1, 4000, 1), cp, dt).reshape(-1)
    assert np.array_equal(a, (qs / cp) * dt) and not np.array_equal(a, qs * (dt / cp)) and not np.array_equal(a, (qs * dt) / cp)


def test_restatement_radiation_every_rad_cell_distinct():
    """fx = 3, fy = 2 and a distinct value per (k, rad cell, member): a swapped or off-by-one rad index shows"""
    nz, ny, nx, nens, rad_ny, rad_nx = 2, 4, 6, 3, 2, 2
    tend = (1.0 + np.arange(nz * rad_ny * rad_nx * nens, dtype=np.float64)).reshape(nz, rad_ny, rad_nx, nens)
    got = ref.radiation_forced(np.zeros((nz, ny, nx, nens)), tend, cp_d=1.0, dt=1.0)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for e in range(nens):
                    assert got[k, j, i, e] == tend[k, j // 2, i // 3, e], (k, j, i, e)
    assert len(np.unique(got)) == tend.size
    # the scalar transcription of radiation.h:40-44 on random data
    temp, q = temperature((nz, ny, nx, nens), 1), tendency((nz, rad_ny, rad_nx, nens), 2)
    want = temp.copy()
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    for e in range(nens):
                        want[k, j, i, e] += np.float64(q[k, j // (ny // rad_ny), i // (nx // rad_nx), e]) / np.float64(CP_D) * np.float64(CRM_DT)
    assert same_bits(ref.radiation_forced(temp, q, CP_D, CRM_DT), want)


def test_restatement_refuses_what_the_reference_cannot_index():
    for nx, ny, rx, ry in ((5, 1, 2, 1), (4, 4, 8, 1), (4, 4, 0, 1), (4, 6, 2, 4), (4, 4, 2, -1)):
        with pytest.raises(ValueError):
            ref.rad_grid_check(nx, ny, rx, ry)
    assert list(ref.rad_indices(6, 2)) == [0, 0, 0, 1, 1, 1] and list(ref.rad_indices(65, 5)) == [i // 13 for i in range(65)]


def test_restatement_pressure_by_hand():
    got = ref.compute_pressure(np.array([1.0, 0.5]), np.array([0.0, 0.25]), np.array([300.0, 256.0]), 287.0, 461.0)
    assert got[0] == 287.0 * 300.0 and got[1] == 0.5 * 287.0 * 256.0 + 0.25 * 461.0 * 256.0
    # left to right: (rho_d R_d) T + (rho_v R_v) T, not (rho_d R_d + rho_v R_v) T
    rho_d, rho_v = densities(5000, 3)
    T = temperature(5000, 4)
    a = ref.compute_pressure(rho_d, rho_v, T, R_D, R_V)
    with np.errstate(all="ignore"):
        assert same_bits(a, rho_d * R_D * T + rho_v * R_V * T) and not same_bits(a, (rho_d * R_D + rho_v * R_V) * T)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the pin to the reference's own text

def test_restatement_equals_the_reference_outputs_bit_for_bit():
    g = np.load(GOLDEN)
    cp_d, crm_dt, R_d, R_v, calls = g["params"]
    grids = [k[len("tend_"):] for k in g.files if k.startswith("tend_")]
    assert sorted(grids) == ["1x1", "3x2", "6x4"]
    for grid in grids:
        t = g["temp"]
        for _ in range(int(calls)):
            t = ref.radiation_forced(t, g["tend_" + grid], cp_d, crm_dt)
        assert same_bits(t, g["temp_out_" + grid]), grid
        assert np.isnan(g["temp_out_" + grid]).any() and not np.isnan(g["temp_out_" + grid]).all()
    assert same_bits(ref.compute_pressure(g["rho_d"], g["rho_v"], g["temp"], R_d, R_v), g["pressure"])


def test_micro_none_constants_and_tracer_are_the_reference_init():
    from pam_amd.physics import MicrophysicsNone as M
    g = np.load(GOLDEN)
    assert list(g["micro_none_consts"]) == [M.R_d, M.R_v, M.cp_d, M.cp_v, M.grav, M.p0]
    assert list(g["micro_none_info"]) == [M.get_num_tracers(), 1, 1, 1]
    assert bytes(g["micro_none_name"]).rstrip(b"\0").decode() == M.micro_name()
    assert not g["micro_none_water_vapor"].any() and not np.isnan(g["micro_none_water_vapor"]).any()
    text = tb._strip_comments(open(os.path.join(HOST, "physics", "micro", "none", "Microphysics.h")).read())
    for k, v in zip(("R_d", "R_v", "cp_d", "cp_v", "grav", "p0"), g["micro_none_consts"]):
        m = [float(x) for x in __import__("re").findall(r"\b%s\s*=\s*([0-9.e+]+)\s*[,;]" % k, text)]
        assert m == [v], (k, m, v)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "physics", "radiation", "forced")), reason="no reference tree at hand")
def test_the_fixture_is_reproduced_from_the_reference_tree():
    r = subprocess.run([os.sys.executable, os.path.join(ROOT, "tests", "golden", "make_ref_plugins_golden.py"), REFERENCE, "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the host emulation of the device bodies

def emu():
    lib = C.CDLL(emu_library("plugins_emu"))
    lib.emu_radiation_forced.argtypes = [C.c_int] * 6 + [_DP, _DP, C.c_double, C.c_double]
    lib.emu_compute_pressure.argtypes = [C.c_longlong] + [_DP] * 3 + [C.c_double, C.c_double, _DP]
    return lib


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


@pytest.mark.parametrize("nens", NENS)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_emulation_radiation_matches_restatement_bit_for_bit(grid, nens):
    ny, nx = grid
    lib = emu()
    temp = temperature((NZ, ny, nx, nens), seed=nens)
    for n, (rad_ny, rad_nx) in enumerate(rad_grids(ny, nx)):
        q = tendency((NZ, rad_ny, rad_nx, nens), seed=100 * nens + n)
        got = temp.copy()
        lib.emu_radiation_forced(nens, nx, ny, NZ, rad_nx, rad_ny, _p(got), _p(q), CP_D, CRM_DT)
        want = ref.radiation_forced(temp, q, CP_D, CRM_DT)
        assert same_bits(got, want), (rad_ny, rad_nx)
        assert np.isnan(want).sum() == np.isnan(q[:, ref.rad_indices(ny, rad_ny)][:, :, ref.rad_indices(nx, rad_nx)]).sum() > 0   # NaN passes through


@pytest.mark.parametrize("nens", NENS)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_emulation_pressure_matches_restatement_bit_for_bit(grid, nens):
    ny, nx = grid
    lib = emu()
    shape = (NZ, ny, nx, nens)
    rho_d, rho_v = densities(shape, seed=nens + 7)
    T = temperature(shape, seed=nens + 8)
    got = np.empty(shape)
    lib.emu_compute_pressure(got.size, _p(rho_d), _p(rho_v), _p(T), R_D, R_V, _p(got))
    assert same_bits(got, ref.compute_pressure(rho_d, rho_v, T, R_D, R_V))


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the C ABI

NEW_SYMBOLS = ("pam_amd_radiation_forced", "pam_amd_compute_pressure")


def test_new_entry_points_are_exported_and_declared():
    import re
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    assert lib.pam_amd_awfl_abi_version() == 5


def test_new_entry_points_reject_bad_arguments_before_touching_a_device():
    lib = capi.load()
    rad, pres = lib.pam_amd_radiation_forced, lib.pam_amd_compute_pressure
    nan, inf = float("nan"), float("inf")
    T, Q = 1 << 20, 1 << 30            # never dereferenced: validation fails first.  4 x 6 x 4 x 3 cells = 2304 B of temp at T
    A, B, Cc, P = 1 << 20, 1 << 21, 1 << 22, 1 << 23
    n = 3 * 4 * 6 * 4 * 8
    cases = [
        ("radiation", lambda: rad(0, 4, 6, 3, 2, 3, T, Q, CP_D, CRM_DT, None)),
        ("radiation", lambda: rad(4, 0, 6, 3, 2, 3, T, Q, CP_D, CRM_DT, None)),
        ("radiation", lambda: rad(4, 4, -1, 3, 2, 3, T, Q, CP_D, CRM_DT, None)),
        ("radiation", lambda: rad(4, 4, 6, 0, 2, 3, T, Q, CP_D, CRM_DT, None)),
        ("radiation", lambda: rad(4, 4, 6, 3, 0, 3, T, Q, CP_D, CRM_DT, None)),      # rad_nx < 1
        ("radiation", lambda: rad(4, 4, 6, 3, 2, -3, T, Q, CP_D, CRM_DT, None)),
        ("radiation", lambda: rad(4, 4, 6, 3, 8, 3, T, Q, CP_D, CRM_DT, None)),      # rad_nx > nx: the reference divides by zero
        ("radiation", lambda: rad(4, 5, 6, 3, 2, 3, T, Q, CP_D, CRM_DT, None)),      # nx = 5, rad_nx = 2: the reference reads i_rad = 2
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 4, T, Q, CP_D, CRM_DT, None)),      # a remainder in y
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, None, Q, CP_D, CRM_DT, None)),
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, T, None, CP_D, CRM_DT, None)),
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, T, Q, 0.0, CRM_DT, None)),
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, T, Q, -CP_D, CRM_DT, None)),
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, T, Q, nan, CRM_DT, None)),
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, T, Q, inf, CRM_DT, None)),
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, T, Q, CP_D, nan, None)),
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, T, Q, CP_D, -inf, None)),
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, T, T, CP_D, CRM_DT, None)),              # the tendency is temp
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, T, T + n - 8, CP_D, CRM_DT, None)),      # starts at temp's last element
        ("radiation", lambda: rad(4, 4, 6, 3, 2, 3, T, T - 8, CP_D, CRM_DT, None)),          # ends inside temp
        ("compute_pressure_array", lambda: pres(0, 4, 6, 3, A, B, Cc, R_D, R_V, P, None)),
        ("compute_pressure_array", lambda: pres(4, 4, 6, -3, A, B, Cc, R_D, R_V, P, None)),
        ("compute_pressure_array", lambda: pres(4, 4, 6, 3, None, B, Cc, R_D, R_V, P, None)),
        ("compute_pressure_array", lambda: pres(4, 4, 6, 3, A, None, Cc, R_D, R_V, P, None)),
        ("compute_pressure_array", lambda: pres(4, 4, 6, 3, A, B, None, R_D, R_V, P, None)),
        ("compute_pressure_array", lambda: pres(4, 4, 6, 3, A, B, Cc, R_D, R_V, None, None)),
        ("compute_pressure_array", lambda: pres(4, 4, 6, 3, A, B, Cc, nan, R_V, P, None)),
        ("compute_pressure_array", lambda: pres(4, 4, 6, 3, A, B, Cc, R_D, inf, P, None)),
        ("compute_pressure_array", lambda: pres(4, 4, 6, 3, A, B, Cc, R_D, R_V, A, None)),
        ("compute_pressure_array", lambda: pres(4, 4, 6, 3, A, B, Cc, R_D, R_V, B + 8, None)),
        ("compute_pressure_array", lambda: pres(4, 4, 6, 3, A, B, Cc, R_D, R_V, Cc - n + 8, None)),
    ]
    for who, call in cases:
        assert call() == -1, who                                   # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert who.encode() in lib.pam_amd_awfl_last_error(), (who, lib.pam_amd_awfl_last_error())


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the boundary of the C++ plug-in classes

PHYSICS = os.path.join(HOST, "physics")
PLUGINS = {"forced": os.path.join(PHYSICS, "radiation", "forced_amd", "radiation.h"),
           "rad_none": os.path.join(PHYSICS, "radiation", "none", "radiation.h"),
           "sgs_none": os.path.join(PHYSICS, "sgs", "none", "SGS.h"),
           "micro_none": os.path.join(PHYSICS, "micro", "none", "Microphysics.h")}
# header -> signature -> the reference line it must match (tests/golden/make_ref_plugins_golden.py records the digests)
SIGNATURES = {
    "forced": {"std::string radiation_name() const": "physics/radiation/forced/radiation.h:12",
               "void init(pam::PamCoupler &coupler)": "physics/radiation/forced/radiation.h:16",
               "void timeStep( pam::PamCoupler &coupler )": "physics/radiation/forced/radiation.h:26",
               "void finalize(pam::PamCoupler &coupler)": "physics/radiation/forced/radiation.h:47"},
    "rad_none": {"std::string radiation_name() const": "physics/radiation/none/radiation.h:11",
                 "void init(pam::PamCoupler &coupler)": "physics/radiation/none/radiation.h:16",
                 "void timeStep( pam::PamCoupler &coupler )": "physics/radiation/none/radiation.h:20",
                 "void finalize(pam::PamCoupler &coupler)": "physics/radiation/none/radiation.h:23"},
    "sgs_none": {"static int constexpr get_num_tracers()": "physics/sgs/none/SGS.h:15",
                 "void init(pam::PamCoupler &coupler)": "physics/sgs/none/SGS.h:20",
                 "void timeStep( pam::PamCoupler &coupler )": "physics/sgs/none/SGS.h:26",
                 "std::string sgs_name() const": "physics/sgs/none/SGS.h:31",
                 "void finalize(pam::PamCoupler &coupler)": "physics/sgs/none/SGS.h:36"},
    "micro_none": {"static int constexpr get_num_tracers()": "physics/micro/none/Microphysics.h:39",
                   "void init(pam::PamCoupler &coupler)": "physics/micro/none/Microphysics.h:51",
                   "void timeStep( pam::PamCoupler &coupler )": "physics/micro/none/Microphysics.h:81",
                   "std::string micro_name() const": "physics/micro/none/Microphysics.h:87",
                   "void finalize(pam::PamCoupler &coupler)": "physics/micro/none/Microphysics.h:91"},
    "coupler": {"real4d compute_pressure_array() const": "pam_core/pam_coupler.h:360"},
}


@pytest.mark.parametrize("which", sorted(PLUGINS))
def test_plugin_headers_call_only_members_the_reference_has(which):
    coupler, dm = tb._used_members(open(PLUGINS[which]).read())
    assert coupler, "scan found no coupler calls"
    allowed = tb.REF_COUPLER | {"compute_pressure_array"}
    assert "compute_pressure_array" in json.load(open(tb.GOLDEN))["boundary_surface"]["pam_coupler_h_names"]
    assert coupler <= allowed, sorted(coupler - allowed)
    assert dm <= tb.REF_DM, sorted(dm - tb.REF_DM)
    ours = tb._declared(os.path.join(HOST, "pam_coupler.h"))
    assert (coupler | dm) <= ours, sorted((coupler | dm) - ours)


def test_the_listed_host_sources_do_not_call_compute_pressure_array():
    """tests/test_boundary_surface.py's member list predates it: the driver and the sources scanned there stay within that list"""
    for src in tb.SOURCES:
        assert "compute_pressure_array" not in tb._strip_comments(open(src).read()), src


def test_plugin_headers_have_the_reference_signatures():
    rec = json.load(open(EXTRACT))["signature_sha256"]
    assert sorted(rec) == sorted(w for sigs in SIGNATURES.values() for w in sigs.values())
    for which, sigs in SIGNATURES.items():
        path = os.path.join(HOST, "pam_coupler.h") if which == "coupler" else PLUGINS[which]
        text = tb._norm(tb._strip_comments(open(path).read()))
        for sig, where in sigs.items():
            assert tb._digest(tb._norm(sig)) == rec[where], (sig, where)
            assert tb._norm(sig) + "{" in text, (which, sig)


@pytest.mark.parametrize("rad", ["none", "forced_amd"])
def test_plugin_headers_compile_together_with_the_workalike(tmp_path, rad):
    """what a PAM driver does: one translation unit with a Microphysics, an SGS and a Radiation class (and the work-alike coupler)"""
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "physics/micro/none/Microphysics.h"\n#include "physics/sgs/none/SGS.h"\n'
                   '#include "physics/radiation/%s/radiation.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  Microphysics micro;\n  SGS sgs;\n  Radiation rad;\n"
                   "  micro.init(coupler);\n  sgs.init(coupler);\n  rad.init(coupler);\n"
                   '  coupler.run_module("radiation", [&](pam::PamCoupler &c) { rad.timeStep(c); });\n'
                   "  micro.timeStep(coupler);\n  sgs.timeStep(coupler);\n"
                   "  real4d p = coupler.compute_pressure_array();\n"
                   "  static_assert(Microphysics::get_num_tracers() == 1 && SGS::get_num_tracers() == 0, \"\");\n"
                   "  static_assert(Microphysics::get_num_diffused_tracers() == 1, \"\");\n"
                   "  micro.finalize(coupler);\n  sgs.finalize(coupler);\n  rad.finalize(coupler);\n"
                   "  return (int)p.size() + (int)(micro.micro_name() + sgs.sgs_name() + rad.radiation_name()).size();\n}\n" % rad)
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------------------------------------
# GPU

def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def gpu_radiation(temp, tend, cp_d=CP_D, dt=CRM_DT, calls=1):
    import torch
    nz, ny, nx, nens = temp.shape
    rad_ny, rad_nx = tend.shape[1:3]
    t = torch.from_numpy(np.ascontiguousarray(temp)).cuda()
    q = torch.from_numpy(np.ascontiguousarray(tend)).cuda()
    for _ in range(calls):
        capi.check(capi.load().pam_amd_radiation_forced(nens, nx, ny, nz, rad_nx, rad_ny, t.data_ptr(), q.data_ptr(), cp_d, dt, _stream()))
    torch.cuda.synchronize()
    return t.cpu().numpy()


def gpu_pressure(rho_d, rho_v, temp, R_d=R_D, R_v=R_V):
    import torch
    nz, ny, nx, nens = temp.shape
    a, b, c = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (rho_d, rho_v, temp))
    p = torch.full(temp.shape, -7.0, dtype=torch.float64, device="cuda")
    capi.check(capi.load().pam_amd_compute_pressure(nens, nx, ny, nz, a.data_ptr(), b.data_ptr(), c.data_ptr(), R_d, R_v, p.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return p.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("nens", NENS)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_gpu_radiation_matches_restatement_bit_for_bit(grid, nens):
    """every divisor pair of the grid as the rad grid, radiation applied three times in a row"""
    ny, nx = grid
    temp = temperature((NZ, ny, nx, nens), seed=nens)
    for n, (rad_ny, rad_nx) in enumerate(rad_grids(ny, nx)):
        q = tendency((NZ, rad_ny, rad_nx, nens), seed=100 * nens + n)
        want = temp
        for _ in range(3):
            want = ref.radiation_forced(want, q, CP_D, CRM_DT)
        assert same_bits(gpu_radiation(temp, q, calls=3), want), (rad_ny, rad_nx)


@pytest.mark.gpu
@pytest.mark.parametrize("nens", NENS)
@pytest.mark.parametrize("grid", GRIDS + [(7, 9)], ids=GRID_IDS + ["7x9_nz37"])
def test_gpu_pressure_matches_restatement_bit_for_bit(grid, nens):
    ny, nx = grid
    shape = (37 if grid == (7, 9) else NZ, ny, nx, nens)
    rho_d, rho_v = densities(shape, seed=nens + 7)
    T = temperature(shape, seed=nens + 8)
    assert same_bits(gpu_pressure(rho_d, rho_v, T), ref.compute_pressure(rho_d, rho_v, T, R_D, R_V))


@pytest.mark.gpu
def test_gpu_reference_fixture_through_the_device():
    g = np.load(GOLDEN)
    cp_d, crm_dt, R_d, R_v, calls = g["params"]
    for grid in ("1x1", "3x2", "6x4"):
        assert same_bits(gpu_radiation(g["temp"], g["tend_" + grid], cp_d, crm_dt, int(calls)), g["temp_out_" + grid]), grid
    assert same_bits(gpu_pressure(g["rho_d"], g["rho_v"], g["temp"], R_d, R_v), g["pressure"])


def _coupler(nens, nz, ny, nx, crm_dt=CRM_DT, micro=True):
    from pam_amd import MicrophysicsNone, PamCoupler
    c = PamCoupler("cuda:0")
    if crm_dt is not None:
        c.set_option("crm_dt", crm_dt)
    c.allocate_coupler_state(nz, ny, nx, nens)
    if micro:
        MicrophysicsNone().init(c)
    return c


def _put(c, name, arr):
    import torch
    c.get_data_manager_device_readwrite().get(name).copy_(torch.from_numpy(np.ascontiguousarray(arr)))


def _get(c, name):
    import torch
    torch.cuda.synchronize()
    return c.get_data_manager_device_readwrite().get(name, readonly=True).cpu().numpy()


@pytest.mark.gpu
def test_gpu_members_split_over_two_couplers_give_the_whole_bits():
    from pam_amd import Radiation
    n1, n2, nz, ny, nx, rad_ny, rad_nx = 37, 93, 5, 6, 8, 3, 2
    shape = (nz, ny, nx, n1 + n2)
    temp, q = temperature(shape, 1), tendency((nz, rad_ny, rad_nx, n1 + n2), 2)
    rho_d, rho_v = densities(shape, 3)

    def run(sl, nens):
        c = _coupler(nens, nz, ny, nx)
        c.set_option("rad_nx", rad_nx)
        c.set_option("rad_ny", rad_ny)
        rad = Radiation()
        rad.init(c)
        for name, v in (("temp", temp), ("rad_enthalpy_tend", q), ("density_dry", rho_d), ("water_vapor", rho_v)):
            _put(c, name, v[..., sl])
        c.run_module("radiation", rad.timeStep)
        c.run_module("radiation", rad.timeStep)
        p = c.compute_pressure_array()
        return _get(c, "temp"), p.cpu().numpy()

    whole = run(slice(None), n1 + n2)
    first, second = run(slice(0, n1), n1), run(slice(n1, None), n2)
    want_t = ref.radiation_forced(ref.radiation_forced(temp, q, 1003.0, CRM_DT), q, 1003.0, CRM_DT)
    assert same_bits(whole[0], want_t) and same_bits(whole[1], ref.compute_pressure(rho_d, rho_v, want_t, 287.0, 461.0))
    for k in range(2):
        assert same_bits(np.concatenate([first[k], second[k]], axis=-1), whole[k]), k


@pytest.mark.gpu
def test_gpu_python_classes_register_and_behave_as_the_reference():
    import torch
    from pam_amd import Dycore, MicrophysicsNone, Radiation, RadiationNone, SGSNone
    nens, nz, ny, nx = 5, 6, 4, 6
    c = _coupler(nens, nz, ny, nx, micro=False)
    dm = c.get_data_manager_device_readwrite()
    c.set_grid(nx * 500.0, ny * 500.0, np.linspace(0.0, 6000.0, nz + 1))
    micro, sgs, none = MicrophysicsNone(), SGSNone(), RadiationNone()
    # MicrophysicsNone: one zeroed tracer (positive, adds mass), the constants, the option
    dm.register_and_allocate("scratch_like_water_vapor", "", (nz, ny, nx, nens)).fill_(3.5)
    micro.init(c)
    assert c.get_tracer_names() == ["water_vapor"] and c.get_tracer_info("water_vapor") == ("Water Vapor", True, True, True)
    wv = _get(c, "water_vapor")
    assert wv.shape == (nz, ny, nx, nens) and not wv.any() and not np.signbit(wv).any()
    assert c.get_option("micro") == "none" == micro.micro_name() and micro.get_num_tracers() == 1
    assert [c.get_option(k) for k in ("R_d", "R_v", "cp_d", "cp_v", "grav", "p0")] == [287.0, 461.0, 1003.0, 1859.0, 9.81, 1.0e5]
    dm.get("water_vapor").fill_(2.0)
    with pytest.raises(capi.PamAmdError, match="Duplicate entry"):
        micro.init(c)
    assert c.get_tracer_names() == ["water_vapor"] and (_get(c, "water_vapor") == 2.0).all()
    dm.get("water_vapor").zero_()
    sgs.init(c)
    none.init(c)
    assert c.get_option("sgs") == "none" == sgs.sgs_name() and sgs.get_num_tracers() == 0
    assert c.get_option("radiation") == "none" == none.radiation_name()
    before = {n: _get(c, n).copy() for n in ("temp", "water_vapor", "density_dry")}
    for plug in (micro, sgs, none):
        assert c.run_module("x", plug.timeStep) == []                 # nothing obtained for writing
        plug.finalize(c)
    assert all(same_bits(_get(c, n), v) for n, v in before.items())
    # the dycore after it sees one tracer
    d = Dycore()
    d.init(c)
    assert dm.get_shape("tracer_adds_mass") == [1] and dm.get_shape("tracer_positive") == [1] and c.get_option("idWV") == 0   # NT = 1
    d.finalize(c)
    # Radiation: the entry, its dimensions, the option
    rad = Radiation()
    c.set_option("rad_nx", 3)
    c.set_option("rad_ny", 2)
    rad.init(c)
    assert c.get_option("radiation") == "forced" == rad.radiation_name()
    assert dm.get_shape("rad_enthalpy_tend") == [nz, 2, 3, nens] and not _get(c, "rad_enthalpy_tend").any()
    assert dm.get_dimension_size("rad_x") == 3 and dm.get_dimension_size("rad_y") == 2
    temp, q = temperature((nz, ny, nx, nens), 5), tendency((nz, 2, 3, nens), 6)
    _put(c, "temp", temp)
    _put(c, "rad_enthalpy_tend", q)
    assert c.run_module("radiation", rad.timeStep) == ["temp"]
    assert same_bits(_get(c, "temp"), ref.radiation_forced(temp, q, 1003.0, CRM_DT))
    with pytest.raises(capi.PamAmdError, match="Duplicate entry"):
        rad.init(c)
    assert same_bits(_get(c, "rad_enthalpy_tend"), q)
    # the pressure array: the coupler's storage, reused
    _put(c, "density_dry", densities((nz, ny, nx, nens), 7)[0])
    _put(c, "water_vapor", np.abs(densities((nz, ny, nx, nens), 8)[1]))
    p1 = c.compute_pressure_array()
    want = ref.compute_pressure(_get(c, "density_dry"), _get(c, "water_vapor"), _get(c, "temp"), 287.0, 461.0)
    torch.cuda.synchronize()
    assert same_bits(p1.cpu().numpy(), want)
    c.get_data_manager_device_readwrite().clean_all_entries()
    assert c.compute_pressure_array().data_ptr() == p1.data_ptr() and dm.get_dirty_entries() == []     # reads only
    rad.finalize(c)


@pytest.mark.gpu
def test_gpu_every_deviation_raises_and_changes_nothing():
    from pam_amd import Radiation
    nens, nz, ny, nx = 3, 4, 6, 5
    temp = temperature((nz, ny, nx, nens), 9)

    def fresh(**opts):
        c = _coupler(nens, nz, ny, nx, crm_dt=opts.pop("crm_dt", CRM_DT))
        for k, v in dict(dict(rad_nx=5, rad_ny=3), **opts).items():
            if v is not None:
                c.set_option(k, v)
        _put(c, "temp", temp)
        return c

    # init: missing or bad rad grid, disagreeing size options -> nothing registered, no option set
    for opts, msg in ((dict(rad_nx=None), "rad_nx"), (dict(rad_ny=None), "rad_ny"), (dict(rad_nx=2), "divide"), (dict(rad_nx=10), "divide"),
                      (dict(rad_ny=4), "divide"), (dict(rad_nx=0), "divide"), (dict(rad_ny=-1), "divide"), (dict(ncrms=nens + 1), "ncrms"),
                      (dict(crm_nz=nz - 1), "crm_nz"), (dict(crm_nx=nx + 1), "crm_nx"), (dict(crm_ny=1), "crm_ny")):
        c = fresh(**opts)
        with pytest.raises(capi.PamAmdError, match=msg):
            Radiation().init(c)
        assert not c.get_data_manager_device_readwrite().entry_exists("rad_enthalpy_tend") and not c.option_exists("radiation"), opts
    # agreeing size options are fine
    c = fresh(ncrms=nens, crm_nz=nz, crm_nx=nx, crm_ny=ny)
    rad = Radiation()
    rad.init(c)
    q = tendency((nz, 3, 5, nens), 10)
    _put(c, "rad_enthalpy_tend", q)
    # timeStep: each bad option leaves temp's bits
    for key, bad, msg in (("crm_dt", None, "crm_dt"), ("crm_dt", float("nan"), "crm_dt"), ("crm_dt", float("inf"), "crm_dt"),
                          ("cp_d", None, "cp_d"), ("cp_d", 0.0, "cp_d"), ("cp_d", -1003.0, "cp_d"), ("cp_d", float("nan"), "cp_d"),
                          ("cp_d", float("inf"), "cp_d"), ("rad_nx", None, "rad_nx"), ("rad_ny", None, "rad_ny"), ("rad_nx", 1, "rad_enthalpy_tend"),
                          ("rad_ny", 6, "rad_enthalpy_tend"), ("rad_nx", 2, "divide"), ("crm_nx", nx + 5, "crm_nx")):
        old = c.get_option(key) if c.option_exists(key) else None
        if bad is None:
            c.options.delete_option(key)
        else:
            c.set_option(key, bad)
        with pytest.raises(capi.PamAmdError, match=msg):
            rad.timeStep(c)
        assert same_bits(_get(c, "temp"), temp), (key, bad)
        if old is None:
            c.options.delete_option(key)
        else:
            c.set_option(key, old)
    rad.timeStep(c)
    assert same_bits(_get(c, "temp"), ref.radiation_forced(temp, q, 1003.0, CRM_DT))
    # the pressure array without its constants or its tracer
    c2 = _coupler(nens, nz, ny, nx, micro=False)
    with pytest.raises(capi.PamAmdError, match="water_vapor"):
        c2.compute_pressure_array()
    c.options.delete_option("R_v")
    with pytest.raises(capi.PamAmdError, match="R_v"):
        c.compute_pressure_array()


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: a CRM step with radiative forcing

@pytest.mark.gpu
def test_gpu_crm_step_radiation_dycore_sponge_kessler():
    """one CRM step radiation -> dycore -> sponge_layer -> Kessler on a small 3-D case, the Python classes against the restatement
    (radiation) followed by the oracle (dycore, sponge layer, Kessler), at the case's own noise floor (tests/parity_gate.py)"""
    import torch
    from oracle import awfl_oracle as ao
    from pam_amd import Dycore, Microphysics, PamCoupler, Radiation, idealized as idz, modules
    from parity_gate import compare, noise_floor
    nens, nx, ny, nz, crm_dt, rad_nx, rad_ny = 4, 8, 6, 16, 4.0, 4, 2
    tr = (("water_vapor", True, True), ("cloud_liquid", True, True), ("precip_liquid", True, True))
    names, pos, mass, idwv = idz.tracer_flags(tr)
    consts = dict(R_d=287.0, cp_d=1003.0, R_v=461.0, cp_v=1859.0, p0=1.0e5, grav=9.81)
    zint = idz.stretched_interfaces(nz, 15000.0)
    zi = np.ascontiguousarray(np.broadcast_to(zint[:, None], (nz + 1, nens)))
    zm = 0.5 * (zi[:-1] + zi[1:])
    xlen, ylen = nx * 500.0, ny * 500.0
    f = idz.supercell_fields(nens, nx, ny, nz, zint, tracers=tr, magnitude=0.5, consts=consts)
    f["tracers"][0] *= 1.0 + 0.5 * np.cos(np.arange(nx))[None, None, :, None] ** 2
    f["tracers"][2][0:6] = 2e-3 * f["density_dry"][0:6]
    # heating of up to ~0.05 K per step (J/kg/s: 1003 x 0.05 / 4 ~ 12), cooling aloft, different in every rad cell and member
    rng = np.random.default_rng(11)
    q = 12.0 * rng.uniform(-1.0, 1.0, (nz, rad_ny, rad_nx, nens))

    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", crm_dt)
    c.set_option("rad_nx", rad_nx)
    c.set_option("rad_ny", rad_ny)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(xlen, ylen, zint)
    micro, rad, dyc = Microphysics(), Radiation(), Dycore()
    micro.init(c)
    rad.init(c)
    dyc.init(c)
    c.load_fields(f)
    _put(c, "rad_enthalpy_tend", q)
    dyc.declare_current_profile_as_hydrostatic(c)
    c.run_module("radiation", rad.timeStep)
    nsub = dyc.timeStep(c)
    modules.sponge_layer(c)
    micro.timeStep(c)
    torch.cuda.synchronize()
    got = c.dump_fields()
    dyc.finalize(c)

    def crm_step(ff):
        o = ao.OracleDycore(nens, nx, ny, nz, xlen, ylen, np.diff(zint), pos, mass, idwv, consts=consts)
        o.declare_current_profile_as_hydrostatic(ff)
        ff["temp"] = ref.radiation_forced(ff["temp"], q, consts["cp_d"], crm_dt)
        n = o.time_step(ff, crm_dt)[0]
        ao.sponge_layer(ff, zi, zm, crm_dt)
        trc = [np.ascontiguousarray(ff["tracers"][t]) for t in range(3)]
        ao.kessler(trc[0], trc[1], trc[2], ff["density_dry"], ff["temp"], zm, crm_dt, consts)
        for t in range(3):
            ff["tracers"][t] = trc[t]
        return n
    f0 = copy.deepcopy(f)
    unforced = copy.deepcopy(f)
    assert crm_step(f) == nsub
    compare(got, f, names, nsub, case="py_crm_step_radiation_dycore_sponge_kessler", floor=noise_floor(crm_step, f0, names, 0, base=f))
    # and the forcing is not lost in the gate: the same step without it ends elsewhere
    q_keep, q[...] = q.copy(), 0.0
    crm_step(unforced)
    q[...] = q_keep
    assert np.abs(unforced["temp"] - f["temp"]).max() > 1e-3


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: the driver

def _run_driver(*args, timeout=900):
    r = subprocess.run([DRIVER, "--yaml", CI_YAML] + list(args), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


CI = dict(nx=65, ny=1, nz=50, xlen=128000.0, ylen=64000.0, crm_dt=20.0)


@pytest.mark.gpu
def test_gpu_driver_zero_radiation_leaves_the_run_unchanged(tmp_path):
    """T + 0.0 == T for the case's positive temperatures: with a file of zeros the output and every printed line are the plain run's"""
    a, b, z = tmp_path / "plain.bin", tmp_path / "rad.bin", tmp_path / "zeros.bin"
    nens = 3
    np.zeros((CI["nz"], 1, 5, nens)).tofile(z)
    plain = _run_driver("--nens", str(nens), "--steps", "6", str(a))
    forced = _run_driver("--nens", str(nens), "--steps", "6", "--radiation", "5", "1", str(z), str(b))
    assert plain == forced
    assert a.read_bytes() == b.read_bytes()
    # a file of another size, or a rad grid that does not divide nx = 65, ends the run with an error
    for args in (["--radiation", "13", "1", str(z)], ["--radiation", "4", "1", str(z)]):
        r = subprocess.run([DRIVER, "--yaml", CI_YAML, "--nens", str(nens), "--steps", "1"] + args + ["-"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "endrun" in r.stderr, (args, r.stderr[-500:])


@pytest.mark.gpu
def test_gpu_driver_radiation_first_crm_step_equals_the_python_path(tmp_path):
    """a non-zero tendency on a 5 x 1 rad grid of the CI input (nx = 65): the driver's first CRM step against the same calls through
    the Python classes, within the gate of the HIP-vs-oracle comparisons with the noise floor of the oracle's step"""
    import torch
    from oracle import awfl_oracle as ao
    from pam_amd import Dycore, Microphysics, PamCoupler, Radiation, modules
    from parity_gate import compare, noise_floor
    nens, nx, ny, nz, crm_dt = 2, CI["nx"], CI["ny"], CI["nz"], CI["crm_dt"]
    rng = np.random.default_rng(12)
    q = 10.0 * rng.uniform(-1.0, 1.0, (nz, 1, 5, nens))
    qf, out = tmp_path / "tend.bin", tmp_path / "out.bin"
    q.tofile(qf)
    stdout = _run_driver("--nens", str(nens), "--steps", "1", "--radiation", "5", "1", str(qf), str(out))
    stats = json.loads(stdout.strip().split("\n")[-1])
    ncell = nz * ny * nx * nens
    raw = np.fromfile(out, dtype="<f8")[:8 * ncell].reshape(8, nz, ny, nx, nens)
    got = {"density_dry": raw[0], "uvel": raw[1], "vvel": raw[2], "wvel": raw[3], "temp": raw[4], "tracers": raw[5:]}

    zint = np.linspace(0.0, 20000.0, nz + 1)
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", crm_dt)
    c.set_option("gcm_physics_dt", 900.0)
    c.set_option("rad_nx", 5)
    c.set_option("rad_ny", 1)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(CI["xlen"], CI["ylen"], zint)
    micro, rad, dyc = Microphysics(), Radiation(), Dycore()
    micro.init(c)
    dyc.init(c)
    rad.init(c)
    dm = c.get_data_manager_device_readwrite()
    cols = modules.supercell_init(torch.from_numpy(zint).cuda(), c.get_option("R_d"), c.get_option("R_v"), c.get_option("grav"))
    for name, col in zip(("gcm_density_dry", "gcm_uvel", "gcm_vvel", "gcm_wvel", "gcm_temp", "gcm_water_vapor"), cols):
        dm.get(name).copy_(col[:, None].expand(nz, nens))
    modules.broadcast_initial_gcm_column(c)
    keep = modules.perturb_temperature(c, np.zeros(nens, dtype=np.int32), 0.1)
    _put(c, "rad_enthalpy_tend", q)
    torch.cuda.synchronize()
    start = c.dump_fields()
    dyc.declare_current_profile_as_hydrostatic(c)
    c.run_module("radiation", rad.timeStep)
    nsub = dyc.timeStep(c)
    modules.sponge_layer(c)
    micro.timeStep(c)
    torch.cuda.synchronize()
    want = c.dump_fields()
    dyc.finalize(c)
    del keep
    assert nsub == stats["substeps"]
    names = ["water_vapor", "cloud_liquid", "precip_liquid"]
    consts = dict(R_d=287.0, cp_d=1003.0, R_v=461.0, cp_v=1859.0, p0=1.0e5, grav=9.81)
    zi = np.ascontiguousarray(np.broadcast_to(zint[:, None], (nz + 1, nens)))
    zm = 0.5 * (zi[:-1] + zi[1:])

    def crm_step(ff):
        o = ao.OracleDycore(nens, nx, ny, nz, CI["xlen"], CI["ylen"], np.diff(zint), [True] * 3, [True] * 3, 0, consts=consts)
        o.declare_current_profile_as_hydrostatic(ff)
        ff["temp"] = ref.radiation_forced(ff["temp"], q, consts["cp_d"], crm_dt)
        o.time_step(ff, crm_dt)
        ao.sponge_layer(ff, zi, zm, crm_dt)
        trc = [np.ascontiguousarray(ff["tracers"][t]) for t in range(3)]
        ao.kessler(trc[0], trc[1], trc[2], ff["density_dry"], ff["temp"], zm, crm_dt, consts)
        for t in range(3):
            ff["tracers"][t] = trc[t]
    compare(got, want, names, nsub, floor=noise_floor(crm_step, start, names, 0))
    # the forcing reached the driver's state: the plain run's temperature differs
    plain = tmp_path / "plain.bin"
    _run_driver("--nens", str(nens), "--steps", "1", str(plain))
    t_plain = np.fromfile(plain, dtype="<f8")[4 * ncell:5 * ncell].reshape(nz, ny, nx, nens)
    assert np.abs(t_plain - got["temp"]).max() > 1e-3
