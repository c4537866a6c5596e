"""modules::saturation_adjustment and modules::surface_friction_init / compute_surface_friction
(pam_core/modules/saturation_adjustment.h, surface_friction.h): the CPU restatement's properties (tests/moist_surface_ref.py), the host
emulation of the device bodies (pam_amd/csrc/moist_surface_device.h under g++) against it bit for bit, the C ABI's argument checks,
the adaptors' boundary, and on the GPU the HIP path against the restatement."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import moist_surface_cases as mc
import moist_surface_ref as ref
import test_boundary_surface as tb
from moist_surface_cases import CONDENSATE, CP_D, CP_V, R_V, TRACER_SETS, _p, emu, emu_saturation_adjustment, moist_state  # noqa: F401
from pam_amd import capi
from pam_amd import idealized as idz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
# the states (moist_state), the binding of the host emulation (emu, emu_saturation_adjustment) and the gates of the GPU tests live in
# tests/moist_surface_cases.py; the names above are kept here for the tests that import them from this module


def _emu_cells(lib, rv, rc=None, t=None, rho_d=1.0):
    """single-species cells (rho = rho_d + rho_v + rho_c) through the emulation"""
    rv = np.ascontiguousarray(rv, dtype=np.float64)
    n = rv.size
    rc = np.zeros(n) if rc is None else np.ascontiguousarray(np.broadcast_to(rc, (n,)), dtype=np.float64)
    t = np.full(n, 290.0) if t is None else np.ascontiguousarray(np.broadcast_to(t, (n,)), dtype=np.float64)
    rd = np.full(n, rho_d)
    massy = np.ascontiguousarray(np.stack([rv, rc]))
    out = [rv.copy(), rc.copy(), t.copy()]
    it = np.zeros(n, dtype=np.int32)
    lib.emu_saturation_adjustment(n, 2, _p(rd), _p(massy), _p(out[0]), _p(out[1]), _p(out[2]), R_V, CP_D, CP_V, ref.CP_L,
                                  it.ctypes.data_as(C.POINTER(C.c_int)))
    return out, it


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement

@pytest.mark.parametrize("micro", ["kessler", "p3"])
def test_restatement_properties(micro):
    tr = TRACER_SETS[micro]
    f = moist_state(tr, 6, 5, 4, 5, seed=1)
    g, info = ref.saturation_adjustment(f, tr, micro, R_V, CP_D, CP_V)
    cn = CONDENSATE[micro]
    rv0, rc0, t0 = f["water_vapor"].ravel(), f[cn].ravel(), f["temp"].ravel()
    rv1, rc1, t1 = g["water_vapor"].ravel(), g[cn].ravel(), g["temp"].ravel()
    rho_d = f["density_dry"].ravel()
    massy = [f[n].ravel() for n, _, m in tr if m]
    br = info["branch"]
    # every field but water vapour, the condensate and temperature is untouched, as are the cells in neither branch
    for k in f:
        if k not in ("water_vapor", cn, "temp"):
            assert np.array_equal(g[k], f[k]), k
    none = br == 0
    assert np.array_equal(rv1[none], rv0[none]) and np.array_equal(rc1[none], rc0[none]) and np.array_equal(t1[none], t0[none])
    # water is conserved to round-off
    assert np.all(np.abs((rv1 + rc1) - (rv0 + rc0)) <= 4e-16 * (rv0 + rc0))
    kinds = {"cond": 0, "partial": 0, "complete": 0, "none": int(none.sum())}
    for i in np.nonzero(br)[0]:
        rho = rho_d[i] + sum(m[i] for m in massy)
        args = (rho, rho_d[i], rv0[i], rc0[i], t0[i], R_V, CP_D, CP_V, ref.CP_L)
        step = ref.condensed_state if br[i] == 1 else ref.evaporated_state
        x = info["amount"][i]
        if br[i] == 2 and step(rc0[i], *args)[3] < 0:
            # complete evaporation: even all of the cloud leaves the cell unsaturated; what is left is below the tolerance
            kinds["complete"] += 1
            assert rc1[i] <= ref.TOL and step(x, *args)[3] < 0
            continue
        kinds["cond" if br[i] == 1 else "partial"] += 1
        # the adjusted state is saturated to within the bisection tolerance: the residual pv - svp changes sign within +-tol
        lo, hi = step(max(x - 1.01 * ref.TOL, 0.0), *args)[3], step(x + 1.01 * ref.TOL, *args)[3]
        assert lo * hi <= 0, (i, lo, hi)
        assert info["iters"][i] < 60
    assert all(v > 0 for v in kinds.values()), kinds


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the host emulation of the device bodies

@pytest.mark.parametrize("micro", ["kessler", "p3"])
def test_emulation_matches_restatement_bit_for_bit(micro):
    tr = TRACER_SETS[micro]
    lib = emu()
    f = moist_state(tr, 7, 4, 3, 6, seed=2)
    g, info = ref.saturation_adjustment(f, tr, micro, R_V, CP_D, CP_V)
    rv, rc, t, it = emu_saturation_adjustment(lib, f, tr, micro)
    cn = CONDENSATE[micro]
    assert np.array_equal(rv, g["water_vapor"].ravel())
    assert np.array_equal(rc, g[cn].ravel())
    assert np.array_equal(t, g["temp"].ravel())
    assert np.array_equal(it, info["iters"])


def test_emulation_terminates_on_absurd_inputs():
    lib = emu()
    cap = lib.emu_saturation_max_iter()
    assert cap == 2048
    (rv, rc, t), it = _emu_cells(lib, [math.inf, 1e12, math.nan, 0.005], rc=[0.0, 0.0, 1e-3, math.nan])
    assert it[0] == cap                  # the bracket is inf / NaN: the reference's loop would never end
    assert 0 < it[1] <= cap              # returns; the midpoint may stall one ulp away from a bound wider than tol
    # NaN falls into neither branch and passes through unchanged
    assert it[2] == 0 and math.isnan(rv[2]) and rc[2] == 1e-3 and t[2] == 290.0
    assert it[3] == 0 and rv[3] == 0.005 and math.isnan(rc[3]) and t[3] == 290.0   # (NaN > 0 is false)
    # an infinite cloud amount with a sub-saturated cell: the evaporation bracket is inf
    (_, _, _), it = _emu_cells(lib, [1e-3], rc=[math.inf])
    assert it[0] == cap


def test_emulation_cap_never_binds_on_finite_states_up_to_1e9():
    lib = emu()
    rv = np.logspace(-8, 9, 400)
    most = 0
    for temp in (200.0, 250.0, 290.0, 320.0):
        for rho_d in (1e-3, 1.0, 1e3):
            # condensation over the whole range; evaporation of clouds of every size into dry air
            _, it = _emu_cells(lib, rv, rc=0.0, t=temp, rho_d=rho_d)
            most = max(most, int(it.max()))
            _, it = _emu_cells(lib, np.full(rv.size, 1e-9), rc=rv, t=temp, rho_d=rho_d)
            most = max(most, int(it.max()))
    assert most < 64, most               # 2048 is never reached: within 54 halvings of a bracket <= 1e9 down to 1e-6


def test_emulation_surface_friction_matches_restatement_bit_for_bit():
    lib = emu()
    rng = np.random.default_rng(3)
    n = 400
    zmid0 = rng.uniform(10, 100, n)
    bflx = np.where(rng.random(n) < 0.3, 0.0, rng.uniform(-0.05, 0.05, n))
    gu, gv = rng.normal(0, 6, n), rng.normal(0, 6, n)
    gu[:20] = 0.1                         # calm: max(1, |u|)
    tau, rho_mean = rng.uniform(1e-3, 0.5, n), rng.uniform(1.0, 1.2, n)
    z0 = np.zeros(n)
    lib.emu_surface_friction_z0(n, *[_p(a) for a in (zmid0, bflx, gu, gv, tau, rho_mean, z0)])
    want = np.array([ref.surface_friction_z0(*a) for a in zip(zmid0, bflx, gu, gv, tau, rho_mean)])
    assert np.array_equal(z0, want)
    assert z0.min() >= 1e-5 and z0.max() <= 1.0 and (z0 == 1e-5).any()
    u, v = rng.normal(3, 4, n), rng.normal(-1, 4, n)
    u[:30], v[:30] = 0.2, -0.3
    um, vm = rng.normal(3, 1, n), rng.normal(-1, 1, n)
    r0 = rng.uniform(1.1, 1.2, n)
    r1, r2 = r0 - rng.uniform(0, 0.01, n), r0 - rng.uniform(0.01, 0.02, n)
    dz = rng.uniform(20, 200, n)
    fu, fv = np.zeros(n), np.zeros(n)
    lib.emu_surface_friction_cell(n, *[_p(a) for a in (u, v, um, vm, rho_mean, zmid0, bflx, z0, r0, r1, r2, dz, fu, fv)])
    want = np.array([ref.surface_friction_cell(*a) for a in zip(u, v, um, vm, rho_mean, zmid0, bflx, z0, r0, r1, r2, dz)])
    assert np.array_equal(fu, want[:, 0]) and np.array_equal(fv, want[:, 1])


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the C ABI

NEW_SYMBOLS = ("pam_amd_saturation_adjustment", "pam_amd_surface_friction_init", "pam_amd_surface_friction_compute")


def test_new_entry_points_are_exported_and_declared():
    lib = capi.load()
    declared = tb_header_symbols()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name


def tb_header_symbols():
    import re
    text = open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))


def test_new_modules_reject_bad_arguments_before_touching_a_device():
    lib = capi.load()
    P = C.c_void_p(64)                    # never dereferenced: validation fails first
    M3 = (C.c_void_p * 3)(64, 64, 64)
    M3null = (C.c_void_p * 3)(64, None, 64)
    sat = lib.pam_amd_saturation_adjustment
    fr_init, fr = lib.pam_amd_surface_friction_init, lib.pam_amd_surface_friction_compute
    cases = [
        ("saturation_adjustment", lambda: sat(0, 4, 1, 8, P, P, P, P, 3, M3, R_V, CP_D, CP_V, 4188.0, None)),
        ("saturation_adjustment", lambda: sat(2, 4, 1, 8, P, None, P, P, 3, M3, R_V, CP_D, CP_V, 4188.0, None)),
        ("saturation_adjustment", lambda: sat(2, 4, 1, 8, P, P, P, P, 3, None, R_V, CP_D, CP_V, 4188.0, None)),
        ("saturation_adjustment", lambda: sat(2, 4, 1, 8, P, P, P, P, 3, M3null, R_V, CP_D, CP_V, 4188.0, None)),
        ("saturation_adjustment", lambda: sat(2, 4, 1, 8, P, P, P, P, 56, M3, R_V, CP_D, CP_V, 4188.0, None)),
        ("saturation_adjustment", lambda: sat(2, 4, 1, 8, P, P, P, P, 3, M3, math.nan, CP_D, CP_V, 4188.0, None)),
        ("saturation_adjustment", lambda: sat(2, 4, 1, 8, P, P, P, P, 3, M3, R_V, CP_D, CP_V, 0.0, None)),
        ("surface_friction_init", lambda: fr_init(2, 4, 1, 8, *([P] * 10 + [None]), None)),
        ("surface_friction_init", lambda: fr_init(2, 0, 1, 8, *([P] * 11), None)),
        ("compute_surface_friction", lambda: fr(2, 4, 1, 8, *([None] + [P] * 9), None)),
        ("compute_surface_friction", lambda: fr(-1, 4, 1, 8, *([P] * 10), None)),
    ]
    for who, call in cases:
        assert call() == -1, who                                   # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert who.encode() in lib.pam_amd_awfl_last_error(), who


@pytest.mark.parametrize("nz", [1, 2])
def test_surface_friction_needs_three_levels(nz):
    lib = capi.load()
    P = C.c_void_p(64)
    assert lib.pam_amd_surface_friction_compute(2, 4, 1, nz, *([P] * 10), None) == -1
    err = lib.pam_amd_awfl_last_error()
    assert b"compute_surface_friction" in err and b"nz >= 3" in err


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the boundary of the C++ adaptors

ADAPTORS = [os.path.join(HOST, "modules", "saturation_adjustment.h"), os.path.join(HOST, "modules", "surface_friction.h")]
SIGNATURES = {   # signature -> the reference line it must match (tests/golden/extract_moist_surface.py records the digests)
    "inline void saturation_adjustment(pam::PamCoupler &coupler)": "pam_core/modules/saturation_adjustment.h:116",
    "inline void surface_friction_init(pam::PamCoupler &coupler, realConst1d &tau_in, realConst1d &bflx_in)":
        "pam_core/modules/surface_friction.h:66",
    "inline void compute_surface_friction(pam::PamCoupler &coupler)": "pam_core/modules/surface_friction.h:107",
}


@pytest.mark.parametrize("src", ADAPTORS, ids=[os.path.basename(s) for s in ADAPTORS])
def test_adaptors_call_only_members_the_reference_has(src):
    coupler, dm = tb._used_members(open(src).read())
    assert coupler and dm
    assert coupler <= tb.REF_COUPLER, sorted(coupler - tb.REF_COUPLER)
    assert dm <= tb.REF_DM, sorted(dm - tb.REF_DM)
    ours = tb._declared(os.path.join(HOST, "pam_coupler.h"))
    assert (coupler | dm) <= ours, sorted((coupler | dm) - ours)


def test_adaptors_have_the_reference_signatures():
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "moist_surface_extract.json")))["signature_sha256"]
    assert sorted(rec) == sorted(SIGNATURES.values())
    text = "".join(tb._norm(tb._strip_comments(open(s).read())) for s in ADAPTORS)
    for sig, where in SIGNATURES.items():
        assert tb._digest(tb._norm(sig)) == rec[where], (sig, where)
        assert tb._norm(sig) + "{" in text, sig


def test_realconst1d_is_declared_by_the_work_alike_coupler():
    text = open(os.path.join(HOST, "pam_coupler.h")).read()
    assert "typedef pam::DeviceView<real const> realConst1d;" in text


# ------------------------------------------------------------------------------------------------------------------------------
# GPU

def _coupler(tracers, f, micro=None, zint=None):
    import torch
    from pam_amd import PamCoupler
    nz, ny, nx, nens = f["density_dry"].shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", 2.0)
    if micro is not None:
        c.set_option("micro", micro)
    for k, v in (("R_v", R_V), ("cp_d", CP_D), ("cp_v", CP_V)):
        c.set_option(k, v)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(nx * 500.0, ny * 500.0, idz.stretched_interfaces(nz, 12000.0) if zint is None else zint)
    for n, p, m in tracers:
        c.add_tracer(n, "", p, m)
    dm = c.get_data_manager_device_readwrite()
    for k, v in f.items():
        if dm.entry_exists(k):
            dm.get(k).copy_(torch.from_numpy(v))
    return c


def _dump(c, names):
    dm = c.get_data_manager_device_readwrite()
    return {n: dm.get(n, readonly=True).cpu().numpy() for n in names}


SHAPES = mc.MODULE_SHAPES     # (nens, nx, ny, nz): ragged nens with nx*ny >= 16, nx*ny < 16, one member


@pytest.mark.gpu
@pytest.mark.parametrize("micro", ["kessler", "p3"])
@pytest.mark.parametrize("shape", SHAPES, ids=mc.MODULE_SHAPE_IDS)
def test_gpu_saturation_adjustment_matches_restatement(micro, shape):
    import torch
    from pam_amd import modules
    d = mc.saturation_case("%s_%s" % (micro, mc.MODULE_SHAPE_IDS[SHAPES.index(shape)]))
    tr, f = d["tracers"], d["fields"]
    c = _coupler(tr, f, micro)
    dirty = c.run_module("saturation_adjustment", modules.saturation_adjustment)
    torch.cuda.synchronize()
    names = list(f)
    got = _dump(c, names)
    info = d["info"]
    cn = CONDENSATE[micro]
    # the reference hands out density_dry, temp, water vapour, the condensate and every tracer that adds mass non-const
    assert set(dirty) == {"density_dry", "temp", "water_vapor", cn} | {n for n, _, m in tr if m}, dirty
    # every other field, and every field the module does not adjust, is unchanged bit for bit
    for k in names:
        if k not in ("water_vapor", cn, "temp"):
            assert np.array_equal(got[k], f[k]), k
    # the adjusted fields against the restatement, bit for bit (tests/moist_surface_cases.py: assert_adjusted_bits): exp enters the
    # bisection only through its decisions, none of which is within 1e-10 of a tie on these states, so no cell is exempt
    exempt = mc.assert_adjusted_bits({"rho_v": got["water_vapor"], "rho_c": got[cn], "temp": got["temp"]}, d["want"], info, d["before"],
                                     rho_min=0.5)
    print("saturation_adjustment %s %s: %d of %d cells adjusted, %d exempted (decision margin < 1e-12)"
          % (micro, shape, int((info["branch"] > 0).sum()), info["branch"].size, exempt))
    assert exempt == 0


@pytest.mark.gpu
def test_gpu_saturation_adjustment_rejects_an_unknown_micro():
    from pam_amd import modules
    tr = TRACER_SETS["kessler"]
    f = moist_state(tr, 4, 3, 2, 3)
    c = _coupler(tr, f, "sam1mom")
    with pytest.raises(capi.PamAmdError, match="kessler and p3"):
        modules.saturation_adjustment(c)
    assert all(np.array_equal(v, f[k]) for k, v in _dump(c, list(f)).items())


_friction_state = mc.module_friction_state


def _friction_run(tr, f, tau, bflx, zi, computes=1):
    import torch
    from pam_amd import modules
    c = _coupler(tr, f, "kessler", zint=zi)
    d_init = c.run_module("surface_friction_init", lambda cc: modules.surface_friction_init(cc, tau, bflx))
    torch.cuda.synchronize()
    got = {"init": _dump(c, ["z0", "sfc_bflx", "sfc_mom_flx_u", "sfc_mom_flx_v"]), "dirty_init": set(d_init), "compute": []}
    for _ in range(computes):
        d = c.run_module("surface_friction", modules.compute_surface_friction)
        torch.cuda.synchronize()
        got["compute"].append(_dump(c, ["sfc_mom_flx_u", "sfc_mom_flx_v"]))
        got["dirty"] = set(d)
    got["fields"] = _dump(c, [k for k in f if c.get_data_manager_device_readwrite().entry_exists(k)])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("shape", mc.MODULE_FRICTION_SHAPES, ids=mc.MODULE_FRICTION_IDS)
def test_gpu_surface_friction_matches_restatement(shape):
    """the last shape has 144 columns: the compute kernel splits them into three chunks, each summing the means itself.  z0 per member
    and the fluxes per cell against the longdouble reference at the slot-order means (tests/moist_surface_cases.py: assert_z0_within,
    assert_fluxes_within); the fluxes' reference takes the z0 the device's init left, which has passed its own gate by then."""
    nens, nx, ny, nz = shape
    tr, f, tau, bflx, zi = _friction_state(nens, nx, ny, nz, seed=20 + nens)
    got = _friction_run(tr, f, tau, bflx, zi, computes=2)
    d = mc.friction_case("module_" + mc.MODULE_FRICTION_IDS[mc.MODULE_FRICTION_SHAPES.index(shape)])
    assert all(np.array_equal(d[k], f[n]) for k, n in (("rho_d", "density_dry"), ("rho_v", "water_vapor"), ("uvel", "uvel"), ("vvel", "vvel")))
    gi = got["init"]
    raw, want = mc.z0_reference(d)
    worst_z0 = mc.assert_z0_within(gi["z0"], raw, want)
    assert np.array_equal(gi["sfc_bflx"], bflx)
    assert assert_zero_then_filled(gi, got)
    g = got["compute"][0]
    worst = mc.assert_fluxes_within(g["sfc_mom_flx_u"], g["sfc_mom_flx_v"], mc.friction_reference(d, z0=gi["z0"]))
    print("surface friction %s: z0 %.2f units at the worst (gate %g), fluxes %.2f (gate %g)" % (shape, worst_z0, mc.G_Z0, worst, mc.G_FLUX))
    for k in ("sfc_mom_flx_u", "sfc_mom_flx_v"):
        assert np.array_equal(g[k], got["compute"][1][k]), k          # two identical calls: identical bits
    assert got["dirty_init"] == {"z0", "sfc_bflx", "sfc_mom_flx_u", "sfc_mom_flx_v", "density_dry", "water_vapor",
                                 "vertical_midpoint_height", "gcm_uvel", "gcm_vvel"}, got["dirty_init"]
    assert got["dirty"] == {"z0", "sfc_bflx", "sfc_mom_flx_u", "sfc_mom_flx_v"}, got["dirty"]
    for k, v in got["fields"].items():                          # the module writes nothing else
        assert np.array_equal(v, f[k]), k


def assert_zero_then_filled(gi, got):
    return not gi["sfc_mom_flx_u"].any() and not gi["sfc_mom_flx_v"].any() and got["compute"][0]["sfc_mom_flx_u"].any()


@pytest.mark.gpu
def test_gpu_surface_friction_ensemble_split_is_bitwise_the_whole():
    """the modules work per member: two halves of an ensemble give the whole's bits (the shard path needs nothing new)"""
    nens, nx, ny, nz = 70, 5, 4, 4
    tr, f, tau, bflx, zi = _friction_state(nens, nx, ny, nz, seed=7)
    whole = _friction_run(tr, f, tau, bflx, zi)
    h = 33
    halves = []
    for sl in (slice(0, h), slice(h, nens)):
        fh = {k: np.ascontiguousarray(v[..., sl]) for k, v in f.items()}
        halves.append(_friction_run(tr, fh, tau[sl], bflx[sl], np.ascontiguousarray(zi[:, sl])))
    assert np.array_equal(np.concatenate([x["init"]["z0"] for x in halves]), whole["init"]["z0"])
    for k in ("sfc_mom_flx_u", "sfc_mom_flx_v"):
        assert np.array_equal(np.concatenate([x["compute"][0][k] for x in halves], axis=-1), whole["compute"][0][k]), k


@pytest.mark.gpu
def test_gpu_driver_runs_with_saturation_adjustment_and_surface_friction():
    exe = os.path.join(ROOT, "examples", "driver")
    yaml = os.path.join(ROOT, "tests", "golden", "ci_input_pama.yaml")
    r = subprocess.run([exe, "--yaml", yaml, "--steps", "10", "--check", "--sat-adjust", "--surface-friction", "0.1", "0.01", "-"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    res = json.loads(lines[-1])
    assert res["crm_steps"] == 10 and res["finite"] and res["conservation_checked"]
    assert res["conservation_violations"] == 0, res
    assert 150.0 < res["temp_min"] and res["temp_max"] < 350.0 and res["rho_d_min"] > 0, res
    sf = [ln for ln in lines if ln.startswith("surface friction:")]
    assert len(sf) == 1 and "finite true" in sf[0], sf
    z0 = [float(x) for x in sf[0].split("z0 [")[1].rstrip("]").split(",")]
    assert 1e-5 <= z0[0] <= z0[1] <= 1.0
    print(lines[-1])
    print(sf[0])
