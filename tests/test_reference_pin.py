"""The pin of the parity oracle: the reference's OWN source text, compiled serially at IEEE fp64 against the YAKL stand-in
(oracle/ref/, oracle/_ref/libpam_ref.so, oracle/pam_ref.py), against oracle/awfl_oracle.c, the g++ emulation of the HIP kernel
bodies (tests/emu) and the HIP path.

 * Fixtures (always run, no reference tree needed): tests/golden/ref_*.npz are reference outputs (tests/golden/make_ref_golden.py).
   The oracle must reproduce them BIT FOR BIT: it restates the reference in the same operation order, and the serial atomicAdd
   of the stand-in (j outer, i inner) is the oracle's order too.  The emulation at the tolerances it keeps against the oracle
   (tests/test_emu_parity.py: the noise fields at the floor of the fixture's inputs through the oracle).
 * Live reference (when oracle/_ref/ was built): the oracle against the reference on the hydrostatic outputs of both balance
   modes and of the GCM column, the vertical matrices on uniform / stretched / per-member grids, compute_time_step, a timeStep of
   every make_golden case, the D1 replay count, and a seeded sweep over test_fuzz_parity.draw_case (PAM_AMD_REF_SEEDS=N seeds,
   default 16; the odd seeds that draw a 3-D grid run it with dx != dy and the sounding's shear along y or along both, as three of
   the make_golden cases do).  All bit for bit.
 * Coupler modules: the oracle and tests/moist_surface_ref.py against the reference's sponge_layer, GCM forcing (three hole-filling
   paths of the liquid, and two states of tests/gcm_forcing_cases.py: every species in the level pass and the fallback), broadcasts, saturation_adjustment (Kessler and P3 tracer sets), surface friction, Kessler (one and several sub-cycles)
   and supercell_init on L60 -- bit for bit, through tests/golden/ref_mod_*.npz and live.
 * GPU (-m gpu): the HIP path against the fixtures through tests/parity_gate.py (at each case's noise floor) and the modules' own
   tolerances, and against the
   live reference on fuzz draws and on modules at ragged nens (1, 63, 65, 130) with nx*ny of 1, 5 and 15.

The differences that remain are deliberate and documented in DESIGN.md section 4: D1 (the replay below makes the reference's
bottom-ghost read-after-write order-independent; test_mode_a_without_replay_differs_at_the_bottom_ghost shows the reference without
it), D2 (a throw-away solve in init, no effect on state) and D3 (matinv_ge: the stand-in and the oracle share the project's
Gauss-Jordan assumption, so it stays unpinned, as do the device atomicAdd order and minval of YAKL itself).
"""
import copy
import glob
import os

import numpy as np
import pytest

from oracle import awfl_oracle as ao
from oracle import pam_ref
from pam_amd import idealized as idz
from parity_cases import build_inputs
from parity_gate import compare, noise_floor
from test_emu_parity import assert_within_floor

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
import importlib.util   # noqa: E402

_spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(GOLD, "make_ref_golden.py"))
mrg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mrg)

NSEEDS = int(os.environ.get("PAM_AMD_REF_SEEDS", "16"))
MAX_CELLS = 6000        # the reference runs ~1e5 cell-updates/s on one core: the default sweep stays within about a minute
live = pytest.mark.skipif(not pam_ref.available(), reason="oracle/_ref/libpam_ref.so not built (reference tree absent)")
FIELDS = ("density_dry", "uvel", "vvel", "wvel", "temp", "tracers")


def _fixture(name):
    return np.load(mrg.fixture_path(name))


def _inputs(g):
    return {k: np.ascontiguousarray(g["in_" + k]) for k in FIELDS}


def _checker(cls, c, g):
    """an OracleDycore / RefDycore / EmuDycore for make_ref_golden case `c`"""
    tr, consts, zi, xlen, ylen, _ = mrg.mg.build_case(c)
    names, pos, mass, idwv = idz.tracer_flags(tr)
    kw = {"names": names} if cls is pam_ref.RefDycore else {}
    o = cls(c["nens"], c["nx"], c["ny"], c["nz"], xlen, ylen, np.diff(zi, axis=0), pos, mass, idwv, consts=consts, **kw)
    o.set_grav_balance(c["mode_a"])
    return o, names


def _fixture_floor(c, g, names, base):
    """parity_gate.noise_floor of make_ref_golden case `c`: its inputs through the oracle (which reproduces the fixture `base`
    bit for bit, test_oracle_reproduces_reference_fixture_bitwise)"""
    def run(f):
        o, _ = _checker(ao.OracleDycore, c, g)
        o.declare_current_profile_as_hydrostatic(f)
        for _ in g["ncycles"]:
            o.time_step(f, c["crm_dt"])
    return noise_floor(run, _inputs(g), names, 0, base=base)


def _assert_identical(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        d = np.abs(got - exp)
        i = np.unravel_index(np.nanargmax(d), d.shape) if np.isfinite(d).any() else None
        raise AssertionError("%s differs: max |diff| %.3e at %s (%d of %d elements)" % (what, np.nanmax(d), i, (got != exp).sum(), got.size))


def test_fixtures_are_reference_outputs():
    """every case of make_ref_golden is committed, with the provenance of the build that made it (data, no source text)"""
    assert sorted(glob.glob(os.path.join(GOLD, "ref_*.npz"))) == sorted([mrg.fixture_path(n) for n in mrg.CASES] +
                                                                         [mrg.module_fixture_path(n) for n in mrg.MODULE_CASES])
    import json
    prov = json.load(open(mrg.PROVENANCE))
    assert "dynamics/awfl/Dycore.h" in prov["reference_headers_sha256"] and prov["compiler"]
    assert set(prov["standin_sha256"]) == set(mrg.STANDIN_FILES)
    for name in mrg.CASES:
        g = _fixture(name)
        assert all(np.isfinite(g[k]).all() for k in g.files if k.startswith("out_"))


@pytest.mark.parametrize("name", sorted(mrg.CASES))
def test_oracle_reproduces_reference_fixture_bitwise(name):
    c = mrg.CASES[name]
    g = _fixture(name)
    o, _ = _checker(ao.OracleDycore, c, g)
    f = _inputs(g)
    assert o.compute_time_step(f) == float(g["dt_cfl"])
    o.declare_current_profile_as_hydrostatic(f)
    _assert_identical(o.vert_sten_to_coefs, g["vert_sten_to_coefs"], "vert_sten_to_coefs")
    _assert_identical(o.vert_weno_recon_lower, g["vert_weno_recon_lower"], "vert_weno_recon_lower")
    for key in ("variable_gravity",) if c["mode_a"] else ("hy_dens_cells", "hy_pressure_cells"):
        _assert_identical(getattr(o, key), g[key], key)
    for n, dt in zip(g["ncycles"], g["dt_dyn"]):
        assert o.time_step(f, c["crm_dt"]) == (int(n), float(dt))
    for k in FIELDS:
        _assert_identical(f[k], g["out_" + k], k)


@pytest.mark.parametrize("name", sorted(mrg.CASES))
def test_emulation_reproduces_reference_fixture(name):
    """the g++ emulation of the HIP kernel bodies, at the tolerances it keeps against the oracle (tests/test_emu_parity.py)"""
    import emu_harness as eh
    c = mrg.CASES[name]
    g = _fixture(name)
    e, names = _checker(eh.EmuDycore, c, g)
    f = _inputs(g)
    assert e.compute_time_step(f) == float(g["dt_cfl"])
    e.declare_current_profile_as_hydrostatic(f)
    for key in ("variable_gravity",) if c["mode_a"] else ("hy_dens_cells",):
        got = e.buffer(key, (c["nz"], c["nens"]))
        assert np.abs(got - g[key]).max() <= 1e-13 * np.abs(g[key]).max(), key
    for n, dt in zip(g["ncycles"], g["dt_dyn"]):
        assert e.time_step(f, c["crm_dt"]) == (int(n), float(dt))

    def rel(k, t=None):
        a, b = (f[k], g["out_" + k]) if t is None else (f[k][t], g["out_" + k][t])
        return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    for k, tol in (("density_dry", 1e-13), ("temp", 1e-13)):
        assert rel(k) < tol, (k, rel(k))
    # u, v, w, tracers: the noise floor of the fixture's inputs through the oracle (tests/parity_gate.py)
    exp = {k: g["out_" + k] for k in FIELDS}
    assert_within_floor(f, exp, names, _fixture_floor(c, g, names, exp))


# ---- live reference ------------------------------------------------------------------------------------------------

@pytest.mark.skipif(mrg.reference_tree() is None, reason="needs the reference tree oracle/_ref/ was built from")
def test_make_ref_golden_check_reproduces_fixtures():
    assert mrg.main(check=True) == 0


@live
@pytest.mark.parametrize("name", sorted(mrg.mg.CASES))
@pytest.mark.parametrize("mode_a", [True, False], ids=["mode_A", "mode_B"])
def test_oracle_matches_reference_one_time_step(name, mode_a):
    """hydrostatic outputs of both balance modes, compute_time_step and one timeStep of every make_golden case, bit for bit"""
    c = dict(mrg.mg.CASES[name], mode_a=mode_a)
    tr, consts, zi, xlen, ylen, f = mrg.mg.build_case(c)
    fo = copy.deepcopy(f)
    r, _ = _checker(pam_ref.RefDycore, c, None)
    o, _ = _checker(ao.OracleDycore, c, None)
    assert r.compute_time_step(f) == o.compute_time_step(fo)
    r.declare_current_profile_as_hydrostatic(f)
    o.declare_current_profile_as_hydrostatic(fo)
    for key in ("variable_gravity",) if mode_a else ("hy_dens_cells", "hy_pressure_cells"):
        _assert_identical(getattr(o, key), getattr(r, key), key)
    pam_ref.reset_replay_count()
    n, dt = r.time_step(f, c["crm_dt"])
    assert o.time_step(fo, c["crm_dt"]) == (n, dt)
    for k in FIELDS:
        _assert_identical(fo[k], f[k], k)


@live
def test_d1_replay_fires_once_per_compute_tendencies():
    """the replay is keyed by the file:line label of the boundary kernel: a wrong line number leaves the count at zero"""
    c = mrg.mg.CASES["case_2d_nt1_uniform_A"]
    tr, consts, zi, xlen, ylen, f = mrg.mg.build_case(c)
    r, _ = _checker(pam_ref.RefDycore, c, None)
    pam_ref.reset_replay_count()
    r.declare_current_profile_as_hydrostatic(f)      # mode A: one halo exchange
    assert pam_ref.replay_count() == 1
    pam_ref.reset_replay_count()
    n, _ = r.time_step(f, c["crm_dt"])
    assert n >= 1 and pam_ref.replay_count() == 3 * n      # SSPRK3: three compute_tendencies per sub-cycle


@live
def test_mode_a_without_replay_differs_at_the_bottom_ghost():
    """D1 documented, not gated: without the replay the reference builds the bottom ghost pressure from a potential temperature it
    has not written yet (fresh memory: NaN here), so variable_gravity goes wrong at the three lowest levels -- those whose interface
    pressure reconstruction reaches the bottom ghost -- and only there"""
    c = mrg.mg.CASES["case_2d_nt1_uniform_A"]
    tr, consts, zi, xlen, ylen, f = mrg.mg.build_case(c)
    o, _ = _checker(ao.OracleDycore, c, None)
    o.declare_current_profile_as_hydrostatic(copy.deepcopy(f))
    pam_ref.set_replay_label(None)
    try:
        r, _ = _checker(pam_ref.RefDycore, c, None)
        r.declare_current_profile_as_hydrostatic(f)
        gv = r.variable_gravity
    finally:
        pam_ref.set_replay_label(pam_ref.D1_REPLAY_LABEL)
    assert not np.isfinite(gv[:3]).any()
    np.testing.assert_array_equal(gv[3:], o.variable_gravity[3:])


@live
def test_oracle_matches_reference_declare_with_gcm_column():
    c = dict(mrg.mg.CASES["case_3d_nt4_stretched_B"])
    tr, consts, zi, xlen, ylen, f = mrg.mg.build_case(c)
    nz, nens = c["nz"], c["nens"]
    rng = np.random.default_rng(7)
    gcm = {"gcm_density_dry": f["density_dry"].mean(axis=(1, 2)), "gcm_temp": f["temp"].mean(axis=(1, 2)),
           "gcm_water_vapor": f["tracers"][0].mean(axis=(1, 2)),
           "gcm_cloud_water": 1e-5 * rng.random((nz, nens)), "gcm_cloud_ice": 1e-6 * rng.random((nz, nens))}
    gcm = {k: np.ascontiguousarray(v) for k, v in gcm.items()}
    for mode_a in (True, False):
        c["mode_a"] = mode_a
        r, _ = _checker(pam_ref.RefDycore, c, None)
        o, _ = _checker(ao.OracleDycore, c, None)
        r.declare_current_profile_as_hydrostatic(f, gcm)
        o.declare_current_profile_as_hydrostatic(copy.deepcopy(f), gcm)
        for key in ("variable_gravity",) if mode_a else ("hy_dens_cells", "hy_pressure_cells"):
            _assert_identical(getattr(o, key), getattr(r, key), key)


@live
@pytest.mark.parametrize("grid", ["uniform", "stretched", "per_member"])
def test_oracle_matches_reference_vertical_matrices(grid):
    nz, nens = 12, 4
    zint = idz.uniform_interfaces(nz, 10000.0) if grid == "uniform" else idz.stretched_interfaces(nz, 15000.0)
    dz = np.diff(zint)[:, None] * np.ones((1, nens))
    if grid == "per_member":
        dz = dz * (1 + 0.037 * np.arange(nens))[None, :]
    names, pos, mass, idwv = idz.tracer_flags(idz.TRACERS_NONE)
    r = pam_ref.RefDycore(nens, 4, 1, nz, 2000.0, 2000.0, dz, pos, mass, idwv, names=names)
    o = ao.OracleDycore(nens, 4, 1, nz, 2000.0, 2000.0, dz, pos, mass, idwv)
    _assert_identical(o.vert_sten_to_coefs, r.vert_sten_to_coefs, "vert_sten_to_coefs")
    _assert_identical(o.vert_weno_recon_lower, r.vert_weno_recon_lower, "vert_weno_recon_lower")


def _fuzz_inputs(c):
    """inputs of a test_fuzz_parity draw, exactly as test_fuzz_parity.run_case builds them"""
    f, xlen, ylen, _, dz = build_inputs(c["nens"], c["nx"], c["ny"], c["nz"], c["tracers"], c["zint"], c["consts"], per_ens=c["per_ens"],
                                        mag=0.5, dxy=c["dxy"], dry_air=c["dry_air"], dy=c.get("dy"), flow=c.get("flow", "x"),
                                        id0=c["seed"])
    return f, xlen, ylen, dz


def _small_draw(seed):
    import test_fuzz_parity as tfp
    s = seed
    while True:                # the same draws as the GPU sweep, those above MAX_CELLS left out (the next seed instead)
        c = tfp.draw_case(s)
        if c["nens"] * c["nx"] * c["ny"] * c["nz"] <= MAX_CELLS:
            break
        s += 100000
    # every other seed: the same draw on a grid with dx != dy and with the shear along y or along both, where it is 3-D (from a
    # generator of its own: the draws above stay what they were)
    if seed % 2 and c["ny"] > 1:
        rng = np.random.default_rng(9000011 * seed + 37)
        c["dy"] = c["dxy"] * float(rng.choice(tfp.ANISO_RATIOS))
        c["flow"] = str(rng.choice(["y", "diag"]))
    return c


def _run(cls, c, f, xlen, ylen, dz, **kw):
    names, pos, mass, idwv = idz.tracer_flags(c["tracers"])
    if cls is pam_ref.RefDycore:
        kw["names"] = names
    o = cls(c["nens"], c["nx"], c["ny"], c["nz"], xlen, ylen, dz, pos, mass, idwv, consts=c["consts"], **kw)
    o.set_grav_balance(c["mode_a"])
    dt = o.compute_time_step(f)
    o.declare_current_profile_as_hydrostatic(f)
    hydro = (o.variable_gravity if c["mode_a"] else o.hy_dens_cells).copy()
    steps = [o.time_step(f, c["crm_dt"]) for _ in range(c["nsteps"])]
    return dt, hydro, steps


@live
@pytest.mark.parametrize("seed", range(NSEEDS))
def test_oracle_matches_reference_random_case(seed):
    c = _small_draw(seed)
    f, xlen, ylen, dz = _fuzz_inputs(c)
    fo = copy.deepcopy(f)
    dt_r, hydro_r, steps_r = _run(pam_ref.RefDycore, c, f, xlen, ylen, dz)
    dt_o, hydro_o, steps_o = _run(ao.OracleDycore, c, fo, xlen, ylen, dz)
    assert dt_o == dt_r
    _assert_identical(hydro_o, hydro_r, "hydrostatic profile")
    assert steps_o == steps_r
    for k in FIELDS:
        _assert_identical(fo[k], f[k], k)


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _gpu_run(c, names, tr, consts, xlen, ylen, zi, inputs):
    import torch
    from pam_amd import Dycore, PamCoupler
    coupler = PamCoupler("cuda:0")
    coupler.set_option("crm_dt", c["crm_dt"])
    for k, v in consts.items():
        coupler.set_option(k, v)
    coupler.allocate_coupler_state(c["nz"], c["ny"], c["nx"], c["nens"])
    coupler.set_grid(xlen, ylen, zi)
    for n, p, m in tr:
        coupler.add_tracer(n, "", p, m)
    dycore = Dycore()
    dycore.init(coupler)
    coupler.load_fields(inputs)
    if not c["mode_a"]:
        coupler.set_option("balance_hydrostasis_with_gravity", False)
    dycore.declare_current_profile_as_hydrostatic(coupler)
    hydro = coupler.dm.get("variable_gravity" if c["mode_a"] else "hy_dens_cells", readonly=True).cpu().numpy()
    steps = [(dycore.timeStep(coupler), dycore.last_dt_dyn) for _ in range(c["nsteps"])]
    torch.cuda.synchronize()
    got = coupler.dump_fields()
    dycore.finalize(coupler)
    return hydro, steps, got


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(mrg.CASES))
def test_gpu_matches_reference_fixture(name):
    c = mrg.CASES[name]
    g = _fixture(name)
    tr, consts, zi, xlen, ylen, _ = mrg.mg.build_case(c)
    names = [t[0] for t in tr]
    hydro, steps, got = _gpu_run(c, names, tr, consts, xlen, ylen, zi, _inputs(g))
    key = "variable_gravity" if c["mode_a"] else "hy_dens_cells"
    assert np.abs(hydro - g[key]).max() <= 1e-12 * np.abs(g[key]).max()
    assert [n for n, _ in steps] == [int(n) for n in g["ncycles"]]
    for (_, dt), dt_ref in zip(steps, g["dt_dyn"]):
        assert abs(dt - dt_ref) <= 1e-15 * dt_ref       # the CFL minimum of fp64 divides and square roots (test_fuzz_parity)
    exp = {k: g["out_" + k] for k in FIELDS}
    compare(got, exp, names, int(np.sum(g["ncycles"])), "ref_" + name, floor=_fixture_floor(c, g, names, exp))


@pytest.mark.gpu
@pytest.mark.skipif(not pam_ref.available(), reason="oracle/_ref/ did not travel")
@pytest.mark.parametrize("seed", range(4))
def test_gpu_matches_live_reference_random_case(seed):
    c = _small_draw(seed)
    f, xlen, ylen, dz = _fuzz_inputs(c)
    zi = np.asarray(c["zint"])[:, None] * np.ones((1, c["nens"]))
    if c["per_ens"]:
        zi = zi * (1 + 0.01 * np.arange(c["nens"]))[None, :]
    names = [t[0] for t in c["tracers"]]
    floor = noise_floor(lambda ff: _run(ao.OracleDycore, c, ff, xlen, ylen, dz), f, names, c["seed"])
    hydro, steps, got = _gpu_run(c, names, c["tracers"], c["consts"], xlen, ylen, zi, copy.deepcopy(f))
    _, hydro_r, steps_r = _run(pam_ref.RefDycore, c, f, xlen, ylen, dz)
    assert np.abs(hydro - hydro_r).max() <= 1e-12 * np.abs(hydro_r).max()
    assert [n for n, _ in steps] == [n for n, _ in steps_r]
    factor = 4.0 if min(c["nx"], c["nz"], c["ny"] if c["ny"] > 1 else c["nx"]) <= 4 else 1.0   # as test_fuzz_parity
    compare(got, f, names, sum(n for n, _ in steps_r), None, factor, floor)     # the oracle's floor: it is the reference bit for bit


# ---- coupler modules -----------------------------------------------------------------------------------------------

def _project_module(kind, kw, inp):
    """the same module by the project's own CPU checkers: the oracle (sponge, GCM forcing, broadcast, Kessler, supercell_init) and
    the Python restatement tests/moist_surface_ref.py (saturation adjustment, surface friction)"""
    import moist_surface_ref as msr
    inp = {k: np.array(v, dtype=np.float64, copy=True) for k, v in inp.items()}
    if kind == "supercell":
        return dict(zip(("rho_d", "uvel", "vvel", "wvel", "temp", "rho_v"), ao.supercell_init(inp["zint"], idz.CONSTS_DEFAULT)))
    if kind == "kessler":
        import test_micro_kessler as tk
        zm = 0.5 * (inp["zint"][:-1] + inp["zint"][1:])
        precl, _ = ao.kessler(inp["rho_v"], inp["rho_c"], inp["rho_r"], inp["rho_dry"], inp["temp"], zm, kw["dt"], tk.C0)
        return dict(rho_v=inp["rho_v"], rho_c=inp["rho_c"], rho_r=inp["rho_r"], temp=inp["temp"], precl=precl)
    if kind == "broadcast":
        nz, nens = inp["gcm_density_dry"].shape
        crm = {n: np.zeros((nz, kw["ny"], kw["nx"], nens)) for n in ao.BROADCAST_CRM}
        ao.broadcast_initial_gcm_column(crm, inp, dry_density_only=True)
        out = {"dry_density_dry": crm["density_dry"].copy()}
        ao.broadcast_initial_gcm_column(crm, inp)
        return dict(out, **crm)
    if kind == "sponge":
        zm = 0.5 * (inp["zint"][:-1] + inp["zint"][1:])
        ao.sponge_layer(inp, inp["zint"], zm, 2.0, num_layers=4, time_scale=30.0)
        return {k: inp[k] for k in mrg.FIELD5 + ("tracers",)}
    if kind == "gcm":
        crm = {n: inp[n] for n in ao.GCM_FORCING_CRM}
        gcm = {n: inp[n] for n in ao.GCM_FORCING_GCM}
        tend = ao.compute_gcm_forcing_tendencies(crm, gcm, mrg.GCM_DT)
        out = {"computed_" + n: v.copy() for n, v in tend.items() if n[-5:] not in ("rho_v", "rho_l", "rho_i")}
        dz = np.diff(inp["zint"], axis=0)
        for _ in range(mrg.GCM_APPLICATIONS):
            ao.apply_gcm_forcing_tendencies(crm, gcm, tend, dz, mrg.GCM_CRM_DT, mrg.GCM_DT)
        return dict(out, **crm, **tend)
    if kind == "satadj":
        import test_moist_surface_modules as tms
        tr = tms.TRACER_SETS[kw["micro"]]
        f = {n: inp[n] for n in ["density_dry", "temp"] + [t[0] for t in tr]}
        c = mrg.SATADJ_CONSTS
        out, _ = msr.saturation_adjustment(f, tr, kw["micro"], c["R_v"], c["cp_d"], c["cp_v"])
        return out
    if kind == "friction":
        zi = inp["zint"]
        zm = 0.5 * (zi[:-1] + zi[1:])
        z0, sb, fu0, fv0 = msr.surface_friction_init(inp["density_dry"], inp["water_vapor"], zm, inp["gcm_uvel"], inp["gcm_vvel"],
                                                     inp["tau"], inp["bflx"])
        fu, fv = msr.compute_surface_friction(inp["density_dry"], inp["water_vapor"], inp["uvel"], inp["vvel"], zm, zi, z0, sb)
        return dict(init_z0=z0, init_sfc_bflx=sb, init_sfc_mom_flx_u=fu0, init_sfc_mom_flx_v=fv0, sfc_mom_flx_u=fu, sfc_mom_flx_v=fv)
    raise ValueError(kind)


def _module_fixture(name):
    g = np.load(mrg.module_fixture_path(name))
    return ({k[3:]: g[k] for k in g.files if k.startswith("in_")}, {k[4:]: g[k] for k in g.files if k.startswith("out_")})


@pytest.mark.parametrize("name", sorted(mrg.MODULE_CASES))
def test_project_checkers_reproduce_reference_module_fixture_bitwise(name):
    kind, kw = mrg.MODULE_CASES[name]
    inp, exp = _module_fixture(name)
    got = _project_module(kind, kw, inp)
    assert set(got) == set(exp)
    for k in sorted(exp):
        assert np.isfinite(exp[k]).all(), k
        _assert_identical(np.asarray(got[k]), exp[k], k)


@live
def test_only_surface_friction_init_needs_zero_filled_memory():
    """under the stand-in's NaN fill every module case above is finite (it reads nothing it did not write); surface_friction_init
    is the one exception: its mean density is summed into a fresh array.  The NaN reaches z0_est, and the
    clamp std::max(1e-5, std::min(1.0, z0)) turns it into 1.0 (std::min returns its first argument when the comparison with NaN
    fails): z0 is finite but wrong, so the test asserts that it departs from the zero-filled result"""
    import test_moist_surface_modules as tms
    kind, kw = mrg.MODULE_CASES["friction"]
    inp = mrg.module_inputs(kind, kw)
    nz, ny, nx, nens = inp["density_dry"].shape
    c = mrg._ref_coupler(inp, (nz, ny, nx, nens), tms.TRACER_SETS["kessler"])
    for n in ("sfc_mom_flx_u", "sfc_mom_flx_v"):
        c.register(n, [ny, nx, nens])
    for n in ("density_dry", "uvel", "vvel", "water_vapor", "gcm_uvel", "gcm_vvel"):
        c.write(n, inp[n])
    c.run("surface_friction_init", inp["tau"], inp["bflx"])
    _, exp = _module_fixture("friction")
    z0 = c.read("z0", (nens,))
    assert np.all(z0 == 1.0) and not np.array_equal(z0, exp["init_z0"]), (z0, exp["init_z0"])
    assert np.array_equal(c.read("sfc_bflx", (nens,)), inp["bflx"])
    for name, (kind, kw) in mrg.MODULE_CASES.items():
        if kind != "friction":
            out = mrg.run_module_reference(kind, kw, mrg.module_inputs(kind, kw))
            assert all(np.isfinite(v).all() for v in out.values()), name


@live
@pytest.mark.parametrize("name", sorted(mrg.MODULE_CASES))
def test_project_checkers_match_live_reference_modules(name):
    kind, kw = mrg.MODULE_CASES[name]
    inp = mrg.module_inputs(kind, kw)
    exp = mrg.run_module_reference(kind, kw, inp)
    got = _project_module(kind, kw, inp)
    for k in sorted(exp):
        _assert_identical(np.asarray(got[k]), exp[k], k)


def _gpu_module(kind, kw, inp):
    """the HIP module on the inputs `inp`, outputs keyed as the fixtures"""
    import torch
    from pam_amd import modules
    if kind == "supercell":
        c = idz.CONSTS_DEFAULT
        got = modules.supercell_init(torch.from_numpy(np.ascontiguousarray(inp["zint"])).to("cuda:0"), c["R_d"], c["R_v"], c["grav"])
        torch.cuda.synchronize()
        return dict(zip(("rho_d", "uvel", "vvel", "wvel", "temp", "rho_v"), (g.cpu().numpy() for g in got)))
    if kind == "kessler":
        import test_micro_kessler as tk
        nz, ny, nx, nens = inp["temp"].shape
        s = {k: np.array(inp[k]) for k in ("rho_v", "rho_c", "rho_r", "rho_dry", "temp")}
        got, _, _, _ = tk._gpu_run(s, inp["zint"], nens, nx, ny, nz, kw["dt"])
        return got
    if kind == "sponge":
        from pam_amd import PamCoupler
        nz, ny, nx, nens = inp["density_dry"].shape
        tr = idz.TRACERS_KESSLER_SHOC
        coupler = PamCoupler("cuda:0")
        coupler.set_option("crm_dt", 2.0)
        coupler.set_option("sponge_num_layers", 4)
        coupler.set_option("sponge_time_scale", 30.0)
        coupler.allocate_coupler_state(nz, ny, nx, nens)
        coupler.set_grid(nx * 500.0, ny * 500.0, inp["zint"])
        for n, p, m in tr:
            coupler.add_tracer(n, "", p, m)
        coupler.load_fields({k: np.array(inp[k]) for k in mrg.FIELD5 + ("tracers",)})
        coupler.run_module("sponge_layer", modules.sponge_layer)
        torch.cuda.synchronize()
        got = coupler.dump_fields()
        return {k: got[k] for k in mrg.FIELD5 + ("tracers",)}
    if kind == "gcm":
        import test_modules as tm
        crm = {n: np.array(inp[n]) for n in ao.GCM_FORCING_CRM}
        gcm = {n: np.array(inp[n]) for n in ao.GCM_FORCING_GCM}
        coupler, dm, _ = tm._gcm_gpu_coupler(crm, gcm, np.diff(inp["zint"], axis=0), mrg.GCM_DT, mrg.GCM_CRM_DT)
        coupler.run_module("compute_gcm_forcing_tendencies", modules.compute_gcm_forcing_tendencies)
        out = {"computed_" + n: dm.get(n, readonly=True).cpu().numpy() for n in ao.GCM_FORCING_TEND
               if n[-5:] not in ("rho_v", "rho_l", "rho_i")}
        for _ in range(mrg.GCM_APPLICATIONS):
            coupler.run_module("apply_gcm_forcing_tendencies", modules.apply_gcm_forcing_tendencies)
        torch.cuda.synchronize()
        out.update({n: dm.get(n, readonly=True).cpu().numpy() for n in ao.GCM_FORCING_CRM + ao.GCM_FORCING_TEND})
        return out
    if kind == "satadj":
        import test_moist_surface_modules as tms
        tr = tms.TRACER_SETS[kw["micro"]]
        f = {n: np.array(inp[n]) for n in ["density_dry", "temp"] + [t[0] for t in tr]}
        c = tms._coupler(tr, f, kw["micro"], zint=inp["zint"])
        c.run_module("saturation_adjustment", modules.saturation_adjustment)
        torch.cuda.synchronize()
        return tms._dump(c, list(f))
    if kind == "friction":
        import test_moist_surface_modules as tms
        f = {k: np.array(v) for k, v in inp.items() if k not in ("tau", "bflx", "zint")}
        got = tms._friction_run(tms.TRACER_SETS["kessler"], f, inp["tau"], inp["bflx"], inp["zint"])
        out = {"init_" + k: v for k, v in got["init"].items()}
        out.update(got["compute"][0])
        return out
    raise ValueError(kind)


def _assert_module_close(kind, kw, inp, got, exp):
    """HIP against the reference at the tolerances the module's own GPU tests use (tests/test_modules.py, test_micro_kessler.py,
    test_moist_surface_modules.py): device libm and slot sums make the last bits differ, so every bound is relative to the field's
    maximum -- or, for the GCM tendencies and the diagnosed density forcing, to the state they are made from"""
    for k in sorted(exp):
        e, g = exp[k], np.asarray(got[k])
        assert g.shape == e.shape, k
        scale = np.abs(e).max()
        if kind == "supercell":
            tol = 1e-13 * max(scale, 1e-300)
        elif kind == "gcm" and "tend" in k:
            # a tendency is (gcm - mean)/dt_gcm: its round-off scales with the state, not with the (small) difference
            tol = (1e-14 if k.startswith("computed_") else 1e-13) * max(np.abs(inp[n]).max() for n in ao.GCM_FORCING_GCM) / mrg.GCM_DT
        elif kind == "satadj" and k in ("water_vapor", "temp", "cloud_liquid", "cloud_water"):
            import moist_surface_ref as msr
            import test_moist_surface_modules as tms
            tr = tms.TRACER_SETS[kw["micro"]]
            c = mrg.SATADJ_CONSTS
            _, info = msr.saturation_adjustment({n: inp[n] for n in ["density_dry", "temp"] + [t[0] for t in tr]}, tr, kw["micro"],
                                                c["R_v"], c["cp_d"], c["cp_v"])
            exempt = info["margin"].reshape(e.shape) < 1e-12     # a bisection decision within 1e-12 of its root may flip
            allow = 2 * msr.TOL * (2.6e6 / (0.5 * c["cp_d"]) if k == "temp" else 1.0)
            err = np.abs(g - e)
            assert np.all(err[~exempt] <= 1e-12 * scale), (k, err[~exempt].max())
            assert np.all(err[exempt] <= allow + 1e-12 * scale), k
            continue
        elif kind == "satadj" or kind == "broadcast":
            tol = 0.0                       # fields the module does not adjust: untouched
        else:
            tol = 1e-12 * max(scale, 1e-300)
        assert np.isfinite(g).all(), k
        assert np.abs(g - e).max() <= tol, (k, np.abs(g - e).max(), tol)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(n for n, (kind, _) in mrg.MODULE_CASES.items() if kind != "broadcast"))
def test_gpu_module_matches_reference_fixture(name):
    kind, kw = mrg.MODULE_CASES[name]
    inp, exp = _module_fixture(name)
    _assert_module_close(kind, kw, inp, _gpu_module(kind, kw, inp), exp)


RAGGED = [(1, 1, 1), (63, 5, 1), (65, 5, 3), (130, 3, 5)]     # (nens, nx, ny): ragged member counts, nx*ny = 1, 5, 15, 15


@pytest.mark.gpu
@pytest.mark.skipif(not pam_ref.available(), reason="oracle/_ref/ did not travel")
@pytest.mark.parametrize("shape", RAGGED, ids=["%dx%dx%d" % s for s in RAGGED])
@pytest.mark.parametrize("name", ["sponge", "gcm_plain", "gcm_starve_liquid", "satadj_kessler", "satadj_p3", "friction"])
def test_gpu_module_matches_live_reference_ragged(name, shape):
    kind, kw = mrg.MODULE_CASES[name]
    nens, nx, ny = shape
    kw = dict(kw, nens=nens, nx=nx, ny=ny)
    inp = mrg.module_inputs(kind, kw)
    exp = mrg.run_module_reference(kind, kw, inp)
    _assert_module_close(kind, kw, inp, _gpu_module(kind, kw, inp), exp)
