"""examples/driver --yaml with the full flag set of the native CRM loop against the same run rebuilt from the Python classes, bit for bit:
both sit on the same C ABI, so what this holds is the driver's plumbing: which option every flag sets, the order of the inits and of the
calls, and that nothing depends on where the host synchronises.  Two grids (vcoords : uniform): 3-D in flat lanes with the TKE closure,
2-D in member lanes with ESMT and the Smagorinsky closure.  The supercell sounding stays cloud-free for three steps, so the ice branches
are not what is tested here (tests/test_crm_loop_gpu.py carries those).

The 3-D grid is (nz,ny,nx) = (12,5,6): pam_amd_hyperdiffusion refuses 1 < ny < 5, as in tests/crm_loop_ref.py."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
STEPS, DT, ZLEN = 3, 2.0, 12000.0
GRIDS = {
    # name: (nz, ny, nx, nens, closure)
    "3d_flat_tke": (12, 5, 6, 3, "tke"),
    "2d_members_esmt_smag": (12, 1, 9, 66, "smag"),
}
CS, CK, PRANDTL, COSZEN, SST, DEPTH, FCOR, TAU, EVERY = "0.2", "0.1", "0.333", "0.8", "300", "1.0", "1e-4", "600", "2"


def _profiles(nz):
    """the rows of the --ls-forcing file that are given (the others are all NaN: absent)"""
    z = (np.arange(nz) + 0.5) / nz
    return dict(wsub=-0.02 * np.sin(np.pi * z), temp_tend=-2.0e-5 * (1.0 - z), qv_tend=2.0e-8 * (1.0 - z), ug=4.0 + 12.0 * z, vg=-3.0 + 2.0 * z,
                nudge_u=4.0 + 12.0 * z, nudge_v=-3.0 + 2.0 * z, nudge_rate_uv=np.full(nz, 1.0 / 1800.0))


ROWS = ("wsub", "temp_tend", "qv_tend", "ug", "vg", "nudge_temp", "nudge_qv", "nudge_u", "nudge_v", "nudge_rate_temp", "nudge_rate_qv",
        "nudge_rate_uv")


def _inputs(tmp_path, grid, steps=STEPS):
    nz, ny, nx, nens, closure = GRIDS[grid]
    xlen = nx * 500.0
    ylen = ny * 800.0 if ny > 1 else xlen
    yml = tmp_path / "loop.yaml"
    yml.write_text("sim_time : %g\ncrm_nx : %d\ncrm_ny : %d\nnens : %d\nvcoords : uniform\ncrm_nz : %d\nzlen : %g\nxlen : %g\nylen : %g\n"
                   "dt_gcm : %g\ndt_crm_phys : %g\nout_freq : %g\n" % (steps * DT, nx, ny, nens, nz, ZLEN, xlen, ylen, steps * DT, DT, DT))
    prof = _profiles(nz)
    ls = tmp_path / "ls.bin"
    np.stack([prof.get(r, np.full(nz, np.nan)) for r in ROWS]).astype("<f8").tofile(str(ls))
    flags = ["--micro-ice", "--sgs-horizontal", "--sgs-moist", "--radiation-gray", EVERY, "--shortwave", COSZEN, "--surface", SST, DEPTH,
             "--ls-forcing", str(ls), "--coriolis", FCOR, "--hyperdiff", TAU]
    flags += ["--sgs-tke", CS, CK] if closure == "tke" else ["--sgs-smag", CS, PRANDTL, "--esmt"]
    return yml, flags, prof, xlen, ylen


def _driver(yml, nens, flags, out, *more):
    r = subprocess.run([DRIVER, "--yaml", str(yml), "--nens", str(nens)] + list(flags) + list(more) + [str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return r


ACCEL, VT_RATE, RAD_NX, RAD_NY, ACCEL_STEPS = 2.0, 1.0e-4, 3, 1, 6


def _python_loop(grid, prof, xlen, ylen, steps=STEPS, handoff=False, every=int(EVERY), horizontal=True):
    """the driver's run from the Python classes: the options its flags are documented to set (the header comment of examples/driver.cpp),
    the inits and the calls in its order.  -> the names of the output file's fields, the initial fields, the final ones, precl.
    handoff: the run of --accelerate 2 --accel-uv --vt 1e-4 --gcm-handoff 3 1 --column-diag --flux-profiles, the CRM loop on the clock and
    every one of those modules called where the driver calls it, with the step's weight"""
    import torch
    from pam_amd import Dycore, MicrophysicsIce, PamCoupler, RadiationGray, SGSSmagorinsky, SGSTke, modules
    nz, ny, nx, nens, closure = GRIDS[grid]
    dz = ZLEN / (nz - 1)
    zint = np.array([0.0] + [k * dz - dz / 2 for k in range(1, nz)] + [ZLEN])
    c = PamCoupler("cuda:0")
    c.set_option("gcm_physics_dt", steps * DT)
    c.set_option("crm_dt", DT)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(xlen, ylen, zint)
    micro = MicrophysicsIce()
    micro.init(c)
    if closure == "tke":
        sgs = SGSTke(cs=float(CS), ck=float(CK), moist=True, surface_fluxes=True, horizontal=horizontal)
    else:
        sgs = SGSSmagorinsky(cs=float(CS), prandtl=float(PRANDTL), moist=True, surface_fluxes=True)
        sgs.horizontal = horizontal
    sgs.init(c)
    if closure == "smag":
        modules.esmt_init(c)
    dycore = Dycore()
    dycore.init(c)
    c.set_option("rad_gray_every", every)
    rad = RadiationGray().shortwave(coszen=float(COSZEN), albedo=0.07)
    rad.init(c)
    dm = c.get_data_manager_device_readwrite()
    cols = modules.supercell_init(torch.from_numpy(zint).to("cuda:0"), c.get_option("R_d"), c.get_option("R_v"), c.get_option("grav"))
    for name, col in zip(("gcm_density_dry", "gcm_uvel", "gcm_vvel", "gcm_wvel", "gcm_temp", "gcm_water_vapor"), cols):
        dm.get(name).copy_(col[:, None].expand(nz, nens))
    modules.broadcast_initial_gcm_column(c)
    keep = modules.perturb_temperature(c, np.zeros(nens, dtype=np.int32), 0.1)
    if handoff:
        c.set_option("crm_accel_factor", ACCEL)
        c.set_option("crm_accel_uv", True)
        c.set_option("crm_accel_max_ttend", 5.0)
    modules.hyperdiffusion_init(c, float(TAU))
    if handoff:
        c.set_option("rad_nx", RAD_NX)
        c.set_option("rad_ny", RAD_NY)
        modules.crm_feedback_init(c)
        c.set_option("crm_vt_u", False)
        c.set_option("crm_vt_scale_limit", 0.05)
    modules.surface_fluxes_init(c, sst=float(SST), slab_depth=float(DEPTH))
    modules.ls_forcing_init(c, fcor=float(FCOR), **prof)
    if closure == "smag":
        modules.esmt_set(c, "crm")
    names = ["density_dry", "uvel", "vvel", "wvel", "temp"] + c.get_tracer_names()
    torch.cuda.synchronize()
    first = [dm.get(n, readonly=True).cpu().numpy() for n in names]
    dycore.declare_current_profile_as_hydrostatic(c)
    clock = modules.MsaClock(steps, ACCEL if handoff else 0.0)
    if handoff:
        modules.msa_init(c)
        modules.vt_init(c)
        for q in ("t", "q"):      # no GCM: the variance tendency is a relative growth rate of the starting variance
            dm.get("vt_tend_" + q).copy_(VT_RATE * dm.get("vt_var_start_" + q, readonly=True))
        modules.rad_aggregate_init(c)
        modules.column_diagnostics_init(c)
        modules.flux_profiles_init(c)
    crm_steps = 0
    while not clock.done():
        accel = clock.accelerating()
        if accel:
            modules.msa_diagnose(c)
        rad.timeStep(c)
        dycore.timeStep(c)
        modules.sponge_layer(c)
        modules.ls_forcing(c)
        if closure == "smag":
            modules.esmt_pgf(c, forcing=False)
        modules.surface_fluxes(c)
        modules.hyperdiffusion(c)
        sgs.timeStep(c)
        micro.timeStep(c)
        cease = modules.msa_accelerate(c) if accel else False
        weight = clock.advance(cease)
        if handoff:
            modules.vt_apply_forcing(c, weight * DT)
            modules.rad_aggregate(c, weight)
            modules.column_diagnostics(c, weight)
            modules.flux_profiles(c, weight)
        crm_steps += 1
    if handoff:
        modules.vt_compute_feedback(c)
        modules.compute_crm_feedback(c)
    torch.cuda.synchronize()
    last = [dm.get(n, readonly=True).cpu().numpy() for n in names]
    precl = dm.get("precl", readonly=True).cpu().numpy()
    extra = {n: dm.get(n, readonly=True).cpu().numpy() for n in ("sfc_temp", "tk", "rad_sw_heating")}
    if handoff:
        extra = {n: e["data"].cpu().numpy() for n, e in dm._e.items()}
        extra["crm_steps"] = crm_steps
    dycore.finalize(c)
    del keep
    return names, first, last, precl, extra


def _read(path, names, shape):
    nz, ny, nx, nens = shape
    raw = np.fromfile(str(path), dtype="<f8")
    ncell = nz * ny * nx * nens
    fields = [raw[i * ncell:(i + 1) * ncell].reshape(shape) for i in range(len(names))]
    return fields, raw[len(names) * ncell:]


@pytest.mark.parametrize("grid", tuple(GRIDS))
def test_driver_with_the_full_flag_set_equals_the_python_loop_bit_for_bit(tmp_path, grid):
    """--micro-ice, --sgs-tke or --sgs-smag with --esmt, --sgs-horizontal --sgs-moist, --radiation-gray 2 --shortwave 0.8, --surface 300
    1.0, --ls-forcing FILE --coriolis 1e-4, --hyperdiff 600 for three steps: the state --dump-init writes equals the Python loop's initial
    state, the output file equals its final fields and precl, both bit for bit; and the same run with --sync writes the same bytes"""
    nz, ny, nx, nens, closure = GRIDS[grid]
    shape = (nz, ny, nx, nens)
    yml, flags, prof, xlen, ylen = _inputs(tmp_path, grid)
    out, init, synced = tmp_path / "out.bin", tmp_path / "init.bin", tmp_path / "sync.bin"
    flags = ["--steps", str(STEPS)] + flags
    r = _driver(yml, nens, flags, out, "--dump-init", str(init))
    assert r.stdout.count("Etime , dtphys, maxw:") == STEPS
    names, first, last, precl, extra = _python_loop(grid, prof, xlen, ylen)
    assert names[5:10] == ["water_vapor", "cloud_liquid", "cloud_ice", "precip_liquid", "precip_ice"]
    assert names[10:] == (["tke"] if closure == "tke" else ["esmt_u", "esmt_v"])
    got, rest = _read(init, names, shape)
    assert rest.size == 0
    bad = [n for n, a, b in zip(names, got, first) if a.tobytes() != np.ascontiguousarray(b).tobytes()]
    assert bad == [], ("initial state", bad)
    got, rest = _read(out, names, shape)
    bad = [n for n, a, b in zip(names, got, last) if a.tobytes() != np.ascontiguousarray(b).tobytes()]
    assert bad == [], ("final state", bad)
    assert rest.tobytes() == np.ascontiguousarray(precl).tobytes()
    # the run did something in every part the flags switch on
    # (no condensate forms in three steps; esmt_v starts as rho times the level mean of the 2-D run's vvel, zero, and takes a force that
    # is proportional to the gradient of its own level mean)
    still = ("cloud_liquid", "cloud_ice", "precip_liquid", "precip_ice", "esmt_v")
    moved = [n for n, a, b in zip(names, first, last) if a.tobytes() == b.tobytes() and n not in still]
    assert moved == [], moved
    assert np.abs(extra["sfc_temp"] - float(SST)).max() > 0 and extra["tk"].max() > 0 and extra["rad_sw_heating"].max() > 0
    # the comparison sees the plumbing: the Python loop with one option other than the flag's differs from the driver's file
    for wrong in (dict(every=1), dict(horizontal=False)):
        other = _python_loop(grid, prof, xlen, ylen, **wrong)[2]
        assert any(a.tobytes() != np.ascontiguousarray(b).tobytes() for a, b in zip(got, other)), wrong
    _driver(yml, nens, flags, synced, "--sync")
    assert open(str(synced), "rb").read() == open(str(out), "rb").read()


def _values_equal(got, entry):
    """a JSON value against a DataManager entry: every number printed with %.17g reads back as the double it was (the text carries no
    sign of a zero, so values are compared, not bytes)"""
    return np.array_equal(np.asarray(got, dtype=np.float64).reshape(entry.shape), entry)


def test_accelerated_driver_run_with_the_handoff_modules_equals_the_python_loop(tmp_path):
    """the 3-D grid, six CRM steps of model time in one GCM step, with --accelerate 2 --accel-uv, --vt 1e-4, --gcm-handoff 3 1,
    --column-diag and --flux-profiles beside the full flag set: the state file equals the Python loop's fields and precl bit for bit, and
    every number of the four JSON files equals the entry the Python loop holds (msa_*, vt_*, rad_aggregate, compute_crm_feedback,
    column_diagnostics and flux_profiles called where the driver calls them, with the clock's weight)"""
    import json
    grid = "3d_flat_tke"
    nz, ny, nx, nens, closure = GRIDS[grid]
    shape = (nz, ny, nx, nens)
    yml, flags, prof, xlen, ylen = _inputs(tmp_path, grid, ACCEL_STEPS)
    out, init = tmp_path / "out.bin", tmp_path / "init.bin"
    paths = {n: tmp_path / (n + ".json") for n in ("vt", "handoff", "coldiag", "fluxprof")}
    more = ["--accelerate", "%g" % ACCEL, "--accel-uv", "--vt", "%g" % VT_RATE, str(paths["vt"]), "--gcm-handoff", str(RAD_NX), str(RAD_NY),
            str(paths["handoff"]), "--column-diag", str(paths["coldiag"]), "--flux-profiles", str(paths["fluxprof"]), "--dump-init", str(init)]
    _driver(yml, nens, flags, out, *more)
    names, first, last, precl, E = _python_loop(grid, prof, xlen, ylen, ACCEL_STEPS, handoff=True)
    assert 1 <= E["crm_steps"] < ACCEL_STEPS          # the clock ran: fewer CRM steps than the model time counts
    got, rest = _read(init, names, shape)
    assert [n for n, a, b in zip(names, got, first) if a.tobytes() != np.ascontiguousarray(b).tobytes()] == []
    got, rest = _read(out, names, shape)
    assert [n for n, a, b in zip(names, got, last) if a.tobytes() != np.ascontiguousarray(b).tobytes()] == []
    assert rest.tobytes() == np.ascontiguousarray(precl).tobytes()
    vt = json.loads(paths["vt"].read_text().strip())
    for what in ("var_start", "var", "feedback"):
        assert sorted(vt[what]) == ["q", "t"]
        for q, v in vt[what].items():
            assert _values_equal(v, E["vt_%s_%s" % (what, q)]), (what, q)
    assert np.abs(E["vt_feedback_t"]).max() > 0
    col = json.loads(paths["coldiag"].read_text().strip())
    assert col["crm_steps"] == E["crm_steps"] and {"diag_pw", "diag_precip_liq", "diag_precip_ice", "diag_iwp"} <= set(col["diagnostics"])
    for n, v in col["diagnostics"].items():
        assert _values_equal(v, E[n]), n
    prf = json.loads(paths["fluxprof"].read_text().strip())
    assert prf["crm_steps"] == E["crm_steps"] and {"prof_flux_t", "prof_tke", "prof_cld"} <= set(prf["profiles"])
    for n, v in prf["profiles"].items():
        assert _values_equal(v, E[n]), n
    assert np.abs(E["prof_flux_t"]).max() > 0
    hand = json.loads(paths["handoff"].read_text())["gcm_steps"]
    assert len(hand) == 1 and hand[0]["crm_steps"] == E["crm_steps"]
    assert {"rad_temperature", "rad_qv", "rad_qc", "rad_qi", "rad_cld"} == set(hand[0]["aggregates"])
    for n, v in hand[0]["aggregates"].items():
        assert _values_equal(v, E[n]), n
    assert len(hand[0]["feedback"]) == 12
    for n, v in hand[0]["feedback"].items():
        assert _values_equal(v, E["crm_feedback_" + n]), n
