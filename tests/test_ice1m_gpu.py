"""The one-moment ice microphysics on the GPU: pam_amd_ice1m_time_step against the numpy restatement (tests/ice1m_ref.py) bit for bit (a
NaN by its place) on every shape and named case, with the narrow and with the wide index, and run to run; members split over calls
against the whole; bystanders and read-only inputs; MicrophysicsIce through a coupler; the modules that read ice on a coupler that
holds some, each against its own restatement fed cloud_ice; the C++ class through tests/cxx/ice_micro; and examples/driver --micro-ice
on a shortened CI input."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ice1m_ref as ref
import ice1m_cases as ic
from ice1m_harness import GpuBackend, POISON, run_split
from tools.native_build import cxx_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")


@pytest.mark.gpu
@pytest.mark.parametrize("wide", (False, True), ids=("narrow", "wide"))
@pytest.mark.parametrize("shape", ic.SHAPES, ids=ref.shape_id)
def test_gpu_matches_restatement_bit_for_bit(shape, wide):
    """every named case; one case twice: two runs are identical; the rates were poisoned before the call"""
    be = GpuBackend(wide)
    for name in ic.CASE_NAMES:
        got = be.run(ic.cases(shape)[name])
        assert ref.results_differ(got, ic.reference(shape, name), nan_by_place=True) == [], name
        assert not (got["precl"] == POISON).any() and not (got["preci"] == POISON).any(), name
    a, b = (be.run(ic.cases(shape)["deep_fall"]) for _ in range(2))
    assert ref.results_differ(a, b) == []


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in ic.SHAPES if s[3] >= 64], ids=ref.shape_id)
def test_gpu_members_split_over_calls_equal_the_whole(shape):
    be = GpuBackend()
    for name in ("mixed_a", "deep_fall", "nan_cell"):
        got = run_split(be, ic.cases(shape)[name], (0, 1, 37, shape[3]))
        assert ref.results_differ(got, ic.reference(shape, name), nan_by_place=True) == [], name


@pytest.mark.gpu
def test_gpu_bystanders_and_read_only_inputs_keep_their_bits():
    import torch
    shape = (7, 3, 2, 65)
    before = torch.full((4096,), 3.25, dtype=torch.float64, device="cuda:0")
    be = GpuBackend()
    for name in ("mixed_a", "deep_fall"):
        case = ic.cases(shape)[name]
        out = be.run(case)
        after = torch.full((4096,), 3.25, dtype=torch.float64, device="cuda:0")
        assert ref.results_differ(out, ic.reference(shape, name)) == [], name
        assert ref.same_bits(be.last_inputs["density_dry"], case["fields"]["density_dry"]) and ref.same_bits(be.last_inputs["zint"], case["zint"])
        assert (before == 3.25).all() and (after == 3.25).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python class through a coupler

CONST = dict(grav=9.81, cp_d=1003.0, R_d=287.0, R_v=461.0)


def _coupler(shape, zint, dt):
    """a coupler initialised with MicrophysicsIce, its grid the case's"""
    import torch
    from pam_amd import PamCoupler, MicrophysicsIce
    nz, ny, nx, nens = shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", dt)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(nx * 500.0, ny * 500.0, zint[:, 0].copy())
    micro = MicrophysicsIce()
    micro.init(c)
    dm = c.get_data_manager_device_readwrite()
    dm.get("vertical_interface_height").copy_(torch.from_numpy(zint))
    dm.get("vertical_midpoint_height").copy_(torch.from_numpy(0.5 * (zint[:-1] + zint[1:])))
    return c, dm, micro


def _fill(dm, fields):
    import torch
    for n, v in fields.items():
        dm.get(n).copy_(torch.from_numpy(np.ascontiguousarray(v)))


def _read(dm, names):
    return {n: dm.get(n, readonly=True).cpu().numpy() for n in names}


@pytest.mark.gpu
def test_gpu_python_class_through_a_coupler():
    """init registers five positive mass-adding tracers in the contract's order, precl and preci, the option micro and Kessler's
    constants; timeStep gives the restatement's bits; the winds and density_dry keep theirs; compute_total_mass is the column sum"""
    import torch
    shape = (7, 3, 2, 65)
    for name in ("mixed_a", "deep_fall"):
        case = ic.cases(shape)[name]
        c, dm, micro = _coupler(shape, case["zint"], case["dt"])
        assert tuple(c.get_tracer_names()) == ref.SPECIES and all(c.get_tracer_info(n)[2] and c.get_tracer_info(n)[3] for n in ref.SPECIES)
        assert c.get_option("micro") == "ice1m" and dm.get_shape("precl") == list(shape[1:]) and dm.get_shape("preci") == list(shape[1:])
        assert [c.get_option(k) for k in ("R_d", "R_v", "cp_d", "cp_v", "grav", "p0")] == [287.0, 461.0, 1003.0, 1859.0, 9.81, 1.0e5]
        assert all(not dm.get(n).any() for n in ref.SPECIES + ("precl", "preci"))
        rng = np.random.default_rng(5)
        winds = {n: rng.random(shape) for n in ("uvel", "vvel", "wvel")}
        _fill(dm, dict(case["fields"], **winds))
        mass = micro.compute_total_mass(c)
        assert abs(mass - float(ref.column_water(case["fields"], case["zint"]).sum())) <= 1.0e-12 * mass
        micro.timeStep(c)
        torch.cuda.synchronize()
        want = ic.reference(shape, name)
        assert ref.results_differ(_read(dm, list(want)), want) == [], name
        held = dict(winds, density_dry=case["fields"]["density_dry"])
        assert ref.results_differ(_read(dm, list(held)), held) == [], name
        micro.finalize(c)


# ------------------------------------------------------------------------------------------------------------------------------
# the modules that read ice, on a coupler initialised with MicrophysicsIce and holding some: each against its own restatement fed
# cloud_liquid as the liquid and cloud_ice as the ice

CRM_DT, GCM_DT = 20.0, 240.0
MICRO = dict(R_d=287.0, R_v=461.0, cp_d=1003.0, grav=9.81)          # what MicrophysicsIce.init writes to the options


def _ice_coupler(shape, zint=None, **options):
    import torch
    from pam_amd import PamCoupler, MicrophysicsIce
    nz, ny, nx, nens = shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", CRM_DT)
    c.set_option("gcm_physics_dt", GCM_DT)
    for k, v in options.items():
        c.set_option(k, v)
    c.allocate_coupler_state(nz, ny, nx, nens)
    MicrophysicsIce().init(c)
    dm = c.get_data_manager_device_readwrite()
    if zint is not None:
        c.set_grid(nx * 500.0, ny * 500.0, zint[:, 0].copy())
        dm.get("vertical_interface_height").copy_(torch.from_numpy(zint))
        dm.get("vertical_midpoint_height").copy_(torch.from_numpy(0.5 * (zint[:-1] + zint[1:])))
    return c, dm


STATE_NAMES = dict(temp="temp", rho_d="density_dry", rho_v="water_vapor", rho_c="cloud_liquid", rho_i="cloud_ice", uvel="uvel", vvel="vvel",
                   wvel="wvel")


def _load_state(dm, f, shape=None):
    import torch
    for ours, theirs in STATE_NAMES.items():
        if f.get(ours) is not None:
            a = np.ascontiguousarray(f[ours])
            dm.get(theirs).copy_(torch.from_numpy(a if shape is None else a.reshape(shape)))


@pytest.mark.gpu
def test_gpu_radiation_gray_takes_cloud_ice():
    import torch
    import grayrad_ref
    import grayrad_cases
    from pam_amd import RadiationGray
    shape = (7, 3, 2, 65)
    base = grayrad_cases.cases(shape)["p3_set"]
    fields = dict(base["fields"], cloud_liquid=base["fields"]["cloud_water"], cloud_ice=base["fields"]["ice"])
    case = dict(base, fields=fields, liquid=("cloud_liquid",), ice=("cloud_ice",), cp_d=MICRO["cp_d"], dt=CRM_DT)
    assert fields["cloud_ice"].any()
    c, dm = _ice_coupler(shape, case["zint"])
    rad = RadiationGray(lw_down_top=case["lw_down_top"])
    rad.init(c)
    for n in ("temp", "density_dry", "water_vapor", "cloud_liquid", "cloud_ice"):
        dm.get(n).copy_(torch.from_numpy(fields[n]))
    rad.timeStep(c)
    torch.cuda.synchronize()
    want = grayrad_ref.radiation(case)
    assert grayrad_ref.results_differ(_read(dm, list(grayrad_ref.OUTPUTS)), want) == []
    without = grayrad_ref.radiation(dict(case, ice=()))
    assert not ref.same_bits(want["rad_olr"], without["rad_olr"])            # the ice is seen


@pytest.mark.gpu
def test_gpu_handoff_takes_cloud_ice():
    """rad_aggregate (rad_qi) and compute_crm_feedback (qi) after one CRM step"""
    import torch
    import rad_ref
    from pam_amd import modules
    config = ((3, 8, 8, 70), (2, 4))
    case = rad_ref.cases(config)["three_steps"]
    f = case["steps"][0][0]
    assert f["rho_i"].any()
    c, dm = _ice_coupler(config[0], rad_nx=4, rad_ny=2)
    modules.rad_aggregate_init(c)
    modules.crm_feedback_init(c)
    assert dm.entry_exists("rad_qi") and dm.entry_exists("crm_feedback_mean_qi") and dm.entry_exists("crm_feedback_tend_qi")
    _load_state(dm, f)
    for n, a in case["gcm"].items():
        dm.get(n).copy_(torch.from_numpy(a))
    modules.rad_aggregate(c, 1)
    modules.compute_crm_feedback(c)
    torch.cuda.synchronize()
    zeros = {x: np.zeros((3, 2, 4, 70)) for x in rad_ref.RAD}
    want = rad_ref.run_case(rad_ref.RefBackend(), dict(case, rad0=zeros, steps=[(dict(f, cldfrac=None), CRM_DT / GCM_DT * 1.0)]))
    for x in rad_ref.RAD:
        assert rad_ref.same_bits(dm.get("rad_" + x, readonly=True).cpu().numpy(), want["rad"][x]), x
    for q in rad_ref.QUANTITIES:
        for what in ("mean", "tend"):
            assert rad_ref.same_bits(dm.get("crm_feedback_%s_%s" % (what, q), readonly=True).cpu().numpy(), want[what][q]), (what, q)
    assert want["rad"]["qi"].any()


@pytest.mark.gpu
def test_gpu_column_diagnostics_take_cloud_ice_and_preci():
    import torch
    import coldiag_ref
    from pam_amd import modules
    config = (4, 8, 8, 65)
    cs = coldiag_ref.cases(config)
    f, p = cs["base"]["steps"][0][:2]
    f = dict(f, cldfrac=None)
    assert f["rho_i"].any() and p["precip_ice"].any()
    c, dm = _ice_coupler(config)
    dm.get("vertical_interface_height").copy_(torch.from_numpy(cs["base"]["zint"]))
    modules.column_diagnostics_init(c)
    assert all(dm.entry_exists("diag_" + x) for x in coldiag_ref.OUT)
    _load_state(dm, f)
    dm.get("precl").copy_(torch.from_numpy(p["precip_liq"]))
    dm.get("preci").copy_(torch.from_numpy(p["precip_ice"]))
    modules.column_diagnostics(c, 1)
    torch.cuda.synchronize()
    params = dict(coldiag_ref.PARAMS, R_d=MICRO["R_d"], R_v=MICRO["R_v"])
    want = coldiag_ref.run_case(coldiag_ref.RefBackend(), dict(zint=cs["base"]["zint"], params=params, out0={x: np.zeros(65) for x in coldiag_ref.OUT},
                                                               steps=[(f, p, CRM_DT / GCM_DT * 1.0)]))
    for x in coldiag_ref.OUT:
        assert coldiag_ref.same_bits(dm.get("diag_" + x, readonly=True).cpu().numpy(), want[x]), x
    assert (want["iwp"] > 0).all() and (want["precip_ice"] > 0).any()


@pytest.mark.gpu
def test_gpu_flux_profiles_take_cloud_ice():
    import torch
    import fluxprof_ref
    from pam_amd import modules
    config = (4, 8, 8, 65)
    f = fluxprof_ref.cases(config)["base"]["steps"][0][0]
    assert f["rho_i"].any()
    c, dm = _ice_coupler(config)
    modules.flux_profiles_init(c)
    assert all(dm.entry_exists("prof_" + x) for x in fluxprof_ref.OUT)
    _load_state(dm, f)
    modules.flux_profiles(c, 1)
    torch.cuda.synchronize()
    case = dict(qc=1.0e-5, out0={x: np.zeros((4, 65)) for x in fluxprof_ref.OUT}, steps=[(f, CRM_DT / GCM_DT * 1.0)])
    want = fluxprof_ref.run_case(fluxprof_ref.RefBackend(), case)
    for x in fluxprof_ref.OUT:
        assert fluxprof_ref.same_bits(dm.get("prof_" + x, readonly=True).cpu().numpy(), want[x]), x
    without = fluxprof_ref.run_case(fluxprof_ref.RefBackend(), dict(case, steps=[(dict(f, rho_i=None), CRM_DT / GCM_DT * 1.0)]))
    assert not fluxprof_ref.same_bits(want["flux_qt"], without["flux_qt"])    # the ice is seen


MSA_NAMES = dict(temp="temp", water_vapor="water_vapor", cloud="cloud_liquid", ice="cloud_ice", uvel="uvel", vvel="vvel")


def _load_named(dm, st, names, shape):
    import torch
    for ours, theirs in names.items():
        if st.get(ours) is not None:
            dm.get(theirs).copy_(torch.from_numpy(np.ascontiguousarray(st[ours]).reshape(shape)))


@pytest.mark.gpu
def test_gpu_mean_state_acceleration_takes_cloud_ice():
    import torch
    import msa_ref
    from pam_amd import modules
    shape = ((3, 4, 5), 65)
    full = shape[0] + (shape[1],)
    case, want = msa_ref.cases(shape)["base"], msa_ref.reference(shape, "base")
    assert case["after"]["ice"].any()
    c, dm = _ice_coupler(full, crm_accel_factor=case["a"], crm_accel_uv=case["accel_uv"])
    modules.msa_init(c)
    _load_named(dm, case["before"], MSA_NAMES, full)
    modules.msa_diagnose(c)
    _load_named(dm, case["after"], MSA_NAMES, full)
    assert modules.msa_accelerate(c) == bool(want["cease"])
    torch.cuda.synchronize()
    for ours, theirs in MSA_NAMES.items():
        assert msa_ref.same_bits(dm.get(theirs, readonly=True).cpu().numpy().reshape(want["fields"][ours].shape), want["fields"][ours]), ours
    for q in msa_ref.QUANTITIES:
        assert msa_ref.same_bits(dm.get("accel_tend_" + q, readonly=True).cpu().numpy(), want["tend"][q]), q


@pytest.mark.gpu
def test_gpu_variance_transport_takes_cloud_ice():
    import torch
    import vt_ref
    from pam_amd import modules
    shape = ((3, 4, 5), 65)
    full = shape[0] + (shape[1],)
    case, want = vt_ref.cases(shape)["base"], vt_ref.reference(shape, "base")
    names = {k: v for k, v in MSA_NAMES.items() if k != "vvel"}
    assert case["now"]["ice"].any()
    c, dm = _ice_coupler(full, crm_vt_u=True)
    _load_named(dm, case["start"], names, full)
    modules.vt_init(c)
    qs = vt_ref.quantities(True)
    for q in qs:
        assert vt_ref.same_bits(dm.get("vt_var_start_" + q, readonly=True).cpu().numpy(), want["var_start"][q]), q
        dm.get("vt_tend_" + q).copy_(torch.from_numpy(case["tend"][q]))
    _load_named(dm, case["now"], names, full)
    modules.vt_apply_forcing(c)
    modules.vt_compute_feedback(c)
    torch.cuda.synchronize()
    for ours, theirs in names.items():
        if want["fields"].get(ours) is not None:
            assert vt_ref.same_bits(dm.get(theirs, readonly=True).cpu().numpy().reshape(want["fields"][ours].shape), want["fields"][ours]), ours
    for q in qs:
        assert vt_ref.same_bits(dm.get("vt_feedback_" + q, readonly=True).cpu().numpy(), want["feedback"][q]), q


@pytest.mark.gpu
def test_gpu_moist_smagorinsky_takes_the_five_species():
    """cloud = cloud_liquid, cloud_ice; precip = precip_liquid, precip_ice; every one of the five tracers is diffused"""
    import torch
    import sgs_moist_ref as mref
    from pam_amd import SGSSmagorinsky
    shape = (7, 3, 5, 130)
    nz, ny, nx, nens = shape
    base = mref.cases(shape)["p3_set"]
    bf = base["fields"]
    fields = {n: a for n, a in bf.items() if n not in mref.CONDENSATE}
    fields.update(cloud_liquid=bf["cloud_water"], cloud_ice=bf["ice"], precip_liquid=bf["rain"], precip_ice=bf["precip_liquid"])
    case = dict(base, fields=fields, tracers=ref.SPECIES, cloud=("cloud_liquid", "cloud_ice"), precip=("precip_liquid", "precip_ice"),
                latvap=2501000.0, **MICRO)
    assert fields["cloud_ice"].any() and fields["precip_ice"].any()
    want = mref.run_case(mref.RefBackend(), case)
    from pam_amd import PamCoupler, MicrophysicsIce
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", case["dt"])
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(nx * case["dx"], ny * case["dy"], case["zint"][:, 0].copy())
    MicrophysicsIce().init(c)
    sgs = SGSSmagorinsky(moist=True)
    sgs.init(c)
    dm = c.get_data_manager_device_readwrite()
    for n in ("uvel", "vvel", "wvel", "temp", "density_dry") + ref.SPECIES:
        dm.get(n).copy_(torch.from_numpy(fields[n]))
    dm.get("vertical_interface_height").copy_(torch.from_numpy(case["zint"]))
    dm.get("vertical_midpoint_height").copy_(torch.from_numpy(case["zmid"]))
    for entry, key in (("sfc_mom_flx_u", "sfc_flx_u"), ("sfc_mom_flx_v", "sfc_flx_v")):
        dm.get(entry).copy_(torch.from_numpy(case[key]))
    sgs.timeStep(c)
    torch.cuda.synchronize()
    assert mref.results_differ(_read(dm, list(want)), want) == []
    dry = mref.run_case(mref.RefBackend(), dict(case, cloud=("cloud_liquid",)))
    assert not mref.same_bits(want["tk"], dry["tk"])                          # the ice is seen


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ class through tests/cxx/ice_micro, and through the driver

@pytest.mark.gpu
@pytest.mark.parametrize("name", ("mixed_a", "deep_fall"))
def test_gpu_cxx_class_matches_restatement(tmp_path, name):
    shape = (7, 3, 2, 65)
    nz, ny, nx, nens = shape
    case = ic.cases(shape)[name]
    path, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("4i", nz, ny, nx, nens))
        for a in [np.array([case["dt"]]), case["zint"]] + [case["fields"][n] for n in ("density_dry", "temp") + ref.SPECIES]:
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([cxx_program("ice_micro"), str(path), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert re.search(r"### tracers (.*)", r.stdout).group(1).split() == list(ref.SPECIES)
    assert re.search(r"### micro (.*)", r.stdout).group(1).split() == ["ice1m", "ice1m"]
    assert re.search(r"### constants (.*)", r.stdout).group(1).split() == ["287", "461", "1003", "1859", "9.81", "100000"]
    raw = np.fromfile(out, dtype=np.float64)
    n4, n3 = nz * ny * nx * nens, ny * nx * nens
    got = dict(zip(ref.WRITTEN, raw[:6 * n4].reshape((6,) + shape)))
    got["precl"], got["preci"] = raw[6 * n4:6 * n4 + n3].reshape(shape[1:]), raw[6 * n4 + n3:6 * n4 + 2 * n3].reshape(shape[1:])
    want = ic.reference(shape, name)
    assert ref.results_differ(got, want) == []
    assert ref.same_bits(raw[6 * n4 + 2 * n3:].reshape(shape), case["fields"]["density_dry"])
    before, after = (float(v) for v in re.search(r"### mass (\S+) (\S+)", r.stdout).groups())
    total = lambda F: float(ref.column_water(F, case["zint"]).sum())
    assert abs(before - total(case["fields"])) <= 1e-12 * before and abs(after - total(want)) <= 1e-12 * before


ICE_LINE = r"micro ice: etime (\S+) , iwp (\S+) , precl (\S+) , preci (\S+) , water (\S+) , water_start (\S+) , precipitated (\S+)"


@pytest.mark.gpu
def test_gpu_driver_runs_the_scheme_and_its_water_budget_closes(tmp_path):
    """--micro-ice on a shortened CI input: every field finite, one "micro ice:" line per output step, the five tracers in the output, and
    water + precipitated == water_start to 1e-10 relative, the reference's own runtime mass tolerance"""
    out = tmp_path / "ice.bin"
    r = subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3", "--micro-ice", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert "Micro : ice1m" in lines
    rows = [re.fullmatch(ICE_LINE, l) for l in lines if l.startswith("micro ice:")]
    assert rows and all(rows) and len(rows) == sum(l.startswith("Etime ,") for l in lines)
    for m in rows:
        v = [float(m.group(i)) for i in range(1, 8)]
        assert all(np.isfinite(v)), v
        water, start, fallen = v[4], v[5], v[6]
        print("water budget:", water, start, fallen, abs(water + fallen - start) / start)
        assert start > 0 and abs(water + fallen - start) <= 1.0e-10 * start, v
    import json
    stats = json.loads(lines[-1])
    assert stats["finite"] is True and stats["tracer_min"] >= 0.0
    nz, ny, nx, nens = stats["nz"], stats["ny"], stats["nx"], stats["nens"]
    assert os.path.getsize(out) == 8 * (10 * nz * ny * nx * nens + ny * nx * nens)      # five state fields, five tracers, precl
    plain = subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3", "--steps", "1", str(tmp_path / "k.bin")], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and "micro ice:" not in plain.stdout and "Micro : kessler" in plain.stdout
