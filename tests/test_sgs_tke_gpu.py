"""The prognostic-TKE closure of the native SGS plug-in on the GPU: both new entry points against the numpy restatement
(tests/sgs_tke_ref.py) bit for bit (a NaN by its place) on every shape and named case, run to run, members split over calls against the
whole, the inputs untouched; the whole SGSTke.timeStep for three consecutive steps against the restatement composed the same way;
SGSSmagorinsky.timeStep beside a tke tracer; the refusals on device arrays; the Python class through a coupler; the C++ class through
tests/cxx/tke_sgs; and examples/driver --sgs-tke on a shortened CI input (tests/golden/msa_input.yaml)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sgs_ref as ref
import sgs_tke_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")
SIX = ref.WINDS + ("temp", "density_dry", "water_vapor")


class GpuBackend:
    """the interface of sgs_tke_ref.RefBackend over the C ABI: the dry entry point where the case is not moist"""

    def __init__(self):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check = torch, capi.load(), capi.check

    def _dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def upload(self, case):
        dev = {n: self._dev(a) for n, a in case["fields"].items()}
        for n in ("zint", "zmid"):
            dev[n] = self._dev(case[n])
        return dev

    def call(self, case, dev, tk, tkh):
        nz, ny, nx, nens = dev["temp"].shape
        stream = self.torch.cuda.current_stream().cuda_stream
        six = [dev[n].data_ptr() for n in SIX]
        if case["moist"]:
            ctab = (C.c_void_p * 4)(*[dev[n].data_ptr() for n in case["cloud"]])
            ptab = (C.c_void_p * 8)(*[dev[n].data_ptr() for n in case["precip"]])
            self.check(self.lib.pam_amd_sgs_tke_coefficients_moist(nens, nx, ny, nz, *six, dev["tke"].data_ptr(), len(case["cloud"]), ctab,
                                                                   len(case["precip"]), ptab, dev["zint"].data_ptr(), dev["zmid"].data_ptr(),
                                                                   case["dx"], case["dy"], case["dt"], case["grav"], case["cp_d"], case["R_d"],
                                                                   case["R_v"], case["cloud_threshold"], case["ck"], case["ce1"], case["ce2"],
                                                                   case["seed"], tk.data_ptr(), tkh.data_ptr(), stream))
        else:
            self.check(self.lib.pam_amd_sgs_tke_coefficients(nens, nx, ny, nz, *six, dev["tke"].data_ptr(), dev["zint"].data_ptr(),
                                                             dev["zmid"].data_ptr(), case["dx"], case["dy"], case["dt"], case["grav"],
                                                             case["cp_d"], case["ck"], case["ce1"], case["ce2"], case["seed"], tk.data_ptr(),
                                                             tkh.data_ptr(), stream))

    def coefficients(self, case, keep=None):
        dev = self.upload(case)
        tk, tkh = (self.torch.full(dev["temp"].shape, float("nan"), dtype=self.torch.float64, device="cuda:0") for _ in range(2))
        self.call(case, dev, tk, tkh)
        self.torch.cuda.synchronize()
        if keep is not None:
            keep.update({n: dev[n].cpu().numpy() for n in SIX + case["cloud"] + case["precip"] + ("zint", "zmid")})
        return dev["tke"].cpu().numpy(), tk.cpu().numpy(), tkh.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", tref.SHAPES, ids=tref.shape_id)
def test_gpu_matches_restatement_bit_for_bit(shape):
    """every named case through the dry or the moist entry point: tke, tk and tkh; the base case twice: two runs are identical; and the
    winds, temp, rho_d, rho_v, the condensates and the grid keep their bits"""
    be = GpuBackend()
    for name in tref.CASE_NAMES:
        case, kept = tref.cases(shape)[name], {}
        tke, tk, tkh = be.coefficients(case, kept)
        got = dict(tke=tke, tk=tk, tkh=tkh)
        assert tref.results_differ(got, tref.reference(shape, name), nan_by_place=True) == [], name
        for n, a in kept.items():
            assert tref.same_bits(a, np.ascontiguousarray(case["fields"][n] if n in case["fields"] else case[n])), (name, n)
    a, b = (tref.run_case(be, tref.cases(shape)["p3_set"]) for _ in range(2))
    assert tref.results_differ(a, b) == []


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in tref.SHAPES if s[3] == 130], ids=tref.shape_id)
def test_gpu_members_split_over_calls_equal_the_whole(shape):
    """the members in one call and split into two member ranges (37 and 93): the same bits"""
    be = GpuBackend()
    for name in ("base", "ice1m_set", "nan_wind_cell"):
        case, want = tref.cases(shape)[name], tref.reference(shape, name)
        parts = [tref.run_case(be, tref.members(case, list(range(lo, hi)))) for lo, hi in ((0, 37), (37, 130))]
        got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
        assert tref.results_differ(got, want, nan_by_place=True) == [], name


def _coupler(case, shape, sgs, extra_options=()):
    """a coupler that carries the case: the tracers in the case's order, tke registered by the class's own init where it stands"""
    import torch
    from pam_amd import PamCoupler
    nz, ny, nx, nens = shape
    c = PamCoupler("cuda:0")
    for n, v in (("crm_dt", case["dt"]), ("grav", case["grav"]), ("cp_d", case["cp_d"]), ("R_d", case["R_d"]), ("R_v", case["R_v"]),
                 ("latvap", case["latvap"])) + tuple(extra_options):
        c.set_option(n, v)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(nx * case["dx"], ny * case["dy"], case["zint"][:, 0].copy())
    for n in case["tracers"]:
        if n == "tke" and sgs.sgs_name() == "tke":
            sgs.init(c)
        else:
            c.add_tracer(n, "", True, n != "tke")
    if sgs.sgs_name() != "tke":
        sgs.init(c)
    dm = c.get_data_manager_device_readwrite()
    for n, v in case["fields"].items():
        if n in SIX or n in case["tracers"]:
            dm.get(n).copy_(torch.from_numpy(np.ascontiguousarray(v)))
    dm.get("vertical_interface_height").copy_(torch.from_numpy(case["zint"]))
    dm.get("vertical_midpoint_height").copy_(torch.from_numpy(case["zmid"]))
    dm.get("sfc_mom_flx_u").copy_(torch.from_numpy(case["sfc_flx_u"]))
    dm.get("sfc_mom_flx_v").copy_(torch.from_numpy(case["sfc_flx_v"]))
    for n in ("sfc_shf", "sfc_lhf"):
        if case.get(n) is not None:
            dm.get(n).copy_(torch.from_numpy(case[n]))
    return c, dm


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["base", "kessler_set", "fluxes_both"])
@pytest.mark.parametrize("shape", [(3, 1, 2, 65), (7, 3, 5, 130)], ids=tref.shape_id)
def test_gpu_three_time_steps_of_the_class_are_the_restatement_composed_the_same_way(shape, name):
    """SGSTke.timeStep three times (coefficients, then the existing solve, tke in the tracer table beside the vapour and the others):
    tk, tkh, the winds, temp and every tracer equal the restatement; density_dry keeps its bits"""
    import torch
    from pam_amd import SGSTke
    case = tref.cases(shape)[name]
    want = tref.time_step(case, 3)
    fluxes = case["sfc_shf"] is not None
    sgs = SGSTke(cs=tref.CS, ck=tref.CK, seed=tref.SEED, moist=case["moist"], surface_fluxes=fluxes)
    c, dm = _coupler(case, shape, sgs, (("micro", "kessler"),) if case["moist"] else ())
    for _ in range(3):
        sgs.timeStep(c)
    torch.cuda.synchronize()
    got = {n: dm.get(n, readonly=True).cpu().numpy() for n in want}
    assert "tke" in want and tref.results_differ(got, want) == []
    assert tref.same_bits(dm.get("density_dry", readonly=True).cpu().numpy(), case["fields"]["density_dry"])
    sgs.finalize(c)


@pytest.mark.gpu
def test_gpu_smagorinsky_beside_a_tke_tracer_gives_the_bits_it_gives_today():
    """SGSSmagorinsky.timeStep on a coupler that also carries "tke": its own coefficients and solve (sgs_ref's restatement), tke mixed like
    any tracer and not stepped"""
    import torch
    from pam_amd import SGSSmagorinsky
    shape = (7, 3, 5, 130)
    case = tref.cases(shape)["base"]
    tk, tkh = ref.coefficients(case)
    want = dict(ref.diffuse(case, tk, tkh), tk=tk, tkh=tkh)
    sgs = SGSSmagorinsky()
    c, dm = _coupler(case, shape, sgs)
    sgs.timeStep(c)
    torch.cuda.synchronize()
    got = {n: dm.get(n, readonly=True).cpu().numpy() for n in want}
    assert "tke" in want and ref.results_differ(got, want) == []


@pytest.mark.gpu
def test_gpu_entry_points_refuse_bad_arguments_on_device_arrays_and_leave_them_untouched():
    """every refusal of the contract with device pointers: PAM_AMD_EINVAL, and tke, tk, tkh and every other array keep their pattern"""
    import torch
    from pam_amd import capi
    from test_sgs_tke import refusals
    lib = capi.load()
    arrays = [torch.full((4 * 2 * 3 * 4 + 16,), 7.25, dtype=torch.float64, device="cuda:0") for _ in range(16)]
    calls, _ = refusals(lib, [a.data_ptr() for a in arrays])
    for i, call in enumerate(calls):
        assert call() == -1, i
        assert b"sgs_tke" in lib.pam_amd_awfl_last_error(), i
    torch.cuda.synchronize()
    assert all(bool((a == 7.25).all()) for a in arrays)


@pytest.mark.gpu
def test_gpu_class_registers_its_tracer_fields_and_options_once():
    """init registers the tracer, the fields and the options; a second init changes nothing; options set before init are kept; micro
    outside the tables is refused with moist=True"""
    import torch
    from pam_amd import PamCoupler, SGSTke
    from pam_amd.capi import PamAmdError
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", 10.0)
    c.set_option("sgs_tke_ck", 0.09)
    c.allocate_coupler_state(4, 2, 3, 5)
    c.set_grid(1500.0, 1000.0, np.linspace(0.0, 2000.0, 5))
    c.add_tracer("water_vapor", "", True, True)
    sgs = SGSTke(moist=True, surface_fluxes=True, cloud_threshold=1e-5)
    assert sgs.get_num_tracers() == 1 and sgs.sgs_name() == "tke"
    sgs.init(c)
    dm = c.get_data_manager_device_readwrite()
    assert c.get_tracer_names() == ["water_vapor", "tke"]
    for n in ("tke", "tk", "tkh", "sfc_mom_flx_u", "sfc_mom_flx_v", "sfc_shf", "sfc_lhf"):
        assert dm.entry_exists(n) and float(dm.get(n, readonly=True).abs().max()) == 0.0, n
    want = dict(sgs="tke", sgs_tke_cs=0.2, sgs_tke_ck=0.09, sgs_tke_seed=1e-3, sgs_tke_moist=True, sgs_tke_surface_fluxes=True,
                sgs_tke_cloud_threshold=1e-5)
    assert {n: c.get_option(n) for n in want} == want and set(want) == set(SGSTke.OPTIONS)
    dm.get("tke").fill_(0.5)
    ptr = dm.get("tke").data_ptr()
    sgs.init(c)
    assert c.get_tracer_names() == ["water_vapor", "tke"] and dm.get("tke").data_ptr() == ptr and float(dm.get("tke").min()) == 0.5
    assert {n: c.get_option(n) for n in want} == want
    c.set_option("micro", "morrison")
    for n in ("grav", "cp_d", "R_d", "R_v"):
        c.set_option(n, dict(grav=9.8, cp_d=1004.0, R_d=287.0, R_v=461.0)[n])
    with pytest.raises(PamAmdError, match="moist branch knows the species"):
        sgs.timeStep(c)
    torch.cuda.synchronize()
    assert float(dm.get("tke").min()) == 0.5 and float(dm.get("tk").abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ class through tests/cxx/tke_sgs, and through the driver

@pytest.mark.gpu
def test_gpu_cxx_class_reproduces_the_python_class_bit_for_bit(tmp_path):
    import torch
    from pam_amd import SGSTke
    from tools.native_build import cxx_program
    shape = (5, 1, 4, 130)
    nz, ny, nx, nens = shape
    case = tref.cases(shape)["base"]
    assert case["tracers"] == ("water_vapor", "tke", "tracer_a", "tracer_b")
    sgs = SGSTke()
    c, dm = _coupler(case, shape, sgs)
    sgs.timeStep(c)
    torch.cuda.synchronize()
    names = ("tke", "tk", "tkh", "uvel", "vvel", "wvel", "temp", "water_vapor", "tracer_a", "tracer_b", "density_dry")
    want = {n: dm.get(n, readonly=True).cpu().numpy() for n in names}
    path, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(path, "wb") as f:
        np.array(shape, dtype=np.int32).tofile(f)
        np.array([case["dt"], case["grav"], case["cp_d"], nx * case["dx"], ny * case["dy"]]).tofile(f)
        for a in (case["zint"], case["zmid"]):
            np.ascontiguousarray(a).tofile(f)
        for n in SIX + ("tke", "tracer_a", "tracer_b"):
            np.ascontiguousarray(case["fields"][n]).tofile(f)
        for n in ("sfc_flx_u", "sfc_flx_v"):
            np.ascontiguousarray(case[n]).tofile(f)
    r = subprocess.run([cxx_program("tke_sgs"), str(path), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert "### tracers water_vapor tke tracer_a tracer_b" in lines and "### sgs tke tke" in lines
    consts = [l for l in lines if l.startswith("### constants")]
    assert len(consts) == 1 and tuple(float(x) for x in consts[0].split()[2:]) == SGSTke.constants(0.2, 0.1) == tref.constants(0.2, 0.1)
    raw = np.fromfile(out, dtype=np.float64).reshape((len(names),) + shape)
    got = {n: raw[q] for q, n in enumerate(names)}
    assert tref.results_differ(got, want) == []


def _run_driver(*args, timeout=600, expect=0):
    r = subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3"] + list(args), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == expect, r.stderr[-2000:]
    return r.stdout.strip().split("\n") if expect == 0 else r.stderr


def _fields(path, last):
    """the driver's output file: density_dry, uvel, vvel, wvel, temp, the tracers, (nz,ny,nx,nens) each, then precl (ny,nx,nens)"""
    shape = (last["nz"], last["ny"], last["nx"], last["nens"])
    raw = np.fromfile(path, dtype=np.float64)
    ncell, n2 = int(np.prod(shape)), shape[1] * shape[2] * shape[3]
    assert (raw.size - n2) % ncell == 0
    return [raw[i * ncell:(i + 1) * ncell].reshape(shape) for i in range((raw.size - n2) // ncell)]


TKE_LINE = r"sgs tke: etime (\S+) , e_mean (\S+) , tke_min (\S+) , tke_max (\S+) , tk_max (\S+)"


@pytest.mark.gpu
def test_gpu_driver_runs_the_class_in_the_sgs_slot(tmp_path):
    """--sgs-tke 0.2 0.1 on the CI input runs to the end: one finite "sgs tke:" line per output step with tke >= 0; every tracer stays non-negative; one CRM step without sponge layer and microphysics keeps the plain run's dry mass bit
    for bit and carries one more tracer; together with --sgs-smag the flag is refused"""
    whole, plain, tke = tmp_path / "whole.bin", tmp_path / "plain.bin", tmp_path / "tke.bin"
    lines = _run_driver("--sgs-tke", "0.2", "0.1", str(whole))
    assert "SGS   : tke" in lines and json.loads(lines[-2]) == dict(sgs_tke_cs=0.2, sgs_tke_ck=0.1)
    last = json.loads(lines[-1])
    assert last["finite"] is True and last["crm_steps"] == 12 and last["tracer_min"] >= 0
    rows = [re.fullmatch(TKE_LINE, l) for l in lines if l.startswith("sgs tke:")]
    assert rows and all(rows) and len(rows) == sum(l.startswith("Etime ,") for l in lines)
    for m in rows:
        etime, e_mean, tke_min, tke_max, tk_max = (float(x) for x in m.groups())
        assert all(np.isfinite(v) for v in (e_mean, tke_min, tke_max, tk_max)) and tke_min >= 0 and e_mean >= 0 and tk_max >= 0
    f = _fields(whole, last)
    assert len(f) == 9 and (f[8] >= 0).all()                                     # tke is the tracer after Kessler's three
    la = _run_driver("--steps", "1", "--no-micro", "--no-sponge", str(plain))
    lb = _run_driver("--steps", "1", "--no-micro", "--no-sponge", "--sgs-tke", "0.2", "0.1", str(tke))
    lastb = json.loads(lb[-1])
    a, b = _fields(plain, json.loads(la[-1])), _fields(tke, lastb)
    assert lastb["crm_steps"] == 1 and lastb["finite"] is True and len(a) == 8 and len(b) == 9
    assert tref.same_bits(b[0], a[0])                                            # density_dry: the reference run's mass invariant
    err = _run_driver("--sgs-tke", "0.2", "0.1", "--sgs-smag", "0.2", "0.3333333333333333", str(tmp_path / "none.bin"), expect=2)
    assert "--sgs-smag and --sgs-tke" in err
