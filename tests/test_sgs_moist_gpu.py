"""The moist branch of the Smagorinsky SGS closure and the surface fluxes of heat and vapour on the GPU: both new entry points against
the numpy restatement (tests/sgs_moist_ref.py) bit for bit (a NaN by its place) on every shape, named case and placement of c'; members
split over calls against the whole; a bystander tensor and a side stream; the Python class through a coupler with Kessler's and with
P3's tracer names; and the C++ class through examples/driver --sgs-smag --sgs-moist --sfc-fluxes on a shortened CI input."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import sgs_ref as ref
import sgs_moist_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")
AUTO, LDS, WORKSPACE = 0, 1, 2
SIX = ref.WINDS + ("temp", "density_dry", "water_vapor")
SURFACE = ("sfc_flx_u", "sfc_flx_v", "sfc_shf", "sfc_lhf")


class GpuBackend:
    """the interface of sgs_moist_ref.RefBackend over the C ABI; path: pam_amd_sgs_smag_debug_path, set for the call and reset after it.
    The vapour of the tracer table is the rho_v pointer itself, as a coupler has it"""

    def __init__(self, path=AUTO):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check, self.path = torch, capi.load(), capi.check, path

    def _dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def _stream(self, stream):
        return self.torch.cuda.current_stream().cuda_stream if stream is None else stream

    def call_coefficients(self, case, dev, tk, tkh, stream=None):
        nz, ny, nx, nens = dev["temp"].shape
        cloud = (C.c_void_p * 4)(*[dev[n].data_ptr() for n in case["cloud"]])
        precip = (C.c_void_p * 8)(*[dev[n].data_ptr() for n in case["precip"]])
        self.check(self.lib.pam_amd_sgs_smag_coefficients_moist(nens, nx, ny, nz, *[dev[n].data_ptr() for n in SIX], len(case["cloud"]), cloud,
                                                                len(case["precip"]), precip, dev["zint"].data_ptr(), dev["zmid"].data_ptr(),
                                                                case["dx"], case["dy"], case["grav"], case["cp_d"], case["R_d"], case["R_v"],
                                                                case["cloud_threshold"], case["cs"], case["prandtl"], tk.data_ptr(), tkh.data_ptr(),
                                                                self._stream(stream)))

    def call_diffuse(self, case, dev, tk, tkh, stream=None):
        nz, ny, nx, nens = dev["temp"].shape
        tr = case["tracers"]
        table = (C.c_void_p * max(len(tr), 1))(*[dev[n].data_ptr() for n in tr])
        sfc = [None if dev.get(n) is None else dev[n].data_ptr() for n in SURFACE]
        self.check(self.lib.pam_amd_sgs_smag_debug_path(self.path))
        try:
            self.check(self.lib.pam_amd_sgs_smag_diffuse_fluxes(nens, nx, ny, nz, *[dev[n].data_ptr() for n in ref.WINDS + ("temp",)], len(tr), table,
                                                                dev["density_dry"].data_ptr(), dev["water_vapor"].data_ptr(), tk.data_ptr(),
                                                                tkh.data_ptr(), dev["zint"].data_ptr(), dev["zmid"].data_ptr(), sfc[0], sfc[1],
                                                                case["dt"], case["grav"], case["cp_d"], sfc[2], sfc[3], case["latvap"],
                                                                self._stream(stream)))
        finally:
            self.check(self.lib.pam_amd_sgs_smag_debug_path(AUTO))

    def upload(self, case):
        dev = {n: self._dev(a) for n, a in case["fields"].items()}
        for n in ("zint", "zmid") + SURFACE:
            dev[n] = self._dev(case.get(n))
        return dev

    def coefficients(self, case):
        dev = self.upload(case)
        tk, tkh = (self.torch.full(dev["temp"].shape, float("nan"), dtype=self.torch.float64, device="cuda:0") for _ in range(2))
        self.call_coefficients(case, dev, tk, tkh)
        self.torch.cuda.synchronize()
        return tk.cpu().numpy(), tkh.cpu().numpy()

    def diffuse(self, case, tk, tkh):
        dev = self.upload(case)
        self.call_diffuse(case, dev, self._dev(tk), self._dev(tkh))
        self.torch.cuda.synchronize()
        return {n: dev[n].cpu().numpy() for n in ref.WINDS + ("temp",) + tuple(case["tracers"])}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_gpu_matches_restatement_bit_for_bit(shape):
    """every named case on the automatic path and on each forced one; one case twice: two runs are identical"""
    for name in mref.CASE_NAMES:
        want = mref.reference(shape, name)
        for path in (AUTO, LDS, WORKSPACE):
            got = mref.run_case(GpuBackend(path), mref.cases(shape)[name])
            assert mref.results_differ(got, want, nan_by_place=True) == [], (name, path)
    a, b = (mref.run_case(GpuBackend(), mref.cases(shape)["fluxes_both"]) for _ in range(2))
    assert mref.results_differ(a, b) == []


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_gpu_empty_tables_and_null_fluxes_give_the_dry_entry_points_bits(shape):
    """the new entry points against the old ones on the device itself, on both placements of c'"""
    from test_sgs_smag_gpu import GpuBackend as DryGpuBackend
    case = mref.cases(shape)["empty_tables"]
    for path in (LDS, WORKSPACE):
        dry, new = DryGpuBackend(path), GpuBackend(path)
        tk, tkh = dry.coefficients(case)
        want = dict(dry.diffuse(case, tk, tkh), tk=tk, tkh=tkh)
        got = dict(new.diffuse(case, tk, tkh))
        got["tk"], got["tkh"] = new.coefficients(case)
        assert mref.results_differ(got, want) == [], path


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[3] == 130], ids=ref.shape_id)
def test_gpu_members_split_over_two_calls_equal_the_whole(shape):
    """members 0 .. 36 and 37 .. 129, and 0 .. 63 and 64 .. 129: the whole call's bits, on both paths"""
    for name in ("threshold_positive", "vapour_last_with_lhf", "nan_cell"):
        case, want = mref.cases(shape)[name], mref.reference(shape, name)
        for path in (LDS, WORKSPACE):
            be = GpuBackend(path)
            for cut in (37, 64):
                parts = [mref.run_case(be, mref.members(case, slice(lo, hi))) for lo, hi in ((0, cut), (cut, 130))]
                got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
                assert mref.results_differ(got, want, nan_by_place=True) == [], (name, path, cut)


@pytest.mark.gpu
def test_gpu_bystander_tensor_and_a_side_stream():
    """a tensor that is in no table keeps its bits, and so do the read-only inputs; both calls on a non-default stream, the fields produced
    on that stream just before them, give the restatement's bits"""
    import torch
    shape = (7, 3, 5, 130)
    case, want = mref.cases(shape)["vapour_last_with_lhf"], mref.reference(shape, "vapour_last_with_lhf")
    be = GpuBackend(AUTO)
    bystander = torch.from_numpy(case["fields"]["uvel"].copy()).to("cuda:0")
    host = {n: torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for n, a in case["fields"].items()}
    for n in ("zint", "zmid", "sfc_shf", "sfc_lhf"):
        host[n] = torch.from_numpy(np.ascontiguousarray(case[n])).pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = {n: torch.empty(h.shape, dtype=torch.float64, device="cuda:0") for n, h in host.items()}
        for n, h in host.items():
            dev[n].copy_(h, non_blocking=True)
        tk, tkh = (torch.empty(shape, dtype=torch.float64, device="cuda:0") for _ in range(2))
        be.call_coefficients(case, dev, tk, tkh, stream=side.cuda_stream)
        be.call_diffuse(case, dev, tk, tkh, stream=side.cuda_stream)
    side.synchronize()
    got = {n: dev[n].cpu().numpy() for n in ref.WINDS + ("temp",) + case["tracers"]}
    got["tk"], got["tkh"] = tk.cpu().numpy(), tkh.cpu().numpy()
    assert mref.results_differ(got, want, nan_by_place=True) == []
    assert mref.same_bits(bystander.cpu().numpy(), case["fields"]["uvel"])
    for n in ("density_dry", "zint", "zmid", "sfc_shf", "sfc_lhf"):
        assert mref.same_bits(dev[n].cpu().numpy(), np.ascontiguousarray(case["fields"][n] if n in case["fields"] else case[n])), n


@pytest.mark.gpu
@pytest.mark.parametrize("micro", ["kessler", "p3"])
@pytest.mark.parametrize("shape", [(3, 1, 2, 65), (7, 3, 5, 130)], ids=ref.shape_id)
def test_gpu_python_class_through_a_coupler(shape, micro):
    """SGSSmagorinsky(moist=True, surface_fluxes=True).init / timeStep with Kessler's and with P3's tracer names: tk, tkh, the winds, temp
    and every registered tracer equal the restatement.  P3 sets option "latvap", which the class then reads; without it 2501000.0"""
    import torch
    from pam_amd import PamCoupler, SGSSmagorinsky
    nz, ny, nx, nens = shape
    cs = mref.cases(shape)
    fluxes = dict(sfc_shf=cs["fluxes_both"]["sfc_shf"], sfc_lhf=cs["fluxes_both"]["sfc_lhf"])
    if micro == "kessler":
        case, threshold = dict(cs["kessler_set"], **fluxes), 0.0
    else:
        case, threshold = dict(cs["threshold_positive"], latvap=2.5e6, **fluxes), mref.THRESHOLD
    want = mref.run_case(mref.RefBackend(), case)
    c = PamCoupler("cuda:0")
    for n in ("grav", "cp_d", "R_d", "R_v"):
        c.set_option(n, case[n])
    c.set_option("crm_dt", case["dt"])
    c.set_option("micro", micro)
    if micro == "p3":
        c.set_option("latvap", 2.5e6)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(nx * case["dx"], ny * case["dy"], case["zint"][:, 0].copy())
    for n in case["tracers"]:
        c.add_tracer(n, "", True, True)
    sgs = SGSSmagorinsky(moist=True, surface_fluxes=True, cloud_threshold=threshold)
    sgs.init(c)
    assert c.get_option("sgs_smag_moist") is True and c.get_option("sgs_smag_surface_fluxes") is True
    assert c.get_option("sgs_smag_cloud_threshold") == threshold
    dm = c.get_data_manager_device_readwrite()
    for n in ("tk", "tkh", "sfc_mom_flx_u", "sfc_mom_flx_v", "sfc_shf", "sfc_lhf"):
        assert dm.entry_exists(n) and float(dm.get(n, readonly=True).abs().max()) == 0.0
    for n, v in case["fields"].items():
        if n in SIX or n in case["tracers"]:
            dm.get(n).copy_(torch.from_numpy(v))
    dm.get("vertical_interface_height").copy_(torch.from_numpy(case["zint"]))
    dm.get("vertical_midpoint_height").copy_(torch.from_numpy(case["zmid"]))
    for entry, key in (("sfc_mom_flx_u", "sfc_flx_u"), ("sfc_mom_flx_v", "sfc_flx_v"), ("sfc_shf", "sfc_shf"), ("sfc_lhf", "sfc_lhf")):
        dm.get(entry).copy_(torch.from_numpy(case[key]))
    sgs.timeStep(c)
    torch.cuda.synchronize()
    got = {n: dm.get(n, readonly=True).cpu().numpy() for n in want}
    assert mref.results_differ(got, want) == []
    assert mref.same_bits(dm.get("density_dry", readonly=True).cpu().numpy(), case["fields"]["density_dry"])
    # without the two keywords the class does not register the flux entries, and init leaves the options off
    c2 = PamCoupler("cuda:0")
    c2.allocate_coupler_state(nz, ny, nx, nens)
    SGSSmagorinsky().init(c2)
    assert c2.get_option("sgs_smag_moist") is False and not c2.get_data_manager_device_readwrite().entry_exists("sfc_shf")
    sgs.finalize(c)


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ class through the driver

def _run_driver(*args, timeout=600):
    r = subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3"] + list(args), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().split("\n")


@pytest.mark.gpu
def test_gpu_driver_runs_the_moist_closure_with_surface_fluxes(tmp_path):
    """two CRM steps of the whole loop (Kessler, sponge layer) with --sgs-smag 0.2 0.3333 --sgs-moist --sfc-fluxes 50 200: it completes,
    every field is finite, no tracer is negative, and the fields are not those of the run without the two flags; either flag without
    --sgs-smag is refused"""
    from test_sgs_smag_gpu import _fields
    a, b = tmp_path / "moist.bin", tmp_path / "dry.bin"
    la = _run_driver("--steps", "2", "--sgs-smag", "0.2", "0.3333", "--sgs-moist", "--sfc-fluxes", "50", "200", str(a))
    lb = _run_driver("--steps", "2", "--sgs-smag", "0.2", "0.3333", str(b))
    assert "SGS   : smagorinsky" in la
    assert json.loads(la[-3]) == dict(sgs_smag_moist=True, sgs_smag_surface_fluxes=True, sfc_shf=50, sfc_lhf=200)
    assert json.loads(la[-2]) == json.loads(lb[-2]) == dict(sgs_smag_cs=0.2, sgs_smag_prandtl=0.3333)
    last = json.loads(la[-1])
    assert last["crm_steps"] == 2 and last["finite"] is True and last["tracer_min"] >= 0
    fa, fb = _fields(a, last), _fields(b, last)
    assert all(np.isfinite(f).all() for f in fa) and all((f >= 0).all() for f in fa[5:])
    assert not mref.same_bits(fa[4], fb[4]) and not mref.same_bits(fa[5], fb[5])             # temp and the vapour took the fluxes
    assert fa[4][0].mean() > fb[4][0].mean() and fa[5][0].mean() > fb[5][0].mean()           # upward fluxes warm and moisten the lowest level
    for flags in (["--sgs-moist"], ["--sfc-fluxes", "50", "200"]):
        r = subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3", "--steps", "1"] + flags + ["-"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "need --sgs-smag" in r.stderr + r.stdout
