"""The native Smagorinsky SGS closure on the GPU: both launches against the numpy restatement (tests/sgs_ref.py) bit for bit (a NaN by
its place: sgs_ref.same_bits) on every shape, named case and placement of c', run to run, members split over calls against the whole; a
bystander tensor; a non-default stream; the Python class through a coupler; and the C++ class through examples/driver --sgs-smag on a
shortened CI input (tests/golden/msa_input.yaml)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import sgs_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")
AUTO, LDS, WORKSPACE = 0, 1, 2
SIX = ref.WINDS + ("temp", "density_dry", "water_vapor")


class GpuBackend:
    """the interface of sgs_ref.RefBackend over the C ABI; path: pam_amd_sgs_smag_debug_path, set for the call and reset after it.  The
    vapour of the tracer table is the rho_v pointer itself, as a coupler has it"""

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
        self.check(self.lib.pam_amd_sgs_smag_coefficients(nens, nx, ny, nz, *[dev[n].data_ptr() for n in SIX], dev["zint"].data_ptr(),
                                                          dev["zmid"].data_ptr(), case["dx"], case["dy"], case["grav"], case["cp_d"], case["cs"],
                                                          case["prandtl"], tk.data_ptr(), tkh.data_ptr(), self._stream(stream)))

    def call_diffuse(self, case, dev, tk, tkh, stream=None):
        nz, ny, nx, nens = dev["temp"].shape
        tr = case["tracers"]
        table = (C.c_void_p * max(len(tr), 1))(*[dev[n].data_ptr() for n in tr])
        sfc = [None if dev.get(n) is None else dev[n].data_ptr() for n in ("sfc_flx_u", "sfc_flx_v")]
        self.check(self.lib.pam_amd_sgs_smag_debug_path(self.path))
        try:
            self.check(self.lib.pam_amd_sgs_smag_diffuse(nens, nx, ny, nz, *[dev[n].data_ptr() for n in ref.WINDS + ("temp",)], len(tr), table,
                                                         dev["density_dry"].data_ptr(), dev["water_vapor"].data_ptr(), tk.data_ptr(), tkh.data_ptr(),
                                                         dev["zint"].data_ptr(), dev["zmid"].data_ptr(), sfc[0], sfc[1], case["dt"], case["grav"],
                                                         case["cp_d"], self._stream(stream)))
        finally:
            self.check(self.lib.pam_amd_sgs_smag_debug_path(AUTO))

    def upload(self, case):
        dev = {n: self._dev(a) for n, a in case["fields"].items()}
        for n in ("zint", "zmid", "sfc_flx_u", "sfc_flx_v"):
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
    """every named case on the automatic path and on each forced one; the base case twice: two runs are identical"""
    for name in ref.CASE_NAMES:
        want = ref.reference(shape, name)
        for path in (AUTO, LDS, WORKSPACE):
            got = ref.run_case(GpuBackend(path), ref.cases(shape)[name])
            assert ref.results_differ(got, want, nan_by_place=True) == [], (name, path)
    a, b = (ref.run_case(GpuBackend(), ref.cases(shape)["base"]) for _ in range(2))
    assert ref.results_differ(a, b) == []


def _members(case, lo, hi):
    sub = dict(case, fields={n: np.ascontiguousarray(a[..., lo:hi]) for n, a in case["fields"].items()},
               zint=np.ascontiguousarray(case["zint"][:, lo:hi]), zmid=np.ascontiguousarray(case["zmid"][:, lo:hi]))
    for n in ("sfc_flx_u", "sfc_flx_v", "tk", "tkh"):
        if case.get(n) is not None:
            sub[n] = np.ascontiguousarray(case[n][..., lo:hi])
    return sub


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[3] == 130], ids=ref.shape_id)
def test_gpu_members_split_over_calls_equal_the_whole(shape):
    """member chunks of 1, 37 and 64: the whole call's bits, on both paths"""
    for name in ("vapour_middle", "zero_k_faces", "nan_cell"):
        case, want = ref.cases(shape)[name], ref.reference(shape, name)
        for path in (LDS, WORKSPACE):
            be = GpuBackend(path)
            for chunk in (1, 37, 64):
                if chunk == 1 and (path != LDS or name != "vapour_middle"):
                    continue
                parts = [ref.run_case(be, _members(case, lo, min(lo + chunk, 130))) for lo in range(0, 130, chunk)]
                got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
                assert ref.results_differ(got, want, nan_by_place=True) == [], (name, path, chunk)


@pytest.mark.gpu
def test_gpu_bystander_tensor_and_a_side_stream():
    """a tensor that is in no table keeps its bits, and so do the read-only inputs; both calls on a non-default stream, the fields produced
    on that stream just before them, give the restatement's bits on both paths"""
    import torch
    shape = (7, 3, 5, 130)
    case, want = ref.cases(shape)["vapour_last"], ref.reference(shape, "vapour_last")
    for path in (LDS, WORKSPACE):
        be = GpuBackend(path)
        bystander = torch.from_numpy(case["fields"]["uvel"].copy()).to("cuda:0")
        host = {n: torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for n, a in case["fields"].items()}
        for n in ("zint", "zmid", "sfc_flx_u", "sfc_flx_v"):
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
        assert ref.results_differ(got, want, nan_by_place=True) == [], path
        assert ref.same_bits(bystander.cpu().numpy(), case["fields"]["uvel"])
        for n in ("density_dry", "zint", "zmid", "sfc_flx_u", "sfc_flx_v"):
            assert ref.same_bits(dev[n].cpu().numpy(), np.ascontiguousarray(case["fields"][n] if n in case["fields"] else case[n])), n


@pytest.mark.gpu
def test_gpu_workspace_grows_with_the_shape():
    """the workspace path from no workspace at all: the smallest shape, then the largest, then one between them on the workspace the
    largest left, then the largest again from nothing after pam_amd_modules_finalize"""
    from pam_amd import capi
    lib = capi.load()
    by_size = sorted(ref.SHAPES, key=lambda s: s[0] * s[1] * s[2] * s[3])
    smallest, between, largest = by_size[0], by_size[len(by_size) // 2], by_size[-1]
    capi.check(lib.pam_amd_modules_finalize())
    be = GpuBackend(WORKSPACE)
    for shape in (smallest, largest, between):
        got = ref.run_case(be, ref.cases(shape)["base"])
        assert ref.results_differ(got, ref.reference(shape, "base"), nan_by_place=True) == [], shape
    capi.check(lib.pam_amd_modules_finalize())
    got = ref.run_case(be, ref.cases(largest)["vapour_last"])
    assert ref.results_differ(got, ref.reference(largest, "vapour_last"), nan_by_place=True) == []


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 1, 2, 65), (7, 3, 5, 130)], ids=ref.shape_id)
def test_gpu_python_class_through_a_coupler(shape):
    """SGSSmagorinsky.init / timeStep: tk, tkh, the winds, temp and every registered tracer equal the restatement; density_dry keeps its
    bits; the options and the fields the class registers"""
    import torch
    from pam_amd import PamCoupler, SGSSmagorinsky
    nz, ny, nx, nens = shape
    case, want = ref.cases(shape)["vapour_middle"], ref.reference(shape, "vapour_middle")
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", case["dt"])
    c.set_option("grav", case["grav"])
    c.set_option("cp_d", case["cp_d"])
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(nx * case["dx"], ny * case["dy"], case["zint"][:, 0].copy())
    for n in case["tracers"]:
        c.add_tracer(n, "", True, True)
    sgs = SGSSmagorinsky()
    assert sgs.get_num_tracers() == 0 and sgs.sgs_name() == "smagorinsky"
    sgs.init(c)
    assert c.get_option("sgs") == "smagorinsky" and c.get_option("sgs_smag_cs") == 0.2 and c.get_option("sgs_smag_prandtl") == 1.0 / 3.0
    dm = c.get_data_manager_device_readwrite()
    for n in ("tk", "tkh", "sfc_mom_flx_u", "sfc_mom_flx_v"):
        assert dm.entry_exists(n) and float(dm.get(n, readonly=True).abs().max()) == 0.0
    for n, v in case["fields"].items():
        if n in SIX or n in case["tracers"]:
            dm.get(n).copy_(torch.from_numpy(v))
    dm.get("vertical_interface_height").copy_(torch.from_numpy(case["zint"]))
    dm.get("vertical_midpoint_height").copy_(torch.from_numpy(case["zmid"]))
    dm.get("sfc_mom_flx_u").copy_(torch.from_numpy(case["sfc_flx_u"]))
    dm.get("sfc_mom_flx_v").copy_(torch.from_numpy(case["sfc_flx_v"]))
    sgs.timeStep(c)
    torch.cuda.synchronize()
    got = {n: dm.get(n, readonly=True).cpu().numpy() for n in want}
    assert ref.results_differ(got, want) == []
    assert ref.same_bits(dm.get("density_dry", readonly=True).cpu().numpy(), case["fields"]["density_dry"])
    sgs.finalize(c)


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ class through the driver

def _run_driver(*args, timeout=600):
    r = subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3"] + list(args), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().split("\n")


def _fields(path, last):
    """the driver's output file: density_dry, uvel, vvel, wvel, temp, the tracers, (nz,ny,nx,nens) each, then precl (ny,nx,nens)"""
    shape = (last["nz"], last["ny"], last["nx"], last["nens"])
    raw = np.fromfile(path, dtype=np.float64)
    ncell, n2 = int(np.prod(shape)), shape[1] * shape[2] * shape[3]
    assert (raw.size - n2) % ncell == 0
    return [raw[i * ncell:(i + 1) * ncell].reshape(shape) for i in range((raw.size - n2) // ncell)]


@pytest.mark.gpu
def test_gpu_driver_runs_the_class_in_the_sgs_slot_and_consumes_the_surface_fluxes(tmp_path):
    """one CRM step without sponge layer and microphysics, so the run ends in the SGS step: the fields are finite, the dry mass is the
    plain run's bit for bit, the other fields are not; with --surface-friction the lowest-level horizontal winds differ from the run
    without it: the fluxes are consumed now.  The supercell sounding is stable against its shear at a Prandtl number of 1/3
    (Ri > Pr everywhere, so tk == 0 and the closure rightly mixes nothing); the flag's PRANDTL of 100 makes the sheared levels mix"""
    plain, smag, fric = tmp_path / "plain.bin", tmp_path / "smag.bin", tmp_path / "fric.bin"
    la = _run_driver("--steps", "1", "--no-micro", "--no-sponge", str(plain))
    lb = _run_driver("--steps", "1", "--no-micro", "--no-sponge", "--sgs-smag", "0.2", "100", str(smag))
    lc = _run_driver("--steps", "1", "--no-micro", "--no-sponge", "--surface-friction", "0.1", "0.01", "--sgs-smag", "0.2", "100",
                     str(fric))
    assert "SGS   : smagorinsky" in lb and "SGS   : smagorinsky" in lc and "SGS   : none (SHOC is out of scope)" in la
    assert json.loads(lb[-2]) == dict(sgs_smag_cs=0.2, sgs_smag_prandtl=100)
    last = json.loads(lb[-1])
    assert last["crm_steps"] == 1 and last["finite"] is True and json.loads(lc[-1])["finite"] is True
    a, b, c = _fields(plain, last), _fields(smag, last), _fields(fric, last)
    assert len(a) == 8 and all(np.isfinite(f).all() for f in b + c)
    assert ref.same_bits(b[0], a[0]) and ref.same_bits(c[0], a[0])                # density_dry
    assert not ref.same_bits(b[1], a[1]) and not ref.same_bits(b[4], a[4])
    assert not np.array_equal(c[1][0], b[1][0])                                    # uvel at the lowest level takes the drag
    assert (a[2] == 0).all() and ref.same_bits(c[2], b[2])                         # the input is two-dimensional: no vvel, no flux of it
    assert ref.same_bits(c[3], b[3]) and ref.same_bits(c[4], b[4])                # wvel and temp take no surface flux


@pytest.mark.gpu
def test_gpu_driver_whole_run_with_the_other_flags(tmp_path):
    """the whole GCM step with sponge layer, surface friction, hyperdiffusion and Kessler: finite, every tracer non-negative, and not the
    run without the flag"""
    a, b = tmp_path / "smag.bin", tmp_path / "none.bin"
    lines = _run_driver("--surface-friction", "0.1", "0.01", "--hyperdiff", "120", "--sgs-smag", "0.2", "0.3333333333333333", str(a))
    last = json.loads(lines[-1])
    assert last["finite"] is True and last["crm_steps"] == 12 and last["tracer_min"] >= 0
    _run_driver("--surface-friction", "0.1", "0.01", "--hyperdiff", "120", str(b))
    assert a.read_bytes() != b.read_bytes()
