"""Horizontal hyperdiffusion on the GPU: the HIP kernels against the numpy restatement (tests/hd_ref.py) bit for bit (a NaN by its
place: hd_ref.same_bits) on every shape, named case and internal path, run to run, members and field lists split over calls against
the whole; fields outside the table; a non-default stream; the Python adaptor through a coupler; and the C++ adaptor through examples/driver --hyperdiff on a shortened CI
input (tests/golden/msa_input.yaml)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import hd_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")
AUTO, IN_PLACE, WORKSPACE, NARROW = 0, 1, 2, 3


class GpuBackend:
    """the interface of hd_ref.RefBackend over the C ABI; path: pam_amd_hyperdiffusion_debug_path, set for the call and reset after it"""

    def __init__(self, path=AUTO):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check, self.path = torch, capi.load(), capi.check, path

    def call(self, tensors, positive, dt, tau, stream=None):
        nz, ny, nx, nens = tensors[0].shape
        ptrs = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        flags = (C.c_ubyte * len(tensors))(*[int(bool(p)) for p in positive])
        self.check(self.lib.pam_amd_hyperdiffusion_debug_path(self.path))
        try:
            self.check(self.lib.pam_amd_hyperdiffusion(nens, nx, ny, nz, len(tensors), ptrs, flags, float(dt), float(tau),
                                                       self.torch.cuda.current_stream().cuda_stream if stream is None else stream))
        finally:
            self.check(self.lib.pam_amd_hyperdiffusion_debug_path(AUTO))

    def run(self, fields, positive, dt, tau):
        dev = [self.torch.from_numpy(np.ascontiguousarray(f)).to("cuda:0") for f in fields]
        self.call(dev, positive, dt, tau)
        self.torch.cuda.synchronize()
        return [t.cpu().numpy() for t in dev]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_gpu_matches_restatement_bit_for_bit(shape):
    """every named case on the automatic path and on each forced one; the base case twice: two runs are identical"""
    for name in ref.CASE_NAMES:
        want = ref.reference(shape, name)
        for path in (AUTO, IN_PLACE, WORKSPACE, NARROW):
            got = ref.run_case(GpuBackend(path), ref.cases(shape)[name])
            assert ref.results_differ(got, want, nan_by_place=True) == [], (name, path)
    a, b = (ref.run_case(GpuBackend(), ref.cases(shape)["base"]) for _ in range(2))
    assert ref.results_differ(a, b) == []


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[3] == 130], ids=ref.shape_id)
def test_gpu_members_and_field_lists_split_over_calls_equal_the_whole(shape):
    """member chunks of 1, 37 and 64, and the field list in two calls: the whole call's bits, on every path"""
    for name in ("base", "edge", "nan_cell"):
        case, want = ref.cases(shape)[name], ref.reference(shape, name)
        for path in (AUTO, WORKSPACE, NARROW):
            be = GpuBackend(path)
            for chunk in (1, 37, 64):
                if chunk == 1 and path != AUTO:
                    continue
                parts = [be.run([np.ascontiguousarray(f[..., lo:lo + chunk]) for f in case["fields"]], case["positive"], case["dt"], case["tau"])
                         for lo in range(0, 130, chunk)]
                got = [np.concatenate([p[i] for p in parts], axis=-1) for i in range(3)]
                assert ref.results_differ(got, want, nan_by_place=True) == [], (name, path, chunk)
            got = be.run(case["fields"][:1], case["positive"][:1], case["dt"], case["tau"])
            got += be.run(case["fields"][1:], case["positive"][1:], case["dt"], case["tau"])
            assert ref.results_differ(got, want, nan_by_place=True) == [], (name, path)


@pytest.mark.gpu
def test_gpu_field_outside_the_table_and_a_side_stream():
    """a tensor that is not in the table keeps its bits; the call on a non-default stream, the fields produced on that stream just
    before it, gives the restatement's bits on every path"""
    import torch
    shape = (3, 6, 8, 130)
    case, want = ref.cases(shape)["edge"], ref.reference(shape, "edge")
    for path in (AUTO, WORKSPACE):
        be = GpuBackend(path)
        bystander = torch.from_numpy(case["fields"][2].copy()).to("cuda:0")
        host = [torch.from_numpy(np.ascontiguousarray(f)).pin_memory() for f in case["fields"]]
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            dev = [torch.empty(shape, dtype=torch.float64, device="cuda:0") for _ in host]
            for d, h in zip(dev, host):
                d.copy_(h, non_blocking=True)
            be.call(dev, case["positive"], case["dt"], case["tau"], stream=side.cuda_stream)
        side.synchronize()
        assert ref.results_differ([d.cpu().numpy() for d in dev], want, nan_by_place=True) == [], path
        assert ref.same_bits(bystander.cpu().numpy(), case["fields"][2])


@pytest.mark.gpu
def test_gpu_workspace_grows_with_the_shape():
    """the workspace path from no workspace at all: the smallest shape with ny >= 5, then the largest, then one between them on the
    workspace the largest left, then the largest again from nothing after pam_amd_modules_finalize"""
    from pam_amd import capi
    lib = capi.load()
    with_y = sorted((s for s in ref.SHAPES if s[1] >= 5), key=lambda s: s[0] * s[1] * s[2] * s[3])
    smallest, between, largest = with_y[0], with_y[len(with_y) // 2], with_y[-1]
    capi.check(lib.pam_amd_modules_finalize())
    be = GpuBackend(WORKSPACE)
    for shape in (smallest, largest, between):
        got = ref.run_case(be, ref.cases(shape)["base"])
        assert ref.results_differ(got, ref.reference(shape, "base"), nan_by_place=True) == [], shape
    capi.check(lib.pam_amd_modules_finalize())
    got = ref.run_case(be, ref.cases(largest)["edge"])
    assert ref.results_differ(got, ref.reference(largest, "edge"), nan_by_place=True) == []


def _coupler(shape, tracers):
    from pam_amd import PamCoupler
    nz, ny, nx, nens = shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", ref.DT)
    c.allocate_coupler_state(nz, ny, nx, nens)
    for name, positive in tracers:
        c.add_tracer(name, "", positive, True)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 1, 8, 65), (3, 6, 8, 130)], ids=ref.shape_id)
def test_gpu_python_adaptor_through_a_coupler(shape):
    """hyperdiffusion_init / hyperdiffusion: temp, the three winds and every tracer, a tracer's own flag deciding the fill; density_dry
    keeps its bits; dt defaults to crm_dt"""
    import torch
    from pam_amd import modules
    cs = ref.cases(shape)
    state = dict(temp=cs["base"]["fields"][0], uvel=cs["base"]["fields"][1], vvel=-cs["base"]["fields"][1], wvel=cs["nan_cell"]["fields"][1],
                 water_vapor=cs["edge"]["fields"][2], free=cs["spike"]["fields"][2], density_dry=cs["base"]["fields"][2])
    positive = dict(water_vapor=1, free=0)
    c = _coupler(shape, [("water_vapor", True), ("free", False)])
    dm = c.get_data_manager_device_readwrite()
    for n, v in state.items():
        dm.get(n).copy_(torch.from_numpy(v))
    modules.hyperdiffusion_init(c, ref.TAU)
    assert c.get_option("crm_hyperdiff_timescale") == ref.TAU
    modules.hyperdiffusion(c)
    torch.cuda.synchronize()
    for n, v in state.items():
        got = dm.get(n, readonly=True).cpu().numpy()
        if n == "density_dry":
            assert ref.same_bits(got, v)
        else:
            assert ref.same_bits(got, ref.hyperdiffusion([v], [positive.get(n, 0)], ref.DT, ref.TAU)[0], nan_by_place=True), n
    assert (dm.get("free", readonly=True) < 0).any() and (dm.get("water_vapor", readonly=True) >= 0).all()
    dm.get("temp").copy_(torch.from_numpy(state["temp"]))
    modules.hyperdiffusion(c, dt=ref.TAU)
    torch.cuda.synchronize()
    assert ref.same_bits(dm.get("temp", readonly=True).cpu().numpy(), ref.hyperdiffusion([state["temp"]], [0], ref.TAU, ref.TAU)[0])


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ adaptor through the driver

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
def test_gpu_driver_one_step_equals_the_c_abi_call_on_the_plain_step(tmp_path):
    """one CRM step without sponge layer and physics: the run with --hyperdiff ends in the module, so its fields are the C ABI's call on
    the fields of the run without it (Kessler's three tracers are registered as positive); density_dry is the plain run's"""
    a, b = tmp_path / "plain.bin", tmp_path / "hd.bin"
    la = _run_driver("--steps", "1", "--no-micro", "--no-sponge", str(a))
    lb = _run_driver("--steps", "1", "--no-micro", "--no-sponge", "--hyperdiff", "60", str(b))
    assert json.loads(lb[-2]) == dict(hyperdiff_timescale=60)
    last = json.loads(lb[-1])
    assert last["crm_steps"] == 1 and last["finite"] is True and json.loads(la[-1])["crm_steps"] == 1
    plain, got = _fields(a, last), _fields(b, last)
    assert len(plain) == 8 and ref.same_bits(got[0], plain[0])
    want = GpuBackend().run(plain[1:], [0, 0, 0, 0, 1, 1, 1], last["dt_crm_phys"], 60.0)
    assert ref.results_differ(got[1:], want) == []
    assert not ref.same_bits(got[4], plain[4])


@pytest.mark.gpu
def test_gpu_driver_kessler_run_with_hyperdiffusion_keeps_the_tracers_non_negative(tmp_path):
    """the whole GCM step of 12 CRM steps with sponge layer and Kessler: nothing is refused, every tracer ends non-negative, and the
    run is not the plain one; with --accelerate and --vt the option composes"""
    a, b, vt = tmp_path / "hd.bin", tmp_path / "all.bin", tmp_path / "vt.json"
    lines = _run_driver("--hyperdiff", "120", str(a))
    last = json.loads(lines[-1])
    assert last["finite"] is True and last["crm_steps"] == 12 and last["tracer_min"] >= 0
    for t in _fields(a, last)[5:]:
        assert (t >= 0).all()
    lines = _run_driver("--hyperdiff", "120", "--accelerate", "2", "--vt", "1e-4", str(vt), str(b))
    last = json.loads(lines[-1])
    assert last["finite"] is True and last["crm_steps"] == 4 and json.loads(lines[-4]) == dict(hyperdiff_timescale=120)
    assert a.read_bytes() != b.read_bytes()


@pytest.mark.gpu
def test_gpu_binary_input_driver_takes_the_option(tmp_path):
    """the binary-input driver with dycore -> sponge_layer -> hyperdiffusion -> Kessler: one handle against three ranks, the same bits,
    and not the run without the option"""
    from test_cpp_driver import _kessler_case, _write_input
    nx, ny, nz, crm_dt, tr, consts, zint, f = _kessler_case(nens=6)
    inp = str(tmp_path / "in.bin")
    _write_input(inp, f, tr, zint, nx * 500.0, nx * 500.0, crm_dt, 2, 1 | 2 | 4, consts=None)
    outs = []
    for args in (["--gpus", "1", "--hyperdiff", "30"], ["--gpus", "3", "--hyperdiff", "30"], []):
        outp = str(tmp_path / ("out%d.bin" % len(outs)))
        r = subprocess.run([DRIVER] + args + [inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(np.fromfile(outp, dtype="<f8"))
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1])
    assert not np.array_equal(outs[0], outs[2])
