"""CRM variance transport on the GPU: the HIP path against the numpy restatement (tests/vt_ref.py) bit for bit on every shape and named
case, run to run, and members split over two calls against the whole ensemble; the Python adaptor through a coupler; and the C++
driver's loop end to end on a shortened CI input (tests/golden/msa_input.yaml)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import vt_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")


class GpuBackend:
    """the interface of vt_ref.RefBackend over the C ABI; grid: (ny, nx) of the fields' ncol.  Without use_u the uvel pointer and entry
    [2] of every table are NULL."""

    def __init__(self, grid):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check = torch, capi.load(), capi.check
        self.ny, self.nx = grid

    def _dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def _fields(self, st, use_u):
        return [self._dev(st.get(f)) if (f != "uvel" or use_u) else None for f in ref.FIELDS]

    @staticmethod
    def _ptrs(ts):
        return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])

    def _table(self, d, use_u):
        return self._ptrs([d[q] if q in ref.quantities(use_u) else None for q in ref.QUANTITIES])

    def _new(self, nz, nens, use_u):
        return {q: self.torch.full((nz, nens), float("nan"), dtype=self.torch.float64, device="cuda:0") for q in ref.quantities(use_u)}

    def _up(self, d, use_u):
        return {q: self._dev(d[q]) for q in ref.quantities(use_u)}

    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def _host(self, d):
        self.torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}

    def diagnose(self, st, use_u):
        nz, ncol, nens = st["temp"].shape
        assert ncol == self.ny * self.nx
        fields, mean, var = self._fields(st, use_u), self._new(nz, nens, use_u), self._new(nz, nens, use_u)
        self.check(self.lib.pam_amd_vt_diagnose(nens, self.nx, self.ny, nz, self._ptrs(fields), int(use_u), self._table(mean, use_u),
                                                self._table(var, use_u), self._stream()))
        return self._host(mean), self._host(var)

    def forcing(self, st, use_u, tend, dt, lim):
        nz, ncol, nens = st["temp"].shape
        fields, td = self._fields(st, use_u), self._up(tend, use_u)
        mean, var, scale = (self._new(nz, nens, use_u) for _ in range(3))
        self.check(self.lib.pam_amd_vt_forcing(nens, self.nx, self.ny, nz, self._ptrs(fields), int(use_u), self._table(td, use_u), float(dt),
                                               float(lim), self._table(mean, use_u), self._table(var, use_u), self._table(scale, use_u),
                                               self._stream()))
        return self._host(mean), self._host(var), self._host(scale)

    def apply(self, st, use_u, mean, scale):
        nz, ncol, nens = st["temp"].shape
        dev = {f: (self._dev(st.get(f)) if (f != "uvel" or use_u) else None) for f in ref.FIELDS}
        mn, sc = self._up(mean, use_u), self._up(scale, use_u)
        self.check(self.lib.pam_amd_vt_apply(nens, self.nx, self.ny, nz, self._ptrs([dev[f] for f in ref.FIELDS]), int(use_u),
                                             self._table(mn, use_u), self._table(sc, use_u), self._stream()))
        return self._host(dev)

    def feedback(self, st, use_u, var_start, gcm_dt):
        nz, ncol, nens = st["temp"].shape
        fields, vs = self._fields(st, use_u), self._up(var_start, use_u)
        mean, var, fb = (self._new(nz, nens, use_u) for _ in range(3))
        self.check(self.lib.pam_amd_vt_feedback(nens, self.nx, self.ny, nz, self._ptrs(fields), int(use_u), self._table(vs, use_u),
                                                float(gcm_dt), self._table(mean, use_u), self._table(var, use_u), self._table(fb, use_u),
                                                self._stream()))
        return self._host(mean), self._host(var), self._host(fb)


def _check(got, shape, name):
    """mean, var, scale and feedback against the restatement bit for bit -- the scale too: a correctly rounded root and a true division.
    Then the fields and what follows them against the restatement FED THE DEVICE'S OWN SCALE TABLE, so that a difference in the root can
    neither hide in the apply nor be blamed on it."""
    want = ref.reference(shape, name)
    assert ref.results_differ(got, want, tables=("start_mean", "var_start", "mean", "var", "scale")) == [], name
    fed = ref.run_case(ref.RefBackend(), ref.cases(shape)[name], scale_from=got)
    assert ref.results_differ(got, fed, tables=("end_mean", "end_var", "feedback")) == [], name
    assert ref.results_differ(got, want) == [], name


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_gpu_matches_restatement_bit_for_bit(shape):
    """every table and every field of every named case; the base case twice: two runs are identical"""
    be = GpuBackend(shape[0][1:])
    for name in ref.CASE_NAMES:
        _check(ref.run_case(be, ref.cases(shape)[name]), shape, name)
    _check(ref.run_case(be, ref.cases(shape)["base"]), shape, "base")


def _members(st, sl):
    return {k: (None if v is None else np.ascontiguousarray(v[..., sl])) for k, v in st.items()}


def _join(parts):
    return {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts], axis=-1)) for k in parts[0]}


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ref.GRIDS, ids=lambda g: "%dx%dx%d" % g)
def test_gpu_members_in_two_calls_equal_the_whole_ensemble(grid):
    """members [0:37] and [37:130] as separate calls: the whole ensemble's bits, everything being per member"""
    shape = (grid, 130)
    be = GpuBackend(grid[1:])
    cuts = (slice(0, 37), slice(37, 130))
    for name in ref.CASE_NAMES:
        case = ref.cases(shape)[name]
        parts = [ref.run_case(be, dict(case, start=_members(case["start"], sl), now=_members(case["now"], sl), tend=_members(case["tend"], sl)))
                 for sl in cuts]
        got = {k: _join([p[k] for p in parts]) for k in parts[0]}
        _check(got, shape, name)


def _coupler(shape, micro, **options):
    from pam_amd import PamCoupler
    (nz, ny, nx), nens = shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", 20.0)
    c.set_option("gcm_physics_dt", 240.0)
    for k, v in options.items():
        c.set_option(k, v)
    c.allocate_coupler_state(nz, ny, nx, nens)
    tracers = {"kessler": ("water_vapor", "cloud_liquid", "precip_liquid"), "p3": ("water_vapor", "cloud_water", "ice"),
               "none": ("water_vapor",)}[micro]
    for t in tracers:
        c.add_tracer(t, "", True, True)
    c.set_option("micro", micro)
    return c


def _load(c, st, names):
    import torch
    (nz, ny, nx, nens) = (c.get_nz(), c.get_ny(), c.get_nx(), c.get_nens())
    dm = c.get_data_manager_device_readwrite()
    for ours, theirs in names.items():
        if st.get(ours) is not None:
            dm.get(theirs).copy_(torch.from_numpy(st[ours].reshape(nz, ny, nx, nens)))


@pytest.mark.gpu
@pytest.mark.parametrize("micro, case_name, use_u", [("kessler", "no_ice", True), ("p3", "base", True), ("none", "vapour_only", True),
                                                     ("p3", "use_u_off", False), ("p3", "dry_cells", True)])
def test_gpu_python_adaptor_through_a_coupler(micro, case_name, use_u):
    """vt_init / vt_apply_forcing / vt_compute_feedback with the entry names each microphysics registers: the restatement's bits in the
    fields and in the coupler's vt_* entries; the options and their defaults; vt_tend_* zero-filled; no _u entry without crm_vt_u"""
    import torch
    from pam_amd import modules
    shape = ((3, 4, 5), 65)
    case, want = ref.cases(shape)[case_name], ref.reference(shape, case_name)
    names = dict(temp="temp", water_vapor="water_vapor", uvel="uvel")
    if micro != "none":
        names["cloud"] = "cloud_liquid" if micro == "kessler" else "cloud_water"
    if micro == "p3":
        names["ice"] = "ice"
    c = _coupler(shape, micro, **({"crm_vt_u": True} if use_u else {}))
    dm = c.get_data_manager_device_readwrite()
    _load(c, case["start"], names)
    u_before = dm.get("uvel", readonly=True).clone()
    modules.vt_init(c)
    assert c.get_option("crm_vt_scale_limit") == 0.05 and c.get_option("crm_vt_u") is use_u
    qs = ref.quantities(use_u)
    for n in ("mean", "var", "var_start", "scale", "tend", "feedback"):
        assert dm.entry_exists("vt_%s_u" % n) is use_u
        assert all(tuple(dm.get("vt_%s_%s" % (n, q), readonly=True).shape) == (3, 65) for q in qs)
    for q in qs:
        assert (dm.get("vt_tend_" + q, readonly=True) == 0).all()
        assert ref.same_bits(dm.get("vt_var_start_" + q, readonly=True).cpu().numpy(), want["var_start"][q]), q
        dm.get("vt_tend_" + q).copy_(torch.from_numpy(case["tend"][q]))
    _load(c, case["now"], names)
    modules.vt_apply_forcing(c)
    modules.vt_compute_feedback(c)
    torch.cuda.synchronize()
    for ours, theirs in names.items():
        if want["fields"].get(ours) is not None:
            assert ref.same_bits(dm.get(theirs, readonly=True).cpu().numpy().reshape(want["fields"][ours].shape), want["fields"][ours]), ours
    if not use_u:
        assert torch.equal(dm.get("uvel", readonly=True), u_before)
    for q in qs:
        for entry, key in (("scale", "scale"), ("var", "end_var"), ("mean", "end_mean"), ("feedback", "feedback"), ("var_start", "var_start")):
            assert ref.same_bits(dm.get("vt_%s_%s" % (entry, q), readonly=True).cpu().numpy(), want[key][q]), (entry, q)
    modules.vt_init(c)                                   # the next GCM step: the tendencies stay, the start variance is the state's
    for q in qs:
        assert ref.same_bits(dm.get("vt_tend_" + q, readonly=True).cpu().numpy(), case["tend"][q])
        assert ref.same_bits(dm.get("vt_var_start_" + q, readonly=True).cpu().numpy(), want["end_var"][q]), q


@pytest.mark.gpu
def test_gpu_python_adaptor_takes_the_step_length_of_an_accelerated_step():
    from pam_amd import modules
    import torch
    shape = ((3, 4, 5), 3)
    case = ref.cases(shape)["base"]
    names = dict(temp="temp", water_vapor="water_vapor", uvel="uvel")
    c = _coupler(shape, "none", crm_vt_u=True, crm_vt_scale_limit=0.25)
    _load(c, case["now"], names)
    modules.vt_init(c)
    dm = c.get_data_manager_device_readwrite()
    for q in ref.QUANTITIES:
        dm.get("vt_tend_" + q).copy_(torch.from_numpy(case["tend"][q]))
    modules.vt_apply_forcing(c, dt=60.0)
    torch.cuda.synchronize()
    st = {k: (None if k in ("cloud", "ice") else v) for k, v in case["now"].items()}
    _, _, scale = ref.forcing(st, True, case["tend"], 60.0, 0.25)
    for q in ref.QUANTITIES:
        assert ref.same_bits(dm.get("vt_scale_" + q, readonly=True).cpu().numpy(), scale[q]), q


# ------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ driver: one GCM step of nstop = 12 CRM steps

def _run_driver(*args, timeout=600):
    r = subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3"] + list(args), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().split("\n")


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("vt_plain")
    out = d / "plain.bin"
    lines = _run_driver(str(out))
    return dict(lines=lines, out=out.read_bytes())


def _vt_lines(path):
    return [json.loads(line) for line in open(path).read().splitlines()]


@pytest.mark.gpu
def test_gpu_driver_zero_rate_is_the_plain_run_bit_for_bit(plain_run, tmp_path):
    out, vt = tmp_path / "zero.bin", tmp_path / "zero.json"
    lines = _run_driver("--vt", "0", str(vt), str(out))
    assert json.loads(lines[-2]) == dict(vt_rate=0, vt_u=False, vt_limit=0.05)
    assert lines[-1] == plain_run["lines"][-1]
    assert out.read_bytes() == plain_run["out"]
    rec = _vt_lines(vt)
    assert len(rec) == 1 and set(rec[0]["var"]) == {"t", "q"}


@pytest.mark.gpu
def test_gpu_driver_nonzero_rate_changes_the_run_and_reports_the_feedback(plain_run, tmp_path):
    out, vt = tmp_path / "vt.bin", tmp_path / "vt.json"
    lines = _run_driver("--vt", "2e-4", str(vt), "--vt-u", "--vt-limit", "0.1", str(out))
    assert json.loads(lines[-2]) == dict(vt_rate=2e-4, vt_u=True, vt_limit=0.1)
    last = json.loads(lines[-1])
    assert last["finite"] is True and last["crm_steps"] == 12
    raw = np.fromfile(out, dtype=np.float64)
    assert raw.size == len(plain_run["out"]) // 8 and np.isfinite(raw).all() and raw.tobytes() != plain_run["out"]
    rec = _vt_lines(vt)
    assert len(rec) == 1 and rec[0]["gcm_step"] == 0
    n = last["nz"] * last["nens"]
    for q in ("t", "q", "u"):
        vs, v, fb = (np.array(rec[0][k][q]) for k in ("var_start", "var", "feedback"))
        assert vs.shape == v.shape == fb.shape == (n,) and np.isfinite(v).all()
        assert ref.same_bits(fb, (v - vs) / 240.0), q
    assert any((np.array(rec[0]["var_start"][q]) > 0).any() for q in ("t", "q", "u"))


@pytest.mark.gpu
def test_gpu_driver_accelerated_run_with_a_zero_rate_is_the_accelerated_run(tmp_path):
    a, b, vt = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "b.json"
    la = _run_driver("--accelerate", "2", str(a))
    lb = _run_driver("--accelerate", "2", "--vt", "0", str(vt), str(b))
    assert la[-1] == lb[-1] and la[-2] == lb[-3] and json.loads(lb[-1])["crm_steps"] == 4
    assert a.read_bytes() == b.read_bytes()


@pytest.mark.gpu
def test_gpu_driver_refuses_a_limit_outside_the_unit_interval(tmp_path):
    r = subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3", "--vt", "1e-4", str(tmp_path / "x.json"), "--vt-limit", "1.5", "-"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "crm_vt_scale_limit" in r.stderr


@pytest.mark.gpu
def test_gpu_driver_sharded_run_equals_unsharded_bit_for_bit(tmp_path):
    """the binary-input driver with dycore -> sponge_layer -> Kessler, nstop = 2 and --vt RATE: one handle against three ranks
    (44 + 43 + 43 members).  Everything is per member, so no rank waits for another; the fields are the same bits and not the plain run's"""
    from test_cpp_driver import _kessler_case, _write_input
    nx, ny, nz, crm_dt, tr, consts, zint, f = _kessler_case(nens=130)
    inp = str(tmp_path / "in.bin")
    _write_input(inp, f, tr, zint, nx * 500.0, nx * 500.0, crm_dt, 2, 1 | 2 | 4, consts=None)
    outs = []
    for args in (["--gpus", "1", "--vt", "1e-3", "--vt-u"], ["--gpus", "3", "--vt", "1e-3", "--vt-u"], []):
        outp = str(tmp_path / ("out%d.bin" % len(outs)))
        r = subprocess.run([DRIVER] + args + [inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(np.fromfile(outp, dtype="<f8"))
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1])
    assert not np.array_equal(outs[0], outs[2])
