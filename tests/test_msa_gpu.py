"""CRM mean-state acceleration on the GPU: the HIP path against the numpy restatement (tests/msa_ref.py) bit for bit on every shape and
named case, run to run, and members split over two calls against the whole ensemble; the Python adaptor through a coupler; the
time-average weight; and the C++ driver's accelerated loop end to end on a shortened CI input (tests/golden/msa_input.yaml)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import msa_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
MSA_YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")


class GpuBackend:
    """the interface of msa_ref.RefBackend over the C ABI; grid: (ny, nx) of the fields' ncol"""

    def __init__(self, grid):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check = torch, capi.load(), capi.check
        self.ny, self.nx = grid

    def _dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    @staticmethod
    def _table(ts):
        return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])

    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def _host(self, d):
        self.torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}

    def diagnose(self, st):
        nz, ncol, nens = st["temp"].shape
        assert ncol == self.ny * self.nx
        fields = [self._dev(st.get(f)) for f in ref.FIELDS]
        save = {q: self.torch.full((nz, nens), float("nan"), dtype=self.torch.float64, device="cuda:0") for q in ref.QUANTITIES}
        self.check(self.lib.pam_amd_msa_diagnose(nens, self.nx, self.ny, nz, self._table(fields), self._table(list(save.values())),
                                                 self._stream()))
        return self._host(save)

    def tendencies(self, st, save, max_ttend, cease, host_flag=True):
        nz, ncol, nens = st["temp"].shape
        fields = [self._dev(st.get(f)) for f in ref.FIELDS]
        sv = [self._dev(save[q]) for q in ref.QUANTITIES]
        tend = {q: self.torch.full((nz, nens), float("nan"), dtype=self.torch.float64, device="cuda:0") for q in ref.QUANTITIES}
        flag = self.torch.tensor([int(cease)], dtype=self.torch.int32, device="cuda:0")
        host = C.c_int(-1)
        self.check(self.lib.pam_amd_msa_tendencies(nens, self.nx, self.ny, nz, self._table(fields), self._table(sv),
                                                   self._table(list(tend.values())), float(max_ttend), flag.data_ptr(),
                                                   C.byref(host) if host_flag else None, self._stream()))
        out = self._host(tend)
        dev = int(flag.item())
        assert not host_flag or host.value == dev
        return out, dev

    def apply(self, st, tend, a, accel_uv, cease):
        nz, ncol, nens = st["temp"].shape
        dev = {f: self._dev(st.get(f)) for f in ref.FIELDS}
        td = [self._dev(tend[q]) for q in ref.QUANTITIES]
        flag = self.torch.tensor([int(cease)], dtype=self.torch.int32, device="cuda:0")
        self.check(self.lib.pam_amd_msa_apply(nens, self.nx, self.ny, nz, self._table([dev[f] for f in ref.FIELDS]), self._table(td), float(a),
                                              int(bool(accel_uv)), flag.data_ptr(), self._stream()))
        return self._host(dev)


def _members(st, sl):
    return {k: (None if v is None else np.ascontiguousarray(v[..., sl])) for k, v in st.items()}


def _join(parts):
    return {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts], axis=-1)) for k in parts[0]}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_gpu_matches_restatement_bit_for_bit(shape):
    """save, tend, every field and the flag of every named case; the base case twice: two runs are identical"""
    be = GpuBackend(shape[0][1:])
    for name in ref.CASE_NAMES:
        got = ref.run_case(be, ref.cases(shape)[name])
        assert ref.results_differ(got, ref.reference(shape, name)) == [], name
    again = ref.run_case(be, ref.cases(shape)["base"])
    assert ref.results_differ(again, ref.reference(shape, "base")) == []


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ref.GRIDS, ids=lambda g: "%dx%dx%d" % g)
def test_gpu_members_in_two_calls_equal_the_whole_ensemble(grid):
    """members [0:37] and [37:130] as separate calls, their flags ORed by hand between tendencies and apply (the flag is global over
    the members, everything else is per member): the whole ensemble's bits, flag included, in every named case"""
    shape = (grid, 130)
    be = GpuBackend(grid[1:])
    cuts = (slice(0, 37), slice(37, 130))
    for name in ref.CASE_NAMES:
        case = ref.cases(shape)[name]
        saves = [be.diagnose(_members(case["before"], sl)) for sl in cuts]
        tends, flags = zip(*[be.tendencies(_members(case["after"], sl), sv, case["max_ttend"], case["cease_in"])
                             for sl, sv in zip(cuts, saves)])
        cease = flags[0] | flags[1]
        outs = [be.apply(_members(case["after"], sl), td, case["a"], case["accel_uv"], cease) for sl, td in zip(cuts, tends)]
        got = dict(save=_join(saves), tend=_join(tends), cease=cease, fields=_join(outs))
        assert ref.results_differ(got, ref.reference(shape, name)) == [], name
        if name == "nan_in_temp":
            assert sorted(flags) == [0, 1]            # one shard alone saw it; the other one's apply held still all the same


@pytest.mark.gpu
def test_gpu_tendencies_without_a_host_flag_set_the_device_word_all_the_same():
    shape = ((5, 1, 17), 3)
    be = GpuBackend((1, 17))
    case = ref.cases(shape)["nan_in_temp"]
    want = ref.reference(shape, "nan_in_temp")
    tend, flag = be.tendencies(case["after"], want["save"], case["max_ttend"], 0, host_flag=False)
    assert flag == 1 and all(ref.same_bits(tend[q], want["tend"][q]) for q in ref.QUANTITIES)


def _coupler(shape, micro):
    from pam_amd import PamCoupler
    (nz, ny, nx), nens = shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", 20.0)
    c.set_option("gcm_physics_dt", 240.0)
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


def _dump(c, names, like):
    import torch
    torch.cuda.synchronize()
    dm = c.get_data_manager_device_readwrite()
    return {ours: (None if like.get(ours) is None else dm.get(theirs, readonly=True).cpu().numpy().reshape(like[ours].shape))
            for ours, theirs in names.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("micro, case_name", [("kessler", "no_ice"), ("p3", "base"), ("none", "vapour_only"), ("p3", "nan_in_temp")])
def test_gpu_python_adaptor_through_a_coupler(micro, case_name):
    """msa_init / msa_diagnose / msa_accelerate with the entry names each microphysics registers: the restatement's bits, the saved
    means and tendencies in the coupler's accel_* entries, the option crm_accel_ceaseflag, and a flag that stays up until the next init"""
    from pam_amd import modules
    shape = ((3, 4, 5), 65)
    case, want = ref.cases(shape)[case_name], ref.reference(shape, case_name)
    names = dict(temp="temp", water_vapor="water_vapor", uvel="uvel", vvel="vvel")
    if micro != "none":
        names["cloud"] = "cloud_liquid" if micro == "kessler" else "cloud_water"
    if micro == "p3":
        names["ice"] = "ice"
    c = _coupler(shape, micro)
    c.set_option("crm_accel_factor", case["a"])
    c.set_option("crm_accel_uv", case["accel_uv"])
    modules.msa_init(c)
    assert c.get_option("crm_accel_max_ttend") == 5.0 and c.get_option("crm_accel_ceaseflag") is False
    _load(c, case["before"], names)
    modules.msa_diagnose(c)
    _load(c, case["after"], names)
    ceased = modules.msa_accelerate(c)
    assert ceased == bool(want["cease"]) and c.get_option("crm_accel_ceaseflag") == ceased
    got = _dump(c, names, case["after"])
    for f in names:
        assert ref.same_bits(got[f], want["fields"][f]), f
    dm = c.get_data_manager_device_readwrite()
    for q in ref.QUANTITIES:
        assert ref.same_bits(dm.get("accel_save_" + q, readonly=True).cpu().numpy(), want["save"][q]), q
        assert ref.same_bits(dm.get("accel_tend_" + q, readonly=True).cpu().numpy(), want["tend"][q]), q
    if ceased:                          # sticky: a clean step after it is not accelerated either, until the next GCM step's init
        _load(c, case["before"], names)
        modules.msa_diagnose(c)
        _load(c, ref.cases(shape)["base"]["after"], names)
        assert modules.msa_accelerate(c) is True
        assert ref.same_bits(_dump(c, names, case["after"])["temp"], ref.cases(shape)["base"]["after"]["temp"])
        modules.msa_init(c)
        assert c.get_option("crm_accel_ceaseflag") is False
        modules.msa_diagnose(c)
        assert modules.msa_accelerate(c) is False


@pytest.mark.gpu
def test_gpu_time_average_weight_multiplies_the_factor():
    """weight w: tavg += var * (crm_dt / gcm_dt * w), the product rounded before the add; the default is the call of before"""
    import torch
    from pam_amd import modules
    shape = ((3, 4, 5), 3)
    c = _coupler(shape, "none")
    v = ref.cases(shape)["base"]["after"]["uvel"].reshape(3, 4, 5, 3)
    c.get_data_manager_device_readwrite().get("uvel").copy_(torch.from_numpy(v))
    modules.time_average_init(c, ["uvel"])
    modules.time_average_accumulate(c, ["uvel"])
    modules.time_average_accumulate(c, ["uvel"], weight=3)
    modules.time_average_accumulate(c, ["uvel"], 1)
    torch.cuda.synchronize()
    f = 20.0 / 240.0
    want = ((0.0 + v * f) + v * (f * 3.0)) + v * (f * 1.0)
    assert ref.same_bits(c.get_data_manager_device_readwrite().get("uvel_time_average", readonly=True).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ driver: one GCM step of nstop = 12 CRM steps

def _run_driver(*args, timeout=600):
    r = subprocess.run([DRIVER, "--yaml", MSA_YAML, "--nens", "3"] + list(args), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().split("\n")


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("msa_plain")
    out, stats = d / "plain.bin", d / "plain.json"
    lines = _run_driver("--stats", str(stats), str(out))
    return dict(last=json.loads(lines[-1]), lines=lines, out=out.read_bytes(), stats=json.loads(stats.read_text()))


@pytest.mark.gpu
def test_gpu_driver_accelerated_run_takes_a_third_of_the_steps(plain_run, tmp_path):
    assert plain_run["last"]["crm_steps"] == 12
    out = tmp_path / "accel.bin"
    lines = _run_driver("--accelerate", "2", "--accel-uv", str(out))
    last, accel = json.loads(lines[-1]), json.loads(lines[-2])
    assert last["crm_steps"] == 4 and last["finite"] is True and last["etime"] == plain_run["last"]["etime"] == 240.0
    assert accel == dict(accel_factor=2, accel_uv=True, accel_max_ttend=5, accelerated_steps=4, ceased_gcm_steps=0)
    raw = np.fromfile(out, dtype=np.float64)
    assert raw.size == len(plain_run["out"]) // 8 and np.isfinite(raw).all()
    assert raw.tobytes() != plain_run["out"]


@pytest.mark.gpu
def test_gpu_driver_ceased_run_is_the_plain_run_bit_for_bit(plain_run, tmp_path):
    """--accel-max-ttend 1e-300: the first step's tendencies cease, nothing is ever applied, 12 steps run; diagnose and tendencies
    write no state, so the output, the final line and the --stats profiles are the plain run's"""
    out, stats = tmp_path / "ceased.bin", tmp_path / "ceased.json"
    lines = _run_driver("--accelerate", "2", "--accel-max-ttend", "1e-300", "--stats", str(stats), str(out))
    accel = json.loads(lines[-2])
    assert accel["accelerated_steps"] == 0 and accel["ceased_gcm_steps"] == 1
    assert json.loads(lines[-1])["crm_steps"] == 12
    assert lines[-1] == plain_run["lines"][-1]
    assert out.read_bytes() == plain_run["out"]
    st = json.loads(stats.read_text())
    assert [g["crm_steps"] for g in st["gcm_steps"]] == [12]
    assert json.dumps(st, sort_keys=True) == json.dumps(plain_run["stats"], sort_keys=True)


@pytest.mark.gpu
def test_gpu_driver_refuses_a_factor_that_does_not_divide_the_steps(tmp_path):
    r = subprocess.run([DRIVER, "--yaml", MSA_YAML, "--accelerate", "4", "-"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "must be an integer that divides" in r.stderr


# ------------------------------------------------------------------------------------------------------------------------------
# driver --gpus N: the ranks OR their cease flags on the host

@pytest.mark.gpu
@pytest.mark.parametrize("max_ttend, steps, ceased", [("5", 2, False), ("1e-300", 4, True)], ids=["accelerated", "ceased"])
def test_gpu_driver_sharded_accelerated_loop_equals_unsharded_bit_for_bit(tmp_path, max_ttend, steps, ceased):
    """the binary-input driver with dycore -> sponge_layer -> Kessler, nstop = 4 and --accelerate 1: one handle against three ranks
    (44 + 43 + 43 members), with and without a cease.  Every rank takes the same number of steps, and the fields are the same bits."""
    from pam_amd import idealized as idz
    from test_cpp_driver import _kessler_case, _write_input
    nx, ny, nz, crm_dt, tr, consts, zint, f = _kessler_case(nens=130)
    inp = str(tmp_path / "in.bin")
    _write_input(inp, f, tr, zint, nx * 500.0, nx * 500.0, crm_dt, 4, 1 | 2 | 4, consts=None)
    outs = []
    for n in (1, 3):
        outp = str(tmp_path / ("out%d.bin" % n))
        r = subprocess.run([DRIVER, "--gpus", str(n), "--accelerate", "1", "--accel-uv", "--accel-max-ttend", max_ttend, inp, outp],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
        assert line == dict(accel_factor=1, crm_steps=steps, ceased=ceased)
        outs.append(np.fromfile(outp, dtype="<f8"))
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1])
    if ceased:                                     # nothing was applied: the plain four steps
        plain = str(tmp_path / "plain.bin")
        r = subprocess.run([DRIVER, inp, plain], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.fromfile(plain, dtype="<f8"), outs[0])
