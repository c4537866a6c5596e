"""modules::horizontal_average and modules::time_average_init / time_average_accumulate (pam_core/modules/horizontal_average.h,
time_average.h): the CPU restatement (tests/statistics_ref.py) against a scalar loop, the host emulation of the device bodies
(pam_amd/csrc/statistics_device.h under g++) against the restatement bit for bit, the C ABI's argument checks, the adaptors' boundary,
and on the GPU the HIP path against the restatement bit for bit, the deviations of DESIGN.md section 8 and the driver's --stats."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import statistics_ref as ref
import test_boundary_surface as tb
from pam_amd import capi
from tools.native_build import emu_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
DRIVER = os.path.join(ROOT, "examples", "driver")
CI_YAML = os.path.join(ROOT, "tests", "golden", "ci_input_pama.yaml")
_DP = C.POINTER(C.c_double)

# (shape without the member dimension, has_vertical_dim): the state's (nz,ny,nx), a 2-D slice (ny = 1), (nz,ncol), one level,
# (ny,nx) and (ncol) without a vertical dimension
SHAPES = [((60, 32, 32), True), ((50, 1, 65), True), ((7, 33), True), ((1, 7), True), ((5, 6), False), ((19,), False)]
SHAPE_IDS = ["nz60_32x32", "nz50_1x65", "nz7_ncol33", "nz1_ncol7", "ny5_nx6", "ncol19"]
NENS = [1, 3, 64, 65, 130]


def field(shape, seed):
    """values of mixed sign and magnitude (10^-3 .. 10^3), so that the order of summation shows in the last bits"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape))


# ------------------------------------------------------------------------------------------------------------------------------
# host emulation

def emu():
    lib = C.CDLL(emu_library("statistics_emu"))
    lib.emu_horizontal_average.argtypes = [C.c_int] * 3 + [_DP] * 2
    lib.emu_time_average_accumulate.argtypes = [C.c_longlong, _DP, _DP, C.c_double]
    return lib


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def emu_horizontal_average(lib, var, has_vertical_dim):
    nz, ncol, nens = ref.collapse(var.shape, has_vertical_dim)
    out = np.empty((nz, nens))
    lib.emu_horizontal_average(nz, ncol, nens, _p(np.ascontiguousarray(var)), _p(out))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement

def test_restatement_is_the_reference_loop():
    """the vectorised restatement equals a scalar transcription of horizontal_average.h:67-73 -- and differs from np.sum's
    pairwise order on this data, so the order is what the comparisons pin"""
    v = field((3, 37, 5), seed=1)
    want = np.zeros((3, 5))
    for k in range(3):
        for e in range(5):
            acc, r = 0.0, 1.0 / 37
            for i in range(37):
                acc += float(v[k, i, e]) * r
            want[k, e] = acc
    assert np.array_equal(ref.horizontal_average(v), want)
    big = field((1, 4096, 64), seed=2)
    pairwise = np.ascontiguousarray((big * (1.0 / 4096)).transpose(0, 2, 1)).sum(axis=2)   # contiguous axis: numpy sums pairwise
    assert not np.array_equal(ref.horizontal_average(big), pairwise)


def test_restatement_shapes_follow_the_reference():
    assert ref.collapse((60, 32, 32, 4), True) == (60, 1024, 4)
    assert ref.collapse((7, 33, 4), True) == (7, 33, 4)
    assert ref.collapse((5, 6, 4), False) == (1, 30, 4)
    assert ref.collapse((19, 4), False) == (1, 19, 4)
    for shape, vert in (((4,), True), ((3, 4), True), ((2, 2, 2, 2, 4), True), ((4,), False), ((2, 3, 5, 4), False)):
        with pytest.raises(ValueError):
            ref.collapse(shape, vert)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the host emulation of the device bodies

@pytest.mark.parametrize("nens", NENS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_emulation_horizontal_average_matches_restatement_bit_for_bit(shape, nens):
    dims, vert = shape
    lib = emu()
    v = field(dims + (nens,), seed=nens + len(dims))
    assert np.array_equal(emu_horizontal_average(lib, v, vert), ref.horizontal_average(v, vert))


def test_emulation_time_average_matches_restatement_bit_for_bit():
    lib = emu()
    f = ref.time_average_factor(20.0, 900.0)
    t = np.zeros(5000)
    want = np.zeros(5000)
    for s in range(6):
        v = field(5000, seed=100 + s)
        lib.emu_time_average_accumulate(t.size, _p(v), _p(t), f)
        want = ref.time_average_accumulate(want, v, f)
    assert np.array_equal(t, want)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the C ABI

NEW_SYMBOLS = ("pam_amd_horizontal_average", "pam_amd_time_average_zero", "pam_amd_time_average_accumulate")


def _header_symbols():
    import re
    text = open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))


def test_new_entry_points_are_exported_and_declared():
    lib = capi.load()
    declared = _header_symbols()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name


def test_new_entry_points_reject_bad_arguments_before_touching_a_device():
    lib = capi.load()
    P2 = (C.c_void_p * 2)(64, 64)              # never dereferenced: validation fails first
    P2null = (C.c_void_p * 2)(64, None)
    I2 = (C.c_int * 2)(3, 4)
    I2zero = (C.c_int * 2)(3, 0)
    L2 = (C.c_longlong * 2)(12, 7)
    L2zero = (C.c_longlong * 2)(12, 0)
    L2neg = (C.c_longlong * 2)(-1, 7)
    havg, zero, acc = lib.pam_amd_horizontal_average, lib.pam_amd_time_average_zero, lib.pam_amd_time_average_accumulate
    cases = [
        ("horizontal_average", lambda: havg(0, 2, I2, I2, P2, P2, None)),
        ("horizontal_average", lambda: havg(4, 0, I2, I2, P2, P2, None)),
        ("horizontal_average", lambda: havg(4, 2, None, I2, P2, P2, None)),
        ("horizontal_average", lambda: havg(4, 2, I2, None, P2, P2, None)),
        ("horizontal_average", lambda: havg(4, 2, I2zero, I2, P2, P2, None)),
        ("horizontal_average", lambda: havg(4, 2, I2, I2zero, P2, P2, None)),
        ("horizontal_average", lambda: havg(4, 2, I2, I2, P2null, P2, None)),
        ("horizontal_average", lambda: havg(4, 2, I2, I2, P2, P2null, None)),
        ("horizontal_average", lambda: havg(4, 2, I2, I2, None, P2, None)),
        ("time_average_zero", lambda: zero(0, L2, P2, None)),
        ("time_average_zero", lambda: zero(2, None, P2, None)),
        ("time_average_zero", lambda: zero(2, L2zero, P2, None)),
        ("time_average_zero", lambda: zero(2, L2neg, P2, None)),
        ("time_average_zero", lambda: zero(2, L2, P2null, None)),
        ("time_average_accumulate", lambda: acc(2, L2, P2, P2, float("nan"), None)),
        ("time_average_accumulate", lambda: acc(2, L2, P2, P2, float("inf"), None)),
        ("time_average_accumulate", lambda: acc(2, L2, P2null, P2, 0.5, None)),
        ("time_average_accumulate", lambda: acc(2, L2, P2, P2null, 0.5, None)),
        ("time_average_accumulate", lambda: acc(2, L2, None, P2, 0.5, None)),
        ("time_average_accumulate", lambda: acc(2, L2zero, P2, P2, 0.5, None)),
        ("time_average_accumulate", lambda: acc(-1, L2, P2, P2, 0.5, None)),
    ]
    for who, call in cases:
        assert call() == -1, who                                   # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert who.encode() in lib.pam_amd_awfl_last_error(), who


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the boundary of the C++ adaptors and the Python DataManager

ADAPTORS = [os.path.join(HOST, "modules", "horizontal_average.h"), os.path.join(HOST, "modules", "time_average.h")]
SIGNATURES = {   # signature -> the reference line it must match (tests/golden/extract_statistics.py records the digests)
    "void horizontal_average(pam::PamCoupler &coupler, std::vector<std::tuple<std::string,bool>> var_list)":
        "pam_core/modules/horizontal_average.h:25",
    "void time_average_init(pam::PamCoupler &coupler, std::vector<std::string> var_names)": "pam_core/modules/time_average.h:8",
    "void time_average_accumulate(pam::PamCoupler &coupler, std::vector<std::string> var_names)": "pam_core/modules/time_average.h:39",
}


@pytest.mark.parametrize("src", ADAPTORS, ids=[os.path.basename(s) for s in ADAPTORS])
def test_adaptors_call_only_members_the_reference_has(src):
    coupler, dm = tb._used_members(open(src).read())
    assert coupler and {"get_shape", "get_collapsed"} <= dm, (coupler, dm)
    assert coupler <= tb.REF_COUPLER, sorted(coupler - tb.REF_COUPLER)
    assert dm <= tb.REF_DM, sorted(dm - tb.REF_DM)
    ours = tb._declared(os.path.join(HOST, "pam_coupler.h"))
    assert (coupler | dm) <= ours, sorted((coupler | dm) - ours)


def test_adaptors_have_the_reference_signatures():
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "statistics_extract.json")))["signature_sha256"]
    assert sorted(rec) == sorted(SIGNATURES.values())
    text = "".join(tb._norm(tb._strip_comments(open(s).read())) for s in ADAPTORS)
    for sig, where in SIGNATURES.items():
        assert tb._digest(tb._norm(sig)) == rec[where], (sig, where)
        assert tb._norm(sig) + "{" in text, sig


def test_python_datamanager_get_shape_and_get_collapsed():
    import torch
    from pam_amd.coupler import DataManager
    dm = DataManager(torch.device("cpu"))
    t = dm.register_and_allocate("a", "", (3, 4, 5))
    assert dm.get_shape("a") == [3, 4, 5]
    dm.clean_all_entries()
    c = dm.get_collapsed("a", readonly=True)
    assert tuple(c.shape) == (60,) and c.data_ptr() == t.data_ptr() and dm.get_dirty_entries() == []
    dm.get_collapsed("a")[7] = 2.5
    assert t.view(-1)[7] == 2.5 and dm.get_dirty_entries() == ["a"]
    with pytest.raises(capi.PamAmdError):
        dm.get_shape("missing")


# ------------------------------------------------------------------------------------------------------------------------------
# GPU

def _coupler(nens, nz=2, ny=2, nx=2, crm_dt=20.0, gcm_dt=900.0):
    from pam_amd import PamCoupler
    c = PamCoupler("cuda:0")
    if crm_dt is not None:
        c.set_option("crm_dt", crm_dt)
    if gcm_dt is not None:
        c.set_option("gcm_physics_dt", gcm_dt)
    c.allocate_coupler_state(nz, ny, nx, nens)
    return c


def _put(c, name, arr):
    import torch
    dm = c.get_data_manager_device_readwrite()
    if not dm.entry_exists(name):
        dm.register_and_allocate(name, "", arr.shape)
    dm.get(name).copy_(torch.from_numpy(np.ascontiguousarray(arr)))


def _get(c, name):
    import torch
    torch.cuda.synchronize()
    return c.get_data_manager_device_readwrite().get(name, readonly=True).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("nens", NENS)
def test_gpu_horizontal_average_matches_restatement_for_every_shape_in_one_call(nens):
    """all shapes of SHAPES in one mixed-shape list (one launch), then each alone: the restatement's bits every time"""
    from pam_amd import modules
    c = _coupler(nens)
    names, want = [], {}
    for n, (dims, vert) in enumerate(SHAPES):
        v = field(dims + (nens,), seed=10 * nens + n)
        _put(c, "f%d" % n, v)
        names.append(("f%d" % n, vert))
        want["f%d" % n] = ref.horizontal_average(v, vert)
    modules.horizontal_average(c, names)
    for name, _ in names:
        got = _get(c, name + "_horizontal_average")
        assert got.shape == want[name].shape and np.array_equal(got, want[name]), name
    for name, vert in names:
        _put(c, name + "_horizontal_average", np.full(want[name].shape, -7.0))
        modules.horizontal_average(c, [(name, vert)])
        assert np.array_equal(_get(c, name + "_horizontal_average"), want[name]), name


@pytest.mark.gpu
def test_gpu_list_longer_than_one_launch_table_equals_per_field_calls():
    """70 fields -- three kernarg tables of at most 32 -- give the bits of 70 single-field calls"""
    from pam_amd import modules
    nens = 65
    c = _coupler(nens)
    lst = []
    for n in range(70):
        dims, vert = SHAPES[1 + n % (len(SHAPES) - 1)]
        _put(c, "g%d" % n, field(dims + (nens,), seed=500 + n))
        lst.append(("g%d" % n, vert))
    modules.horizontal_average(c, lst)
    whole = {n: _get(c, n + "_horizontal_average") for n, _ in lst}
    for n, vert in lst:
        modules.horizontal_average(c, [(n, vert)])
        assert np.array_equal(_get(c, n + "_horizontal_average"), whole[n]), n
    # the time averages too: one 70-field accumulate against the restatement
    names = [n for n, _ in lst]
    modules.time_average_init(c, names)
    modules.time_average_accumulate(c, names)
    f = ref.time_average_factor(20.0, 900.0)
    for n in names:
        assert np.array_equal(_get(c, n + "_time_average"), ref.time_average_accumulate(0.0, _get(c, n), f)), n


@pytest.mark.gpu
def test_gpu_members_split_over_two_couplers_give_the_whole_bits():
    from pam_amd import modules
    n1, n2 = 37, 93
    vals = {n: field(dims + (n1 + n2,), seed=900 + i) for i, (n, dims) in enumerate((("a", (60, 32, 32)), ("b", (50, 1, 65)),
                                                                                      ("p", (5, 6))))}
    lst = [("a", True), ("b", True), ("p", False)]

    def run(sl, nens):
        c = _coupler(nens)
        for n, v in vals.items():
            _put(c, n, v[..., sl])
        modules.horizontal_average(c, lst)
        modules.time_average_init(c, list(vals))
        modules.time_average_accumulate(c, list(vals))
        modules.time_average_accumulate(c, list(vals))
        return {n: _get(c, n + "_horizontal_average") for n, _ in lst} | {n + "_t": _get(c, n + "_time_average") for n in vals}

    whole = run(slice(None), n1 + n2)
    first, second = run(slice(0, n1), n1), run(slice(n1, None), n2)
    for k in whole:
        assert np.array_equal(np.concatenate([first[k], second[k]], axis=-1), whole[k]), k


@pytest.mark.gpu
def test_gpu_second_horizontal_average_overwrites_and_keeps_the_entry():
    from pam_amd import modules
    nens = 64
    c = _coupler(nens)
    dm = c.get_data_manager_device_readwrite()
    v1, v2 = field((7, 33, nens), seed=1), field((7, 33, nens), seed=2)
    _put(c, "x", v1)
    modules.horizontal_average(c, [("x", True)])
    ptr = dm.get("x_horizontal_average").data_ptr()
    assert np.array_equal(_get(c, "x_horizontal_average"), ref.horizontal_average(v1))
    _put(c, "x", v2)
    modules.horizontal_average(c, [("x", True)])
    assert dm.get("x_horizontal_average").data_ptr() == ptr and dm.get_shape("x_horizontal_average") == [7, nens]
    assert np.array_equal(_get(c, "x_horizontal_average"), ref.horizontal_average(v2))


@pytest.mark.gpu
def test_gpu_time_average_init_registers_then_rezeroes():
    from pam_amd import modules
    nens = 65
    c = _coupler(nens, nz=4, ny=3, nx=5)
    dm = c.get_data_manager_device_readwrite()
    names = ["temp", "uvel"]
    modules.time_average_init(c, names)
    for n in names:
        assert dm.get_shape(n + "_time_average") == [4, 3, 5, nens] and not _get(c, n + "_time_average").any()
    ptrs = [dm.get(n + "_time_average").data_ptr() for n in names]
    for n in names:
        _put(c, n + "_time_average", np.full((4, 3, 5, nens), 3.25))
    modules.time_average_init(c, names)
    assert [dm.get(n + "_time_average").data_ptr() for n in names] == ptrs
    for n in names:
        got = _get(c, n + "_time_average")
        assert not got.any() and not np.signbit(got).any(), n


@pytest.mark.gpu
@pytest.mark.parametrize("nens", [1, 65, 130])
def test_gpu_accumulates_of_changing_states_match_restatement(nens):
    from pam_amd import modules
    crm_dt, gcm_dt = 20.0, 900.0 / 7
    c = _coupler(nens, nz=6, ny=5, nx=7, crm_dt=crm_dt, gcm_dt=gcm_dt)
    _put(c, "precl", np.zeros((5, 7, nens)))
    names = ["density_dry", "temp", "precl"]
    modules.time_average_init(c, names)
    f = ref.time_average_factor(crm_dt, gcm_dt)
    want = {n: 0.0 for n in names}
    for s in range(5):
        for i, n in enumerate(names):
            v = field(tuple(c.get_data_manager_device_readwrite().get_shape(n)), seed=1000 * s + 10 * i + nens)
            _put(c, n, v)
            want[n] = ref.time_average_accumulate(want[n], v, f)
        modules.time_average_accumulate(c, names)
    for n in names:
        assert np.array_equal(_get(c, n + "_time_average"), want[n]), n
    modules.horizontal_average(c, [("density_dry_time_average", True), ("precl_time_average", False)])
    assert np.array_equal(_get(c, "density_dry_time_average_horizontal_average"), ref.horizontal_average(want["density_dry"]))
    assert np.array_equal(_get(c, "precl_time_average_horizontal_average"), ref.horizontal_average(want["precl"], False))


BAD_SHAPES = [((4,), True, "1-D"), ((3, 4), True, "nz,nens"), ((2, 2, 2, 2, 4), True, "two horizontal"),
              ((4,), False, "1-D"), ((2, 3, 5, 4), False, "two horizontal"), ((3, 5, 6), True, "nens"), ((5, 3), False, "nens")]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,vert,msg", BAD_SHAPES, ids=["1d_vert", "nz_nens", "5d", "1d_flat", "4d_flat", "last_not_nens_3d",
                                                            "last_not_nens_2d"])
def test_gpu_invalid_shapes_raise_and_register_nothing(shape, vert, msg):
    from pam_amd import modules
    c = _coupler(4)
    dm = c.get_data_manager_device_readwrite()
    _put(c, "good", field((3, 5, 4), seed=3))
    _put(c, "bad", np.ones(shape))
    before = set(dm._e)
    with pytest.raises(capi.PamAmdError, match=msg):
        modules.horizontal_average(c, [("good", True), ("bad", vert)])
    assert set(dm._e) == before


@pytest.mark.gpu
def test_gpu_failures_write_nothing():
    """every failure is raised before a launch: sentinel-filled outputs keep their bits"""
    from pam_amd import modules
    nens = 65
    c = _coupler(nens, nz=4, ny=3, nx=5)
    dm = c.get_data_manager_device_readwrite()
    sentinel = np.full((4, 3, 5, nens), -123.5)
    names = ["temp", "uvel"]
    modules.time_average_init(c, names)
    _put(c, "temp", field((4, 3, 5, nens), seed=4))

    def fill():
        for n in names:
            _put(c, n + "_time_average", sentinel)

    def untouched():
        return all(np.array_equal(_get(c, n + "_time_average"), sentinel) for n in names)

    # gcm_physics_dt missing, zero, negative
    for gcm_dt in (None, 0.0, -900.0):
        fill()
        if gcm_dt is None:
            c.options.delete_option("gcm_physics_dt")
        else:
            c.set_option("gcm_physics_dt", gcm_dt)
        with pytest.raises(capi.PamAmdError, match="gcm_physics_dt"):
            modules.time_average_accumulate(c, names)
        assert untouched(), gcm_dt
    c.set_option("gcm_physics_dt", 900.0)
    # a name without its time average (no init) after one that has it
    fill()
    with pytest.raises(capi.PamAmdError, match="time_average_init"):
        modules.time_average_accumulate(c, ["temp", "vvel", "uvel"])
    assert untouched() and not dm.entry_exists("vvel_time_average")
    # the init with a missing variable in the middle of the list: nothing zeroed, nothing registered
    with pytest.raises(capi.PamAmdError, match="nosuchfield"):
        modules.time_average_init(c, ["temp", "nosuchfield", "wvel"])
    assert untouched() and not dm.entry_exists("wvel_time_average")
    # a bad shape in the middle of a horizontal_average list: the earlier output keeps its bits, the later one is not registered
    modules.horizontal_average(c, [("temp", True)])
    _put(c, "temp_horizontal_average", np.full((4, nens), -9.0))
    _put(c, "flat", np.ones((3, nens)))
    with pytest.raises(capi.PamAmdError, match="nz,nens"):
        modules.horizontal_average(c, [("temp", True), ("flat", True), ("uvel", True)])
    assert np.array_equal(_get(c, "temp_horizontal_average"), np.full((4, nens), -9.0))
    assert not dm.entry_exists("flat_horizontal_average") and not dm.entry_exists("uvel_horizontal_average")


@pytest.mark.gpu
def test_gpu_horizontal_average_recovers_the_broadcast_gcm_column():
    import torch
    from pam_amd import modules
    nens, nz, ny, nx = 65, 30, 5, 8
    c = _coupler(nens, nz=nz, ny=ny, nx=nx)
    c.add_tracer("water_vapor", "", True, True)
    dm = c.get_data_manager_device_readwrite()
    rng = np.random.default_rng(5)
    cols = {}
    for g, scale in (("gcm_density_dry", 1.0), ("gcm_uvel", 20.0), ("gcm_vvel", 20.0), ("gcm_wvel", 1.0), ("gcm_temp", 300.0),
                     ("gcm_water_vapor", 0.01)):
        cols[g] = scale * rng.uniform(0.5, 1.5, (nz, nens)) * np.where(g in ("gcm_uvel", "gcm_vvel", "gcm_wvel"),
                                                                       rng.choice([-1.0, 1.0], (nz, nens)), 1.0)
        dm.get(g).copy_(torch.from_numpy(cols[g]))
    modules.broadcast_initial_gcm_column(c)
    crm = ["density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor"]
    modules.horizontal_average(c, [(n, True) for n in crm])
    eps = np.finfo(np.float64).eps
    for n in crm:
        x = cols["gcm_" + n]
        got = _get(c, n + "_horizontal_average")
        assert np.all(np.abs(got - x) <= nx * ny * eps * np.abs(x)), n


def _run_driver(*args, timeout=900):
    r = subprocess.run([DRIVER, "--yaml", CI_YAML] + list(args), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().split("\n")


@pytest.mark.gpu
def test_gpu_driver_stats_leave_the_run_unchanged(tmp_path):
    """the whole CI run (two GCM steps): with --stats the output file and the final JSON line are those of a run without it"""
    a, b, s = tmp_path / "plain.bin", tmp_path / "stats.bin", tmp_path / "stats.json"
    plain = _run_driver(str(a))
    with_stats = _run_driver("--stats", str(s), str(b))
    assert plain[-1] == with_stats[-1]
    assert a.read_bytes() == b.read_bytes()
    st = json.loads(s.read_text())
    assert [g["gcm_step"] for g in st["gcm_steps"]] == [0, 1] and [g["crm_steps"] for g in st["gcm_steps"]] == [45, 45]
    for g in st["gcm_steps"]:
        assert set(g["profiles"]) == set(st["fields"])
        assert np.all(np.isfinite(np.array(g["profiles"]["temp"])))
    # a whole GCM step's mean of T: 45 CRM steps weighted by crm_dt / dt_gcm = 1/45, near the state's temperatures
    t = np.array(st["gcm_steps"][1]["profiles"]["temp"])
    assert t.shape == (st["nz"], st["nens"]) and 150 < t.min() and t.max() < 350


@pytest.mark.gpu
def test_gpu_driver_one_step_stats_equal_the_restatement_of_its_output(tmp_path):
    out, s = tmp_path / "out.bin", tmp_path / "stats.json"
    _run_driver("--steps", "1", "--stats", str(s), str(out))
    st = json.loads(s.read_text())
    nens, nz = st["nens"], st["nz"]
    nx, ny = 65, 1
    f = ref.time_average_factor(st["crm_dt"], st["gcm_physics_dt"])
    raw = np.fromfile(out, dtype=np.float64)
    ncell, n2 = nz * ny * nx * nens, ny * nx * nens
    assert raw.size == ncell * (len(st["fields"]) - 1) + n2
    (g,) = st["gcm_steps"]
    assert g["crm_steps"] == 1
    for i, name in enumerate(st["fields"]):
        if name == "precl":
            v, vert = raw[-n2:].reshape(ny, nx, nens), False
        else:
            v, vert = raw[i * ncell:(i + 1) * ncell].reshape(nz, ny, nx, nens), True
        want = ref.horizontal_average(ref.time_average_accumulate(np.zeros(v.shape), v, f), vert)
        got = np.array(g["profiles"][name], dtype=np.float64)
        assert got.shape == want.shape and np.array_equal(got, want), name


@pytest.mark.gpu
def test_gpu_driver_stats_every_member_equals_member_zero(tmp_path):
    """--nens 64: the members start from the same column with the same perturbation, so their profiles are identical"""
    s = tmp_path / "stats.json"
    _run_driver("--nens", "64", "--steps", "5", "--stats", str(s), "-")
    st = json.loads(s.read_text())
    assert st["nens"] == 64
    for name, prof in st["gcm_steps"][0]["profiles"].items():
        p = np.array(prof, dtype=np.float64)
        assert p.shape[1] == 64 and np.array_equal(p, np.repeat(p[:, :1], 64, axis=1)), name
