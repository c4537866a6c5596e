"""Field diagnostics as one device scan (pam_amd_field_diagnostics): least and greatest element with their flat indices, the number of NaNs
and a reproducible sum, per field or per ensemble member.

The chain: tests/diagnostics_ref.py restates the results in numpy -- the sum by the header's tree with elementwise adds only.  The tree's
error against math.fsum is held to the bound of a summation tree of its depth (derived, not measured).  The restatement pins, bit for
bit, the host emulation of the device bodies (pam_amd/csrc/diagnostics_device.h under g++ -ffp-contract=off,
tests/emu/diagnostics_emu.cpp) and, on the GPU, the HIP path; its values pin the C++ adaptor (tests/cxx/diagnose_dm.cpp), the Python
DataManager and the driver's --diag."""
import ctypes as C
import functools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import diagnostics_ref as ref
from pam_amd import capi
from tools.native_build import cxx_program, emu_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
CI_YAML = os.path.join(ROOT, "tests", "golden", "ci_input_pama.yaml")
KIND_NAMES = ["double", "float"]
OFFSETS = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (1, 3)]          # (kind, elements past a 16-byte boundary)
OFFSET_IDS = ["%s_off%d" % (KIND_NAMES[k], o) for k, o in OFFSETS]
RESULT = np.dtype([("vmin", "f8"), ("vmax", "f8"), ("vsum", "f8"), ("argmin", "i8"), ("argmax", "i8"), ("nan_count", "i8")])
_DP, _LP = C.POINTER(C.c_double), C.POINTER(C.c_longlong)


def same(got, want):
    """bit for bit, every NaN sum being one NaN"""
    return ref.bits(got) == ref.bits(want)


def show(d):
    return {k: np.asarray(d[k]).tolist() for k in ref.KEYS}


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement and its bound

def test_the_cases_reach_every_level_and_edge():
    assert [ref.levels(n, ref.FIELD_W, ref.FIELD_K) for n in ref.FIELD_SIZES] == [1] * 7 + [2] * 3 + [2, 3]
    assert [ref.levels(r, ref.MEMBER_W, ref.MEMBER_K) for r, _ in ref.MEMBER_SHAPES] == [1, 1, 1, 1, 2, 2, 3]
    for kind in range(2):
        labels = [l for l, _ in ref.field_cases(kind)] + [l for l, _, _ in ref.member_cases(kind)]
        assert len(labels) == len(set(labels))
        want = ref.field_expected(kind)
        sizes = [a.size for _, a in ref.field_cases(kind)]
        assert any(w["argmin"] == 0 for w in want) and any(w["argmin"] == n - 1 and n > 1 for w, n in zip(want, sizes))
        assert any(w["argmax"] == 0 for w in want) and any(w["argmax"] == n - 1 and n > 1 for w, n in zip(want, sizes))
        assert any(w["argmin"] == -1 and w["vmin"] == np.inf and w["vmax"] == -np.inf and w["nan_count"] == n for w, n in zip(want, sizes))
        assert any(0 < w["nan_count"] < n for w, n in zip(want, sizes))
        assert any(np.isnan(w["vsum"]) and w["nan_count"] == 0 for w in want)                   # inf - inf
        assert any(w["vmin"] == -np.inf for w in want) and any(w["vmax"] == np.inf for w in want)
        assert any(w["vmin"] == 0 and np.signbit(w["vmin"]) and w["argmin"] == 0 for w in want)
        assert any(w["vmin"] == 0 and not np.signbit(w["vmin"]) and not np.signbit(w["vsum"]) for w in want)
        assert any(w["vsum"] == 0 and np.signbit(w["vsum"]) for w in want)                      # a lone -0.0 survives the sum
        # the minimum planted twice: the lower index is the answer
        for (label, a), w in zip(ref.field_cases(kind), want):
            if "min_at" in label and a.size > 3:
                assert (a == w["vmin"]).sum() >= 2 and w["argmin"] == np.flatnonzero(a == w["vmin"])[0], label


def test_restatement_tree_on_small_vectors_by_hand():
    assert ref.tree_sum(np.array([-0.0])) == 0 and np.signbit(ref.tree_sum(np.array([-0.0])))
    assert ref.tree_sum(np.array([1.0, 2.0, 3.0])) == 6.0
    # the lane fold: lanes 1 and 129 meet at d = 128 (1 + 1), and their 2 reaches the 1e16 of lane 0 at d = 1; lanes 1 and 2 reach
    # lane 0 one after the other (d = 2, d = 1), and 1e16 + 1 rounds back to 1e16 both times
    v = np.zeros(256)
    v[0], v[1], v[129] = 1e16, 1.0, 1.0
    assert ref.tree_sum(v) == 1e16 + 2.0
    v = np.zeros(256)
    v[0], v[1], v[2] = 1e16, 1.0, 1.0
    assert ref.tree_sum(v) == 1e16
    # a lane adds its steps in ascending order: (1e16 + 1) + 1 loses both ones, (1 + 1) + 1e16 keeps them
    v = np.zeros(2048)
    v[0], v[256], v[512] = 1e16, 1.0, 1.0
    assert ref.tree_sum(v) == 1e16
    v[0], v[256], v[512] = 1.0, 1.0, 1e16
    assert ref.tree_sum(v) == 1e16 + 2.0
    # the chunk results are the next vector: chunk 1 (one element) joins chunk 0 at level 2, as lane 1
    v = np.zeros(2049)
    v[0], v[2048] = 1e16, 1.0
    assert ref.tree_sum(v) == 1e16 and ref.tree_sum(v[::-1].copy()) == 1e16
    # per member: the rows of one member only
    a = np.arange(12.0).reshape(6, 2)
    assert np.array_equal(ref.tree_sum(a, 2), [30.0, 36.0])


@pytest.mark.parametrize("kind", range(2), ids=KIND_NAMES)
def test_restatement_sum_is_within_the_bound_of_its_tree(kind):
    """|tree - exact| <= gamma_D sum|x|, gamma_D = D u / (1 - D u), D = levels (K - 1 + log2 W): the standard bound of a summation tree
    in which every element passes through D adds; exact = math.fsum"""
    worst = 0.0
    for (label, a), w in zip(ref.field_cases(kind), ref.field_expected(kind)):
        x = a.astype(np.float64)
        if not np.isfinite(x).all():
            continue
        err, scale = abs(float(w["vsum"]) - math.fsum(x)), math.fsum(np.abs(x))
        bound = ref.gamma(x.size, ref.FIELD_W, ref.FIELD_K) * scale
        assert err <= bound, (label, err, bound)
        worst = max(worst, err / bound if bound else 0.0)
    for (label, a, M), w in zip(ref.member_cases(kind), ref.member_expected(kind)):
        x = a.astype(np.float64).reshape(-1, M)
        if not np.isfinite(x).all():
            continue
        for m in range(M):
            err, scale = abs(float(w["vsum"][m]) - math.fsum(x[:, m])), math.fsum(np.abs(x[:, m]))
            bound = ref.gamma(x.shape[0], ref.MEMBER_W, ref.MEMBER_K) * scale
            assert err <= bound, (label, m, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
    print("worst |err| / bound: %.3f" % worst)
    assert worst > 0.0                                                            # the cases do round


def test_whole_field_extremes_are_the_fold_of_the_member_results():
    for kind in range(2):
        for (label, a, M), per in zip(ref.member_cases(kind), ref.member_expected(kind)):
            whole, folded = ref.diagnose(a, 0), ref.fold_members(per, M)
            for k in ("vmin", "vmax", "argmin", "argmax", "nan_count"):
                assert np.asarray(whole[k]).tobytes() == np.asarray(folded[k], dtype=np.asarray(whole[k]).dtype).tobytes(), (label, k)


def _member_chunks(a, M):
    """the ensemble cut into contiguous member chunks: [(m0, m1, contiguous (rows, m1 - m0) copy flattened)]"""
    x = a.reshape(-1, M)
    cuts = sorted({0, 1, M // 2, M - 1, M} & set(range(M + 1)))
    return [(m0, m1, np.ascontiguousarray(x[:, m0:m1]).reshape(-1)) for m0, m1 in zip(cuts[:-1], cuts[1:])]


def _rebased(d, M, m0, m1):
    """the results of a member chunk with its flat indices turned into those of the whole ensemble"""
    out = dict(d)
    for k in ("argmin", "argmax"):
        i = np.asarray(d[k])
        out[k] = np.where(i >= 0, i // (m1 - m0) * M + m0 + i % (m1 - m0), -1)
    return out


def _check_chunking(diagnose_members):
    for kind in range(2):
        for (label, a, M), per in zip(ref.member_cases(kind), ref.member_expected(kind)):
            if M < 3:
                continue
            for m0, m1, part in _member_chunks(a, M):
                got = _rebased(diagnose_members(part, m1 - m0), M, m0, m1)
                assert same(got, {k: per[k][m0:m1] for k in ref.KEYS}), (label, m0, m1)


def test_member_results_do_not_depend_on_member_chunking():
    """a member's results come from its own elements in row order alone: the sums too, bit for bit"""
    _check_chunking(ref.diagnose)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the host emulation of the device bodies

@functools.lru_cache(maxsize=None)
def emu():
    lib = C.CDLL(emu_library("diagnostics_emu"))
    lib.emu_field_diagnostics.restype = C.c_int
    lib.emu_field_diagnostics.argtypes = [C.c_int, C.POINTER(C.c_int), _LP, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_longlong, C.c_void_p]
    return lib


def emu_call(arrays, members=0, per_launch=32, grid=0):
    """the emulated call on a list of host arrays: one dict per array"""
    n, M = len(arrays), max(members, 1)
    kinds = (C.c_int * n)(*[ref.KIND_DTYPES.index(a.dtype.type) for a in arrays])
    sizes = (C.c_longlong * n)(*[a.size for a in arrays])
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrays])
    out = np.zeros(n * M, dtype=RESULT)
    assert emu().emu_field_diagnostics(n, kinds, sizes, ptrs, members, per_launch, grid, out.ctypes.data) == 0
    return [{k: (out[k][f] if members == 0 else out[k][f * M:(f + 1) * M].copy()) for k in ref.KEYS} for f in range(n)]


def _based(a, off):
    """a copy of `a` that starts `off` elements past a 16-byte boundary"""
    raw = np.empty(a.nbytes + 64, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + off * a.itemsize
    view = raw[start:start + a.nbytes].view(a.dtype)
    view[:] = a
    assert (view.ctypes.data - off * a.itemsize) % 16 == 0
    return view


@pytest.mark.parametrize("kind,off", OFFSETS, ids=OFFSET_IDS)
def test_emulation_matches_restatement_exactly(kind, off):
    """every case, whole and per member, at a base `off` elements past a 16-byte boundary; the fields keep their bits"""
    for (label, a), w in zip(ref.field_cases(kind), ref.field_expected(kind)):
        v = _based(a, off)
        before = v.tobytes()
        got = emu_call([v])[0]
        assert same(got, w), (label, show(got), show(w))
        assert v.tobytes() == before, label
    for (label, a, M), w in zip(ref.member_cases(kind), ref.member_expected(kind)):
        v = _based(a, off)
        got = emu_call([v], M)[0]
        assert same(got, w), (label, show(got), show(w))


@pytest.mark.parametrize("kind", range(2), ids=KIND_NAMES)
def test_emulation_does_not_depend_on_the_grid(kind):
    """fewer workgroups than a field has chunks for (the wavefronts' stride loop and their running extremes) and more (idle
    wavefronts): the same bits, the sum included"""
    for (label, a), w in zip(ref.field_cases(kind), ref.field_expected(kind)):
        big = a.size > ref.SMALL_CASE
        if big and not label.startswith("n%d_" % (2048 ** 2 + 1)):
            continue
        for grid in ((1, 37) if big else (1, 2, 3, 1000)):
            got = emu_call([a], grid=grid)[0]
            assert same(got, w), (label, grid, show(got), show(w))


def _mixed_list(num, M):
    """`num` fields of both kinds and of sizes from one element to three levels' worth of rows, each a multiple of M"""
    rng = np.random.default_rng(900 + num + M)
    rows = [1, 2049 * 3, 63, 256, 257, 4097, 7, 300, 2048, 65]
    out = []
    for f in range(num):
        a = ref.mixed(rng, rows[f % len(rows)] * M)
        if f % 7 == 3:
            a[rng.integers(0, a.size)] = np.nan
        if f % 11 == 5:
            a[rng.integers(0, a.size)] = -np.inf
        out.append(a.astype(ref.KIND_DTYPES[f % 2]))
    return out


@pytest.mark.parametrize("members", [0, 5])
def test_emulation_does_not_depend_on_the_split_of_the_list(members):
    arrays = _mixed_list(70, max(members, 1))
    want = [ref.diagnose(a, members) for a in arrays]
    for per_launch in (1, 7, 32, 70):
        got = emu_call(arrays, members, per_launch=per_launch)
        for f in range(len(arrays)):
            assert same(got[f], want[f]), (per_launch, f, show(got[f]), show(want[f]))


def test_emulated_member_results_do_not_depend_on_member_chunking():
    _check_chunking(lambda part, M: emu_call([part], M)[0])


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the C ABI

def test_entry_point_is_exported_and_declared():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    assert hasattr(lib, "pam_amd_field_diagnostics") and "pam_amd_field_diagnostics" in capi.MODULE_SYMBOLS
    assert "pam_amd_field_diagnostics" in set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    assert hasattr(lib, "pam_amd_validate_fields")                                # the validation entry point stays
    import pam_amd
    assert pam_amd.field_diagnostics is pam_amd.modules.field_diagnostics


def test_entry_point_rejects_bad_arguments_before_touching_a_device():
    lib = capi.load()
    fn = lib.pam_amd_field_diagnostics
    P2 = (C.c_void_p * 2)(64, 128)              # never dereferenced: the checks fail first
    P2null = (C.c_void_p * 2)(64, None)
    P2odd4 = (C.c_void_p * 2)(64, 130)          # not a multiple of 4
    P2odd8 = (C.c_void_p * 2)(68, 128)          # a multiple of 4, not of 8
    K2, K2f = (C.c_int * 2)(0, 1), (C.c_int * 2)(1, 1)
    K2int, K2lo = (C.c_int * 2)(0, 2), (C.c_int * 2)(-1, 0)
    S2, S2zero, S2neg = (C.c_longlong * 2)(6, 9), (C.c_longlong * 2)(6, 0), (C.c_longlong * 2)(-1, 9)
    res = [(C.c_double * 6)(*[7.0] * 6) for _ in range(3)] + [(C.c_longlong * 6)(*[7] * 6) for _ in range(3)]

    def call(n=2, kind=K2, size=S2, data=P2, members=0, drop=None):
        out = [None if i == drop else r for i, r in enumerate(res)]
        return fn(n, kind, size, data, members, *out, None)
    cases = [
        lambda: call(kind=None), lambda: call(size=None), lambda: call(data=None),
        lambda: call(n=0), lambda: call(n=-3),
        lambda: call(size=S2zero), lambda: call(size=S2neg),
        lambda: call(kind=K2int), lambda: call(kind=K2lo),
        lambda: call(data=P2null), lambda: call(kind=K2f, data=P2odd4), lambda: call(data=P2odd8),
        lambda: call(members=-1), lambda: call(members=2), lambda: call(members=4),      # 9 % 2, 6 % 4 and 9 % 4 are not 0
    ] + [lambda i=i: call(drop=i) for i in range(6)]
    for n, c in enumerate(cases):
        assert c() == -1, n                                       # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert b"field_diagnostics" in lib.pam_amd_awfl_last_error(), n
        assert all(list(r) == [7] * 6 for r in res), n            # nothing written


def test_python_adaptors_skip_what_is_not_looked_at():
    import torch
    import pam_amd
    from pam_amd.coupler import DataManager
    dm = DataManager(torch.device("cpu"))
    dm.register_existing("flags", "", torch.zeros(4, dtype=torch.bool))
    dm.register_existing("count", "", torch.zeros(4, dtype=torch.int32))
    assert dm.diagnose_all() == {} and dm.diagnose_all(members=2) == {}          # nothing to look at: no device needed
    with pytest.raises(capi.PamAmdError):
        dm.diagnose("missing")
    with pytest.raises(capi.PamAmdError, match="dtype"):
        dm.diagnose("count")
    out = pam_amd.field_diagnostics([], members=3)
    assert set(out) == set(ref.KEYS) and all(v.shape == (0, 3) for v in out.values())


# ------------------------------------------------------------------------------------------------------------------------------
# GPU

def _torch_dtype(kind):
    import torch
    return [torch.float64, torch.float32][kind]


def _pack(arrays, off):
    """the arrays in ONE host buffer, each starting `off` elements past a 16-byte boundary: (buffer, [(start, n)])"""
    per16 = 16 // arrays[0].itemsize
    spans, at = [], 0
    for a in arrays:
        spans.append((at + off, a.size))
        at += -(-(off + a.size) // per16) * per16 + per16
    buf = np.zeros(at, dtype=arrays[0].dtype)
    for (start, n), a in zip(spans, arrays):
        buf[start:start + n] = a
    return buf, spans


def _device_views(arrays, off):
    import torch
    buf, spans = _pack(arrays, off)
    dev = torch.from_numpy(buf).to("cuda:0")
    assert dev.data_ptr() % 16 == 0
    views = [dev[s:s + n] for s, n in spans]
    assert all((v.data_ptr() - off * dev.element_size()) % 16 == 0 for v in views)
    return buf, dev, views


def _rows(out, f):
    return {k: out[k][f] for k in ref.KEYS}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,off", OFFSETS, ids=OFFSET_IDS)
def test_gpu_whole_field_matches_restatement_exactly(kind, off):
    """the HIP path on every whole-field case in one call (many launch tables), whole (off 0) and as views offset by some elements;
    a second run gives the same bits, and the fields keep theirs"""
    import pam_amd
    cases, want = ref.field_cases(kind), ref.field_expected(kind)
    buf, dev, views = _device_views([a for _, a in cases], off)
    out = pam_amd.field_diagnostics(views)
    assert all(out[k].shape == (len(cases),) for k in ref.KEYS)
    bad = [f for f in range(len(cases)) if not same(_rows(out, f), want[f])]
    assert not bad, [(cases[f][0], show(_rows(out, f)), show(want[f])) for f in bad[:4]]
    again = pam_amd.field_diagnostics(views)
    assert all(out[k].tobytes() == again[k].tobytes() for k in ref.KEYS)
    assert dev.cpu().numpy().tobytes() == buf.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,off", OFFSETS, ids=OFFSET_IDS)
def test_gpu_per_member_matches_restatement_exactly(kind, off):
    """the same per member: the cases of one shape form one call"""
    import pam_amd
    cases, want = ref.member_cases(kind), ref.member_expected(kind)
    for M in sorted({M for _, _, M in cases}):
        sel = [f for f, c in enumerate(cases) if c[2] == M]
        buf, dev, views = _device_views([cases[f][1] for f in sel], off)
        out = pam_amd.field_diagnostics(views, members=M)
        assert all(out[k].shape == (len(sel), M) for k in ref.KEYS)
        bad = [(l, f) for l, f in enumerate(sel) if not same(_rows(out, l), want[f])]
        assert not bad, [(cases[f][0], show(_rows(out, l)), show(want[f])) for l, f in bad[:3]]
        again = pam_amd.field_diagnostics(views, members=M)
        assert all(out[k].tobytes() == again[k].tobytes() for k in ref.KEYS)
        assert dev.cpu().numpy().tobytes() == buf.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("members", [0, 5])
@pytest.mark.parametrize("num", [1, 32, 33, 70])
def test_gpu_lists_equal_per_field_calls(num, members):
    import torch
    import pam_amd
    arrays = _mixed_list(num, max(members, 1))
    tens = [torch.from_numpy(a).to("cuda:0") for a in arrays]
    out = pam_amd.field_diagnostics(tens, members)
    for f, (t, a) in enumerate(zip(tens, arrays)):
        one = pam_amd.field_diagnostics([t], members)
        assert same(_rows(one, 0), _rows(out, f)), f
        assert same(_rows(out, f), ref.diagnose(a, members)), f


@pytest.mark.gpu
def test_gpu_scratch_grows_with_the_plan():
    """from no scratch at all: a small whole-field call (the scratch starts at 64 KB), then a per-member call whose plan exceeds 64 KB
    (it grows) -- the fewest members of 5 rows that do --, then a per-member call of half the members and the whole-field call again on
    the scratch the large one left, then the large one again from nothing after pam_amd_modules_finalize"""
    import torch
    import pam_amd
    rows, floor = 5, 1 << 16
    M = next(m for m in range(1, 1 << 16) if ref.member_plan_bytes([rows * m], m) > floor)
    assert ref.member_plan_bytes([rows * (M - 1)], M - 1) <= floor < ref.member_plan_bytes([rows * M], M) and rows * M * 8 < (16 << 20)
    rng = np.random.default_rng(909)
    large, small = ref.mixed(rng, rows * M), ref.mixed(rng, 300)
    large[rng.integers(0, large.size, 7)] = np.nan
    half = np.ascontiguousarray(large[:rows * (M // 2)])
    calls = {"small": (small, 0), "large": (large, M), "half": (half, M // 2)}
    want = {k: ref.diagnose(a, m) for k, (a, m) in calls.items()}
    dev = {k: torch.from_numpy(a).to("cuda:0") for k, (a, _) in calls.items()}
    lib = capi.load()
    capi.check(lib.pam_amd_modules_finalize())
    for k in ("small", "large", "half", "small", None, "large"):
        if k is None:
            capi.check(lib.pam_amd_modules_finalize())
            continue
        assert same(_rows(pam_amd.field_diagnostics([dev[k]], calls[k][1]), 0), want[k]), k


@pytest.mark.gpu
def test_gpu_member_results_do_not_depend_on_member_chunking():
    import torch
    import pam_amd

    def on_device(part, M):
        return _rows(pam_amd.field_diagnostics([torch.from_numpy(np.array(part)).to("cuda:0")], M), 0)
    _check_chunking(on_device)


@pytest.mark.gpu
def test_gpu_whole_field_extremes_are_the_fold_of_the_member_results():
    import torch
    import pam_amd
    for kind in range(2):
        for label, a, M in ref.member_cases(kind)[::3]:
            t = torch.from_numpy(np.array(a)).to("cuda:0")
            whole, per = _rows(pam_amd.field_diagnostics([t]), 0), _rows(pam_amd.field_diagnostics([t], M), 0)
            folded = ref.fold_members(per, M)
            for k in ("vmin", "vmax", "argmin", "argmax", "nan_count"):
                assert np.asarray(whole[k]).tobytes() == np.asarray(folded[k], dtype=whole[k].dtype).tobytes(), (label, k)


@pytest.mark.gpu
def test_gpu_scan_is_ordered_on_the_callers_stream():
    """a field filled by a kernel queued on a non-default stream, scanned on that stream, is seen as filled"""
    import torch
    import pam_amd
    n = (1 << 22) + 3
    t = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        t.fill_(3.0)
        out = pam_amd.field_diagnostics([t])
        per = pam_amd.field_diagnostics([t.view(-1, 1)[: n - 3]], members=64)
    assert out["vmin"][0] == 3.0 and out["vmax"][0] == 3.0 and out["vsum"][0] == 3.0 * n          # every partial an integer
    assert out["argmin"][0] == 0 and out["argmax"][0] == 0 and out["nan_count"][0] == 0
    assert (per["vsum"][0] == 3.0 * ((n - 3) // 64)).all() and np.array_equal(per["argmin"][0], np.arange(64))


@pytest.mark.gpu
def test_gpu_python_requires_contiguous_tensors_of_a_looked_at_dtype():
    import torch
    import pam_amd
    t = torch.zeros((8, 8), dtype=torch.float64, device="cuda:0")
    with pytest.raises(capi.PamAmdError, match="contiguous"):
        pam_amd.field_diagnostics([t[:, ::2]])
    with pytest.raises(capi.PamAmdError, match="dtype"):
        pam_amd.field_diagnostics([t.to(torch.int32)])
    with pytest.raises(capi.PamAmdError, match="multiple"):
        pam_amd.field_diagnostics([t], members=3)


def _adaptor_entries():
    """(name, array): a few cases of both kinds whose sums are finite, and one with NaNs"""
    out = []
    for kind in range(2):
        cases = dict(ref.field_cases(kind))
        for label in ("n257_min_at0", "n2049_min_at1", "n4099_minus_inf", "n2047_nan_and_inf", "n255_zeros"):
            out.append(("%s_%s" % (KIND_NAMES[kind][0], label), cases[label]))
    return out


@pytest.mark.gpu
def test_gpu_python_datamanager_diagnoses_every_entry():
    import torch
    from pam_amd.coupler import DataManager
    dm = DataManager(torch.device("cuda:0"))
    entries = _adaptor_entries()
    for name, a in entries:
        dm.register_existing(name, "", torch.from_numpy(np.array(a)).to("cuda:0"))
    dm.register_existing("flags", "", torch.zeros(5, dtype=torch.bool, device="cuda:0"))
    dm.register_and_allocate("ens", "", (6, 4))
    dm.get("ens").copy_(torch.arange(24.0).reshape(6, 4))
    got = dm.diagnose_all()
    assert list(got) == [n for n, _ in entries] + ["ens"]                         # registration order, the bool entry skipped
    for name, a in entries:
        assert same(got[name], ref.diagnose(a)), name
        assert same(dm.diagnose(name), ref.diagnose(a)), name
    per = dm.diagnose_all(members=4)
    assert "ens" in per and same(per["ens"], ref.diagnose(np.arange(24.0), 4))
    assert np.array_equal(per["ens"]["argmax"], [20, 21, 22, 23]) and np.array_equal(per["ens"]["vsum"], [60.0, 66.0, 72.0, 78.0])
    assert same(dm.diagnose("ens", members=4), per["ens"])


@pytest.mark.gpu
def test_gpu_cxx_adaptor_prints_the_reference_lines_and_returns_the_values(tmp_path):
    """DEBUG_PRINT_SUM / AVG / MIN / MAX on the work-alike's arrays: the reference's lines (pam_const.h:308-322) with the restatement's
    values at the printed precision (the stream's default, six significant digits); DataManager::diagnose / diagnose_all return the
    restatement's values exactly, in registration order, other types skipped"""
    entries = _adaptor_entries()
    uint = {np.float64: np.uint64, np.float32: np.uint32}
    script = []
    for name, a in entries:
        script.append("entry %s %s %d %s" % (name, KIND_NAMES[name[0] == "f"], a.size, " ".join("%x" % b for b in a.view(uint[a.dtype.type]))))
    script.append("entry ints int 3 1 2 3")
    script.append("entry ens double 24 " + " ".join("%x" % b for b in np.arange(24.0).view(np.uint64)))
    for name, a in entries:
        script.append("macros %s %s" % (name, KIND_NAMES[name[0] == "f"]))
    script += ["diagnose %s 0" % n for n, _ in entries] + ["diagnose_all 0", "diagnose ens 4", "diagnose_all 4", "diagnose ints 0"]
    path = tmp_path / "script.txt"
    path.write_text("\n".join(script) + "\n")
    r = subprocess.run([cxx_program("diagnose_dm"), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = re.findall(r"^\*\*\* DEBUG: (\S+): (\d+): (sum|avg|minval|maxval)\(var\)  -->  (\S+)$", r.stdout, flags=re.M)
    assert len(lines) == 4 * len(entries) and all(l[0].endswith("diagnose_dm.cpp") for l in lines)
    fmt = lambda v: re.sub(r"e([+-])(\d)$", r"e\g<1>0\2", "%g" % v)          # ostream's default formatting is printf's %g
    for f, (name, a) in enumerate(entries):
        w = ref.diagnose(a)
        got = {what: text for _, _, what, text in lines[4 * f:4 * f + 4]}
        want = {"sum": w["vsum"], "avg": w["vsum"] / a.size, "minval": w["vmin"], "maxval": w["vmax"]}
        for what, v in want.items():
            assert got[what].lstrip("-") == "nan" if np.isnan(v) else got[what] == fmt(v), (name, what, got[what], v)

    blocks = re.findall(r"^### (\S+) (\d+)\n(.*?)###END$", r.stdout, flags=re.S | re.M)

    def parsed(body):
        rows = [l.split() for l in body.strip().split("\n")]
        d = {k: np.array([float.fromhex(r[i]) for r in rows]) for i, k in enumerate(("vmin", "vmax", "vsum"))}
        d.update({k: np.array([int(r[3 + i]) for r in rows], dtype=np.int64) for i, k in enumerate(("argmin", "argmax", "nan_count"))})
        return d
    names = [n for n, _ in entries]
    assert [b[0] for b in blocks] == names + names + ["ens"] + ["ens"] + ["ens"]  # diagnose_all: registration order; ints skipped;
    arrays = dict(entries)                                                        # with members = 4 only `ens` is a multiple... of 4
    for name, M, body in blocks[:2 * len(names) + 1]:
        a = arrays.get(name, np.arange(24.0))
        got = parsed(body)
        assert same({k: v[0] for k, v in got.items()}, ref.diagnose(a)), name
    for name, M, body in blocks[2 * len(names) + 1:]:
        assert M == "4" and same(parsed(body), ref.diagnose(np.arange(24.0), 4))
    assert "### threw ERROR: diagnose: entry ints is neither double nor float" in r.stdout


@pytest.mark.gpu
def test_gpu_driver_diag_leaves_stdout_unchanged_and_agrees_with_the_host_numbers(tmp_path):
    """--diag: stdout is that of a run without it; per output step the wvel line's max(-vmin, vmax) is the printed maxw, and at the last
    output step, which is the final state here, the least temp is the summary's temp_min; the whole-field extremes are the fold of the
    members'"""
    def run(*args):
        r = subprocess.run([DRIVER, "--yaml", CI_YAML, "--nens", "3", "--steps", "20"] + list(args) + ["-"], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r
    path = tmp_path / "diag.jsonl"
    plain, diag = run(), run("--diag", str(path))
    assert plain.stdout == diag.stdout and plain.stdout.strip()
    steps = [json.loads(l) for l in path.read_text().splitlines()]
    printed = re.findall(r"^Etime , dtphys, maxw: (\S+) , \S+ ,\s*(\S+)$", diag.stdout, flags=re.M)
    assert len(steps) == len(printed) == 2 and [s["crm_step"] for s in steps] == [10, 20]
    summary = json.loads(diag.stdout.strip().splitlines()[-1])
    for s, (etime, maxw) in zip(steps, printed):
        assert s["nens"] == 3 and "%g" % s["etime"] == etime
        assert set(s["fields"]) >= {"density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor"}
        w = s["fields"]["wvel"]["whole"]
        assert ("%10.6g" % max(-w["vmin"], w["vmax"])).strip() == maxw
        for name, d in s["fields"].items():
            per = {k: np.array(d["members"][k]) for k in ref.KEYS}
            assert all(len(per[k]) == 3 for k in ref.KEYS), name
            folded = ref.fold_members(per, 3)
            assert all(folded[k] == d["whole"][k] for k in ("vmin", "vmax", "argmin", "argmax", "nan_count")), name
            assert d["whole"]["nan_count"] == 0 and (per["argmin"] % 3 == np.arange(3)).all(), name
    temp = steps[-1]["fields"]["temp"]
    assert "%.9g" % min(temp["members"]["vmin"]) == "%.9g" % summary["temp_min"]
    assert "%.9g" % temp["whole"]["vmax"] == "%.9g" % summary["temp_max"]
    assert "%.9g" % steps[-1]["fields"]["density_dry"]["whole"]["vmin"] == "%.9g" % summary["rho_d_min"]
