"""DataManager::validate / validate_all as one device scan (pam_core/DataManager.h:408-509; pam_amd_validate_fields).

Everything here is an integer or a line of text, so every comparison is exact.  The chain: the reference's own stderr lines
(tests/golden/validate_ref.json, written by tests/golden/make_ref_validate_golden.py from a run of the reference's header) pin the
numpy restatement (tests/validate_ref.py); the restatement's six integers per field pin the host emulation of the device bodies
(pam_amd/csrc/validate_device.h under g++, tests/emu/validate_emu.cpp) and, on the GPU, the HIP path; the golden's lines pin the C++
adaptor (tests/cxx/validate_dm.cpp), the Python DataManager and the driver's --validate."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_boundary_surface as tb
import validate_ref as ref
from pam_amd import capi
from tools.native_build import cxx_program, emu_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "validate_ref.json")
DRIVER = os.path.join(ROOT, "examples", "driver")
CI_YAML = os.path.join(ROOT, "tests", "golden", "ci_input_pama.yaml")
REFERENCE = os.environ.get("PAM_REF", os.path.join(os.path.dirname(ROOT), "reference"))
_LP = C.POINTER(C.c_longlong)

GOLDEN_DTYPE = {"double": np.float64, "float": np.float32, "int": np.int32, "long long": np.int64, "bool": np.bool_}
GOLDEN_UINT = {"double": np.uint64, "float": np.uint32, "int": np.uint32, "long long": np.uint64, "bool": np.uint8}
KIND_NAMES = ["double", "float", "int", "longlong"]          # kind 0 .. 3 of the C ABI


# ------------------------------------------------------------------------------------------------------------------------------
# the golden

def golden():
    return json.load(open(GOLDEN))["cases"]


def entry_array(e):
    return np.array([int(b, 16) for b in e["bits"]], dtype=GOLDEN_UINT[e["kind"]]).view(GOLDEN_DTYPE[e["kind"]])


def case_entries(case):
    return [(e["name"], entry_array(e), e["positive"]) for e in case["entries"]]


def restated(case, call):
    """(stderr text, threw) of a golden call by the restatement"""
    entries = case_entries(case)
    if call["fn"] == "validate_all":
        out, died = ref.lines_all(entries, call["die"])
    else:
        name, arr, pos = next(e for e in entries if e[0] == call["name"])
        out, died = ref.lines(name, arr, pos, call["die"])
    return "".join(l + "\n" for l in out), died


def test_golden_holds_the_cases_of_the_issue():
    cases = {c["name"]: c for c in golden()}
    assert {"four_entries", "every_kind_clean", "every_kind_dirty", "every_element_offending", "nan_flavours", "integer_minimums",
            "subnormals"} <= set(cases)
    four = cases["four_entries"]
    assert [e["name"] for e in four["entries"]] == ["a", "n", "b", "free"]          # registration order, not alphabetical
    first = next(c for c in four["calls"] if c["fn"] == "validate_all" and not c["die"])
    assert first["stderr"].split("\n") == [
        "WARNING: NaN discovered in: a at global index: 1",
        "WARNING: inf discovered in: a at global index: 3",
        "WARNING: inf discovered in: a at global index: 7",
        "WARNING: negative value discovered in positive-definite entry: a at global index: 3",
        "WARNING: negative value discovered in positive-definite entry: a at global index: 6",
        "WARNING: negative value discovered in positive-definite entry: n at global index: 1",
        "WARNING: NaN discovered in: free at global index: 1", ""]
    die = next(c for c in four["calls"] if c["fn"] == "validate" and c["name"] == "a" and c["die"])
    assert die["threw"] and die["stderr"] == "WARNING: NaN discovered in: a at global index: 1\n\n"
    for c in cases.values():
        fns = {(k["fn"], k["die"]) for k in c["calls"]}
        assert fns == {("validate_all", False), ("validate_all", True), ("validate", False), ("validate", True)}
    kinds = {e["kind"] for c in cases.values() for e in c["entries"]}
    assert kinds == set(GOLDEN_DTYPE)
    assert all(not k["stderr"] and not k["threw"] for k in cases["every_kind_clean"]["calls"])


@pytest.mark.parametrize("case", golden(), ids=[c["name"] for c in golden()])
def test_restatement_writes_the_reference_lines(case):
    for call in case["calls"]:
        assert restated(case, call) == (call["stderr"], call["threw"]), (call["fn"], call["name"], call["die"])


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "pam_core", "DataManager.h")), reason="no reference tree at hand")
def test_the_golden_is_reproduced_from_the_reference_tree():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_ref_validate_golden.py"), REFERENCE, "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------------------------
# the fields of the scan tests: for every power of two n from 1 to 2^17 the sizes n-1, n, n+1 (a wavefront, a workgroup and any
# per-workgroup chunk lie between two of them), each planted: clean; one offender of each class at 0, 1, n/2, n-2, n-1; about 1 % random
# offenders of all classes mixed; every element offending.  Built once per kind; the restatement's integers once per field.

SIZES = sorted({s for p in range(18) for s in ((1 << p) - 1, 1 << p, (1 << p) + 1) if s >= 1})
DTYPES = ref.KIND_DTYPES


def _offenders(kind):
    """values of each class for the kind: (NaNs, infs, negatives that are neither)"""
    if kind == 0:
        nans = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001], dtype=np.uint64).view(np.float64)
        return nans, np.array([np.inf, -np.inf]), np.array([-1.0, -4.9e-324, -1e300])
    if kind == 1:
        nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001], dtype=np.uint32).view(np.float32)
        return nans, np.array([np.inf, -np.inf], dtype=np.float32), np.array([-1.0, -1e-45, -3e38], dtype=np.float32)
    if kind == 2:
        return None, None, np.array([-1, -2 ** 31, -77], dtype=np.int32)
    return None, None, np.array([-1, -2 ** 63, -2 ** 40], dtype=np.int64)


def _clean(kind, n, rng):
    if kind < 2:
        a = rng.uniform(0.0, 1e3, n).astype(DTYPES[kind])
        a[rng.random(n) < 0.1] = 0.0
        a[rng.random(n) < 0.05] = -0.0            # -0.0 is not negative
        return a
    return rng.integers(0, 1000, n).astype(DTYPES[kind])


@functools.lru_cache(maxsize=None)
def fields(kind):
    """[(label, array)]; never modified after this"""
    rng = np.random.default_rng(1000 + kind)
    classes = [c for c in _offenders(kind) if c is not None]
    out = []
    for n in SIZES:
        out.append(("n%d_clean" % n, _clean(kind, n, rng)))
        for ci, vals in enumerate(classes):
            for at in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
                a = _clean(kind, n, rng)
                a[at] = vals[(at + n) % len(vals)]
                out.append(("n%d_class%d_at%d" % (n, ci, at), a))
        a = _clean(kind, n, rng)
        hit = np.flatnonzero(rng.random(n) < 0.01)
        pool = np.concatenate(classes)
        a[hit] = pool[rng.integers(0, len(pool), hit.size)]
        out.append(("n%d_random" % n, a))
        pool = np.concatenate(classes)
        out.append(("n%d_all" % n, pool[rng.integers(0, len(pool), n)].astype(DTYPES[kind])))
    for _, a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(kind, positive=True):
    """the restatement's (count[3], first[3]) of every field of fields(kind), stacked: (nfields, 6)"""
    return np.array([np.concatenate(ref.scan(a, positive)) for _, a in fields(kind)], dtype=np.int64)


def test_the_field_set_reaches_every_class_and_edge():
    for kind in range(4):
        want = expected(kind)
        labels = [l for l, _ in fields(kind)]
        assert len(labels) == len(set(labels))
        classes = (0, 1, 2) if kind < 2 else (2,)
        for c in classes:
            assert (want[:, c] > 0).any() and (want[:, c] == 0).any()
            assert (want[:, 3 + c] == 0).any()                                   # an offender at index 0
        assert all((want[:, c] == 0).all() for c in range(3) if c not in classes)
        assert ((want[:, :3] == 0) == (want[:, 3:] == -1)).all()
        n_all = {a.size: w for (l, a), w in zip(fields(kind), want) if l.endswith("_all")}
        assert all(w[:3].sum() >= n for n, w in n_all.items())                   # every element offends


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the host emulation of the device bodies

def emu():
    lib = C.CDLL(emu_library("validate_emu"))
    lib.emu_validate.restype = C.c_longlong
    lib.emu_validate.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_longlong, _LP]
    return lib


def _based(a, off):
    """a copy of `a` that starts `off` elements past a 16-byte boundary"""
    raw = np.empty(a.nbytes + 64, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + off * a.itemsize
    view = raw[start:start + a.nbytes].view(a.dtype)
    view[:] = a
    assert (view.ctypes.data - off * a.itemsize) % 16 == 0
    return view


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", range(4), ids=KIND_NAMES)
def test_emulation_matches_restatement_exactly(kind, off):
    """every field of the set at a base `off` elements past a 16-byte boundary: the peel, the chunk edges and the fold"""
    lib = emu()
    want = expected(kind)
    out = np.zeros(6, dtype=np.int64)
    for (label, a), w in zip(fields(kind), want):
        v = _based(a, off)
        before = v.tobytes()
        touched = lib.emu_validate(kind, v.size, v.ctypes.data, 1, 0, out.ctypes.data_as(_LP))
        assert np.array_equal(out, w), (label, out, w)
        assert (touched == 0) == (not w[:3].any()), label                       # a clean field issues no atomics
        assert v.tobytes() == before, label


@pytest.mark.parametrize("kind", range(4), ids=KIND_NAMES)
def test_emulation_does_not_depend_on_the_grid(kind):
    """fewer workgroups than the field can keep busy (the stride loop) and more (idle workgroups): the same integers"""
    lib = emu()
    want = expected(kind)
    out = np.zeros(6, dtype=np.int64)
    for (label, a), w in list(zip(fields(kind), want))[-40:]:                    # the sizes 2^17 - 1 .. 2^17 + 1, every planting
        for nblocks in (1, 3, 1000):
            lib.emu_validate(kind, a.size, a.ctypes.data, 1, nblocks, out.ctypes.data_as(_LP))
            assert np.array_equal(out, w), (label, nblocks)


def test_emulation_ignores_negatives_of_a_field_that_is_not_positive():
    lib = emu()
    out = np.zeros(6, dtype=np.int64)
    for kind in range(4):
        label, a = fields(kind)[-1]
        lib.emu_validate(kind, a.size, a.ctypes.data, 0, 0, out.ctypes.data_as(_LP))
        assert np.array_equal(out, np.concatenate(ref.scan(a, False))) and out[2] == 0 and out[5] == -1, label


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the C ABI and the adaptor's boundary

def test_entry_point_is_exported_and_declared():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    assert hasattr(lib, "pam_amd_validate_fields") and "pam_amd_validate_fields" in capi.MODULE_SYMBOLS
    assert "pam_amd_validate_fields" in set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    assert lib.pam_amd_awfl_abi_version() == 5


def test_entry_point_rejects_bad_arguments_before_touching_a_device():
    lib = capi.load()
    fn = lib.pam_amd_validate_fields
    P2 = (C.c_void_p * 2)(64, 128)              # never dereferenced: validation fails first
    P2null = (C.c_void_p * 2)(64, None)
    P2odd4 = (C.c_void_p * 2)(64, 130)          # not a multiple of 4
    P2odd8 = (C.c_void_p * 2)(68, 128)          # a multiple of 4, not of 8
    K2 = (C.c_int * 2)(0, 1)
    K2f = (C.c_int * 2)(1, 1)
    K2hi, K2lo = (C.c_int * 2)(0, 4), (C.c_int * 2)(-1, 0)
    S2, S2zero, S2neg = (C.c_longlong * 2)(5, 7), (C.c_longlong * 2)(5, 0), (C.c_longlong * 2)(-1, 7)
    I2 = (C.c_int * 2)(1, 0)
    out, first = (C.c_longlong * 6)(*[7] * 6), (C.c_longlong * 6)(*[7] * 6)
    cases = [
        lambda: fn(2, None, S2, P2, I2, out, first, None),
        lambda: fn(2, K2, None, P2, I2, out, first, None),
        lambda: fn(2, K2, S2, None, I2, out, first, None),
        lambda: fn(2, K2, S2, P2, None, out, first, None),
        lambda: fn(0, K2, S2, P2, I2, out, first, None),
        lambda: fn(-3, K2, S2, P2, I2, out, first, None),
        lambda: fn(2, K2, S2zero, P2, I2, out, first, None),
        lambda: fn(2, K2, S2neg, P2, I2, out, first, None),
        lambda: fn(2, K2hi, S2, P2, I2, out, first, None),
        lambda: fn(2, K2lo, S2, P2, I2, out, first, None),
        lambda: fn(2, K2, S2, P2null, I2, out, first, None),
        lambda: fn(2, K2f, S2, P2odd4, I2, out, first, None),
        lambda: fn(2, K2, S2, P2odd8, I2, out, first, None),
        lambda: fn(2, K2, S2, P2, I2, None, first, None),
        lambda: fn(2, K2, S2, P2, I2, out, None, None),
    ]
    for n, call in enumerate(cases):
        assert call() == -1, n                                    # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert b"validate" in lib.pam_amd_awfl_last_error(), n
        assert list(out) == [7] * 6 and list(first) == [7] * 6, n  # nothing written


def test_adaptor_text_uses_only_reference_names():
    """tests/test_boundary_surface.py's scans over the new adaptor text: the members it defines are the reference's, and what it calls
    on a coupler or a DataManager (nothing, today) would have to be"""
    text = "".join(open(os.path.join(HOST, f)).read() for f in ("data_validation_helpers.h", "data_validation_members.h"))
    stripped = tb._strip_comments(text)
    defined = set(re.findall(r"\bDataManager::(\w+)\s*\(", stripped))
    assert defined == {"validate_all", "validate", "validate_nan", "validate_inf", "validate_pos"}
    rec = set(json.load(open(tb.GOLDEN))["boundary_surface"]["datamanager_h_names"])
    assert defined <= rec, sorted(defined - rec)
    coupler, dm = tb._used_members(text)
    assert coupler <= tb.REF_COUPLER and dm <= tb.REF_DM, (coupler, dm)
    # inside the class the work-alike only declares them; test_boundary_surface's own scan of pam_coupler.h stays as it is
    header = tb._strip_comments(open(os.path.join(HOST, "pam_coupler.h")).read())
    body = header[header.index("class DataManager"):header.index("class PamCoupler")]
    for name in defined:
        assert re.search(r"void %s\(std::string name, bool die_on_failed_check = false\) const;" % name, body) or name == "validate_all"
    assert "void validate_all(bool die_on_failed_check = false) const;" in body
    assert {"validate", "validate_all"} <= tb._declared(os.path.join(HOST, "pam_coupler.h"))
    drv_coupler, drv_dm = tb._used_members(open(os.path.join(ROOT, "examples", "driver.cpp")).read())
    assert "validate_all" in drv_dm and drv_dm <= tb.REF_DM


def test_python_datamanager_keeps_the_positive_flag_and_skips_other_dtypes():
    import torch
    from pam_amd.coupler import DataManager
    dm = DataManager(torch.device("cpu"))
    dm.register_and_allocate("z", "", (3,), positive=True)
    dm.register_and_allocate("a", "", (3,))
    dm.register_existing("m", "", torch.zeros(2, dtype=torch.bool), positive=True)
    assert [(n, e["positive"]) for n, e in dm._e.items()] == [("z", True), ("a", False), ("m", True)]
    dm.validate("m")                       # a dtype that is not checked: nothing to do, no device needed
    with pytest.raises(capi.PamAmdError):
        dm.validate("missing")


# ------------------------------------------------------------------------------------------------------------------------------
# GPU

def _torch_dtype(kind):
    import torch
    return [torch.float64, torch.float32, torch.int32, torch.int64][kind]


def _pack(kind, off):
    """every field of fields(kind) in ONE host buffer, each starting `off` elements past a 16-byte boundary: (buffer, [(start, n)])"""
    item = np.dtype(DTYPES[kind]).itemsize
    per16 = 16 // item
    spans, at = [], 0
    for _, a in fields(kind):
        spans.append((at + off, a.size))
        at += -(-(off + a.size) // per16) * per16 + per16
    buf = np.zeros(at, dtype=DTYPES[kind])
    for (start, n), (_, a) in zip(spans, fields(kind)):
        buf[start:start + n] = a
    return buf, spans


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", range(4), ids=KIND_NAMES)
def test_gpu_scan_matches_restatement_exactly(kind, off):
    """the HIP path on every field of the set, whole (off 0: 16-byte aligned) and as views offset by 1, 2 and 3 elements; one call for
    the whole list (a few hundred fields: many launch tables), and the inputs keep their bits"""
    import torch
    import pam_amd
    buf, spans = _pack(kind, off)
    dev = torch.from_numpy(buf).to("cuda:0")
    assert dev.data_ptr() % 16 == 0
    views = [dev[s:s + n] for s, n in spans]
    assert all((v.data_ptr() - off * dev.element_size()) % 16 == 0 for v in views)
    count, first = pam_amd.validate_fields(views, [True] * len(views))
    want = expected(kind)
    got = np.concatenate([count, first], axis=1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(fields(kind)[i][0], got[i], want[i]) for i in bad[:5]]
    assert dev.cpu().numpy().tobytes() == buf.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", range(4), ids=KIND_NAMES)
def test_gpu_single_field_calls_match_restatement(kind):
    """one field per call (a table of one) at the largest sizes, every planting"""
    import torch
    import pam_amd
    want = expected(kind)
    for (label, a), w in list(zip(fields(kind), want))[-40:]:
        t = torch.from_numpy(np.array(a)).to("cuda:0")
        count, first = pam_amd.validate_fields([t], [True])
        assert np.array_equal(np.concatenate([count[0], first[0]]), w), label


def _mixed_list(num):
    """`num` fields of mixed kinds and sizes, a 1-element field beside a 2^17 + 1 one; offenders in the first and the last field of
    every chunk of 32"""
    rng = np.random.default_rng(77 + num)
    sizes = [1, (1 << 17) + 1, 63, 64, 65, 255, 1025, 4097, 7, 300]
    out = []
    for f in range(num):
        kind = f % 4
        n = sizes[f % len(sizes)]
        a = _clean(kind, n, rng)
        if f % 32 in (0, 31) or f == num - 1:
            classes = [c for c in _offenders(kind) if c is not None]
            for ci, vals in enumerate(classes):
                a[(n - 1) * ci // max(1, len(classes) - 1) if len(classes) > 1 else n - 1] = vals[f % len(vals)]
        out.append(a)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("num", [1, 31, 32, 33, 70])
def test_gpu_lists_equal_per_field_calls(num):
    import torch
    import pam_amd
    arrays = _mixed_list(num)
    tens = [torch.from_numpy(a).to("cuda:0") for a in arrays]
    positive = [f % 5 != 4 for f in range(num)]
    count, first = pam_amd.validate_fields(tens, positive)
    assert count.shape == (num, 3) and first.shape == (num, 3)
    for f, (t, a) in enumerate(zip(tens, arrays)):
        c1, f1 = pam_amd.validate_fields([t], [positive[f]])
        assert np.array_equal(c1[0], count[f]) and np.array_equal(f1[0], first[f]), f
        wc, wf = ref.scan(a, positive[f])
        assert np.array_equal(count[f], wc) and np.array_equal(first[f], wf), f
    dirty = {f for f in range(num) if count[f].any()}
    assert {f for f in range(num) if f % 32 in (0, 31) or f == num - 1} == dirty


@pytest.mark.gpu
def test_gpu_result_scratch_grows_with_the_list():
    """from no scratch at all: a list of 1 field, then of 300 (past the 256 fields the scratch starts with: it grows), then of 2 on the
    scratch the 300 left, then the 300 again from nothing after pam_amd_modules_finalize.  Fields of a few hundred elements of mixed
    kinds, an offender of the kind's last class at f % n in every third field"""
    import torch
    import pam_amd
    rng = np.random.default_rng(4242)
    arrays = []
    for f in range(300):
        a = _clean(f % 4, 200 + f, rng)
        if f % 3 == 0:
            a[f % a.size] = [c for c in _offenders(f % 4) if c is not None][-1][0]
        arrays.append(a)
    want = [ref.scan(a, True) for a in arrays]
    tens = [torch.from_numpy(a).to("cuda:0") for a in arrays]
    lib = capi.load()
    capi.check(lib.pam_amd_modules_finalize())
    for num in (1, 300, 2, None, 300):
        if num is None:
            capi.check(lib.pam_amd_modules_finalize())
            continue
        count, first = pam_amd.validate_fields(tens[:num], [True] * num)
        assert count.shape == (num, 3) and first.shape == (num, 3)
        for f in range(num):
            assert np.array_equal(count[f], want[f][0]) and np.array_equal(first[f], want[f][1]), (num, f)
    assert sum(int(w[0].any()) for w in want) == 100


@pytest.mark.gpu
def test_gpu_positive_off_ignores_negatives():
    import torch
    import pam_amd
    tens = [torch.full((5000,), -3, dtype=_torch_dtype(k), device="cuda:0") for k in range(4)]
    count, first = pam_amd.validate_fields(tens, [False] * 4)
    assert not count.any() and (first == -1).all()
    count, first = pam_amd.validate_fields(tens, [True] * 4)
    assert np.array_equal(count, [[0, 0, 5000]] * 4) and np.array_equal(first, [[-1, -1, 0]] * 4)


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
        t.fill_(float("nan"))
        count, first = pam_amd.validate_fields([t], [True])
    assert np.array_equal(count, [[n, 0, 0]]) and np.array_equal(first, [[0, -1, -1]])


@pytest.mark.gpu
def test_gpu_python_requires_contiguous_tensors_of_a_checked_dtype():
    import torch
    import pam_amd
    t = torch.zeros((8, 8), dtype=torch.float64, device="cuda:0")
    with pytest.raises(capi.PamAmdError, match="contiguous"):
        pam_amd.validate_fields([t[:, ::2]], [True])
    with pytest.raises(capi.PamAmdError, match="dtype"):
        pam_amd.validate_fields([t.to(torch.float16)], [True])


def _filtered(case, name, which, die):
    """validate_nan / validate_inf / validate_pos: the restatement's lines of one class"""
    _, arr, pos = next(e for e in case_entries(case) if e[0] == name)
    m = ref.masks(arr, pos)
    out = []
    if m is not None:
        fmt = (ref.NAN_LINE, ref.INF_LINE, ref.NEG_LINE)[which]
        for i in np.flatnonzero(m[which]):
            out.append(fmt % (name, i))
            if die:
                return "".join(l + "\n" for l in out) + "\n", True
    return "".join(l + "\n" for l in out), False


@pytest.mark.gpu
def test_gpu_cxx_adaptor_writes_the_reference_lines(tmp_path):
    """the work-alike's validate_all / validate (and validate_nan / validate_inf / validate_pos) on the golden's cases: its stderr is
    the reference's, character for character, in the reference's registration order; a clean validate_all prints nothing"""
    exe = cxx_program("validate_dm")
    for case in golden():
        script, want = [], []
        for e in case["entries"]:
            script.append("entry %s %s %d %d %s" % (e["name"], e["kind"].replace(" ", ""), e["positive"], len(e["bits"]), " ".join(e["bits"])))
        for call in case["calls"]:
            script.append("call %s %s %d" % (call["fn"], call["name"] or "-", call["die"]))
            want.append((call["stderr"], call["threw"]))
        for e in case["entries"]:
            for which, fn in enumerate(("validate_nan", "validate_inf", "validate_pos")):
                for die in (0, 1):
                    script.append("call %s %s %d" % (fn, e["name"], die))
                    want.append(_filtered(case, e["name"], which, die))
        path = tmp_path / (case["name"] + ".txt")
        path.write_text("\n".join(script) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (case["name"], r.returncode, r.stderr[-2000:])
        got = [(m.group(2), bool(int(m.group(1)))) for m in re.finditer(r"### (\d)\n(.*?)###END\n", r.stdout, flags=re.S)]
        assert len(got) == len(want), case["name"]
        for n, (g, w) in enumerate(zip(got, want)):
            assert g == w, (case["name"], script[len(case["entries"]) + n], g, w)
    clean = next(c for c in golden() if c["name"] == "every_kind_clean")
    assert all(c["stderr"] == "" for c in clean["calls"])


@pytest.mark.gpu
def test_gpu_python_datamanager_writes_the_reference_lines(capsys):
    """DataManager.validate_all / validate: the same lines on sys.stderr in the same order; with die_on_failed_check the module's
    endrun("") follows the first line (it raises PamAmdError; the empty line the C++ endrun prints is the exception here)"""
    import torch
    from pam_amd.coupler import DataManager
    for case in golden():
        dm = DataManager(torch.device("cuda:0"))
        for e in case["entries"]:
            a = entry_array(e)
            t = torch.from_numpy(a.view(np.uint8).copy()).to("cuda:0")
            t = t.view(torch.bool) if e["kind"] == "bool" else t.view(_torch_dtype(["double", "float", "int", "long long"].index(e["kind"])))
            dm.register_existing(e["name"], "", t, positive=e["positive"])
        for call in case["calls"]:
            capsys.readouterr()
            threw = False
            try:
                if call["fn"] == "validate_all":
                    dm.validate_all(call["die"])
                else:
                    dm.validate(call["name"], call["die"])
            except capi.PamAmdError:
                threw = True
            err = capsys.readouterr().err
            want = call["stderr"][:-1] if call["threw"] else call["stderr"]       # without endrun's own empty line
            assert (err, threw) == (want, call["threw"]), (case["name"], call["fn"], call["name"], call["die"])


@pytest.mark.gpu
def test_gpu_driver_validate_leaves_stdout_unchanged_and_finds_nothing():
    def run(*args):
        r = subprocess.run([DRIVER, "--yaml", CI_YAML, "--steps", "2"] + list(args) + ["-"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r
    plain, checked = run(), run("--validate")
    assert plain.stdout == checked.stdout and plain.stdout.strip()
    assert "WARNING" not in checked.stderr
