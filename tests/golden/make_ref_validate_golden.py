#!/usr/bin/env python3
"""Write tests/golden/validate_ref.json: the pin of tests/validate_ref.py (and through it of the device scan and of the adaptors) to
the reference's own text of DataManager::validate / validate_all (pam_core/DataManager.h:408-509).

The reference (PAM) is not part of this repository and is not needed to run the tests.  Where a checkout of it is at hand, this
script compiles tests/ref_validate/harness.cpp with g++ against the YAKL stand-in of oracle/ref/ and the reference's
pam_core/DataManager.h, in a temporary directory outside the repository (nothing compiled is kept), registers the entries of every
case below in a reference DataManager, in the order given, and records for every call what the reference wrote to std::cerr and
whether the call ended in endrun's throw.  The inputs are recorded as bit patterns (one hex string per element), so NaN payloads,
signed zeros and subnormals survive.  No source text of the reference is stored.

Per case the calls are: validate_all(), validate_all(true), and validate(name) and validate(name, true) for every entry.

Usage:  python tests/golden/make_ref_validate_golden.py REFERENCE_DIR [--check]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
JSON = os.path.join(HERE, "validate_ref.json")
HARNESS = os.path.join(ROOT, "tests", "ref_validate", "harness.cpp")

KIND_ID = {"double": 0, "float": 1, "int": 2, "long long": 3, "bool": 4}
DTYPE = {"double": np.float64, "float": np.float32, "int": np.int32, "long long": np.int64, "bool": np.uint8}
UINT = {"double": np.uint64, "float": np.uint32, "int": np.uint32, "long long": np.uint64, "bool": np.uint8}

F64_SNAN, F64_NEG_NAN, F64_NEG_SNAN = 0x7ff0000000000001, 0xfff8000000000000, 0xfff0000000000001
F32_SNAN, F32_NEG_NAN, F32_NEG_SNAN = 0x7f800001, 0xffc00000, 0xff800001
INT_MIN, LLONG_MIN = -2 ** 31, -2 ** 63


def vals(kind, values):
    with np.errstate(over="ignore"):
        return np.array(values, dtype=DTYPE[kind])


def bits(kind, patterns):
    return np.array(patterns, dtype=UINT[kind]).view(DTYPE[kind])


def cases():
    """[(case name, [(entry name, kind, positive, array)])], the entries in registration order (NOT alphabetical, so the order shows)"""
    inf, nan = np.inf, np.nan
    out = []
    out.append(("four_entries", [
        ("a", "double", True, vals("double", [1.0, nan, 2.0, -inf, 0.5, -0.0, -1e-300, inf])),
        ("n", "int", True, vals("int", [1, -2, 0])),
        ("b", "bool", False, vals("bool", [1, 0, 1])),
        ("free", "double", False, vals("double", [-1.0, nan, 0.0]))]))
    out.append(("every_kind_clean", [
        ("zd", "double", True, vals("double", [0.0, 1.5, 1e300, 4.9e-324, -0.0])),
        ("yf", "float", True, vals("float", [0.0, 1.5, 3e38, 1e-45, -0.0])),
        ("xi", "int", True, vals("int", [0, 1, 2 ** 31 - 1])),
        ("wl", "long long", True, vals("long long", [0, 1, 2 ** 63 - 1])),
        ("vd", "double", False, vals("double", [-1.0, -1e300, 0.0])),
        ("ui", "int", False, vals("int", [-1, INT_MIN, 0]))]))
    out.append(("every_kind_dirty", [
        ("zd", "double", True, vals("double", [0.0, -1.5, nan, inf, -inf, 1.0, nan])),
        ("yf", "float", True, vals("float", [nan, 0.0, -inf, -2.0, inf, 1.0])),
        ("xi", "int", True, vals("int", [0, -1, 5, -7])),
        ("wl", "long long", True, vals("long long", [-3, 1, -2 ** 40])),
        ("vf", "float", False, vals("float", [-1.0, inf, nan, -inf]))]))
    out.append(("every_element_offending", [
        ("allnan", "double", False, vals("double", [nan] * 5)),
        ("allneginf", "float", True, vals("float", [-inf] * 4)),
        ("allneg", "int", True, vals("int", [-1, -2, -3, -4, -5, -6])),
        ("mixed", "double", True, vals("double", [nan, -inf, -1.0, inf, -2.0]))]))
    out.append(("nan_flavours", [
        ("d", "double", True, bits("double", [F64_SNAN, F64_NEG_NAN, F64_NEG_SNAN, 0x3ff0000000000000, 0x7ff8000000000000])),
        ("f", "float", True, bits("float", [F32_SNAN, 0x3f800000, F32_NEG_NAN, F32_NEG_SNAN, 0x7fc00000]))]))
    out.append(("integer_minimums", [
        ("i", "int", True, vals("int", [INT_MIN, 0, 2 ** 31 - 1, INT_MIN])),
        ("l", "long long", True, vals("long long", [0, LLONG_MIN, 2 ** 63 - 1])),
        ("ifree", "int", False, vals("int", [INT_MIN])),
        ("lfree", "long long", False, vals("long long", [LLONG_MIN]))]))
    out.append(("subnormals", [
        ("d", "double", True, bits("double", [0x0000000000000001, 0x8000000000000001, 0x000fffffffffffff, 0x800fffffffffffff, 0x8000000000000000])),
        ("f", "float", True, bits("float", [0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x80000000])),
        ("dfree", "double", False, bits("double", [0x8000000000000001]))]))
    return out


def hex_bits(kind, arr):
    return ["%x" % int(v) for v in np.ascontiguousarray(arr).view(UINT[kind])]


def run_reference(ref):
    recorded = []
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libref_validate.so")
        inc = ["-I" + os.path.join(ROOT, "oracle", "ref"), "-I" + os.path.join(ref, "pam_core")]
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"] + inc + [HARNESS, "-o", so],
                       check=True)
        lib = C.CDLL(so)
        lib.rv_new.restype = C.c_void_p
        lib.rv_free.argtypes = [C.c_void_p]
        lib.rv_register.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_longlong, C.c_void_p, C.c_int]
        lib.rv_call.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        buf = C.create_string_buffer(1 << 16)
        for case, entries in cases():
            dm = lib.rv_new()
            rec = {"name": case, "entries": [], "calls": []}
            for name, kind, positive, arr in entries:
                arr = np.ascontiguousarray(arr)
                rc = lib.rv_register(dm, name.encode(), KIND_ID[kind], arr.size, arr.ctypes.data_as(C.c_void_p), int(positive))
                assert rc == 0, (case, name, rc)
                rec["entries"].append({"name": name, "kind": kind, "positive": bool(positive), "bits": hex_bits(kind, arr)})
            for name in [None] + [e[0] for e in entries]:
                for die in (False, True):
                    rc = lib.rv_call(dm, None if name is None else name.encode(), int(die), buf, len(buf))
                    assert rc in (0, 1), (case, name, die, rc)
                    rec["calls"].append({"fn": "validate_all" if name is None else "validate", "name": name, "die": die,
                                         "stderr": buf.value.decode(), "threw": bool(rc)})
            lib.rv_free(dm)
            recorded.append(rec)
        del lib
    return {"source": "written by tests/golden/make_ref_validate_golden.py from a run of the reference's pam_core/DataManager.h",
            "cases": recorded}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1 or not os.path.isdir(args[0]):
        raise SystemExit(__doc__)
    text = json.dumps(run_reference(os.path.abspath(args[0])), indent=1) + "\n"
    if "--check" in sys.argv:
        ok = os.path.exists(JSON) and open(JSON).read() == text
        print("validate_ref.json: %s" % ("reproduced" if ok else "DIFFERS"))
        sys.exit(0 if ok else 1)
    with open(JSON, "w") as fh:
        fh.write(text)
    print("wrote", JSON)


if __name__ == "__main__":
    main()
