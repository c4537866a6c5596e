#!/usr/bin/env python3
"""Write tests/golden/plugins_ref.npz and tests/golden/plugins_extract.json: the pin of tests/plugins_ref.py (and through it of the
device code) to the reference's own text of the forced radiation plug-in, PamCoupler::compute_pressure_array and the "none"
microphysics.

The reference (PAM) is not part of this repository and is not needed to run the tests.  Where a checkout of it is at hand, this
script compiles tests/ref_plugins/harness.cpp with `g++ -O2 -ffp-contract=off` against the YAKL stand-in of oracle/ref/ and the
reference's physics/radiation/forced/radiation.h, pam_core/pam_coupler.h and physics/micro/none/Microphysics.h, in a temporary
directory outside the repository (nothing compiled is kept), runs the cases below through it and records

  plugins_ref.npz       inputs and the reference's outputs: radiation at three rad grids (two timeSteps each), the pressure array,
                        and what Microphysics::init of "none" leaves in the coupler
  plugins_extract.json  SHA-256 digests of the reference's signature lines, taken as tests/golden/extract_statistics.py takes them
                        (the line and the next two joined, whitespace and `pam::` removed, up to the opening brace)

No source text of the reference is stored.

Usage:  python tests/golden/make_ref_plugins_golden.py REFERENCE_DIR [--check]
"""
import ctypes as C
import io
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
NPZ = os.path.join(HERE, "plugins_ref.npz")
JSON = os.path.join(HERE, "plugins_extract.json")
HARNESS = os.path.join(ROOT, "tests", "ref_plugins", "harness.cpp")
sys.path.insert(0, os.path.dirname(HERE))

import test_boundary_surface as tb    # noqa: E402

# reference file -> the line numbers of the signatures recorded
LINES = {"physics/radiation/forced/radiation.h": [12, 16, 26, 47], "physics/radiation/none/radiation.h": [11, 16, 20, 23],
         "physics/sgs/none/SGS.h": [15, 20, 26, 31, 36], "physics/micro/none/Microphysics.h": [39, 51, 81, 87, 91],
         "pam_core/pam_coupler.h": [360]}

NENS, NX, NY, NZ = 3, 6, 4, 2
RAD_GRIDS = [(1, 1), (3, 2), (6, 4)]     # (rad_nx, rad_ny)
CP_D, CRM_DT, R_D, R_V = 1003.0, 20.0, 287.0, 461.0
CALLS = 2
_DP = C.POINTER(C.c_double)


def extract(ref):
    out = {}
    for rel, lns in LINES.items():
        lines = open(os.path.join(ref, rel)).read().split("\n")
        for ln in lns:
            got = tb._norm(" ".join(lines[ln - 1:ln + 2]))
            out["%s:%d" % (rel, ln)] = tb._digest(got[:got.index("{")])
    return {"source": "read from the reference's headers by tests/golden/make_ref_plugins_golden.py", "signature_sha256": out}


def inputs():
    """temperatures of the troposphere; tendencies of both signs with a subnormal, a zero of each sign and a NaN among them"""
    rng = np.random.default_rng(20240229)
    shape = (NZ, NY, NX, NENS)
    d = {"temp": rng.uniform(190.0, 310.0, shape), "rho_d": rng.uniform(0.05, 1.3, shape), "rho_v": rng.uniform(0.0, 0.02, shape)}
    for rad_nx, rad_ny in RAD_GRIDS:
        q = rng.standard_normal((NZ, rad_ny, rad_nx, NENS)) * 10.0 ** rng.uniform(-4, 1, (NZ, rad_ny, rad_nx, NENS))
        flat = q.reshape(-1)
        flat[1] = 4.9e-324
        flat[2] = -0.0
        flat[4] = np.nan
        d["tend_%dx%d" % (rad_nx, rad_ny)] = q
    return d


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def run_reference(ref):
    d = inputs()
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libref_plugins.so")
        inc = ["-I" + os.path.join(ROOT, "oracle", "ref"), "-I" + os.path.join(ref, "pam_core"),
               "-I" + os.path.join(ref, "physics", "radiation", "forced"), "-I" + os.path.join(ref, "physics", "micro", "none")]
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"] + inc + [HARNESS, "-o", so],
                       check=True)
        lib = C.CDLL(so)
        lib.ref_radiation_forced.argtypes = [C.c_int] * 6 + [_DP, _DP, C.c_double, C.c_double, C.c_int]
        lib.ref_compute_pressure.argtypes = [C.c_int] * 4 + [_DP] * 3 + [C.c_double, C.c_double, _DP]
        lib.ref_micro_none_init.argtypes = [C.c_int] * 4 + [_DP, _DP, C.POINTER(C.c_int), C.c_char_p]
        for rad_nx, rad_ny in RAD_GRIDS:
            t = d["temp"].copy()
            rc = lib.ref_radiation_forced(NENS, NX, NY, NZ, rad_nx, rad_ny, _p(t), _p(d["tend_%dx%d" % (rad_nx, rad_ny)]), CP_D, CRM_DT, CALLS)
            assert rc == 0, ("ref_radiation_forced", rad_nx, rad_ny, rc)
            d["temp_out_%dx%d" % (rad_nx, rad_ny)] = t
        p = np.full(d["temp"].shape, -1.0)
        assert lib.ref_compute_pressure(NENS, NX, NY, NZ, _p(d["rho_d"]), _p(d["rho_v"]), _p(d["temp"]), R_D, R_V, _p(p)) == 0
        d["pressure"] = p
        consts, wv, info, name = np.zeros(6), np.full(d["temp"].shape, -1.0), (C.c_int * 4)(), C.create_string_buffer(16)
        assert lib.ref_micro_none_init(NENS, NX, NY, NZ, _p(consts), _p(wv), info, name) == 0
        d["micro_none_consts"] = consts           # R_d, R_v, cp_d, cp_v, grav, p0
        d["micro_none_water_vapor"] = wv
        d["micro_none_info"] = np.array(list(info), dtype=np.int64)   # get_num_tracers(), coupler tracers, positive, adds_mass
        d["micro_none_name"] = np.frombuffer(name.value.ljust(16, b"\0"), dtype=np.uint8).copy()
        del lib
    d["params"] = np.array([CP_D, CRM_DT, R_D, R_V, CALLS], dtype=np.float64)
    return d


def npz_bytes(d):
    buf = io.BytesIO()
    np.savez(buf, **{k: d[k] for k in sorted(d)})
    return buf.getvalue()


def same_arrays(d, path):
    if not os.path.exists(path):
        return False
    old = np.load(path)
    return sorted(old.files) == sorted(d) and all(old[k].dtype == np.asarray(d[k]).dtype and old[k].tobytes() == np.asarray(d[k]).tobytes()
                                                  for k in d)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1 or not os.path.isdir(args[0]):
        raise SystemExit(__doc__)
    ref = os.path.abspath(args[0])
    text = json.dumps(extract(ref), indent=1, sort_keys=True) + "\n"
    d = run_reference(ref)
    if "--check" in sys.argv:
        ok_json = os.path.exists(JSON) and open(JSON).read() == text
        ok_npz = same_arrays(d, NPZ)
        print("plugins_extract.json: %s\nplugins_ref.npz: %s" % ("up to date" if ok_json else "DIFFERS", "reproduced" if ok_npz else "DIFFERS"))
        sys.exit(0 if ok_json and ok_npz else 1)
    with open(JSON, "w") as fh:
        fh.write(text)
    with open(NPZ, "wb") as fh:
        fh.write(npz_bytes(d))
    print("wrote", JSON, "and", NPZ)


if __name__ == "__main__":
    main()
