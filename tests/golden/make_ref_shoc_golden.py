#!/usr/bin/env python3
"""Write tests/golden/shoc_coupling_ref.npz and tests/golden/shoc_extract.json: the pin of tests/shoc_coupling_ref.py (and through it of
the device code) to the reference's own text of physics/sgs/shoc/SGS.h.

The reference (PAM) is not part of this repository and is not needed to run the tests.  Where a checkout of it is at hand, this script
compiles tests/ref_shoc/harness.cpp with `g++ -O2 -ffp-contract=off` against the YAKL stand-in of oracle/ref/ (tests/ref_shoc/YAKL.h
adds the reshape<2>({..}) SGS.h needs) and the reference's SGS.h, pam_coupler.h and MultipleFields.h, on the non-SHOC_CXX path, in a
temporary directory outside the repository (nothing compiled is kept).  shoc_init_fortran does nothing and shoc_main_fortran is the
stand-in body of pam_amd/csrc/shoc_device.h.  Recorded per tracer set (kessler_*, p3_*):

  the inputs            the coupler state of tests/shoc_cases.make_state, the grid, the surface momentum fluxes
  received_<name>       every array shoc_main_fortran was given, as the reference laid it out (the Fortran-call layout)
  out_<name>, out_q     the coupler state after SGS::timeStep
  info, consts, sgs     get_num_tracers(), the tke tracer's flags, the number of shoc_main calls; the constructor's constants; option "sgs"

shoc_extract.json holds SHA-256 digests of the reference's signature lines and of its two endrun lines (whitespace and `pam::` removed).
No source text of the reference is stored.

Usage:  python tests/golden/make_ref_shoc_golden.py REFERENCE_DIR [--check]
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
NPZ = os.path.join(HERE, "shoc_coupling_ref.npz")
JSON = os.path.join(HERE, "shoc_extract.json")
HARNESS = os.path.join(ROOT, "tests", "ref_shoc", "harness.cpp")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import test_boundary_surface as tb    # noqa: E402

SGS_H = "physics/sgs/shoc/SGS.h"
SIGNATURE_LINES = [85, 92, 150, 782, 786]
MESSAGE_LINES = [190, 195]
CASES = {"kessler": ((5, 2, 3, 3), 1), "p3": ((4, 1, 5, 2), 7)}     # (nz, ny, nx, nens), extra tracers
XLEN, YLEN, CRM_DT = 16000.0, 12000.0, 2.0
R_D, R_V = 287.0, 461.0                     # the coupler's options (a microphysics sets them); the SGS class has its own R_d, R_v
STATE = ("rho_d", "rho_v", "rho_c", "uvel", "vvel", "wvel", "temp", "tke", "wthv_sec", "tk", "tkh", "cldfrac")
P3 = ("cloud_water_num", "rain", "rain_num", "ice", "ice_num", "ice_rime", "ice_rime_vol")
_DP = C.POINTER(C.c_double)


def extract(ref):
    lines = open(os.path.join(ref, SGS_H)).read().split("\n")
    sig = {}
    for ln in SIGNATURE_LINES:
        got = tb._norm(" ".join(lines[ln - 1:ln + 2]))
        sig["%s:%d" % (SGS_H, ln)] = tb._digest(got[:got.index("{")])
    msg = {"%s:%d" % (SGS_H, ln): tb._digest(tb._norm(lines[ln - 1])) for ln in MESSAGE_LINES}
    return {"source": "read from the reference's header by tests/golden/make_ref_shoc_golden.py", "signature_sha256": sig,
            "endrun_line_sha256": msg}


def received_shapes(nz, ncol, ntr):
    """name -> shape, in the order tests/ref_shoc/harness.cpp records them"""
    c, e, n = (nz, ncol), (nz + 1, ncol), (ncol,)
    return [("host_dx", n), ("host_dy", n), ("thv", c), ("zt_grid", c), ("zi_grid", e), ("pres", c), ("presi", e), ("pdel", c), ("wthl_sfc", n),
            ("wqw_sfc", n), ("uw_sfc", n), ("vw_sfc", n), ("wtracer_sfc", (ntr, ncol)), ("w_field", c), ("inv_exner", c), ("phis", n),
            ("host_dse", c), ("tke", c), ("thetal", c), ("qw", c), ("u_wind", c), ("v_wind", c), ("qtracers", (ntr, nz, ncol)), ("wthv_sec", c),
            ("tkh", c), ("tk", c), ("ql", c), ("cldfrac", c)]


def run_reference(ref):
    import shoc_cases as sc
    d = {}
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libref_shoc.so")
        inc = ["-I" + os.path.join(ROOT, "tests", "ref_shoc"), "-I" + os.path.join(ROOT, "oracle", "ref"), "-I" + os.path.join(ref, "pam_core"),
               "-I" + os.path.join(ref, "physics", "sgs", "shoc")]
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"] + inc + [HARNESS, "-o", so],
                       check=True)
        lib = C.CDLL(so)
        lib.ref_shoc_time_step.argtypes = [C.c_int] * 5 + [C.c_double] * 5 + [_DP, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), _DP,
                                                                             _DP, C.POINTER(C.c_int), _DP, C.c_char_p]
        for label, (shape, ntr) in CASES.items():
            nz, ny, nx, nens = shape
            ncol = ny * nx * nens
            s = sc.make_state(shape, ntr)
            p3 = label == "p3"
            names = ["density_dry", "water_vapor", "cloud_water" if p3 else "cloud_liquid", "uvel", "vvel", "wvel", "temp", "tke", "wthv_sec",
                     "tk", "tkh", "cldfrac"] + list(P3 if p3 else ("precip_liquid",)) + ["sfc_mom_flx_u", "sfc_mom_flx_v"]
            arrays = [np.array(s[k], order="C") for k in STATE] + [np.array(x, order="C") for x in s["q"]] + \
                     [np.array(s["flx_u"], order="C"), np.array(s["flx_v"], order="C")]
            for k in STATE + ("flx_u", "flx_v", "zint", "zmid"):
                d["%s_%s" % (label, k)] = np.array(s[k], order="C")
            d[label + "_q"] = np.stack(s["q"])
            shapes = received_shapes(nz, ncol, ntr)
            received = np.full(sum(int(np.prod(shp)) for _, shp in shapes), -1.0)
            relvar = np.full(shape, -1.0)
            info, consts, opt = (C.c_int * 4)(), np.zeros(16), C.create_string_buffer(16)
            zint = np.array(s["zint"], order="C")
            rc = lib.ref_shoc_time_step(nens, nx, ny, nz, int(p3), XLEN, YLEN, CRM_DT, R_D, R_V, zint.ctypes.data_as(_DP), len(names),
                                        (C.c_char_p * len(names))(*[n.encode() for n in names]),
                                        (C.c_void_p * len(names))(*[a.ctypes.data for a in arrays]), relvar.ctypes.data_as(_DP),
                                        received.ctypes.data_as(_DP), info, consts.ctypes.data_as(_DP), opt)
            assert rc == 0, (label, rc)
            at = 0
            for name, shp in shapes:
                n = int(np.prod(shp))
                d["%s_received_%s" % (label, name)] = received[at:at + n].reshape(shp).copy()
                at += n
            for k, a in zip(STATE, arrays):
                d["%s_out_%s" % (label, k)] = a
            d[label + "_out_q"] = np.stack(arrays[len(STATE):len(STATE) + ntr])
            d[label + "_out_flx_u"], d[label + "_out_flx_v"] = arrays[-2], arrays[-1]
            d[label + "_out_inv_qc_relvar"] = relvar
            d[label + "_info"] = np.array(list(info), dtype=np.int64)
            d[label + "_consts"] = consts
            d[label + "_sgs"] = np.frombuffer(opt.value.ljust(16, b"\0"), dtype=np.uint8).copy()
        del lib
    d["params"] = np.array([XLEN, YLEN, CRM_DT, R_D, R_V])
    return d


def npz_bytes(d):
    buf = io.BytesIO()
    np.savez_compressed(buf, **{k: d[k] for k in sorted(d)})
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
        print("shoc_extract.json: %s\nshoc_coupling_ref.npz: %s" % ("up to date" if ok_json else "DIFFERS", "reproduced" if ok_npz else "DIFFERS"))
        sys.exit(0 if ok_json and ok_npz else 1)
    with open(JSON, "w") as fh:
        fh.write(text)
    with open(NPZ, "wb") as fh:
        fh.write(npz_bytes(d))
    print("wrote", JSON, "and", NPZ)


if __name__ == "__main__":
    main()
