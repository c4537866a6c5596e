"""ctypes binding of tests/emu/esmt_emu.cpp (host emulation of the scalar momentum transport kernels).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
from esmt_ref import RD, RV

_LIB = None
POISON = -7.0e77
FIELDS = ("wvel", RD, RV, "esmt_u", "esmt_v")
PROFILES = ("zmid", "dz", "force_u", "force_v", "gcm_u", "gcm_v", "cos", "sin")
MEANS = ("rho_mean", "u_mean", "v_mean")


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("esmt_emu"))
        lib.emu_esmt_set.restype = None
        lib.emu_esmt_set.argtypes = [C.c_int] * 3 + [C.c_void_p] * 6
        lib.emu_esmt_diagnose.restype = None
        lib.emu_esmt_diagnose.argtypes = [C.c_int] * 3 + [C.c_void_p] * 9 + [C.c_double, C.c_int] + [C.c_void_p] * 2
        lib.emu_esmt_pgf.restype = None
        lib.emu_esmt_pgf.argtypes = [C.c_int] * 3 + [C.c_void_p] * 14 + [C.c_double] * 2 + [C.c_int, C.c_void_p, C.c_int]
        _LIB = lib
    return _LIB


def ptr(a):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def workspace_doubles(nens, nz, kmax):
    return 6 * kmax * nz * nens


def call_arguments(case):
    """the arrays the entry points take: -> the fields (copied: two are written), the sizes (nens, nx, nz), the profiles and tables, the
    three means and the two tendencies (poisoned), and the workspace (poisoned)"""
    F = {n: np.array(case["fields"][n], dtype=np.float64, order="C") for n in FIELDS}
    nz, ny, nx, nens = F["wvel"].shape
    assert ny == 1
    prof = {n: None if case.get(n) is None else np.ascontiguousarray(case[n], dtype=np.float64) for n in PROFILES}
    means = {n: np.full((nz, nens), POISON) for n in MEANS}
    tend = {x: None if prof["gcm_" + x] is None else np.full((nz, nens), POISON) for x in "uv"}
    work = np.full(max(workspace_doubles(nens, nz, int(case["kmax"])), 1), POISON)
    return F, (nens, nx, nz), prof, means, tend, work


class EmuBackend:
    """the interface of esmt_ref.RefBackend over the emulated kernels: diagnose, then the force with the means it gave"""

    def __init__(self, wide=False):
        self.lib, self.wide = load(), wide

    def diagnose(self, case, feedback=False):
        F, sizes, prof, means, tend, _ = call_arguments(case)
        self.lib.emu_esmt_diagnose(*sizes, ptr(F[RD]), ptr(F[RV]), ptr(F["esmt_u"]), ptr(F["esmt_v"]), *[ptr(means[n]) for n in MEANS],
                                   ptr(prof["gcm_u"]), ptr(prof["gcm_v"]), float(case["gcm_dt"]), 1 if feedback else 0, ptr(tend["u"]), ptr(tend["v"]))
        out = dict(means)
        out.update({"tend_" + x: t for x, t in tend.items() if t is not None})
        return out

    def run(self, case):
        F, sizes, prof, means, _, work = call_arguments(case)
        self.lib.emu_esmt_diagnose(*sizes, ptr(F[RD]), ptr(F[RV]), ptr(F["esmt_u"]), ptr(F["esmt_v"]), *[ptr(means[n]) for n in MEANS], None, None,
                                   1.0, 0, None, None)
        self.lib.emu_esmt_pgf(*sizes, ptr(F["esmt_u"]), ptr(F["esmt_v"]), ptr(F["wvel"]), ptr(F[RD]), ptr(F[RV]), ptr(prof["zmid"]), ptr(prof["dz"]),
                              ptr(means["rho_mean"]), ptr(means["u_mean"]), None if case.get("skip_v") else ptr(means["v_mean"]),
                              ptr(prof["force_u"]), ptr(prof["force_v"]), ptr(prof["cos"]), ptr(prof["sin"]), float(case["dx"]), float(case["dt"]),
                              int(case["kmax"]), ptr(work), 1 if self.wide else 0)
        return {n: F[n] for n in ("esmt_u", "esmt_v")}

    def set(self, rho_d, rho_v, src_u, src_v):
        nz, _, nx, nens = rho_d.shape
        eu, ev = np.full(rho_d.shape, POISON), np.full(rho_d.shape, POISON)
        self.lib.emu_esmt_set(nens, nx, nz, *[ptr(np.ascontiguousarray(a, dtype=np.float64)) for a in (rho_d, rho_v, src_u, src_v)], ptr(eu), ptr(ev))
        return eu, ev
