"""ctypes binding of tests/emu/lsforcing_emu.cpp (host emulation of the large-scale forcing kernels).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
from lsforcing_ref import PROFILES, QUANTITIES, STATE, VAPOUR

_LIB = None
POISON = -7.0e77
NUDGE_FIELDS = ("temp", "density_dry", VAPOUR, "uvel", "vvel")


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("lsforcing_emu"))
        lib.emu_ls_nudging.restype = None
        lib.emu_ls_nudging.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p]
        lib.emu_ls_forcing.restype = None
        lib.emu_ls_forcing.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 12 + [C.c_double] * 3 + [C.c_int]
        _LIB = lib
    return _LIB


def ptr(a):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def table(arrays):
    return (C.c_void_p * len(arrays))(*[ptr(a) for a in arrays])


def call_arguments(case):
    """the arrays both entry points take: -> the fields (copied: they are written), the sizes, the profiles, and the tables of the
    targets, the rates and the increments (poisoned) in the order of QUANTITIES, None where a target is absent"""
    F = {n: np.array(case["fields"][n], dtype=np.float64, order="C") for n in set(STATE + NUDGE_FIELDS + tuple(case["tracers"]))}
    nz, ny, nx, nens = F["temp"].shape
    prof = {n: None if case.get(n) is None else np.ascontiguousarray(case[n], dtype=np.float64) for n in PROFILES + ("zmid", "fcor")}
    target = case.get("target") or {x: None for x in QUANTITIES}
    tgt = [None if target[x] is None else np.ascontiguousarray(target[x], dtype=np.float64) for x in QUANTITIES]
    rate = [None if t is None else np.ascontiguousarray(case["rate"][x], dtype=np.float64) for x, t in zip(QUANTITIES, tgt)]
    inc = [None if t is None else np.full((nz, nens), POISON) for t in tgt]
    return F, (nens, nx, ny, nz), prof, tgt, rate, inc


class EmuBackend:
    """the interface of lsforcing_ref.RefBackend over the emulated kernels: the nudging where a target is given, then the forcing"""

    def __init__(self, wide=False):
        self.lib, self.wide = load(), wide

    def run(self, case, with_inc=False):
        F, sizes, prof, tgt, rate, inc = call_arguments(case)
        keep = [F, prof, tgt, rate, inc]
        nudge = any(t is not None for t in tgt)
        if nudge:
            self.lib.emu_ls_nudging(*sizes, table([F[n] for n in NUDGE_FIELDS]), table(tgt), table(rate), float(case["dt"]), table(inc))
        tr = [F[n] for n in case["tracers"]]
        flags = (C.c_ubyte * max(len(tr), 1))(*[1 if p else 0 for p in case["positive"]])
        self.lib.emu_ls_forcing(*sizes, ptr(F["uvel"]), ptr(F["vvel"]), ptr(F["temp"]), len(tr), table(tr) if tr else None, flags if tr else None,
                                ptr(F["density_dry"]), ptr(F[VAPOUR]), ptr(prof["zmid"]), ptr(prof["wsub"]), ptr(prof["temp_tend"]),
                                ptr(prof["qv_tend"]), table(inc) if nudge else None, ptr(prof["fcor"]), ptr(prof["ug"]), ptr(prof["vg"]),
                                float(case["dt"]), float(case["grav"]), float(case["cp_d"]), 1 if self.wide else 0)
        del keep
        out = {n: F[n] for n in STATE + tuple(case["tracers"])}
        if with_inc:
            return out, dict(zip(QUANTITIES, inc))
        return out
