"""ctypes binding of tests/emu/vt_emu.cpp (host emulation of the variance transport kernels).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
from vt_ref import FIELDS, QUANTITIES, quantities

_DP = C.POINTER(C.c_double)
_LIB = None


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("vt_emu"))
        lib.emu_vt_stats.restype = None
        lib.emu_vt_stats.argtypes = [C.c_int] * 4 + [C.POINTER(_DP), C.c_int, C.c_int, C.POINTER(_DP), C.c_double, C.c_double] + [C.POINTER(_DP)] * 3
        lib.emu_vt_apply.restype = None
        lib.emu_vt_apply.argtypes = [C.c_int] * 4 + [C.POINTER(_DP), C.c_int] + [C.POINTER(_DP)] * 2
        _LIB = lib
    return _LIB


def _p(a):
    if a is None:
        return _DP()
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def _table(d, use_u):
    """a table of three (nz,nens) arrays from a dict by quantity; entry [2] is NULL without use_u"""
    if d is None:
        return None
    return (_DP * 3)(*[_p(np.ascontiguousarray(d[q])) if q in quantities(use_u) else _DP() for q in QUANTITIES])


class EmuBackend:
    """the interface of vt_ref.RefBackend over the emulated kernels; me: members per workgroup (None: the kernel's min(nens, 64))"""

    def __init__(self, me=None):
        self.lib, self.me = load(), me

    def _stats(self, st, use_u, epi, inp, p, lim):
        nz, ncol, nens = st["temp"].shape
        me = self.me or min(nens, 64)
        fields = [None if st.get(f) is None or (f == "uvel" and not use_u) else np.ascontiguousarray(st[f]) for f in FIELDS]
        inp = None if inp is None else {q: np.ascontiguousarray(inp[q]) for q in quantities(use_u)}
        mean, var, out = ({q: np.full((nz, nens), np.nan) for q in quantities(use_u)} for _ in range(3))
        self.lib.emu_vt_stats(nens, ncol, nz, me, (_DP * 5)(*[_p(f) for f in fields]), int(bool(use_u)), epi, _table(inp, use_u), float(p),
                              float(lim), _table(mean, use_u), _table(var, use_u), _table(out, use_u))
        return mean, var, out

    def diagnose(self, st, use_u):
        return self._stats(st, use_u, 0, None, 0.0, 0.0)[:2]

    def forcing(self, st, use_u, tend, dt, lim):
        return self._stats(st, use_u, 1, tend, dt, lim)

    def feedback(self, st, use_u, var_start, gcm_dt):
        return self._stats(st, use_u, 2, var_start, gcm_dt, 0.0)

    def apply(self, st, use_u, mean, scale):
        nz, ncol, nens = st["temp"].shape
        me = self.me or min(nens, 64)
        out = {k: (None if v is None else np.ascontiguousarray(v).copy()) for k, v in st.items()}
        fields = [out.get(f) if (f != "uvel" or use_u) else None for f in FIELDS]
        mean = {q: np.ascontiguousarray(mean[q]) for q in quantities(use_u)}
        scale = {q: np.ascontiguousarray(scale[q]) for q in quantities(use_u)}
        self.lib.emu_vt_apply(nens, ncol, nz, me, (_DP * 5)(*[_p(f) for f in fields]), int(bool(use_u)), _table(mean, use_u), _table(scale, use_u))
        return out
