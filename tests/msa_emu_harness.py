"""ctypes binding of tests/emu/msa_emu.cpp (host emulation of the mean-state acceleration kernels).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
from msa_ref import FIELDS, QUANTITIES

_DP = C.POINTER(C.c_double)
_LIB = None


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("msa_emu"))
        lib.emu_msa_mean.restype = None
        lib.emu_msa_mean.argtypes = [C.c_int] * 4 + [C.POINTER(_DP)] * 3 + [C.c_double, C.POINTER(C.c_int), C.c_int]
        lib.emu_msa_apply.restype = None
        lib.emu_msa_apply.argtypes = [C.c_int] * 4 + [_DP] * 4 + [C.POINTER(_DP), C.c_double, C.c_int, C.POINTER(C.c_int)]
        _LIB = lib
    return _LIB


def _p(a):
    if a is None:
        return _DP()
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def _table(arrays):
    return (_DP * len(arrays))(*[_p(a) for a in arrays])


class EmuBackend:
    """the interface of msa_ref.RefBackend over the emulated kernels; me: members per workgroup (None: the kernel's min(nens, 64))"""

    def __init__(self, me=None):
        self.lib, self.me = load(), me

    def _mean(self, st, save):
        nz, ncol, nens = st["temp"].shape
        me = self.me or min(nens, 64)
        fields = [None if st.get(f) is None else np.ascontiguousarray(st[f]) for f in FIELDS]
        out = {q: np.full((nz, nens), np.nan) for q in QUANTITIES}
        return nens, ncol, nz, me, fields, out

    def diagnose(self, st):
        nens, ncol, nz, me, fields, out = self._mean(st, None)
        self.lib.emu_msa_mean(nens, ncol, nz, me, _table(fields), None, _table([out[q] for q in QUANTITIES]), 0.0, None, 1)
        return out

    def tendencies(self, st, save, max_ttend, cease):
        nens, ncol, nz, me, fields, out = self._mean(st, save)
        flag = C.c_int(int(cease))
        self.lib.emu_msa_mean(nens, ncol, nz, me, _table(fields), _table([save[q] for q in QUANTITIES]),
                              _table([out[q] for q in QUANTITIES]), float(max_ttend), C.byref(flag), 0)
        return out, flag.value

    def apply(self, st, tend, a, accel_uv, cease):
        nz, ncol, nens = st["temp"].shape
        me = self.me or min(nens, 64)
        out = {k: (None if v is None else v.copy()) for k, v in st.items()}
        if a == 0:          # the entry point makes no launch
            return out
        flag = C.c_int(int(cease))
        self.lib.emu_msa_apply(nens, ncol, nz, me, _p(out["temp"]), _p(out["water_vapor"]), _p(out["uvel"]), _p(out["vvel"]),
                               _table([tend[q] for q in QUANTITIES]), float(a), int(bool(accel_uv)), C.byref(flag))
        return out
