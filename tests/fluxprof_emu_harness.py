"""ctypes binding of tests/emu/fluxprof_emu.cpp (host emulation of the CRM flux profiles kernel).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
from fluxprof_ref import FIELDS, OUT

_DP = C.POINTER(C.c_double)
_LIB = None
KERNEL, REVERSED, ONE_WALKER = 0, 1, 2                      # who holds the 16 slots of a member, and in which order they run


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("fluxprof_emu"))
        lib.emu_flux_profiles.restype = C.c_int
        lib.emu_flux_profiles.argtypes = [C.c_int] * 4 + [C.POINTER(_DP), C.c_double, C.POINTER(_DP), C.c_double] + [C.c_int] * 2
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
    """the interface of fluxprof_ref.RefBackend over the emulated kernel; mapping: which walkers hold the 16 slots; me: members per
    workgroup (None: the kernel's min(nens, 64))"""

    def __init__(self, mapping=KERNEL, me=None):
        self.lib, self.mapping, self.me = load(), mapping, me

    def profiles(self, f, qc, out, factor):
        nz, ny, nx, nens = f["rho_d"].shape
        fields = [None if f.get(n) is None else np.ascontiguousarray(f[n]) for n in FIELDS]
        new = {x: (None if a is None else a.copy()) for x, a in out.items()}
        rc = self.lib.emu_flux_profiles(nens, nx, ny, nz, _table(fields), float(qc), _table([new[x] for x in OUT]), float(factor),
                                        self.mapping, self.me or min(nens, 64))
        assert rc == 0
        return new
