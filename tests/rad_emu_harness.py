"""ctypes binding of tests/emu/rad_emu.cpp (host emulation of the CRM-to-GCM handoff kernels).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
from rad_ref import FB_FIELDS, FIELDS, GCM, QUANTITIES, RAD, SPECIES

_DP = C.POINTER(C.c_double)
_LIB = None
BLOCK_SLOTS, THREAD_SLOTS, FOUR_WALKERS = 1, 2, 3


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("rad_emu"))
        lib.emu_rad_aggregate.restype = C.c_int
        lib.emu_rad_aggregate.argtypes = [C.c_int] * 6 + [C.POINTER(_DP)] * 2 + [C.c_double, C.c_int, C.c_int]
        lib.emu_crm_feedback.restype = C.c_int
        lib.emu_crm_feedback.argtypes = [C.c_int] * 4 + [C.POINTER(_DP)] * 2 + [C.c_double] + [C.POINTER(_DP)] * 2 + [C.c_int, C.c_int]
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
    """the interface of rad_ref.RefBackend over the emulated kernels; mapping: which walkers hold the 16 slots; me: members per workgroup
    of the block-slots mapping (None: the kernel's min(nens, 64))"""

    def __init__(self, mapping, me=None):
        self.lib, self.mapping, self.me = load(), mapping, me

    def aggregate(self, f, rad_grid, rad, factor):
        nz, ny, nx, nens = f["temp"].shape
        fields = [None if f.get(n) is None else np.ascontiguousarray(f[n]) for n in FIELDS]
        out = {x: (None if a is None else a.copy()) for x, a in rad.items()}
        rc = self.lib.emu_rad_aggregate(nens, nx, ny, nz, rad_grid[1], rad_grid[0], _table(fields), _table([out[x] for x in RAD]), float(factor),
                                        self.mapping, self.me or min(nens, 64))
        assert rc == 0
        return out

    def feedback(self, f, gcm, gcm_dt):
        nz, ny, nx, nens = f["temp"].shape
        fields = [None if f.get(n) is None else np.ascontiguousarray(f[n]) for n in FB_FIELDS]
        absent = {x for x, n in SPECIES.items() if f.get(n) is None}
        g = [None if (n == "gcm_cloud_water" and "qc" in absent) or (n == "gcm_cloud_ice" and "qi" in absent) else np.ascontiguousarray(gcm[n])
             for n in GCM]
        mean = {x: (None if x in absent else np.full((nz, nens), np.nan)) for x in QUANTITIES}
        tend = {x: (None if x in absent else np.full((nz, nens), np.nan)) for x in QUANTITIES}
        rc = self.lib.emu_crm_feedback(nens, nx, ny, nz, _table(fields), _table(g), float(gcm_dt), _table([mean[x] for x in QUANTITIES]),
                                       _table([tend[x] for x in QUANTITIES]), self.mapping, self.me or min(nens, 64))
        assert rc == 0
        return mean, tend
