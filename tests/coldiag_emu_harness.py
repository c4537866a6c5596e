"""ctypes binding of tests/emu/coldiag_emu.cpp (host emulation of the CRM column diagnostics kernels).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
from coldiag_ref import FIELDS, OUT, PRECIP

_DP = C.POINTER(C.c_double)
_LIB = None
ASCENDING, REVERSED, ROLLED = 0, 1, 2                        # the order of the scan's threads; its levels one by one
BLOCK_SLOTS, THREAD_SLOTS, FOUR_WALKERS = 1, 2, 3            # who holds the 16 slots of the mean


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("coldiag_emu"))
        lib.emu_column_diagnostics.restype = C.c_int
        lib.emu_column_diagnostics.argtypes = [C.c_int] * 4 + [C.POINTER(_DP), _DP, C.POINTER(_DP)] + [C.c_double] * 5 + [C.POINTER(_DP), C.c_double] + \
            [C.c_int] * 3
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
    """the interface of coldiag_ref.RefBackend over the emulated kernels; scan_order: the order of the scan's threads; mapping: which walkers
    hold the 16 slots of the mean; me: members per workgroup of the block-slots mapping (None: the kernel's min(nens, 64))"""

    def __init__(self, scan_order=ASCENDING, mapping=BLOCK_SLOTS, me=None):
        self.lib, self.scan_order, self.mapping, self.me = load(), scan_order, mapping, me

    def diagnose(self, f, zint, precip, params, out, factor):
        nz, ny, nx, nens = f["rho_v"].shape
        fields = [None if f.get(n) is None else np.ascontiguousarray(f[n]) for n in FIELDS]
        pr = None if precip is None else [None if precip.get(n) is None else np.ascontiguousarray(precip[n]) for n in PRECIP]
        new = {x: (None if a is None else a.copy()) for x, a in out.items()}
        rc = self.lib.emu_column_diagnostics(nens, nx, ny, nz, _table(fields), _p(np.ascontiguousarray(zint)), None if pr is None else _table(pr),
                                             params["R_d"], params["R_v"], params["p_low"], params["p_high"], params["cwp_threshold"],
                                             _table([new[x] for x in OUT]), float(factor), self.scan_order, self.mapping,
                                             self.me or min(nens, 64))
        assert rc == 0
        return new
