"""ctypes binding of tests/emu/surface_emu.cpp (host emulation of the surface-flux kernel).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
from surface_ref import FIELDS, RADIATION, SCALARS

_DP = C.POINTER(C.c_double)
_LIB = None
POISON = -7.0e77


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("surface_emu"))
        lib.emu_surface_fluxes.restype = None
        lib.emu_surface_fluxes.argtypes = [C.c_int] * 4 + [_DP] * 9 + [C.c_void_p] * 4 + [C.c_double] * 8 + [_DP] * 2
        _LIB = lib
    return _LIB


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


class EmuBackend:
    """the interface of surface_ref.RefBackend over the emulated kernel; the flux outputs poisoned before the call"""

    def __init__(self):
        self.lib = load()

    def run(self, case):
        F = [np.ascontiguousarray(case["fields"][n], dtype=np.float64) for n in FIELDS]
        nz, ny, nx, nens = F[0].shape
        zmid, cn, cstar = (np.ascontiguousarray(case[n], dtype=np.float64) for n in ("zmid", "cn", "cstar"))
        assert zmid.shape == (nz, nens) and cn.shape == (nens,) and cstar.shape == (nens,)
        sfc_temp = np.array(case["sfc_temp"], dtype=np.float64, order="C")
        rad = [None if case.get(n) is None else np.ascontiguousarray(case[n], dtype=np.float64) for n in RADIATION]
        shf, lhf = np.full((ny, nx, nens), POISON), np.full((ny, nx, nens), POISON)
        self.lib.emu_surface_fluxes(nens, nx, ny, nz, *[_p(a) for a in F], _p(zmid), _p(cn), _p(cstar), _p(sfc_temp),
                                    *[None if a is None else C.c_void_p(a.ctypes.data) for a in rad], *[float(case[n]) for n in SCALARS],
                                    _p(shf), _p(lhf))
        return dict(sfc_shf=shf, sfc_lhf=lhf, sfc_temp=sfc_temp)
