"""ctypes binding of tests/emu/grayrad_emu.cpp (host emulation of the grey radiation kernel).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library

_DP = C.POINTER(C.c_double)
_TAB = C.POINTER(C.c_void_p)
_LIB = None
SCALARS = ("k_d", "k_v", "k_l", "k_i", "sigma", "cp_d", "lw_down_top", "dt")


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("grayrad_emu"))
        lib.emu_radiation_gray.restype = None
        lib.emu_radiation_gray.argtypes = [C.c_int] * 4 + [_DP] * 3 + [C.c_int, _TAB] * 2 + [_DP, C.c_void_p] + [C.c_double] * 8 + [_DP] * 4 + [C.c_int]
        _LIB = lib
    return _LIB


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


class EmuBackend:
    """the interface of grayrad_ref.RefBackend over the emulated kernel; outputs poisoned before the call"""

    def __init__(self, wide=False):
        self.lib, self.wide = load(), wide

    def run(self, case):
        F = {n: np.ascontiguousarray(a) for n, a in case["fields"].items()}
        temp = F["temp"].copy()
        nz, ny, nx, nens = temp.shape
        liquid = (C.c_void_p * 2)(*[F[n].ctypes.data for n in case["liquid"]])
        ice = (C.c_void_p * 2)(*[F[n].ctypes.data for n in case["ice"]])
        sfc = None if case.get("sfc_temp") is None else np.ascontiguousarray(case["sfc_temp"])
        heating = np.full(temp.shape, -7.0e77)
        olr, down, up = (np.full(temp.shape[1:], -7.0e77) for _ in range(3))
        self.lib.emu_radiation_gray(nens, nx, ny, nz, _p(temp), _p(F["density_dry"]), _p(F["water_vapor"]), len(case["liquid"]), liquid,
                                    len(case["ice"]), ice, _p(np.ascontiguousarray(case["zint"])), None if sfc is None else C.c_void_p(sfc.ctypes.data),
                                    *[float(case[n]) for n in SCALARS], _p(heating), _p(olr), _p(down), _p(up), int(self.wide))
        return dict(temp=temp, rad_heating=heating, rad_olr=olr, rad_lw_down_sfc=down, rad_lw_up_sfc=up)
