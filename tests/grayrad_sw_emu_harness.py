"""ctypes binding of tests/emu/grayrad_sw_emu.cpp (host emulation of the grey shortwave kernel).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
from grayrad_sw_ref import SCALARS

_DP = C.POINTER(C.c_double)
_TAB = C.POINTER(C.c_void_p)
_LIB = None
POISON = -7.0e77


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("grayrad_sw_emu"))
        lib.emu_radiation_gray_sw.restype = None
        lib.emu_radiation_gray_sw.argtypes = ([C.c_int] * 4 + [_DP] * 3 + [C.c_int, _TAB] * 2 + [_DP, _DP, C.c_void_p] + [C.c_double] * 10 + [_DP] * 4
                                              + [C.c_int])
        _LIB = lib
    return _LIB


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


class EmuBackend:
    """the interface of grayrad_sw_ref.RefBackend over the emulated kernel; outputs poisoned before the call"""

    def __init__(self, wide=False):
        self.lib, self.wide = load(), wide

    def run(self, case):
        F = {n: np.ascontiguousarray(a) for n, a in case["fields"].items()}
        temp = F["temp"].copy()
        nz, ny, nx, nens = temp.shape
        liquid = (C.c_void_p * 2)(*[F[n].ctypes.data for n in case["liquid"]])
        ice = (C.c_void_p * 2)(*[F[n].ctypes.data for n in case["ice"]])
        sfc = None if case.get("sfc_albedo") is None else np.ascontiguousarray(case["sfc_albedo"])
        coszen = np.ascontiguousarray(case["coszen"], dtype=np.float64)
        assert coszen.shape == (nens,)
        heating = np.full(temp.shape, POISON)
        down, up, top = (np.full(temp.shape[1:], POISON) for _ in range(3))
        self.lib.emu_radiation_gray_sw(nens, nx, ny, nz, _p(temp), _p(F["density_dry"]), _p(F["water_vapor"]), len(case["liquid"]), liquid,
                                       len(case["ice"]), ice, _p(np.ascontiguousarray(case["zint"])), _p(coszen),
                                       None if sfc is None else C.c_void_p(sfc.ctypes.data), *[float(case[n]) for n in SCALARS], _p(heating),
                                       _p(down), _p(up), _p(top), int(self.wide))
        return dict(temp=temp, rad_sw_heating=heating, rad_sw_down_sfc=down, rad_sw_up_sfc=up, rad_sw_up_top=top)
