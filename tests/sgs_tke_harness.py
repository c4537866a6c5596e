"""ctypes binding of tests/emu/sgs_tke_emu.cpp (host emulation of the two coefficient kernels of the prognostic-TKE closure).  TEST
INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
import sgs_tke_ref as tref

_DP = C.POINTER(C.c_double)
_TAB = C.POINTER(C.c_void_p)
_LIB = None
SIX = tref.WINDS + ("temp", "density_dry", "water_vapor")


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("sgs_tke_emu"))
        lib.emu_sgs_tke_constants.restype = None
        lib.emu_sgs_tke_constants.argtypes = [C.c_double, C.c_double, _DP]
        lib.emu_sgs_tke_coefficients.restype = None
        lib.emu_sgs_tke_coefficients.argtypes = [C.c_int] * 5 + [_TAB, _DP, C.c_int, _TAB, C.c_int, _TAB, _DP, _DP] + [C.c_double] * 12 + [_DP, _DP]
        lib.emu_sgs_tke_step.restype = None
        lib.emu_sgs_tke_step.argtypes = [C.c_double] * 10 + [_DP]
        _LIB = lib
    return _LIB


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def constants(cs, ck):
    out = np.zeros(3)
    load().emu_sgs_tke_constants(cs, ck, _p(out))
    return tuple(out.tolist())


def step(tke, rho, D, N2, delta, dt, ck, ce1, ce2, seed):
    out = np.zeros(3)
    load().emu_sgs_tke_step(tke, rho, D, N2, delta, dt, ck, ce1, ce2, seed, _p(out))
    return tuple(out.tolist())


class EmuBackend:
    """the interface of sgs_tke_ref.RefBackend over the emulated kernels: the dry kernel where the case is not moist"""

    def __init__(self):
        self.lib = load()

    def coefficients(self, case):
        names = SIX + case["cloud"] + case["precip"]
        F = {n: np.ascontiguousarray(case["fields"][n]) for n in names}
        nz, ny, nx, nens = F["temp"].shape
        table = (C.c_void_p * 6)(*[F[n].ctypes.data for n in SIX])
        cloud = (C.c_void_p * 4)(*[F[n].ctypes.data for n in case["cloud"]])
        precip = (C.c_void_p * 8)(*[F[n].ctypes.data for n in case["precip"]])
        tke = np.ascontiguousarray(case["fields"]["tke"]).copy()
        tk, tkh = np.full(F["temp"].shape, np.nan), np.full(F["temp"].shape, np.nan)
        self.lib.emu_sgs_tke_coefficients(int(case["moist"]), nens, nx, ny, nz, table, _p(tke), len(case["cloud"]), cloud, len(case["precip"]),
                                          precip, _p(np.ascontiguousarray(case["zint"])), _p(np.ascontiguousarray(case["zmid"])), case["dx"],
                                          case["dy"], case["dt"], case["grav"], case["cp_d"], case["R_d"], case["R_v"], case["cloud_threshold"],
                                          case["ck"], case["ce1"], case["ce2"], case["seed"], _p(tk), _p(tkh))
        return tke, tk, tkh
