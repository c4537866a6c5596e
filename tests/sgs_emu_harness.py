"""ctypes binding of tests/emu/sgs_emu.cpp (host emulation of the Smagorinsky SGS kernels).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
import sgs_ref as ref

_DP = C.POINTER(C.c_double)
_LIB = None
PATHS = ("lds", "workspace", "lds_narrow")      # c' in LDS rows of 64 lanes, in the workspace, and in LDS rows of 5 lanes


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("sgs_emu"))
        lib.emu_sgs_coefficients.restype = None
        lib.emu_sgs_coefficients.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_void_p), _DP, _DP] + [C.c_double] * 6 + [_DP, _DP]
        lib.emu_sgs_diffuse.restype = None
        lib.emu_sgs_diffuse.argtypes = [C.c_int] * 4 + [_DP] * 4 + [C.c_int, C.POINTER(C.c_void_p)] + [C.c_void_p] * 8 + [C.c_double] * 3 + [C.c_int] * 2
        lib.emu_sgs_solve_at.restype = None
        lib.emu_sgs_solve_at.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_longlong] + [C.c_void_p] * 5 + \
            [C.c_longlong, C.c_longlong, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_longlong]
        lib.emu_sgs_coef_at.restype = None
        lib.emu_sgs_coef_at.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_longlong] + [C.c_int] * 7 + [C.c_double] * 6 + [C.c_void_p] * 2
        _LIB = lib
    return _LIB


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def _v(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class EmuBackend:
    """the interface of sgs_ref.RefBackend over the emulated kernels; the solve in place, the vapour aliased into the table as a caller
    of the C ABI has it"""

    def __init__(self, path="lds"):
        assert path in PATHS
        self.lib, self.path = load(), path

    def coefficients(self, case):
        F = {n: np.ascontiguousarray(case["fields"][n]) for n in ref.WINDS + ("temp", "density_dry", "water_vapor")}
        nz, ny, nx, nens = F["temp"].shape
        table = (C.c_void_p * 6)(*[F[n].ctypes.data for n in ref.WINDS + ("temp", "density_dry", "water_vapor")])
        tk, tkh = np.full(F["temp"].shape, np.nan), np.full(F["temp"].shape, np.nan)
        self.lib.emu_sgs_coefficients(nens, nx, ny, nz, table, _p(np.ascontiguousarray(case["zint"])), _p(np.ascontiguousarray(case["zmid"])),
                                      case["dx"], case["dy"], case["grav"], case["cp_d"], case["cs"], case["prandtl"], _p(tk), _p(tkh))
        return tk, tkh

    def diffuse(self, case, tk, tkh):
        F = {n: np.ascontiguousarray(a).copy() for n, a in case["fields"].items()}
        nz, ny, nx, nens = F["temp"].shape
        tr = case["tracers"]
        table = (C.c_void_p * max(len(tr), 1))(*[F[n].ctypes.data for n in tr])
        sfc = [None if case.get(n) is None else np.ascontiguousarray(case[n]) for n in ("sfc_flx_u", "sfc_flx_v")]
        # a vapour outside the table is only read; inside it, the same array is read as rho_v and solved
        self.lib.emu_sgs_diffuse(nens, nx, ny, nz, _p(F["uvel"]), _p(F["vvel"]), _p(F["wvel"]), _p(F["temp"]), len(tr), table,
                                 _v(F["density_dry"]), _v(F["water_vapor"]), _v(np.ascontiguousarray(tk)), _v(np.ascontiguousarray(tkh)),
                                 _v(np.ascontiguousarray(case["zint"])), _v(np.ascontiguousarray(case["zmid"])), _v(sfc[0]), _v(sfc[1]),
                                 case["dt"], case["grav"], case["cp_d"], 2 if self.path == "workspace" else 1, 5 if self.path == "lds_narrow" else 64)
        return {n: F[n] for n in ref.WINDS + ("temp",) + tuple(tr)}
