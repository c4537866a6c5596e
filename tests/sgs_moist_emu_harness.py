"""ctypes binding of tests/emu/sgs_moist_emu.cpp (host emulation of the moist coefficient kernel and of the solve with surface fluxes of
heat and vapour).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
import sgs_moist_ref as mref

_DP = C.POINTER(C.c_double)
_TAB = C.POINTER(C.c_void_p)
_LIB = None
PATHS = ("lds", "workspace", "lds_narrow")      # c' in LDS rows of 64 lanes, in the workspace, and in LDS rows of 5 lanes
SIX = mref.WINDS + ("temp", "density_dry", "water_vapor")


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("sgs_moist_emu"))
        lib.emu_sgs_exp_c.restype = None
        lib.emu_sgs_exp_c.argtypes = [_DP, _DP, C.c_longlong]
        lib.emu_sgs_coefficients_moist.restype = None
        lib.emu_sgs_coefficients_moist.argtypes = [C.c_int] * 4 + [_TAB, C.c_int, _TAB, C.c_int, _TAB, _DP, _DP] + [C.c_double] * 9 + [_DP, _DP]
        lib.emu_sgs_diffuse_fluxes.restype = None
        lib.emu_sgs_diffuse_fluxes.argtypes = [C.c_int] * 4 + [_DP] * 4 + [C.c_int, _TAB] + [C.c_void_p] * 8 + [C.c_double] * 3 + \
            [C.c_void_p, _TAB, C.c_double, C.c_int, C.c_int]
        lib.emu_sgs_flux_solve_at.restype = None
        lib.emu_sgs_flux_solve_at.argtypes = [C.c_int, _TAB, C.c_int, _TAB, C.c_longlong] + [C.c_void_p] * 5 + \
            [C.c_longlong, C.c_longlong, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_longlong, C.c_double]
        lib.emu_sgs_moist_coef_at.restype = None
        lib.emu_sgs_moist_coef_at.argtypes = [_TAB, C.c_int, _TAB, C.c_int, _TAB, C.c_void_p, C.c_void_p, C.c_longlong] + [C.c_int] * 7 + \
            [C.c_double] * 9 + [C.c_void_p] * 2
        _LIB = lib
    return _LIB


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def _v(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def exp_c(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    load().emu_sgs_exp_c(_p(x), _p(y), x.size)
    return y


class EmuBackend:
    """the interface of sgs_moist_ref.RefBackend over the emulated kernels; the solve in place, the vapour aliased into the table and the
    latent flux at the vapour's index as the entry point has them"""

    def __init__(self, path="lds"):
        assert path in PATHS
        self.lib, self.path = load(), path

    def coefficients(self, case):
        names = SIX + case["cloud"] + case["precip"]
        F = {n: np.ascontiguousarray(case["fields"][n]) for n in names}
        nz, ny, nx, nens = F["temp"].shape
        table = (C.c_void_p * 6)(*[F[n].ctypes.data for n in SIX])
        cloud = (C.c_void_p * 4)(*[F[n].ctypes.data for n in case["cloud"]])
        precip = (C.c_void_p * 8)(*[F[n].ctypes.data for n in case["precip"]])
        tk, tkh = np.full(F["temp"].shape, np.nan), np.full(F["temp"].shape, np.nan)
        self.lib.emu_sgs_coefficients_moist(nens, nx, ny, nz, table, len(case["cloud"]), cloud, len(case["precip"]), precip,
                                            _p(np.ascontiguousarray(case["zint"])), _p(np.ascontiguousarray(case["zmid"])), case["dx"], case["dy"],
                                            case["grav"], case["cp_d"], case["R_d"], case["R_v"], case["cloud_threshold"], case["cs"],
                                            case["prandtl"], _p(tk), _p(tkh))
        return tk, tkh

    def diffuse(self, case, tk, tkh):
        F = {n: np.ascontiguousarray(a).copy() for n, a in case["fields"].items()}
        nz, ny, nx, nens = F["temp"].shape
        tr = case["tracers"]
        table = (C.c_void_p * max(len(tr), 1))(*[F[n].ctypes.data for n in tr])
        sfc = [None if case.get(n) is None else np.ascontiguousarray(case[n]) for n in ("sfc_flx_u", "sfc_flx_v", "sfc_shf", "sfc_lhf")]
        trsfc = (C.c_void_p * max(len(tr), 1))(*[sfc[3].ctypes.data if (sfc[3] is not None and n == "water_vapor") else None for n in tr])
        self.lib.emu_sgs_diffuse_fluxes(nens, nx, ny, nz, _p(F["uvel"]), _p(F["vvel"]), _p(F["wvel"]), _p(F["temp"]), len(tr), table,
                                        _v(F["density_dry"]), _v(F["water_vapor"]), _v(np.ascontiguousarray(tk)), _v(np.ascontiguousarray(tkh)),
                                        _v(np.ascontiguousarray(case["zint"])), _v(np.ascontiguousarray(case["zmid"])), _v(sfc[0]), _v(sfc[1]),
                                        case["dt"], case["grav"], case["cp_d"], _v(sfc[2]), trsfc, case["latvap"],
                                        2 if self.path == "workspace" else 1, 5 if self.path == "lds_narrow" else 64)
        return {n: F[n] for n in mref.WINDS + ("temp",) + tuple(tr)}
