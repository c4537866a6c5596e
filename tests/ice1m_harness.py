"""ctypes binding of tests/emu/ice1m_emu.cpp (host emulation of the ice1m kernel), and the same interface over the C ABI on a device.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library
from ice1m_ref import SPECIES, WRITTEN

_LIB = None
POISON = -7.0e77


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("ice1m_emu"))
        lib.emu_ice1m_time_step.restype = None
        lib.emu_ice1m_time_step.argtypes = [C.c_int] * 4 + [C.c_void_p] * 10 + [C.c_double] * 3 + [C.c_int]
        lib.emu_ice1m_sub_cycles.restype = None
        lib.emu_ice1m_sub_cycles.argtypes = [C.c_int] * 4 + [C.c_void_p] * 6 + [C.c_double, C.c_void_p]
        _LIB = lib
    return _LIB


def members(case, lo, hi):
    """the case restricted to members lo .. hi - 1"""
    return dict(case, fields={n: np.ascontiguousarray(a[..., lo:hi]) for n, a in case["fields"].items()},
                zint=np.ascontiguousarray(case["zint"][:, lo:hi]))


def run_split(backend, case, bounds):
    """the members in the blocks bounds[i] .. bounds[i + 1], one call each, joined"""
    parts = [backend.run(members(case, lo, hi)) for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo]
    return {n: np.concatenate([p[n] for p in parts], axis=-1) for n in parts[0]}


class EmuBackend:
    """the interface of ice1m_ref.RefBackend over the emulated kernel"""

    def __init__(self, wide=False):
        self.lib, self.wide = load(), wide

    def run(self, case):
        F = {n: np.array(case["fields"][n], dtype=np.float64, order="C") for n in WRITTEN + ("density_dry",)}
        nz, ny, nx, nens = F["temp"].shape
        zint = np.ascontiguousarray(case["zint"], dtype=np.float64)
        precl, preci = np.full((ny, nx, nens), POISON), np.full((ny, nx, nens), POISON)
        self.lib.emu_ice1m_time_step(nens, nx, ny, nz, *[F[n].ctypes.data for n in SPECIES], F["density_dry"].ctypes.data,
                                     F["temp"].ctypes.data, precl.ctypes.data, preci.ctypes.data, zint.ctypes.data, float(case["dt"]),
                                     float(case["R_v"]), float(case["cp_d"]), 1 if self.wide else 0)
        out = {n: F[n] for n in WRITTEN}
        out.update(precl=precl, preci=preci)
        return out

    def sub_cycles(self, case):
        F = {n: np.ascontiguousarray(case["fields"][n], dtype=np.float64) for n in SPECIES + ("density_dry",)}
        nz, ny, nx, nens = F["density_dry"].shape
        zint = np.ascontiguousarray(case["zint"], dtype=np.float64)
        n = np.zeros((ny, nx, nens), dtype=np.int32)
        self.lib.emu_ice1m_sub_cycles(nens, nx, ny, nz, F["water_vapor"].ctypes.data, F["cloud_ice"].ctypes.data,
                                      F["precip_liquid"].ctypes.data, F["precip_ice"].ctypes.data, F["density_dry"].ctypes.data,
                                      zint.ctypes.data, float(case["dt"]), n.ctypes.data)
        return n


class GpuBackend:
    """the same over pam_amd_ice1m_time_step on the current device; wide: the long long instance through the debug switch"""

    def __init__(self, wide=False):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check, self.wide = torch, capi.load(), capi.check, wide

    def run(self, case):
        torch = self.torch
        F = {n: torch.tensor(np.ascontiguousarray(case["fields"][n]), dtype=torch.float64, device="cuda") for n in WRITTEN + ("density_dry",)}
        nz, ny, nx, nens = F["temp"].shape
        zint = torch.tensor(np.ascontiguousarray(case["zint"]), dtype=torch.float64, device="cuda")
        precl = torch.full((ny, nx, nens), POISON, dtype=torch.float64, device="cuda")
        preci = torch.full((ny, nx, nens), POISON, dtype=torch.float64, device="cuda")
        self.check(self.lib.pam_amd_ice1m_debug_wide_index(1 if self.wide else 0))
        try:
            self.check(self.lib.pam_amd_ice1m_time_step(nens, nx, ny, nz, *[F[n].data_ptr() for n in SPECIES], F["density_dry"].data_ptr(),
                                                        F["temp"].data_ptr(), precl.data_ptr(), preci.data_ptr(), zint.data_ptr(),
                                                        float(case["dt"]), float(case["R_v"]), float(case["cp_d"]),
                                                        torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
        finally:
            self.check(self.lib.pam_amd_ice1m_debug_wide_index(0))
        out = {n: F[n].cpu().numpy() for n in WRITTEN}
        out.update(precl=precl.cpu().numpy(), preci=preci.cpu().numpy())
        self.last_inputs = dict(density_dry=F["density_dry"].cpu().numpy(), zint=zint.cpu().numpy())
        return out
