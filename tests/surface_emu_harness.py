"""ctypes binding of tests/emu/surface_emu.cpp (host emulation of the surface-flux kernel).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

from surface_ref import FIELDS, RADIATION, SCALARS

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu", "surface_emu.cpp")
_SO = os.path.join(_HERE, "emu", "libsurface_emu.so")
_DP = C.POINTER(C.c_double)
_LIB = None
POISON = -7.0e77


def load():
    global _LIB
    if _LIB is None:
        csrc = os.path.join(_HERE, "..", "pam_amd", "csrc")
        deps = [_SRC] + [os.path.join(csrc, h) for h in ("surface_device.h", "sgs_device.h", "msa_device.h")]
        if not (os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(d) for d in deps)):
            tmp = "%s.%d.tmp" % (_SO, os.getpid())      # built beside it and moved into place: another process never loads half a file
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, _SRC], check=True)
            os.replace(tmp, _SO)
        lib = C.CDLL(_SO)
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
