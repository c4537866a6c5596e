"""ctypes binding of tests/emu/hd_emu.cpp (host emulation of the hyperdiffusion kernels).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from tools.native_build import emu_library

_DP = C.POINTER(C.c_double)
_LIB = None
PATHS = ("in_place", "workspace", "narrow", "single")      # the entry point's paths; the ring also at member blocks of a quarter and of one


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(emu_library("hd_emu"))
        lib.emu_hd_line.restype = None
        lib.emu_hd_line.argtypes = [C.c_int] * 3 + [_DP, C.c_double]
        lib.emu_hd_ring.restype = None
        lib.emu_hd_ring.argtypes = [C.c_int] * 5 + [_DP, C.c_double]
        lib.emu_hd_workspace.restype = None
        lib.emu_hd_workspace.argtypes = [C.c_int] * 4 + [_DP, _DP, C.c_double]
        lib.emu_hd_fill.restype = None
        lib.emu_hd_fill.argtypes = [C.c_int] * 4 + [_DP, C.POINTER(C.c_int)]
        lib.emu_hd_coefficient.restype = C.c_double
        lib.emu_hd_coefficient.argtypes = [C.c_double] * 2
        lib.emu_hd_line_at.restype = None
        lib.emu_hd_line_at.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_double]
        lib.emu_hd_cell_at.restype = C.c_double
        lib.emu_hd_cell_at.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong] + [C.c_int] * 4 + [C.c_double]
        lib.emu_hd_fill_at.restype = C.c_int
        lib.emu_hd_fill_at.argtypes = [C.c_void_p, C.c_longlong, C.c_int]
        _LIB = lib
    return _LIB


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def ring_block(nens, nx):
    """the entry point's member block: the widest power of two whose ten rows fit 64 KB, no wider than the ensemble needs"""
    row = 10 * nx * 8
    lg = 0
    while lg < 6 and (row << (lg + 1)) <= 65536 and (1 << lg) < nens:
        lg += 1
    return 1 << lg


class EmuBackend:
    """the interface of hd_ref.RefBackend over the emulated kernels, every one of them in place"""

    def __init__(self, path="in_place", fill_me=None):
        assert path in PATHS
        self.lib, self.path, self.fill_me = load(), path, fill_me
        self.written = []

    def run(self, fields, positive, dt, tau):
        c = self.lib.emu_hd_coefficient(float(dt), float(tau))
        out, self.written = [], []
        for f, pos in zip(fields, positive):
            g = np.ascontiguousarray(f).copy()
            nz, ny, nx, nens = g.shape
            if self.path == "workspace":
                ws = np.full(g.shape, np.nan)
                self.lib.emu_hd_workspace(nens, nx, ny, nz, _p(g), _p(ws), c)
            elif ny == 1:
                self.lib.emu_hd_line(nens, nx, nz, _p(g), c)
            else:
                me = ring_block(nens, nx)
                me = {"in_place": me, "narrow": max(me // 4, 1), "single": 1}[self.path]
                self.lib.emu_hd_ring(nens, nx, ny, nz, me, _p(g), c)
            if pos:
                w = np.zeros((nz, nens), dtype=np.int32)
                self.lib.emu_hd_fill(nens, ny * nx, nz, self.fill_me or min(nens, 64), _p(g), w.ctypes.data_as(C.POINTER(C.c_int)))
                self.written.append(w)
            else:
                self.written.append(None)
            out.append(g)
        return out
