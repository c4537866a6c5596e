"""pam::VerticalInterp<ord> (pam_core/vertical_interp.h): a cell-centred (nz,ny,nx,nens) field on its nz+1 vertical interfaces, by a
WENO reconstruction on every member's own vertical grid.  Arithmetic is in libpam_amd_awfl.so (pam_amd/csrc/modules_kernels.hip,
vertical_interp_device.h); orders 3 and 5 (the reference's sample_val for orders 7 and 9 is not an interpolation)."""
import ctypes as C

import torch

from . import capi
from .capi import PamAmdError, check
from .dycore import _device_view


class VerticalInterp:
    BC_ZERO_GRADIENT = 0
    BC_ZERO_VALUE = 1

    def __init__(self, ord):
        if ord not in (3, 5):
            raise PamAmdError("VerticalInterp: ord must be 3 or 5")
        self.ord = ord
        self.hs = (ord - 1) // 2
        self._h = None

    def init(self, zint):
        """zint: float64 (nz+1, nens) tensor on the GPU.  Builds the reconstruction matrices (synchronises the current stream); one
        shared table is kept where every member has the same interfaces."""
        self.finalize()
        if zint.dim() != 2 or zint.dtype != torch.float64 or not zint.is_cuda:
            raise PamAmdError("VerticalInterp.init: zint must be a float64 (nz+1, nens) tensor on the GPU")
        zint = zint.contiguous()
        h = C.c_void_p()
        with torch.cuda.device(zint.device):
            check(capi.load().pam_amd_vertical_interp_init(self.ord, zint.shape[0] - 1, zint.shape[1], zint.data_ptr(),
                                                           torch.cuda.current_stream(zint.device).cuda_stream, C.byref(h)))
        self._h, self.nz, self.nens, self.device = h, zint.shape[0] - 1, zint.shape[1], zint.device

    def _handle(self):
        if self._h is None:
            raise PamAmdError("VerticalInterp: init() has not been called")
        return self._h

    @property
    def shared_table(self):
        return self.tables()[2]

    def set_table_sharing(self, shared):
        """False: per-member tables even where the members' interfaces are identical (same bits; for tests and timing)"""
        with torch.cuda.device(self.device):
            check(capi.load().pam_amd_vertical_interp_set_table_sharing(self._handle(), int(bool(shared)),
                                                                        torch.cuda.current_stream(self.device).cuda_stream))

    def tables(self):
        """copies of recon_lo (nz,hs+1,hs+1,hs+1,T), recon_hi (nz,ord,ord,T) and whether T = 1 (one shared table) or nens"""
        lo, hi, sh = C.c_void_p(), C.c_void_p(), C.c_int()
        check(capi.load().pam_amd_vertical_interp_tables(self._handle(), C.byref(lo), C.byref(hi), C.byref(sh)))
        T, n = (1 if sh.value else self.nens), self.hs + 1
        out = [_device_view(ptr.value, shape, self.device).clone()
               for ptr, shape in ((lo, (self.nz, n, n, n, T)), (hi, (self.nz, self.ord, self.ord, T)))]
        return out[0], out[1], bool(sh.value)

    def cells_to_edges(self, data, bc_lower, bc_upper, out=None):
        """data: float64 (nz,ny,nx,nens) on init's device -> (nz+1,ny,nx,nens), on the current stream, unsynchronised"""
        h = self._handle()
        if data.dim() != 4 or data.dtype != torch.float64 or data.device != self.device:
            raise PamAmdError("VerticalInterp.cells_to_edges: data must be a float64 (nz,ny,nx,nens) tensor on init's device")
        if data.shape[0] != self.nz or data.shape[3] != self.nens:
            raise PamAmdError("VerticalInterp.cells_to_edges: data does not have init's nz and nens")
        data = data.contiguous()
        shape = (self.nz + 1,) + tuple(data.shape[1:])
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float64 or out.device != self.device or not out.is_contiguous():
            raise PamAmdError("VerticalInterp.cells_to_edges: out must be a contiguous float64 (nz+1,ny,nx,nens) tensor")
        with torch.cuda.device(self.device):
            check(capi.load().pam_amd_vertical_interp_cells_to_edges(h, data.shape[1], data.shape[2], data.data_ptr(), int(bc_lower),
                                                                     int(bc_upper), out.data_ptr(),
                                                                     torch.cuda.current_stream(self.device).cuda_stream))
        return out

    def finalize(self):
        if self._h is not None:
            capi.load().pam_amd_vertical_interp_finalize(self._h)
            self._h = None

    def __del__(self):
        try:
            self.finalize()
        except Exception:
            pass
