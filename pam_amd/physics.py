"""The physics plug-ins of the reference that need no external library, with the method names of `micro.Microphysics`:

  Radiation         physics/radiation/forced/radiation.h   the GCM's radiative heating applied to the CRM temperature
  RadiationNone     physics/radiation/none/radiation.h
  SGSNone           physics/sgs/none/SGS.h
  MicrophysicsNone  physics/micro/none/Microphysics.h      registers and zeroes "water_vapor", sets the constants

Arithmetic is in libpam_amd_awfl.so (pam_amd/csrc/modules_kernels.hip); there is no CPU path.  Deviations from the reference
(DESIGN.md section 8): the sizes come from the coupler's own getters (options ncrms / crm_nz / crm_nx / crm_ny must agree where they
exist), the rad grid must divide the CRM grid, and missing options or bad constants raise before anything is written."""
import math

import torch

from . import capi
from .capi import check
from .coupler import endrun

_SIZE_OPTIONS = (("ncrms", "get_nens"), ("crm_nz", "get_nz"), ("crm_nx", "get_nx"), ("crm_ny", "get_ny"))


def _forced_sizes(coupler):
    """(nens, nz, ny, nx, rad_ny, rad_nx) of a forced-radiation call, or endrun"""
    nens, nz, ny, nx = coupler.get_nens(), coupler.get_nz(), coupler.get_ny(), coupler.get_nx()
    if min(nens, nz, ny, nx) < 1:
        endrun("ERROR: radiation: the coupler state is not allocated")
    for opt, getter in _SIZE_OPTIONS:
        if coupler.option_exists(opt) and int(coupler.get_option(opt)) != getattr(coupler, getter)():
            endrun(f"ERROR: radiation: option {opt} = {coupler.get_option(opt)} disagrees with the coupler's {getter}() = "
                   f"{getattr(coupler, getter)()}")
    rad_nx, rad_ny = int(coupler.get_option("rad_nx")), int(coupler.get_option("rad_ny"))
    if rad_nx < 1 or rad_ny < 1 or nx % rad_nx or ny % rad_ny:
        endrun(f"ERROR: radiation: rad_nx = {rad_nx}, rad_ny = {rad_ny} must be >= 1 and divide crm_nx = {nx}, crm_ny = {ny}")
    return nens, nz, ny, nx, rad_ny, rad_nx


class Radiation:
    """physics/radiation/forced/radiation.h: temp += rad_enthalpy_tend / cp_d * crm_dt on rad_ny x rad_nx column groups."""

    @staticmethod
    def radiation_name():
        return "forced"

    def init(self, coupler):
        """radiation.h:16-25: option "radiation" = "forced"; registers "rad_enthalpy_tend" (nz,rad_ny,rad_nx,nens), zero-filled"""
        nens, nz, ny, nx, rad_ny, rad_nx = _forced_sizes(coupler)
        dm = coupler.get_data_manager_device_readwrite()
        if dm.entry_exists("rad_enthalpy_tend"):
            endrun("ERROR: Duplicate entry name rad_enthalpy_tend")
        coupler.set_option("radiation", "forced")
        dm.register_and_allocate("rad_enthalpy_tend", "radiation tendency from external calculation", (nz, rad_ny, rad_nx, nens),
                                 ("z", "rad_y", "rad_x", "nens"))

    def timeStep(self, coupler):
        """radiation.h:27-45, one launch on the current stream"""
        lib = capi.load()
        nens, nz, ny, nx, rad_ny, rad_nx = _forced_sizes(coupler)
        dt, cp_d = float(coupler.get_option("crm_dt")), float(coupler.get_option("cp_d"))
        if not math.isfinite(dt):
            endrun("ERROR: radiation: crm_dt must be finite")
        if not (math.isfinite(cp_d) and cp_d > 0):
            endrun("ERROR: radiation: cp_d must be finite and positive")
        dm = coupler.get_data_manager_device_readwrite()
        if dm.get_shape("rad_enthalpy_tend") != [nz, rad_ny, rad_nx, nens]:
            endrun(f"ERROR: radiation: rad_enthalpy_tend is {dm.get_shape('rad_enthalpy_tend')}, not (nz,rad_ny,rad_nx,nens) = "
                   f"{[nz, rad_ny, rad_nx, nens]}")
        tend = dm.get("rad_enthalpy_tend", readonly=True)
        temp = dm.get("temp")
        with torch.cuda.device(coupler.device):
            check(lib.pam_amd_radiation_forced(nens, nx, ny, nz, rad_nx, rad_ny, temp.data_ptr(), tend.data_ptr(), cp_d, dt,
                                               torch.cuda.current_stream(coupler.device).cuda_stream))

    def finalize(self, coupler):
        pass


class RadiationNone:
    """physics/radiation/none/radiation.h"""

    @staticmethod
    def radiation_name():
        return "none"

    def init(self, coupler):
        coupler.set_option("radiation", "none")

    def timeStep(self, coupler):
        pass

    def finalize(self, coupler):
        pass


class SGSNone:
    """physics/sgs/none/SGS.h"""

    @staticmethod
    def get_num_tracers():
        return 0

    @staticmethod
    def sgs_name():
        return "none"

    def init(self, coupler):
        coupler.set_option("sgs", "none")

    def timeStep(self, coupler):
        pass

    def finalize(self, coupler):
        pass


class MicrophysicsNone:
    """physics/micro/none/Microphysics.h: one tracer, no process."""
    # Microphysics.h:23-32
    R_d, cp_d, R_v, cp_v, p0, grav = 287.0, 1003.0, 461.0, 1859.0, 1.0e5, 9.81

    @staticmethod
    def get_num_tracers():
        return 1

    @staticmethod
    def get_diffused_tracers_indices():
        return [0]

    @staticmethod
    def get_num_diffused_tracers():
        return 1

    @staticmethod
    def micro_name():
        return "none"

    def init(self, coupler):
        """Microphysics.h:50-78: registers "water_vapor" (positive, adds mass), zeroes it on the device, sets the constants"""
        import ctypes as C
        lib = capi.load()
        coupler.add_tracer("water_vapor", "Water Vapor", True, True)
        rho_v = coupler.get_data_manager_device_readwrite().get_collapsed("water_vapor")
        size = (C.c_longlong * 1)(rho_v.numel())
        ptr = (C.c_void_p * 1)(rho_v.data_ptr())
        with torch.cuda.device(coupler.device):
            check(lib.pam_amd_time_average_zero(1, size, ptr, torch.cuda.current_stream(coupler.device).cuda_stream))
        coupler.set_option("micro", "none")
        for k in ("R_d", "R_v", "cp_d", "cp_v", "grav", "p0"):
            coupler.set_option(k, getattr(self, k))

    def timeStep(self, coupler):
        pass

    def finalize(self, coupler):
        pass
