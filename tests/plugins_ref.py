"""CPU restatement of the forced radiation plug-in (physics/radiation/forced/radiation.h:27-45) and of
PamCoupler::compute_pressure_array (pam_core/pam_coupler.h:360-393) in numpy, written from the reference's loops, independently of
the device code: the contract tests/test_physics_plugins.py holds the host emulation and the HIP kernels to, bit for bit.

  radiation   T(k,j,i,e) = fl(T + fl(fl(q / cp_d) * dt)),  q = rad_enthalpy_tend(k, j // (ny // rad_ny), i // (nx // rad_nx), e)
  pressure    p = fl(fl(fl(rho_d * R_d) * T) + fl(fl(rho_v * R_v) * T))

numpy rounds every elementwise operation to double and never contracts a product and a sum, so each operation below is one
rounding; its division is the IEEE one."""
import numpy as np


def rad_grid_check(nx, ny, rad_nx, rad_ny):
    """ValueError where the reference divides by zero (rad_nx > nx) or reads past the tendency (a remainder)"""
    for n, r, d in ((nx, rad_nx, "x"), (ny, rad_ny, "y")):
        if r < 1 or n % r:
            raise ValueError("rad_n%s = %d must be >= 1 and divide crm_n%s = %d" % (d, r, d, n))


def rad_indices(n, rad_n):
    """i_rad of every i = 0 .. n-1: i / (crm_n / rad_n) in integers (radiation.h:41-42)"""
    return np.arange(n) // (n // rad_n)


def radiation_forced(temp, tend, cp_d, dt):
    """temp (nz,ny,nx,nens), tend (nz,rad_ny,rad_nx,nens) -> the new temp"""
    temp = np.asarray(temp, dtype=np.float64)
    tend = np.asarray(tend, dtype=np.float64)
    nz, ny, nx, nens = temp.shape
    rad_ny, rad_nx = tend.shape[1:3]
    assert tend.shape == (nz, rad_ny, rad_nx, nens)
    rad_grid_check(nx, ny, rad_nx, rad_ny)
    q = tend[:, rad_indices(ny, rad_ny)][:, :, rad_indices(nx, rad_nx)]
    with np.errstate(all="ignore"):
        return temp + (q / np.float64(cp_d)) * np.float64(dt)


def compute_pressure(rho_d, rho_v, temp, R_d, R_v):
    rho_d, rho_v, temp = (np.asarray(a, dtype=np.float64) for a in (rho_d, rho_v, temp))
    with np.errstate(all="ignore"):
        return (rho_d * np.float64(R_d)) * temp + (rho_v * np.float64(R_v)) * temp


def divisors(n):
    return [d for d in range(1, n + 1) if n % d == 0]
