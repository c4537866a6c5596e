"""Plain references of the two time-step limits that the project takes as a device minimum over every cell (tests/test_time_step_limits.py):
the dycore's CFL step (Dycore.h:86-101; awfl_cfl_kernel / cfl_body) and Kessler's sedimentation limit (Microphysics.h:376-390;
kessler_limit_kernel / kessler_limit_column).  numpy.longdouble, one value PER CELL: a test that knows every cell's limit knows
which cell the minimum has to come from."""
import numpy as np

LD = np.longdouble
DIRECTIONS = ("x", "y", "z")


def _ld(a):
    return np.asarray(a, dtype=LD)


def cfl_cell(rho_d, u, v, w, temp, rho_v, dx, dy, dz, R_d, R_v, gamma, cfl=0.8):
    """the three limits (x, y, z) of cells given value by value (scalars or arrays that broadcast): a tuple of longdoubles"""
    rho_d, u, v, w, temp, rho_v, dz = (_ld(a) for a in (rho_d, u, v, w, temp, rho_v, dz))
    cs = np.sqrt(LD(gamma) * (rho_d * LD(R_d) + rho_v * LD(R_v)) * temp / (rho_d + rho_v))
    return (LD(cfl) * LD(dx) / (np.abs(u) + cs), LD(cfl) * LD(dy) / (np.abs(v) + cs), LD(cfl) * dz / (np.abs(w) + cs))


def cfl_limits(f, idwv, dx, dy, dz, R_d, R_v, gamma, cfl=0.8):
    """f: the coupler fields (density_dry, uvel, vvel, wvel, temp (nz,ny,nx,nens), tracers (nt,nz,ny,nx,nens)); dz (nz,nens).
    Returns (limit, direction): min(x, y, z) of every cell as longdouble and which of the three it is (0, 1, 2)"""
    nz, ny, nx, nens = f["temp"].shape
    dz4 = np.broadcast_to(np.asarray(dz, dtype=np.float64).reshape(nz, -1), (nz, nens))[:, None, None, :]
    three = np.stack(cfl_cell(f["density_dry"], f["uvel"], f["vvel"], f["wvel"], f["temp"], f["tracers"][idwv], dx, dy, dz4,
                              R_d, R_v, gamma, cfl))
    return three.min(axis=0), three.argmin(axis=0)


def kessler_limits(rho_r, rho_dry, zmid, dt):
    """dt2d of every cell below the top level, (nz-1,ny,nx,nens) longdouble: 0.8 (zmid[k+1,e] - zmid[k,e]) / velqr where the fall speed
    velqr = 36.34 (qr 0.001 rho)^0.1364 sqrt(rho0 / rho) is above 1e-10, dt elsewhere; rho0: the column's lowest dry density"""
    rho_r, rho, zm = _ld(rho_r)[:-1], _ld(rho_dry), _ld(zmid)
    rho0, rho = rho[0][None], rho[:-1]
    qr = rho_r / rho
    # (the scheme's constants are the doubles of its source text, not the decimals)
    velqr = LD(36.34) * (qr * LD(0.001) * rho) ** LD(0.1364) * np.sqrt(rho0 / rho)
    gap = (zm[1:] - zm[:-1])[:, None, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(velqr > LD(1e-10), LD(0.8) * gap / velqr, LD(dt))


def two_smallest(a):
    """(flat index of the minimum, the minimum, the smallest of all the OTHER entries) of an array of two or more"""
    flat = np.asarray(a).reshape(-1)
    i = int(flat.argmin())
    return i, flat[i], np.partition(flat, 1)[1]


def undercuts(a, cell, factor=2):
    """the planting condition: entry `cell` (a flat index) times `factor` is at most every other entry of `a`"""
    i, lo, rest = two_smallest(a)
    return i == cell and lo * factor <= rest
