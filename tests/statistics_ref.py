"""CPU restatement of the CRM statistics modules (pam_core/modules/horizontal_average.h, time_average.h) in numpy, written from the
reference's loops, independently of the device code: the contract tests/test_statistics_modules.py holds the host emulation and the
HIP kernels to, bit for bit.

  horizontal average   acc = 0; for i = 0 .. ncol-1: acc = fl(acc + fl(v_i * fl(1/ncol)))   (horizontal_average.h:67-73)
  time average         t = fl(t + fl(v * f)),  f = fl(crm_dt / gcm_physics_dt)              (time_average.h:67-70)

numpy rounds every elementwise operation to double and never contracts a product and a sum, so each line below is one rounding.
The horizontal sum runs SEQUENTIALLY over the columns, vectorised over (level, member); np.sum would sum pairwise."""
import numpy as np


def collapse(shape, has_vertical_dim):
    """(nz, ncol, nens) of a variable's shape as horizontal_average.h:46-62 reads it; ValueError where the reference calls endrun"""
    shape = tuple(int(d) for d in shape)
    r = len(shape)
    if has_vertical_dim:
        if r == 3:
            return shape[0], shape[1], shape[2]
        if r == 4:
            return shape[0], shape[1] * shape[2], shape[3]
    else:
        if r == 2:
            return 1, shape[0], shape[1]
        if r == 3:
            return 1, shape[0] * shape[1], shape[2]
    raise ValueError("rank %d %s a vertical dimension cannot be horizontally averaged" % (r, "with" if has_vertical_dim else "without"))


def horizontal_average(var, has_vertical_dim=True):
    """(nz, nens) profile of `var`, summed in the reference's order"""
    var = np.asarray(var, dtype=np.float64)
    nz, ncol, nens = collapse(var.shape, has_vertical_dim)
    v = var.reshape(nz, ncol, nens)
    r = np.float64(1.0) / np.float64(ncol)
    acc = np.zeros((nz, nens), dtype=np.float64)
    for i in range(ncol):
        acc = acc + v[:, i, :] * r
    return acc


def time_average_factor(crm_dt, gcm_physics_dt):
    return np.float64(crm_dt) / np.float64(gcm_physics_dt)


def time_average_accumulate(tavg, var, factor):
    """tavg + var * factor, element by element"""
    return np.asarray(tavg, dtype=np.float64) + np.asarray(var, dtype=np.float64) * np.float64(factor)
