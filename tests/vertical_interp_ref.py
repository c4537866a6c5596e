"""CPU restatement of pam::VerticalInterp<ord> (pam_core/vertical_interp.h), orders 3 and 5.  TEST INFRASTRUCTURE ONLY: the yardstick
of tests/test_vertical_interp*.py.

Every loop that fixes an order of operations (the sums over a stencil, the elimination steps of the Gauss-Jordan inverse, the
terms of TV, Horner's rule) is a scalar Python loop, as the reference writes it; the only vectorised axes are the independent ones
(levels, columns, members), where numpy's element-wise + - * / are the same IEEE operations one element at a time.

  ghost_interfaces        :159-169        normalised_locations    :181-189
  sten_to_coefs_variable  :215-251        (the inverse: Gauss-Jordan without pivoting, as pam_amd/csrc/awfl_vertical.h -- YAKL's
                                           matinv_ge is not part of the reference tree, DESIGN.md deviation D3)
  tables                  :171-210        ideal_weights           :25-50, :276-280
  weno_coefs              :285-349        tv                      :353-373
  sample_val              :126-134        cells_to_edges          :54-122
"""
import numpy as np

BC_ZERO_GRADIENT = 0
BC_ZERO_VALUE = 1
EPS = 1.0e-20
ORDERS = (3, 5)


def _hs(ord):
    if ord not in ORDERS:
        raise ValueError("orders 3 and 5 only (the reference's sample_val for 7 and 9 drops a `* z`)")
    return (ord - 1) // 2


def check_interfaces(zint):
    zint = np.asarray(zint, dtype=np.float64)
    if zint.ndim != 2 or zint.shape[0] < 2:
        raise ValueError("zint must be (nz+1, nens) with nz >= 1")
    if not np.all(np.isfinite(zint)) or not np.all(np.diff(zint, axis=0) > 0):
        raise ValueError("every member's interfaces must be finite and strictly increasing")
    return zint


def ghost_interfaces(zint, hs):
    """(nz+1+2hs, nens)"""
    nz = zint.shape[0] - 1
    out = np.empty((nz + 2 * hs + 1,) + zint.shape[1:])
    for k in range(nz + 2 * hs + 1):
        if k < hs:
            dz0 = zint[1] - zint[0]
            out[k] = zint[0] - float(hs - k) * dz0
        elif k < hs + nz + 1:
            out[k] = zint[k - hs]
        else:
            dztop = zint[nz] - zint[nz - 1]
            out[k] = zint[nz] + dztop * float(k - hs - nz)
    return out


def matinv_ge(a):
    """a[icol][irow]: n x n nested lists of arrays; Gauss-Jordan elimination without pivoting, (col,row) order"""
    n = len(a)
    scratch = [[a[c][r] * 1.0 for r in range(n)] for c in range(n)]
    one, zero = np.ones_like(a[0][0]), np.zeros_like(a[0][0])
    inv = [[(one if c == r else zero) * 1.0 for r in range(n)] for c in range(n)]
    for d in range(n):
        factor = 1.0 / scratch[d][d]
        for c in range(d, n):
            scratch[c][d] = scratch[c][d] * factor
        for c in range(n):
            inv[c][d] = inv[c][d] * factor
        for r in range(d + 1, n):
            f = scratch[d][r]
            for c in range(d, n):
                scratch[c][r] = scratch[c][r] - f * scratch[c][d]
            for c in range(n):
                inv[c][r] = inv[c][r] - f * inv[c][d]
    for d in range(n - 1, 0, -1):
        for r in range(d):
            f = scratch[d][r]
            for c in range(r + 1, n):
                scratch[c][r] = scratch[c][r] - f * scratch[c][d]
            for c in range(n):
                inv[c][r] = inv[c][r] - f * inv[c][d]
    return inv


def sten_to_coefs_variable(locs):
    """locs: n+1 arrays -> n x n nested lists, rslt[i][j]"""
    n = len(locs) - 1
    pwr = [x * 1.0 for x in locs]
    c2s = [[None] * n for _ in range(n)]
    for j in range(n):
        c2s[0][j] = np.ones_like(locs[0])
    for i in range(1, n):
        for j in range(n + 1):
            pwr[j] = pwr[j] * locs[j]
        for j in range(n):
            c2s[i][j] = 1. / (i + 1.) * (pwr[j] - pwr[j + 1]) / (locs[j] - locs[j + 1])
    return matinv_ge(c2s)


def tables(zint, ord):
    """recon_lo (nz,hs+1,hs+1,hs+1,nens), recon_hi (nz,ord,ord,nens)"""
    hs = _hs(ord)
    zint = check_interfaces(zint)
    nz, nens = zint.shape[0] - 1, zint.shape[1]
    zg = ghost_interfaces(zint, hs)
    locs = [zg[kk:kk + nz] for kk in range(ord + 1)]            # each (nz, nens): all levels at once
    zmid = (locs[hs + 1] + locs[hs]) / 2
    dzmid = locs[hs + 1] - locs[hs]
    locs = [(x - zmid) / dzmid for x in locs]
    hi = sten_to_coefs_variable(locs)
    recon_hi = np.empty((nz, ord, ord, nens))
    for jj in range(ord):
        for ii in range(ord):
            recon_hi[:, jj, ii, :] = hi[jj][ii]
    recon_lo = np.empty((nz, hs + 1, hs + 1, hs + 1, nens))
    for i in range(hs + 1):
        lo = sten_to_coefs_variable(locs[i:i + hs + 2])
        for jj in range(hs + 1):
            for ii in range(hs + 1):
                recon_lo[:, i, jj, ii, :] = lo[jj][ii]
    return recon_lo, recon_hi


def ideal_weights(ord):
    hs = _hs(ord)
    idl = [1.0] * (hs + 1) + [1000.0]
    s = 0.0
    for w in idl:
        s += w
    return [w / (s + EPS) for w in idl]


def tv(a):
    n = len(a)
    t = 1.0 * (a[1] * a[1])
    if n >= 3:
        t = t + 4.3333333333333333333333333333333333333 * (a[2] * a[2])
    if n >= 5:
        t = t + 0.5 * a[1] * a[3]
        t = t + 39.112500000000000000000000000000000000 * (a[3] * a[3])
        t = t + 4.2 * a[2] * a[4]
        t = t + 625.83571428571428571428571428571428571 * (a[4] * a[4])
    if n not in (2, 3, 5):
        raise ValueError(n)
    return t


def sample_val(c, z):
    r = c[-1]
    for m in range(len(c) - 2, -1, -1):
        r = r * z + c[m]
    return r


def weno_coefs(u, lo, hi, ord):
    """u: ord arrays; lo[i][s][ii], hi[s][ii]: arrays broadcastable against them"""
    hs = _hs(ord)
    idl = ideal_weights(ord)
    zero = np.zeros(np.broadcast(u[0], hi[0][0]).shape)
    a_lo = [[None] * (hs + 1) for _ in range(hs + 1)]
    for i in range(hs + 1):
        for ii in range(hs + 1):
            tmp = zero
            for s in range(hs + 1):
                tmp = tmp + lo[i][s][ii] * u[i + s]
            a_lo[i][ii] = tmp
    a_hi = [None] * ord
    for ii in range(ord):
        tmp = zero
        for s in range(ord):
            tmp = tmp + hi[s][ii] * u[s]
        a_hi[ii] = tmp
    for i in range(hs + 1):
        for ii in range(hs + 1):
            a_hi[ii] = a_hi[ii] - idl[i] * a_lo[i][ii]
    for ii in range(ord):
        a_hi[ii] = a_hi[ii] / idl[hs + 1]
    t = [tv(a_lo[i]) for i in range(hs + 1)] + [tv(a_hi)]
    wts = [idl[i] / (t[i] * t[i] + EPS) for i in range(hs + 2)]
    s = zero
    for w in wts:
        s = s + w
    wts = [w / (s + EPS) for w in wts]
    aw = [wts[hs + 1] * a_hi[i] for i in range(ord)]
    for i in range(hs + 1):
        for ii in range(hs + 1):
            aw[ii] = aw[ii] + wts[i] * a_lo[i][ii]
    return aw


def cells_to_edges(data, recon_lo, recon_hi, ord, bc_lower, bc_upper):
    """data (nz,ny,nx,nens) -> edges (nz+1,ny,nx,nens); the tables of tables(), whose member axis may have length 1 (one shared column)"""
    hs = _hs(ord)
    for bc in (bc_lower, bc_upper):
        if bc not in (BC_ZERO_GRADIENT, BC_ZERO_VALUE):
            raise ValueError("bc must be BC_ZERO_GRADIENT or BC_ZERO_VALUE")
    data = np.asarray(data, dtype=np.float64)
    nz = data.shape[0]
    zeros = np.zeros(data.shape[1:])
    below = data[0] if bc_lower == BC_ZERO_GRADIENT else zeros
    above = data[nz - 1] if bc_upper == BC_ZERO_GRADIENT else zeros
    padded = np.concatenate([np.broadcast_to(below, (hs,) + below.shape), data, np.broadcast_to(above, (hs,) + above.shape)])
    u = [padded[kk:kk + nz] for kk in range(ord)]               # stencil(kk) of every cell
    lo = [[[recon_lo[:, i, s, ii, None, None, :] for ii in range(hs + 1)] for s in range(hs + 1)] for i in range(hs + 1)]
    hi = [[recon_hi[:, s, ii, None, None, :] for ii in range(ord)] for s in range(ord)]
    aw = weno_coefs(u, lo, hi, ord)
    lower, upper = sample_val(aw, -0.5), sample_val(aw, 0.5)     # limits(1,k), limits(0,k+1)
    lim0 = np.empty((nz + 1,) + data.shape[1:])
    lim1 = np.empty((nz + 1,) + data.shape[1:])
    lim1[:nz] = lower
    lim0[1:] = upper
    if bc_lower == BC_ZERO_VALUE:
        lim0[0] = 0.0
        lim1[0] = 0.0
    else:
        lim0[0] = lim1[0]
    if bc_upper == BC_ZERO_VALUE:
        lim0[nz] = 0.0
        lim1[nz] = 0.0
    else:
        lim1[nz] = lim0[nz]
    return 0.5 * (lim0 + lim1)


def interp(data, zint, ord, bc_lower=BC_ZERO_GRADIENT, bc_upper=BC_ZERO_GRADIENT):
    lo, hi = tables(zint, ord)
    return cells_to_edges(data, lo, hi, ord, bc_lower, bc_upper)
