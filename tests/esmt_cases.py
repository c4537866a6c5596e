"""The shapes and the named cases of the scalar momentum transport tests, built once per shape and shared by the CPU and the GPU tests
(nobody writes to them: every backend copies what it changes), and the reference of each, computed once.  TEST INFRASTRUCTURE ONLY.

The shapes (nz, nx, nens), ny == 1, are the smallest at which a kernel can go wrong: nx 2 (the Nyquist wavenumber alone), 8 (even, with
a Nyquist wavenumber), 7 (odd, none), 21 (ten wavenumbers: a full and a ragged block of the forward pass's 8; three blocks of the
inverse pass's 8 cells, the last ragged), 65 (the CI line: four full blocks of wavenumbers, nine of cells); nz 2 (both gradient rows
one-sided, below AHEAD = 4), 5 (above it) and 70 (beyond 64, ragged against AHEAD); nens 1, 3, 64, 65, 70 (one lane, a full wavefront, a
ragged second one).  The implementation has no path that depends on the size other than the index width, so there is no further
threshold.  kmax is 0, 1 and nx // 2, by the case.

Vertical grids are per member: stretched by 1.04 per level in even members and by 1.5 in odd ones (the growth stops after 60 and 8
levels, near 1 km, so that the density stays a normal number at nz = 70), every member's column scaled a little differently; the case shared_grid has one uniform grid for all.  wvel is drawn cell by cell.
Members with e % 4 == 1 carry no shear in either scalar and members with e % 4 == 2 none in u (x_s a power of two on every cell, so
every level mean has the same bits); the case nan_w puts a NaN into one wvel cell of one member."""
import numpy as np

import esmt_ref as ref

SHAPES = ((2, 2, 1), (5, 8, 3), (5, 7, 64), (5, 21, 3), (2, 65, 65), (70, 8, 70), (5, 65, 70))
CASE_NAMES = ("all_on", "kmax1", "kmax0", "kmax0_no_force", "no_force", "force_u_only", "shared_grid", "nan_w", "no_v_mean")
CONSTANTS = dict(dt=10.0, dx=500.0, gcm_dt=1200.0)
_CACHE, _REF = {}, {}


def nan_place(shape):
    """(k, i, e) of the NaN of nan_w"""
    nz, nx, nens = shape
    return nz // 2, nx - 1, nens // 2


def grid(nz, nens, shared=False):
    """-> zmid, dz (nz,nens)"""
    k, e = np.arange(nz), np.arange(nens)
    if shared:
        dz = np.full((nz, nens), 250.0)
    else:
        ratio, cap = np.where(e % 2 == 0, 1.04, 1.5)[None, :], np.where(e % 2 == 0, 60, 8)[None, :]
        dz = 40.0 * ratio ** np.minimum(k[:, None], cap) * (1.0 + 0.03 * (e % 7))[None, :]
    zint = np.concatenate([np.zeros((1, nens)), np.cumsum(dz, axis=0)])
    return np.ascontiguousarray(0.5 * (zint[:-1] + zint[1:])), np.ascontiguousarray(zint[1:] - zint[:-1])


def no_shear(nens):
    e = np.arange(nens)
    return (e % 4 == 1) | (e % 4 == 2), e % 4 == 1


def cases(shape):
    if shape in _CACHE:
        return _CACHE[shape]
    nz, nx, nens = shape
    rng = np.random.default_rng(20261021 + 7 * nz + 1000 * nx + 100000 * nens)
    full = (nz, 1, nx, nens)
    C, S = ref.tables(nx)

    def state(shared):
        zmid, dz = grid(nz, nens, shared)
        Z = zmid[:, None, None, :]
        rho = (1.10 + 0.1 * rng.random(full)) * np.exp(-Z / 8000.0)
        rho_v = (0.004 + 0.012 * rng.random(full)) * np.exp(-Z / 2500.0) * rho
        flat_u, flat_v = no_shear(nens)
        us = np.where(flat_u, 4.0, 8.0 * np.tanh(Z / 3000.0) + rng.random(full) - 0.5)
        vs = np.where(flat_v, -2.0, -3.0 + 6.0 * Z / Z.max() + rng.random(full) - 0.5)
        fields = {ref.RD: rho - rho_v, ref.RV: rho_v, "wvel": 4.0 * rng.random(full) - 2.0}
        rho_sum = fields[ref.RD] + fields[ref.RV]
        fields["esmt_u"], fields["esmt_v"] = rho_sum * us, rho_sum * vs
        prof = lambda lo, hi: lo + (hi - lo) * rng.random((nz, nens))
        return dict(CONSTANTS, fields=fields, zmid=zmid, dz=dz, cos=C, sin=S, kmax=nx // 2, force_u=prof(-1.0e-3, 1.0e-3),
                    force_v=prof(-1.0e-3, 1.0e-3), gcm_u=prof(-8.0, 8.0), gcm_v=prof(-8.0, 8.0))

    base = state(False)
    k, i, e = nan_place(shape)
    w_nan = base["fields"]["wvel"].copy()
    w_nan[k, 0, i, e] = np.nan
    out = dict(
        all_on=base,
        kmax1=dict(base, kmax=1),
        kmax0=dict(base, kmax=0),
        kmax0_no_force=dict(base, kmax=0, force_u=None, force_v=None),
        no_force=dict(base, force_u=None, force_v=None),
        force_u_only=dict(base, force_v=None),
        shared_grid=state(True),
        nan_w=dict(base, fields=dict(base["fields"], wvel=w_nan), force_u=None, force_v=None),
        no_v_mean=dict(base, skip_v=True, force_v=None),
    )
    assert tuple(out) == CASE_NAMES
    _CACHE[shape] = out
    return out


def reference(shape, name):
    key = (shape, name)
    if key not in _REF:
        _REF[key] = ref.pgf(cases(shape)[name])
    return _REF[key]


EPS = 2.0 ** -53


def mean_bound(case, T_max):
    """A bound on |M(x_s') - M(x_s) - dt F| per (level, member), x_s = esmt_x / rho, from the operation count alone; eps = 2^-53, the
    unit roundoff, T_max = max |T|, n = 2 kmax the number of harmonics.
    Per cell x_s' = (esmt + rho inc) / rho with inc = dt T + dt F.  The quotient esmt / rho of the mean before costs eps |x_s|; the
    products dt T and dt F and their sum at most 2 eps (|dt T| + |dt F|) + eps |inc|; the product rho inc eps |inc|; the sum and
    the last quotient eps (|x_s| + |inc|) each: together no more than 7 eps (|x_s| + |inc|).
    Each of the two slot means: one product per cell, at most nx / 16 adds in a slot, 16 adds of the slots, and r = 1 / nx, itself
    rounded: (nx / 16 + 18) eps max |x_s'| each.
    What is left is dt M(T).  In exact arithmetic every harmonic has zero mean over x.  T(i) is a sum of n terms That C or That S with
    |That| <= A; A <= 2 T_max (1 + O(eps)) because the coefficients are the transform of T itself.  The n products cost n eps A, the
    recursive sum at most (n - 1) eps n A, and the rounded table entries (eps each) n eps A more: |M(T)| <= (n^2 + 2 n) eps A
    = 2 (n^2 + 2 n) eps T_max.  The bound is the sum of the three parts."""
    F = case["fields"]
    nx = F["wvel"].shape[2]
    rho = F[ref.RD] + F[ref.RV]
    dt, n = case["dt"], 2 * case["kmax"]
    f_max = max([np.abs(case[k]).max() for k in ("force_u", "force_v") if case.get(k) is not None], default=0.0)
    inc = dt * (T_max + f_max)
    xs = max(np.abs(F[k] / rho).max() for k in ref.SCALARS) + inc
    return EPS * (7.0 * xs + 2.0 * (nx / 16.0 + 18.0) * xs + dt * 2.0 * (n * n + 2.0 * n) * T_max)
