"""The shapes and the named states of the ice1m tests, built once per shape and shared by the CPU and the GPU tests (nobody writes to
them: every backend copies what it changes), and the reference of each, computed once.  TEST INFRASTRUCTURE ONLY.

The shapes (nz, ny, nx, nens): nz 1, 2, 5, 7, 12, 60 (the surface and the lid in one level; below, beside and far above AHEAD = 4, with
and without a ragged last batch); nens 1, 3, 64, 65, 70, 130 (one lane, a ragged wavefront, exactly one, two and three wavefronts).

Every cell of a named state draws its temperature (200 to 305 K), its relative humidity and its four condensed species on its own: a
species is absent with probability 0.3, else log-uniform over ten decades, so that every limit of every process is some cell's.  Every
fourth column of a mixed state holds no precipitation and no cloud ice, so clear and precipitating columns share a wavefront.  The
layers of deep_fall are thin and differ by member (200 m, about 15 m, 0.5 m), so the lanes of one wavefront hold nsub = 1, a few, and
the cap of 64.  The seeds are those at which census() reaches every counter at every shape with nz >= 2; tests/test_ice1m.py asserts
that, so a change here that loses a branch fails there."""
import numpy as np

import ice1m_ref as ref

SHAPES = ((1, 1, 1, 1), (2, 1, 3, 3), (5, 1, 4, 64), (7, 3, 2, 65), (12, 2, 5, 70), (60, 1, 2, 130))
MIXED = ("mixed_a", "mixed_b", "mixed_c", "mixed_d")
STATES = MIXED + ("warm_only", "cold_only", "deep_fall")
CASE_NAMES = STATES + ("dt_zero", "nan_cell")
CONSTANTS = dict(dt=20.0, R_v=461.0, cp_d=1003.0)
SEEDS = {(2, 1, 3, 3): 38}          # shape -> seed; absent: 0.  Eighteen cells reach all 27 counters at the 38th draw, not at the first
_CACHE, _REF, _CENSUS, _TRACE = {}, {}, {}, {}


def nan_place(shape):
    nz, ny, nx, nens = shape
    return (nz // 2, ny - 1, nx // 2, nens // 2)


def grid(nz, nens, top=12000.0):
    """stretched interfaces up to `top`, every member's column scaled a little differently"""
    return ((np.arange(nz + 1) / nz) ** 1.3 * top)[:, None] * (1.0 + 0.03 * (np.arange(nens) % 7))[None, :]


def thin_grid(nz, nens):
    """deep_fall: layers of 200 m, of 12 to 18 m and of 0.5 m, by member"""
    e = np.arange(nens)
    dz = np.where(e % 3 == 0, 200.0, np.where(e % 3 == 1, 12.0 + (e % 7), 0.5))
    return np.arange(nz + 1)[:, None] * dz[None, :]


def draw(rng, shape, tlo=200.0, thi=305.0, ice=True, liquid=True, clear_every=4):
    """one state: temp, density_dry and the five species, every cell on its own"""
    nz, ny, nx, nens = shape
    temp = tlo + (thi - tlo) * rng.random(shape)
    rd = 0.3 + 0.9 * rng.random(shape)
    tc = temp - 273.15
    rsw = 610.94 * np.exp(17.625 * tc / (243.04 + tc)) / (461.0 * temp)
    F = dict(temp=temp, density_dry=rd, water_vapor=rsw * (0.05 + 1.25 * rng.random(shape)))

    def species(lo=-12.0, hi=-2.0):
        return np.where(rng.random(shape) < 0.3, 0.0, 10.0 ** (lo + (hi - lo) * rng.random(shape)))

    F["cloud_liquid"] = species() if liquid else np.zeros(shape)
    F["cloud_ice"] = species() if ice else np.zeros(shape)
    F["precip_liquid"] = species() if liquid else np.zeros(shape)
    F["precip_ice"] = species() if ice else np.zeros(shape)
    if clear_every:
        col = (np.arange(ny)[:, None, None] * nx + np.arange(nx)[None, :, None]) * nens + np.arange(nens)[None, None, :]
        clear = (col % clear_every == 0)[None]
        for n in ("cloud_ice", "precip_liquid", "precip_ice"):
            F[n] = np.where(clear, 0.0, F[n])
    return F


def cases(shape):
    if shape in _CACHE:
        return _CACHE[shape]
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(20261021 + 7 * nz + 100 * ny + 1000 * nx + 10000 * nens + 1000003 * SEEDS.get(shape, 0))
    C = CONSTANTS
    zint = grid(nz, nens)
    out = {}
    for name in MIXED:
        out[name] = dict(C, fields=draw(rng, shape), zint=zint)
    out["warm_only"] = dict(C, fields=draw(rng, shape, tlo=275.0, ice=False), zint=zint)
    out["cold_only"] = dict(C, fields=draw(rng, shape, thi=232.0), zint=zint)
    out["deep_fall"] = dict(C, fields=draw(rng, shape, clear_every=0), zint=thin_grid(nz, nens))
    out["dt_zero"] = dict(out["mixed_a"], dt=0.0)
    f = {n: a.copy() for n, a in out["mixed_b"]["fields"].items()}
    f["precip_liquid"][nan_place(shape)] = np.nan
    out["nan_cell"] = dict(C, fields=f, zint=zint)
    assert tuple(out) == CASE_NAMES
    _CACHE[shape] = out
    return out


def reference(shape, name):
    key = (shape, name)
    if key not in _REF:
        _CENSUS[key], _TRACE[key] = {}, {}
        _REF[key] = ref.time_step(cases(shape)[name], census=_CENSUS[key], trace=_TRACE[key])
    return _REF[key]


def trace(shape, name):
    reference(shape, name)
    return _TRACE[shape, name]


def census(shape):
    """the counters of the named states of a shape, added up"""
    total = {n: 0 for n in ref.COUNTERS}
    for name in STATES:
        reference(shape, name)
        for n, v in _CENSUS[shape, name].items():
            total[n] += v
    return total
