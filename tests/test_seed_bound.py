"""CPU: the lower bound of water vapour's FCT seed (seed_lower_bound, pam_amd/csrc/awfl_device.h) and the x-sweep that loads the seed only
where that bound does not settle the multiplier.  tests/emu/seed_skip_emu.cpp: all of the host emulation plus
  emu_seed_bound           producer and consumer of a seed on arrays of operands, with the library's own functions;
  emu_time_step_seed_skip  the fused NT = 1 stage with the seed always loaded or lazily, counting the rows of either path.
The bound must hold for every seed a stage can read (seed >= bound, hence available(bound) <= available(seed)): the skip then stores
the very bits of the loading path, which the second half checks on whole time steps, array_equal."""
import copy
import ctypes as C

import numpy as np
import pytest

import emu_harness as eh
from pam_amd import idealized as idz
from parity_cases import build_inputs
from tools.native_build import emu_library

_DP = C.POINTER(C.c_double)
_LP = C.POINTER(C.c_longlong)
NZ = 4
FIELDS = ("density_dry", "uvel", "vvel", "wvel", "temp", "tracers")
# the shapes of tests/test_xsweep_pressure_emu.py: (nens, nx, ny, span, mode_a, per-member grid, carve_dry_air, options of build_inputs)
SHAPES = {
    "nx32_3d_span4_dry_air": (3, 32, 5, 4, True, False, True, {}),
    "nx3_2d_whole_perens_B": (2, 3, 1, 0, False, True, False, {}),
    "aniso_800x500_nx9_3d_span4_dry_air_flowy": (3, 9, 5, 4, True, False, True, dict(dxy=800.0, dy=500.0, flow="y")),
    "aniso_500x800_nx6_3d_whole_perens_B_flowy": (2, 6, 5, 0, False, True, False, dict(dxy=500.0, dy=800.0, flow="y")),
}


@pytest.fixture(scope="module")
def lib():
    so = C.CDLL(emu_library("seed_skip_emu"))
    ref = eh.load()
    for name in ("emu_init", "emu_destroy", "emu_set_grav_balance", "emu_set_span", "emu_set_fused", "emu_set_yz_fold", "emu_buffer",
                 "emu_declare_hydrostatic", "emu_time_step"):
        getattr(so, name).restype = getattr(ref, name).restype
        getattr(so, name).argtypes = getattr(ref, name).argtypes
    so.emu_time_step_seed_skip.restype = C.c_int
    so.emu_time_step_seed_skip.argtypes = ref.emu_time_step.argtypes + [C.c_int, C.c_int, _LP]
    so.emu_fct_flags.restype = C.c_longlong
    so.emu_fct_flags.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    so.emu_seed_bound.restype = None
    so.emu_seed_bound.argtypes = [C.c_int, C.c_longlong, _DP, _DP, _DP, C.c_double, C.c_double, C.c_double, _DP, _DP, _DP, _DP]
    return so


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound itself

def _bound(lib, stage, a, b, c, dx=500.0, dy=800.0, dzk=137.5):
    a, b, c = (np.ascontiguousarray(np.broadcast_to(x, np.broadcast(a, b, c).shape), dtype=np.float64) for x in (a, b, c))
    out = [np.empty_like(a) for _ in range(4)]
    lib.emu_seed_bound(stage, a.size, *(x.ctypes.data_as(_DP) for x in (a, b, c)), dx, dy, dzk, *(x.ctypes.data_as(_DP) for x in out))
    return out


def _holds(seed, low, av_low, av_seed):
    """seed >= bound and available(bound) <= available(seed); a NaN seed (a NaN state) has a NaN bound and both sides available 0"""
    nan = np.isnan(seed)
    assert not (np.isnan(low) & ~nan).any()
    ok = ~nan & ~np.isnan(low)
    assert (low[ok] <= seed[ok]).all(), (low[ok][low[ok] > seed[ok]][:5], seed[ok][low[ok] > seed[ok]][:5])
    assert not np.isnan(av_low).any() and not np.isnan(av_seed).any()
    assert (av_low <= av_seed).all()


def _ulp_neighbours(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


# what produces the operands: (name, how the mass a producer clips is drawn).  init_prim_body clips the coupler's value, the stage-3
# updates (state pass, fix-up pass, tile kernels, one-kernel update: all tracer_new_value) clip an rk_combine that may come out negative
PRODUCERS = ("init_prim", "stage_update")


@pytest.mark.parametrize("producer", PRODUCERS)
@pytest.mark.parametrize("stage", (1, 2, 3))
def test_bound_is_below_every_seed_of_a_million_random_positive_triples(lib, stage, producer):
    rng = np.random.default_rng(1000 * stage + PRODUCERS.index(producer))
    n = 1_000_000
    rho = np.exp(rng.uniform(np.log(1.0e-3), np.log(3.0), n))            # air density, kg/m3: the stratosphere to the surface and beyond
    q = np.exp(rng.uniform(np.log(1.0e-12), np.log(0.05), n))            # vapour mixing ratio
    mass = q * rho
    if producer == "stage_update":                                      # the update's result around the mass, one in eight negative
        mass = mass * rng.uniform(-0.15, 2.0, n)
    if stage == 1:
        out = _bound(lib, 1, mass, rho, 0.0)
        S, low = out[0], out[1]
        pos = S > 0
        assert (low[pos] > S[pos] * (1 - 2.0 ** -47)).all(), "the bound is no more than a few ulps below the seed"
    else:
        out = _bound(lib, stage, q, rho, mass)
    _holds(*out)
    assert (out[1] >= 0).all() and (out[1][out[0] > 0] > 0).sum() > n // 2


@pytest.mark.parametrize("stage", (1, 2, 3))
def test_bound_on_the_named_edge_values(lib, stage):
    tiny = np.finfo(np.float64).tiny
    edge = np.array([0.0, -0.0, 5e-324, 1e-320, tiny / 2, tiny, 2 * tiny, 1e-300, 1e-200, 1e-100, 1e-30, 1e-12, 1e-3, 1.0, 3.0, 1e3,
                     1e30, 1e100, 1e200, 1e300, np.finfo(np.float64).max, -1.0, -1e-300, -1e300, np.inf, np.nan])
    A, B, Cc = (x.ravel() for x in np.meshgrid(edge, edge, edge, indexing="ij"))
    if stage == 1:
        # mass and density; also m_0 one ulp either side of m_in -- here: the mass one ulp either side of q * rho
        rho = np.array([1e-3, 0.4, 1.0, 1.2250000000000001, 3.0])
        q = np.array([1e-320, 1e-300, 1e-12, 1e-3, 0.02, 1.0])
        Q, R = (x.ravel() for x in np.meshgrid(q, rho, indexing="ij"))
        _holds(*_bound(lib, 1, _ulp_neighbours(Q * R), np.tile(R, 3), 0.0))
        _holds(*_bound(lib, 1, R, R, 0.0))                               # equal operands
        _holds(*_bound(lib, 1, A, B, 0.0))
        # outside its guards the bound is 0: nothing to trust, the seed is loaded
        s, low, _, _ = _bound(lib, 1, np.array([1.0, 1.0, 1e-310, 1e308, 1.0]), np.array([-1.0, 1e200, 1.0, 1e-3, np.nan]), 0.0)
        assert (low == 0).all()
    else:
        _holds(*_bound(lib, stage, A, B, Cc))
        _holds(*_bound(lib, stage, edge, edge, edge))                    # equal operands
        # v clipped to 0: the seed IS the bound
        s, low, al, as_ = _bound(lib, stage, np.array([1e-3, 0.02]), np.array([1.2, 0.4]), np.array([-5.0, -0.0]))
        assert np.array_equal(s, low) and np.array_equal(al, as_)
        # m_0 one ulp either side of the stage input's mass: the bound follows m_0, whatever v is
        q, rho = 0.0123, 1.1
        for v in _ulp_neighbours([q * rho]):
            _holds(*_bound(lib, stage, _ulp_neighbours([q]), rho, v))


# ---------------------------------------------------------------------------------------------------------------------------------
# whole time steps

class _Emu(eh.EmuDycore):
    def __init__(self, so, *args, **kw):
        load, eh.load = eh.load, lambda: so
        try:
            super().__init__(*args, **kw)
        finally:
            eh.load = load

    def time_step_seed(self, f, crm_dt, lazy, pressure, counts):
        out = C.c_double(0)
        return self.lib.emu_time_step_seed_skip(self.h, *self._f(f), float(crm_dt), 0.0, C.byref(out), int(lazy), int(pressure),
                                                counts.ctypes.data_as(_LP))


def _inputs(shape):
    nens, nx, ny, span, mode_a, per_ens, dry_air, opts = SHAPES[shape]
    tr = idz.TRACERS_NONE
    zint = idz.stretched_interfaces(NZ, 6000.0)
    f, xlen, ylen, _, _ = build_inputs(nens, nx, ny, NZ, tr, zint, mag=0.5, dry_air=dry_air, **opts)
    dz = np.diff(zint)[:, None] * np.ones((1, nens))
    if per_ens:
        dz = dz * (1 + 0.01 * np.arange(nens))[None, :]
    _, pos, mass, idwv = idz.tracer_flags(tr)
    return (nens, nx, ny, NZ, xlen, ylen, dz, pos, mass, idwv), f


def _run(lib, args, f, shape, lazy, pressure, fold=False):
    nens, nx, ny, span, mode_a = SHAPES[shape][:5]
    ff = copy.deepcopy(f)
    d = _Emu(lib, *args)
    d.set_grav_balance(mode_a)
    d.set_fused(True)
    d.set_span(span)
    d.set_yz_fold(fold)
    d.declare_current_profile_as_hydrostatic(ff)
    counts = np.zeros(6, dtype=np.int64)
    ncyc = [d.time_step_seed(ff, crm_dt, lazy, pressure, counts) for crm_dt in (2.0, 0.7)]      # odd and even sub-step counts
    ncell = NZ * ny * nx * nens
    res = dict(ff)
    res["prim0"] = np.array(d.buffer("prim0", (6 + 1, NZ + 6, ny, nx, nens)))
    res["seed"] = np.array(d.buffer("seed", (ncell,)))
    res["mult"] = np.array(d.buffer("mult", (ncell,)))
    res["flags"] = np.zeros(d.lib.emu_fct_flags(d.h, None), dtype=np.int32)
    d.lib.emu_fct_flags(d.h, res["flags"].ctypes.data_as(C.POINTER(C.c_int)))
    return ncyc, res, counts.reshape(3, 2)


@pytest.fixture(scope="module")
def runs(lib):
    """(shape, pressure) -> the run that always loads the seed: computed once, shared, left unchanged"""
    cache = {}

    def get(shape, pressure):
        if (shape, pressure) not in cache:
            args, f = _inputs(shape)
            cache[(shape, pressure)] = (args, f, _run(lib, args, f, shape, False, pressure))
        return cache[(shape, pressure)]
    return get


@pytest.mark.parametrize("pressure", (False, True), ids=("pressure_pass", "in_sweep_pressure"))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_lazy_seed_stores_the_bits_of_the_loading_sweep_and_counts_its_rows(lib, runs, shape, pressure):
    args, f, (n0, a, c0) = runs(shape, pressure)
    n1, b, counts = _run(lib, args, f, shape, True, pressure)
    assert n0 == n1 and min(n0) > 0
    assert not c0.any()
    assert a["flags"].any() == bool(SHAPES[shape][6])
    for k in FIELDS + ("prim0", "seed", "mult", "flags"):          # (mult: poisoned in unflagged rows, on both sides)
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, np.abs(a[k] - b[k]).max())
    for k in FIELDS:
        assert np.isfinite(a[k]).all(), k
    nens, nx, ny = SHAPES[shape][:3]
    rows_per_stage = NZ * ny * nx * ((nens + 63) // 64) * sum(n0)
    assert (counts.sum(axis=1) == rows_per_stage).all(), counts
    if SHAPES[shape][6]:      # carved dry air: rows of either kind in every stage
        assert (counts > 0).all(), counts
    else:                     # a smooth positive field: no wavefront asks for the seed, in any stage
        assert (counts[:, 1] == 0).all(), counts


def test_lazy_seed_with_the_folded_handoff(lib, runs):
    shape = "aniso_800x500_nx9_3d_span4_dry_air_flowy"
    args, f, (n0, a, _) = runs(shape, True)
    n1, b, counts = _run(lib, args, f, shape, True, True, fold=True)
    assert n0 == n1
    for k in FIELDS + ("seed",):
        assert np.array_equal(a[k], b[k]), k
    assert (counts > 0).all()
