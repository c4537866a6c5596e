"""The shapes and the named cases of the grey shortwave tests, built once per shape and shared by the CPU and the GPU tests (nobody writes
to them: every backend copies what it changes), and the reference of each, computed once.  TEST INFRASTRUCTURE ONLY.

The shapes, the grid and the sounding (temp, density_dry, water_vapor) are the longwave tests' (tests/grayrad_cases.py).  The cloud
species are laid out by rule, not by chance, so that the census below can say what every case reaches at every shape.  A case is a dict:
fields (name -> (nz,ny,nx,nens) array), liquid and ice (the names of the two tables), zint (nz+1,nens), coszen (nens), sfc_albedo
((ny,nx,nens) or None) and the scalars of the call."""
import numpy as np

import grayrad_cases as lw
import grayrad_sw_ref as ref
from grayrad_cases import SHAPES, cloud_levels, cloudy_columns, nan_place      # noqa: F401

CASE_NAMES = ("clear_sky", "cloud", "black_absorber", "conservative", "all_zero", "two_and_two", "p3_set", "ice_only", "beer", "albedo_one",
              "dt_zero", "nan_cell", "nan_coszen", "mixed_night", "grazing")
COEF = dict(a_d=1.0e-6, a_v=2.0e-3, a_l=0.1, a_i=0.1, s_l=11.0, s_i=5.0)
ZERO = dict(a_d=0.0, a_v=0.0, a_l=0.0, a_i=0.0, s_l=0.0, s_i=0.0)
DAY = (1.0, 0.5, 0.8, 0.25, 0.65)                       # coszen of member e: DAY[e % 5]
MIXED = (0.9, 0.0, 0.45, -0.0, 0.2, -0.6, 1.0)          # and of mixed_night: MIXED[e % 7], night beside day in every wavefront
SOME, NONE, MULTI = True, False, None                   # MULTI: some wherever the shape has more than one cell
# what a case must reach among its day members: cells with ta == 0, ta == 1, 0 < ta < 1; cells with b == 0, b > 0; and whether some group
# of 64 lanes holds night and day members (MULTI there: wherever there is more than one member)
CENSUS = dict(
    clear_sky=(NONE, NONE, SOME, SOME, NONE, NONE), cloud=(NONE, NONE, SOME, MULTI, SOME, NONE),
    black_absorber=(SOME, NONE, MULTI, MULTI, SOME, NONE), conservative=(NONE, SOME, NONE, MULTI, SOME, NONE),
    all_zero=(NONE, SOME, NONE, SOME, NONE, NONE), two_and_two=(NONE, NONE, SOME, MULTI, SOME, NONE),
    p3_set=(NONE, NONE, SOME, MULTI, SOME, NONE), ice_only=(NONE, NONE, SOME, MULTI, SOME, NONE), beer=(NONE, NONE, SOME, SOME, NONE, NONE),
    albedo_one=(NONE, NONE, SOME, MULTI, SOME, NONE), dt_zero=(NONE, NONE, SOME, MULTI, SOME, NONE),
    nan_cell=(NONE, NONE, MULTI, MULTI, SOME, NONE), nan_coszen=(NONE, NONE, MULTI, MULTI, MULTI, NONE),      # the one cell, the one member
    mixed_night=(NONE, NONE, SOME, MULTI, SOME, MULTI), grazing=(NONE, NONE, SOME, MULTI, SOME, NONE))
_CACHE, _REF = {}, {}


def census(shape, result, case):
    """the six findings of CENSUS for one reference result (with internals)"""
    nz, ny, nx, nens = shape
    day = ~result["night"]
    ta, b = result["ta"][..., day], result["b"][..., day]
    lane_night = np.broadcast_to(result["night"], (ny, nx, nens)).reshape(-1)
    mixed = False
    for lo in range(0, lane_night.size, 64):
        g = lane_night[lo:lo + 64]
        mixed = mixed or bool(g.any() and not g.all())
    return (bool((ta == 0).any()), bool((ta == 1).any()), bool(((ta > 0) & (ta < 1)).any()), bool((b == 0).any()), bool((b > 0).any()), mixed)


def expected(shape, name):
    multi = (np.prod(shape) > 1,) * 5 + (shape[3] > 1,)
    return tuple(m if want is MULTI else want for want, m in zip(CENSUS[name], multi))


def cases(shape):
    if shape in _CACHE:
        return _CACHE[shape]
    nz, ny, nx, nens = shape
    sound = lw.cases(shape)["clear_sky"]
    rng = np.random.default_rng(20261021 + 7 * nz + 1000 * nens)
    cols, top = cloudy_columns(shape), nz - 1
    noise = lambda: 1.0 + 0.1 * rng.random(shape)

    def layer(levels, where, amount):
        f = np.zeros(shape)
        for k in levels:
            f[k] = np.where(where, amount, 0.0)
        return f * noise()

    everywhere = np.ones_like(cols)
    # a water cloud in every other (column, member): 3e-4 kg/m3 over two levels is about 120 g/m2 at 60 levels; fog under the clear
    # columns; cirrus at the top level
    species = dict(cloud_liquid=layer(cloud_levels(nz), cols, 3.0e-4), cloud_water=layer(cloud_levels(nz), cols, 3.0e-4),
                   liquid_b=layer((0,), ~cols, 2.0e-4), ice=layer((top,), cols, 1.0e-4), ice_b=layer((top,), everywhere, 5.0e-5))
    base = dict({n: sound["fields"][n] for n in ("temp", "density_dry", "water_vapor")}, **species)
    e = np.arange(nens)
    day, mixed = np.array(DAY)[e % 5], np.array(MIXED)[e % 7]
    common = dict(zint=sound["zint"], coszen=day, sfc_albedo=None, solar_constant=1361.0, albedo=0.07, cp_d=1004.0, dt=10.0, liquid=(), ice=(),
                  **COEF)

    def case(fields=None, **kw):
        return dict(common, fields=dict(base, **(fields or {})), **kw)

    black = layer(cloud_levels(nz), cols, 0.5)           # 85 m2/kg x 0.5 kg/m3 x dz: beyond 700 from dz = 17 m on, whatever the sun's height
    nan_vapor = base["water_vapor"].copy()
    nan_vapor[nan_place(shape)] = np.nan
    nan_sun = day.copy()
    nan_sun[nens // 2] = np.nan
    sfc = 0.05 + 0.4 * rng.random((ny, nx, nens))
    out = dict(
        clear_sky=case(),
        cloud=case(liquid=("cloud_liquid",)),
        black_absorber=case(fields=dict(cloud_liquid=black), liquid=("cloud_liquid",), a_l=85.0),
        conservative=case(liquid=("cloud_liquid", "liquid_b"), ice=("ice", "ice_b"), a_d=0.0, a_v=0.0, a_l=0.0, a_i=0.0),
        all_zero=case(liquid=("cloud_water",), ice=("ice",), albedo=0.3, **ZERO),
        two_and_two=case(liquid=("cloud_liquid", "liquid_b"), ice=("ice", "ice_b"), sfc_albedo=sfc),
        p3_set=case(liquid=("cloud_water",), ice=("ice",), solar_constant=1000.0),
        ice_only=case(ice=("ice",), sfc_albedo=sfc),
        beer=case(liquid=("cloud_liquid",), s_l=0.0, s_i=0.0, albedo=0.0),
        albedo_one=case(liquid=("cloud_liquid",), albedo=1.0),
        dt_zero=case(liquid=("cloud_liquid",), dt=0.0),
        nan_cell=case(fields=dict(water_vapor=nan_vapor), liquid=("cloud_water",), ice=("ice",)),
        nan_coszen=case(liquid=("cloud_liquid",), coszen=nan_sun),
        mixed_night=case(liquid=("cloud_liquid", "liquid_b"), ice=("ice", "ice_b"), sfc_albedo=sfc, coszen=mixed),
        grazing=case(liquid=("cloud_liquid",), coszen=np.full(nens, 1.0e-3)),
    )
    assert tuple(out) == CASE_NAMES
    _CACHE[shape] = out
    return out


def reference(shape, name):
    key = (shape, name)
    if key not in _REF:
        _REF[key] = ref.radiation(cases(shape)[name], internals=True)
    return _REF[key]


def outputs(result):
    return {n: result[n] for n in ref.OUTPUTS}


def members(case, idx):
    """the members idx of a case, with the matching slices of zint and coszen"""
    out = dict(case, fields={n: np.ascontiguousarray(a[..., idx]) for n, a in case["fields"].items()}, zint=np.ascontiguousarray(case["zint"][:, idx]),
               coszen=np.ascontiguousarray(case["coszen"][idx]))
    if case.get("sfc_albedo") is not None:
        out["sfc_albedo"] = np.ascontiguousarray(case["sfc_albedo"][..., idx])
    return out
