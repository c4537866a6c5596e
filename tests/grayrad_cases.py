"""The shapes and the named cases of the grey radiation tests, built once per shape and shared by the CPU and the GPU tests (nobody writes
to them: every backend copies what it changes), and the reference of each, computed once.  TEST INFRASTRUCTURE ONLY.

A case is a dict: fields (name -> (nz,ny,nx,nens) array), liquid and ice (the names of the two tables), zint (nz+1,nens), sfc_temp
((ny,nx,nens) or None) and the scalars of the call."""
import numpy as np

import grayrad_ref as ref

SHAPES = ((1, 1, 1, 1), (2, 1, 3, 3), (5, 1, 4, 64), (7, 3, 2, 65), (12, 2, 5, 70), (60, 1, 2, 130))
CASE_NAMES = ("clear_sky", "thick_cloud", "k_zero", "two_and_two", "p3_set", "ice_only", "dt_zero", "nan_cell")
# what a case must reach: cells with t == 0, t == 1, 0 < t < 1 (True: some, False: none, None: some wherever the shape has a second cell)
CENSUS = dict(clear_sky=(False, False, True), thick_cloud=(True, False, None), k_zero=(False, True, False), two_and_two=(False, False, True),
              p3_set=(False, False, True), ice_only=(False, False, True), dt_zero=(False, False, True), nan_cell=(False, False, True))
SPECIES = ("cloud_liquid", "cloud_water", "ice", "liquid_b", "ice_b")
K = dict(k_d=1.0e-4, k_v=0.1, k_l=85.0, k_i=40.0)
_CACHE, _REF = {}, {}


def grid(nz, nens, per_member=True):
    """stretched interfaces up to 12 km, every member's column scaled a little differently"""
    s = (np.arange(nz + 1) / nz) ** 1.5 * 12000.0
    scale = 1.0 + (0.02 * (np.arange(nens) % 5) if per_member else np.zeros(nens))
    return s[:, None] * scale[None, :]


def cloud_levels(nz):
    """the levels of the cloud layer of thick_cloud: two in the middle where the column has five or more, else the top one"""
    return (nz // 2, nz // 2 + 1) if nz >= 5 else (nz - 1,)


def cloudy_columns(shape):
    """(ny,nx,nens) bool: every other (column, member) of thick_cloud carries the cloud"""
    nz, ny, nx, nens = shape
    return (np.arange(ny * nx * nens).reshape(ny, nx, nens) % 2) == 0


def nan_place(shape):
    nz, ny, nx, nens = shape
    return nz // 2, ny - 1, nx // 2, nens // 2


def cases(shape, per_member=True):
    key = (shape, per_member)
    if key in _CACHE:
        return _CACHE[key]
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(20261020 + 7 * nz + 1000 * nens + (0 if per_member else 1))
    zint = grid(nz, nens, per_member)
    zmid = (0.5 * (zint[:-1] + zint[1:]))[:, None, None, :] + np.zeros(shape)
    # a smooth sounding with a little noise: 300 K at the ground, 6.5 K/km, density with a scale height of 8 km
    temp = 300.0 - 6.5e-3 * zmid + 0.1 * rng.standard_normal(shape)
    rho_d = 1.15 * np.exp(-zmid / 8000.0) * (1.0 + 0.01 * rng.random(shape))
    rho_v = 0.015 * np.exp(-zmid / 2500.0) * (1.0 + 0.2 * rng.random(shape))
    thin = {n: 2.0e-5 * rng.random(shape) * (rng.random(shape) < 0.5) for n in SPECIES}      # thin cloud in half of the cells
    base = dict(temp=temp, density_dry=rho_d, water_vapor=rho_v, **thin)
    common = dict(zint=zint, sfc_temp=None, sigma=ref.SIGMA, cp_d=1004.0, lw_down_top=0.0, dt=10.0, liquid=(), ice=(), **K)

    def case(fields=None, **kw):
        return dict(common, fields=dict(base, **(fields or {})), **kw)

    thick = np.zeros(shape)
    for k in cloud_levels(nz):
        thick[k] = np.where(cloudy_columns(shape), 0.5, 0.0)          # 85 m2/kg x 0.5 kg/m3 x dz: beyond 700 from dz = 17 m on
    nan_temp = temp.copy()
    nan_temp[nan_place(shape)] = np.nan
    sfc = 302.0 + rng.standard_normal((ny, nx, nens))
    out = dict(
        clear_sky=case(),
        thick_cloud=case(fields=dict(cloud_liquid=thick), liquid=("cloud_liquid",)),
        k_zero=case(liquid=("cloud_liquid",), k_d=0.0, k_v=0.0, k_l=0.0, k_i=0.0),
        two_and_two=case(liquid=("cloud_liquid", "liquid_b"), ice=("ice", "ice_b"), sfc_temp=sfc),
        p3_set=case(liquid=("cloud_water",), ice=("ice",), lw_down_top=30.0),
        ice_only=case(ice=("ice",), sfc_temp=sfc, lw_down_top=5.0),
        dt_zero=case(liquid=("cloud_liquid",), dt=0.0),
        nan_cell=case(fields=dict(temp=nan_temp), liquid=("cloud_water",), ice=("ice",)),
    )
    assert tuple(out) == CASE_NAMES
    _CACHE[key] = out
    return out


def reference(shape, name, per_member=True):
    key = (shape, name, per_member)
    if key not in _REF:
        _REF[key] = ref.radiation(cases(shape, per_member)[name], internals=True)
    return _REF[key]


def outputs(result):
    return {n: result[n] for n in ref.OUTPUTS}


def members(case, idx):
    """the members idx of a case, with the matching slice of zint"""
    out = dict(case, fields={n: np.ascontiguousarray(a[..., idx]) for n, a in case["fields"].items()}, zint=np.ascontiguousarray(case["zint"][:, idx]))
    if case.get("sfc_temp") is not None:
        out["sfc_temp"] = np.ascontiguousarray(case["sfc_temp"][..., idx])
    return out
