"""The shapes and the named cases of the surface-flux tests, built once per shape and shared by the CPU and the GPU tests (nobody writes
to them: every backend copies what it changes), and the reference of each, computed once.  TEST INFRASTRUCTURE ONLY.

A case is a dict: fields (name -> (nz,ny,nx,nens) array, of which the scheme reads level 0), zmid (nz,nens), cn and cstar (nens),
sfc_temp (ny,nx,nens), lw_down, lw_up, sw_down, sw_up ((ny,nx,nens) or None) and the scalars of the call.  Every (row, column, member) has
a random state of its own, and every member its own zmid, z0, cn and cstar."""
import numpy as np

import surface_ref as ref
from sgs_moist_ref import saturation_ratio

# one lane; a partial wavefront; exactly one wavefront; one lane over; two wavefronts plus two lanes with the workload's nz
SHAPES = ((1, 1, 1, 1), (3, 1, 3, 3), (5, 1, 4, 64), (7, 3, 2, 65), (60, 1, 2, 130))
CASE_NAMES = ("mixed", "calm", "neutral", "dew", "slab_off", "no_radiation", "lw_only", "dt_zero", "nan_cell", "dry_surface")
CONSTANTS = dict(gust=1.0, wetness=0.98, grav=9.80616, cp_d=1004.64, R_v=461.505, latvap=2501000.0,
                 slab_heat_capacity=ref.RHO_W * ref.C_W * 1.0, dt=10.0)
_CACHE, _REF = {}, {}


def nan_places(shape):
    """the (j, i, e) of the NaN temp and of the NaN sfc_temp: the last element and the one in the middle (the same in a shape of one)"""
    nz, ny, nx, nens = shape
    return (ny - 1, nx - 1, nens - 1), (ny // 2, nx // 2, nens // 2)


def _neutral_pair(temp0, Ts, rho, qv, z, C):
    """temp0 and Ts moved by a few ulp so that tva == tvs in bits: sa is sought next to tvs / (1 + 0.608 qv), temp0 next to sa - gc z,
    and where no sa gives the product, Ts moves on by one ulp"""
    gcz = (C["grav"] / C["cp_d"]) * z
    fq = 1.0 + 0.608 * qv
    Ts, temp0 = Ts.copy(), temp0.copy()
    todo = np.ones(Ts.shape, dtype=bool)
    for _ in range(64):
        tvs = Ts * (1.0 + 0.608 * (C["wetness"] * saturation_ratio(Ts, rho, C["R_v"])))
        sa0 = tvs / fq
        for ks in range(-3, 4):
            sa = sa0 + ks * np.spacing(sa0)
            t0 = sa - gcz
            for kt in range(-3, 4):
                t = t0 + kt * np.spacing(t0)
                hit = todo & ((t + gcz) * fq == tvs)
                temp0[hit] = t[hit]
                todo &= ~hit
        if not todo.any():
            return temp0, Ts
        Ts[todo] = np.nextafter(Ts[todo], np.inf)
    raise AssertionError("no neutral pair found")


def cases(shape):
    if shape in _CACHE:
        return _CACHE[shape]
    nz, ny, nx, nens = shape
    col = (ny, nx, nens)
    rng = np.random.default_rng(20261022 + 7 * nz + 100 * ny + 1000 * nx + 10000 * nens)
    C = CONSTANTS
    e = np.arange(nens)
    zint = ((np.arange(nz + 1) / nz) ** 1.5 * 12000.0 + 60.0 * np.arange(nz + 1))[:, None] * (1.0 + 0.03 * (e % 7))[None, :]
    zmid = 0.5 * (zint[:-1] + zint[1:])
    z0 = 1.0e-4 * (1.0 + (e % 3))
    cn, cstar = ref.transfer_parameters(zmid[0], z0)

    lapse = 0.0065 * zmid[:, None, None, :]
    temp = 296.0 + 5.0 * rng.random(shape) - lapse
    rho = (1.10 + 0.1 * rng.random(shape)) * np.exp(-zmid / 8000.0)[:, None, None, :]
    qv = (0.008 + 0.008 * rng.random(shape)) * np.exp(-zmid / 2500.0)[:, None, None, :]
    rho_v = qv * rho
    rho_d = rho - rho_v
    uvel, vvel = 16.0 * rng.random(shape) - 8.0, 16.0 * rng.random(shape) - 8.0
    fields = dict(temp=temp, density_dry=rho_d, water_vapor=rho_v, uvel=uvel, vvel=vvel)

    sa = temp[0] + (C["grav"] / C["cp_d"]) * zmid[0]
    flat = np.arange(ny * nx * nens).reshape(col)
    sign = np.where(flat % 2 == 0, 1.0, -1.0)              # neighbours in a wavefront differ
    Ts_mixed = sa + sign * (3.0 + 3.0 * rng.random(col))
    sw_down = 900.0 * rng.random(col)
    rad = dict(lw_down=350.0 + 70.0 * rng.random(col), lw_up=440.0 + 30.0 * rng.random(col), sw_down=sw_down,
               sw_up=(0.05 + 0.05 * rng.random(col)) * sw_down)
    common = dict(C, zmid=zmid, cn=cn, cstar=cstar, sfc_temp=Ts_mixed, **rad)

    def case(f=None, **kw):
        return dict(common, fields=dict(fields, **(f or {})), **kw)

    def level0(name, value):
        a = fields[name].copy()
        a[0] = value
        return a

    rho0, qv0 = rho_d[0] + rho_v[0], rho_v[0] / (rho_d[0] + rho_v[0])
    t_neutral, Ts_neutral = _neutral_pair(temp[0], sa + 1.0, rho0, qv0, zmid[0], C)
    wet = 0.020 + 0.004 * rng.random(col)                   # well above the saturation ratio of the cold surface below
    rv_dew = wet * rho0 / (1.0 - wet) * (rho_d[0] / rho0)   # rho_v with rho_v / (rho_d + rho_v) near wet
    (jt, it, et), (js, is_, es) = nan_places(shape)
    t_nan, Ts_nan = temp[0].copy(), Ts_mixed.copy()
    t_nan[jt, it, et] = np.nan
    Ts_nan[js, is_, es] = np.nan
    none = dict(lw_down=None, lw_up=None, sw_down=None, sw_up=None)
    out = dict(
        mixed=case(),
        calm=case(dict(uvel=level0("uvel", 0.0), vvel=level0("vvel", 0.0))),
        neutral=case(dict(temp=level0("temp", t_neutral)), sfc_temp=Ts_neutral),
        dew=case(dict(water_vapor=level0("water_vapor", rv_dew)), sfc_temp=temp[0] - (6.0 + 4.0 * rng.random(col))),
        slab_off=case(slab_heat_capacity=0.0),
        no_radiation=case(**none),
        lw_only=case(sw_down=None, sw_up=None),
        dt_zero=case(dt=0.0),
        nan_cell=case(dict(temp=level0("temp", t_nan)), sfc_temp=Ts_nan),
        dry_surface=case(wetness=0.0),
    )
    assert tuple(out) == CASE_NAMES
    _CACHE[shape] = out
    return out


def reference(shape, name):
    key = (shape, name)
    if key not in _REF:
        _REF[key] = ref.surface(cases(shape)[name], internals=True)
    return _REF[key]


def outputs(result):
    return {n: result[n] for n in ref.OUTPUTS}
