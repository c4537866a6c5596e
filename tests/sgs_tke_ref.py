"""The prognostic-TKE (1.5-order) closure of the native SGS plug-in: the numpy restatement of the contract (include/pam_amd_modules.h at
pam_amd_sgs_tke_coefficients), its scalar-loop twin, the named cases and the mutants of the restatement.  TEST
INFRASTRUCTURE ONLY.

What is unchanged comes from sgs_ref and sgs_moist_ref: the differences, Def2 (deformation), N2 (stability: on the virtual temperature
with both condensate tables empty, with loading and the saturated branch otherwise), the rows, the Thomas algorithm and the solve.  As
there, numpy's element-wise arithmetic is IEEE and never contracted, no numpy reduction takes part, and every function works in the dtype
of its inputs, so the same restatement in np.longdouble measures the float64 restatement's own rounding error.  The device bodies
(pam_amd/csrc/sgs_device.h: tke_step inside coef_column_t<MOIST, true>) are held to this file bit for bit.  A mutant is a deliberately
wrong variant of ONE line, switched on by name; each must be caught by a named case."""
import math

import numpy as np

import sgs_ref as ref
import sgs_moist_ref as mref
from sgs_ref import WINDS, same_bits, results_differ, shape_id, SHAPES, thomas, rows      # noqa: F401
from sgs_moist_ref import deformation, stability, diffuse                               # noqa: F401

MUTANTS = ("diss_at_e1", "length_no_floor", "length_no_cap", "branch_ge", "buoy_sign", "seed_dropped", "pr_fixed_3", "clip_dropped",
           "tke_without_rho", "keep_bits_dropped", "tkh_from_e0")
CS, CK, SEED = 0.2, 0.1, 1.0e-3


def constants(cs, ck):
    """-> ce, ce1, ce2 in Python floats (IEEE doubles), in the contract's order"""
    ce = ((ck * ck) * ck) / ((cs * cs) * (cs * cs))
    return ce, (ce / 0.7) * 0.19, (ce / 0.7) * 0.51


# ---- 1. one cell's step, element-wise on arrays

def tke_step(tke, rho, D, N2, delta, dt, ck, ce1, ce2, seed, mutant=None, parts=False):
    """-> tke_out, tk, tkh (and the intermediates the census looks at with parts).  Every argument is an array or a scalar of one dtype"""
    T = np.asarray(tke).dtype.type
    dt, ck, ce1, ce2, seed = T(dt), T(ck), T(ce1), T(ce2), T(seed)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = tke + T(0.0) * rho if mutant == "tke_without_rho" else tke / rho
        e0 = np.where(x < 0, T(0.0), x)
        se = np.sqrt(e0)
        delta = delta + T(0.0) * e0
        ls = (T(0.76) * se) / np.sqrt(np.where(N2 > 0, N2, T(1.0)))
        if mutant == "branch_ge":
            ls = (T(0.76) * se) / np.sqrt(np.where(N2 >= 0, N2, T(1.0)))
        lo = T(0.1) * delta
        m = ls if mutant == "length_no_floor" else np.where(ls < lo, lo, ls)
        capped = m if mutant == "length_no_cap" else np.where(m > delta, delta, m)
        stable = N2 >= 0 if mutant == "branch_ge" else N2 > 0
        l = np.where(stable, capped, delta)
        r = l / delta
        pri = T(3.0) + T(0.0) * r if mutant == "pr_fixed_3" else T(1.0) + T(2.0) * r
        ckl = ck * l
        ks = ckl * se if mutant == "seed_dropped" else ckl * se + seed
        P = ks * D
        B = (ks * pri) * N2
        s = P + B if mutant == "buoy_sign" else P - B
        e1u = e0 + dt * s
        e1 = e1u if mutant == "clip_dropped" else np.where(e1u < 0, T(0.0), e1u)
        c = ce1 + ce2 * r
        sd = np.sqrt(e1) if mutant == "diss_at_e1" else se
        e2 = e1 / (T(1.0) + ((dt * c) * sd) / l)
        keep = np.zeros(np.shape(e2), dtype=bool) if mutant == "keep_bits_dropped" else e2 == x
        out = np.where(keep, tke, rho * e2)
        tk = ckl * np.sqrt(e2)
        tkh = pri * (ckl * np.sqrt(e0)) if mutant == "tkh_from_e0" else pri * tk
    if parts:
        return out, tk, tkh, dict(N2=N2, ls=ls, lo=lo, delta=delta, stable=stable, e1u=e1u, keep=keep, x=x)
    return out, tk, tkh


def coefficients(case, mutant=None, dtype=np.float64, parts=False):
    """-> tke_out, tk, tkh of a case"""
    T = dtype
    F = {n: np.asarray(case["fields"][n], dtype=dtype) for n in ("tke", "density_dry", "water_vapor")}
    zint = np.asarray(case["zint"], dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        D = deformation(case, dtype)
        N2 = stability(case, None, dtype)[0]
        rho = F["density_dry"] + F["water_vapor"]
        delta = (zint[1:] - zint[:-1])[:, None, None, :]
    return tke_step(F["tke"], rho, D, N2, delta, T(case["dt"]), T(case["ck"]), T(case["ce1"]), T(case["ce2"]), T(case["seed"]), mutant, parts)


# ---- the scalar-loop twin: one cell at a time in Python floats (IEEE doubles, never contracted); Def2 and N2 are sgs_ref's and
# sgs_moist_ref's, whose own twins cover them

_div = ref._div


def _sqrt(a):
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(np.float64(a)))


def scalar_cell(tke, rho, D, N2, delta, dt, ck, ce1, ce2, seed):
    x = _div(tke, rho)
    e0 = 0.0 if x < 0 else x
    se = _sqrt(e0)
    if N2 > 0:
        ls = _div(0.76 * se, _sqrt(N2))
        lo = 0.1 * delta
        m = lo if ls < lo else ls
        l = delta if m > delta else m
    else:
        l = delta
    r = _div(l, delta)
    pri = 1.0 + 2.0 * r
    ckl = ck * l
    ks = ckl * se + seed
    P = ks * D
    B = (ks * pri) * N2
    s = P - B
    e1 = e0 + dt * s
    e1 = 0.0 if e1 < 0 else e1
    c = ce1 + ce2 * r
    e2 = _div(e1, 1.0 + _div((dt * c) * se, l))
    out = tke if e2 == x else rho * e2
    tk = ckl * _sqrt(e2)
    return out, tk, pri * tk


def scalar_coefficients(case):
    F = case["fields"]
    shape = F["temp"].shape
    nz, ny, nx, nens = shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        D = deformation(case)
        N2 = stability(case)[0]
    out, tk, tkh = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for e in range(nens):
                    at = (k, j, i, e)
                    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                        rho = float(F["density_dry"][at]) + float(F["water_vapor"][at])
                        delta = float(case["zint"][k + 1, e]) - float(case["zint"][k, e])
                        out[at], tk[at], tkh[at] = scalar_cell(float(F["tke"][at]), rho, float(D[at]), float(N2[at]), delta, case["dt"],
                                                               case["ck"], case["ce1"], case["ce2"], case["seed"])
    return out, tk, tkh


# ---- backends: .coefficients(case) -> tke, tk, tkh

class RefBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def coefficients(self, case):
        return coefficients(case, self.mutant)


class ScalarBackend:
    def coefficients(self, case):
        return scalar_coefficients(case)


def run_case(backend, case):
    """-> dict: tke, tk, tkh of the coefficient call"""
    tke, tk, tkh = backend.coefficients(case)
    return dict(tke=tke, tk=tk, tkh=tkh)


def after_coefficients(case, tke):
    """the case as the solve sees it: tke replaced by what the coefficient call left"""
    return dict(case, fields=dict(case["fields"], tke=tke))


def time_step(case, steps=1):
    """-> name -> field after `steps` calls of SGSTke.timeStep as the restatement composes it: the coefficients (tke in place), then the
    existing solve (sgs_moist_ref.diffuse, which is sgs_ref.diffuse without fluxes) on the winds, temp and every tracer, tke among them"""
    out = {}
    for _ in range(steps):
        tke, tk, tkh = coefficients(case)
        mixed = diffuse(after_coefficients(case, tke), tk, tkh)
        case = dict(case, fields=dict(case["fields"], **mixed))
        out = dict(mixed, tk=tk, tkh=tkh)
    return out


members = mref.members


# ---- the named cases
CASE_NAMES = ("base", "zero_tke", "negative_tke", "dt_zero", "nan_tke_cell", "nan_wind_cell", "stable_floor", "unstable", "seed_zero",
              "neutral_exact", "kessler_set", "p3_set", "ice1m_set", "empty_tables", "fluxes_both")
MOIST_CASES = ("kessler_set", "p3_set", "ice1m_set", "empty_tables", "fluxes_both")
_CACHE, _REF = {}, {}


def cases(shape):
    """name -> case, built once per shape and shared (nobody writes to them).  The fields are sgs_moist_ref's (unstable and stable layers in
    pairs, cloudy and clear cells side by side), with the two ice species of ice1m beside them.  tke = rho e with e chosen against the dry
    N2 of the cell so that 0.76 sqrt(e / |N2|) runs from 1e-4 to 10 layer depths (the floor, the range between and the cap are all taken),
    and exactly zero in a fifth of the cells"""
    if shape in _CACHE:
        return _CACHE[shape]
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(11000000 + 100000 * nz + 1000 * ny + 10 * nx + nens)
    m = mref.cases(shape)["kessler_set"]
    fields = dict(m["fields"])
    fields["cloud_ice"], fields["precip_ice"] = fields["ice"], fields["rain"]
    zint, zmid = m["zint"], m["zmid"]
    rho = fields["density_dry"] + fields["water_vapor"]
    delta = (zint[1:] - zint[:-1])[:, None, None, :]
    dry = dict(m, fields=fields, cloud=(), precip=())
    n2 = np.abs(stability(dry)[0]) + 1.0e-7
    f = 10.0 ** rng.uniform(-4.0, 1.0, shape)
    e = (f * delta * np.sqrt(n2) / 0.76) ** 2
    e = np.where(rng.uniform(0.0, 1.0, shape) < 0.2, 0.0, e)
    fields["tke"] = rho * e * rng.uniform(0.7, 1.4, shape)        # not a rounded product with rho: (tke / rho) rho is tke in most cells only
    ce, ce1, ce2 = constants(CS, CK)
    plain = ("water_vapor", "tke", "tracer_a", "tracer_b")

    def case(tracers=plain, cloud=(), precip=(), moist=False, **kw):
        c = dict(m, fields=fields, tracers=tuple(tracers), cloud=tuple(cloud), precip=tuple(precip), moist=moist, ck=CK, ce1=ce1, ce2=ce2,
                 seed=SEED, sfc_shf=None, sfc_lhf=None)
        c.update(kw)
        return c

    def changed(**kw):
        g = dict(fields)
        g.update(kw)
        return g

    out = {"base": case()}
    out["zero_tke"] = case(fields=changed(tke=np.zeros(shape)))
    neg = fields["tke"].copy()
    neg[rng.uniform(0.0, 1.0, shape) < 0.3] *= -1.0
    neg[0, 0, 0, 0] = -1.0e-3
    out["negative_tke"] = case(fields=changed(tke=neg))
    out["dt_zero"] = case(dt=0.0)
    t = fields["tke"].copy()
    t[nz // 2, ny // 2, nx // 2, nens // 2] = np.nan
    out["nan_tke_cell"] = case(fields=changed(tke=t))
    u = fields["uvel"].copy()
    u[nz // 2, ny // 2, nx // 2, nens // 2] = np.nan
    out["nan_wind_cell"] = case(fields=changed(uvel=u))
    # an inversion of 4 K/km everywhere under turbulence weak enough for the floor of the length in every cell (0.76 sqrt(e / N2) < 0.1
    # delta at the thinnest layer, 648 m) and strong enough to outlive the step at the thickest (7757 m)
    z = zmid[:, None, None, :] + np.zeros(shape)
    warm = 280.0 + 0.004 * z + 1.0e-3 * rng.normal(0.0, 1.0, shape)
    out["stable_floor"] = case(fields=changed(temp=warm, tke=rho * rng.uniform(0.5, 2.0, shape)))
    # a lapse rate of 1.5 gc everywhere: N2 < 0 in every cell, buoyancy produces
    steep = 320.0 - 1.5 * (ref.GRAV / ref.CP_D) * z + 1.0e-3 * rng.normal(0.0, 1.0, shape)
    out["unstable"] = case(fields=changed(temp=steep))
    out["seed_zero"] = case(seed=0.0)
    # N2 == 0.0 exactly away from the boundaries: no vapour (Tv is temp), levels 128 m apart, gc = 8 / 1024 = 2^-7, temp = 300 - k;
    # half of the cells hold no tke, where 0.76 sqrt(e) / sqrt(N2) would be 0 / 0
    zi = 128.0 * np.arange(nz + 1)[:, None] + np.zeros((nz + 1, nens))
    lin = 300.0 - np.arange(nz)[:, None, None, None] + np.zeros(shape)
    half = np.where(rng.uniform(0.0, 1.0, shape) < 0.5, 0.0, fields["tke"])
    out["neutral_exact"] = case(fields=changed(temp=lin, water_vapor=np.zeros(shape), tke=half), zint=zi, zmid=0.5 * (zi[:-1] + zi[1:]),
                                grav=8.0, cp_d=1024.0)
    kessler = ("water_vapor", "cloud_liquid", "precip_liquid", "tke", "tracer_a")
    out["kessler_set"] = case(kessler, ("cloud_liquid",), ("precip_liquid",), True)
    out["p3_set"] = case(("cloud_water", "ice", "rain", "water_vapor", "tke", "tracer_a"), ("cloud_water", "ice"), ("rain",), True)
    out["ice1m_set"] = case(("water_vapor", "cloud_liquid", "cloud_ice", "precip_liquid", "precip_ice", "tke"), ("cloud_liquid", "cloud_ice"),
                            ("precip_liquid", "precip_ice"), True, fields=changed(cloud_ice=fields["ice"].copy(), precip_ice=fields["rain"].copy()))
    out["empty_tables"] = case(moist=True)
    fl = mref.cases(shape)["fluxes_both"]
    out["fluxes_both"] = case(kessler, ("cloud_liquid",), ("precip_liquid",), True, sfc_shf=fl["sfc_shf"], sfc_lhf=fl["sfc_lhf"])
    assert tuple(out) == CASE_NAMES
    _CACHE[shape] = out
    return out


def reference(shape, name):
    """the restatement's result of a named case, computed once and shared"""
    key = (shape, name)
    if key not in _REF:
        _REF[key] = run_case(RefBackend(), cases(shape)[name])
    return _REF[key]
