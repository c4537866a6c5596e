"""The CRM column diagnostics (cloud cover, water paths, precipitable water, surface precipitation): the numpy restatement of the contract
(include/pam_amd_modules.h), the shapes, the named cases and the mutants of the restatement.  TEST INFRASTRUCTURE ONLY.

The method is not part of the reference tree, so this restatement is the yardstick, and the device bodies (pam_amd/csrc/coldiag_device.h,
under g++ in tests/emu/coldiag_emu.cpp and under hipcc in modules_kernels.hip) are held to it bit for bit.  numpy's element-wise float64
arithmetic is IEEE and never contracted; every sum below is written out as a loop over levels, columns and slots, so no numpy reduction
(pairwise order) takes part.

Fields are (nz, ny, nx, nens), members fastest; zint is (nz + 1, nens), a precipitation array (ny, nx, nens), an output (nens).  A mutant is
a deliberately wrong variant of ONE line of the restatement, switched on by name; each must be caught by at least one named case
(tests/test_coldiag.py)."""
from fractions import Fraction

import numpy as np

NS = 16
FIELDS = ("temp", "rho_d", "rho_v", "rho_c", "rho_i", "cldfrac")
PRECIP = ("precip_liq", "precip_ice")
OUT = ("cldtot", "cldlow", "cldmed", "cldhgh", "lwp", "iwp", "pw", "precip_liq", "precip_ice")
COVERS = OUT[:4]
LOW, MED, HGH = 1, 2, 3                                    # a level's class; 0 stands for total
MUTANTS = ("bottom_up", "ge_threshold", "classes_swapped", "scale_after_sum", "fma")
PARAMS = dict(R_d=287.042, R_v=461.505, p_low=70000.0, p_high=40000.0, cwp_threshold=1.0e-3)

# (nz, ny, nx): 1, 5, 16, 17, 21 and 64 columns -- empty slots, one full round, one cell over, an odd count, the slot-thread boundary;
# nens 1, 3 and 65 (across a wavefront)
GRIDS = ((1, 1, 1), (2, 1, 5), (7, 1, 16), (3, 1, 17), (5, 3, 7), (4, 8, 8))
NENS = (1, 3, 65)
CONFIGS = [g + (n,) for g in GRIDS for n in NENS]
# one line of 2 .. 15 columns each, so that every number of occupied slots from 1 to 16 occurs: the census and the emulation take them
SLOT_CONFIGS = [(2, 1, n, 3) for n in range(2, 16)]


def config_id(config):
    return "%dx%dx%dx%d" % config


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- the contract

def pressure(f, params):
    """plugins_device.h's compute_pressure: fl(fl(fl(rho_d R_d) T) + fl(fl(rho_v R_v) T))"""
    return (f["rho_d"] * params["R_d"]) * f["temp"] + (f["rho_v"] * params["R_v"]) * f["temp"]


def level_class(p, params, mutant=None):
    """low where p >= p_low, high where p < p_high, middle otherwise: a NaN pressure is middle"""
    with np.errstate(invalid="ignore"):
        if mutant == "classes_swapped":
            return np.where(p >= params["p_low"], HGH, np.where(p < params["p_high"], LOW, MED))
        return np.where(p >= params["p_low"], LOW, np.where(p < params["p_high"], HGH, MED))


def column_values(f, zint, params, mutant=None):
    """-> the column values (ny, nx, nens) of cldtot .. pw (None where absent), walking top-down"""
    nz, ny, nx, nens = f["rho_v"].shape
    c, i = f.get("rho_c"), f.get("rho_i")
    shape = (ny, nx, nens)
    pw = np.zeros(shape)
    lwp = None if c is None else np.zeros(shape)
    iwp = None if i is None else np.zeros(shape)
    cloudy = c is not None or i is not None
    cwp, cf = [np.zeros(shape) for _ in range(4)], [np.zeros(shape) for _ in range(4)]
    levels = range(nz) if mutant == "bottom_up" else range(nz - 1, -1, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in levels:
            dz = (zint[k + 1] - zint[k])[None, None, :]
            pw = pw + f["rho_v"][k] * dz
            if not cloudy:
                continue
            if c is not None:
                w_c = c[k] * dz
                lwp = lwp + w_c
            if i is not None:
                w_i = i[k] * dz
                iwp = iwp + w_i
            cw = w_c + w_i if (c is not None and i is not None) else (w_c if c is not None else w_i)
            if f.get("cldfrac") is not None:
                cld = f["cldfrac"][k]
            else:
                s = c[k] + i[k] if (c is not None and i is not None) else (c[k] if c is not None else i[k])
                cld = np.where(s > 0, 1.0, 0.0)
            cls = level_class(pressure({n: f[n][k] for n in ("temp", "rho_d", "rho_v")}, params), params, mutant)
            for x in range(4):
                on = np.ones(shape, dtype=bool) if x == 0 else cls == x
                cwp[x] = np.where(on, cwp[x] + cw, cwp[x])
                cf[x] = np.where(on & (cld > cf[x]), cld, cf[x])
        out = dict(lwp=lwp, iwp=iwp, pw=pw)
        thr = params["cwp_threshold"]
        for x, name in enumerate(COVERS):
            above = (cwp[x] >= thr) if mutant == "ge_threshold" else (cwp[x] > thr)
            out[name] = np.where(above, cf[x], 0.0) if cloudy else None
    return out, cwp


def column_mean(v, mutant=None):
    """M(v)(e): column c = j nx + i belongs to slot c % 16; a slot adds v r (the product rounded first) over its columns in ascending c
    from +0.0; the 16 slot sums are added in ascending slot order from +0.0"""
    ny, nx, nens = v.shape
    cols = v.reshape(ny * nx, nens)
    r = 1.0 / (ny * nx)
    parts = np.zeros((NS, nens))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(ny * nx):
            parts[c % NS] = parts[c % NS] + (cols[c] if mutant == "scale_after_sum" else cols[c] * r)
        tot = np.zeros(nens)
        for s in range(NS):
            tot = tot + parts[s]
        return tot * r if mutant == "scale_after_sum" else tot


def _fma(a, b, c):
    """fl(a b + c) with one rounding, element by element in exact rational arithmetic (finite values only)"""
    out = np.empty_like(c)
    for j in range(c.size):
        out[j] = float(Fraction(float(a[j])) * Fraction(float(b)) + Fraction(float(c[j])))
    return out


def diagnose(f, zint, precip, params, out, factor, mutant=None):
    """out_x = out_x + M(x) factor, the product rounded, then the add -> new arrays (None stays None)"""
    vals, _ = column_values(f, zint, params, mutant)
    for n in PRECIP:
        vals[n] = None if precip is None else precip.get(n)
    new = {}
    for x in OUT:
        if vals[x] is None:
            assert out.get(x) is None, x
            new[x] = None
            continue
        m = column_mean(vals[x], mutant)
        with np.errstate(invalid="ignore", over="ignore"):
            new[x] = _fma(m, factor, out[x]) if mutant == "fma" else out[x] + m * factor
    return new


class RefBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def diagnose(self, f, zint, precip, params, out, factor):
        return diagnose(f, zint, precip, params, out, factor, self.mutant)


def run_case(backend, case):
    """the accumulations of the case's steps one after the other"""
    out = {x: (None if a is None else a.copy()) for x, a in case["out0"].items()}
    for f, precip, factor in case["steps"]:
        out = backend.diagnose(f, case["zint"], precip, case["params"], out, factor)
    return out


def results_differ(x, y):
    """names of what differs bitwise between two results of run_case"""
    return [n for n in OUT if (x[n] is None) != (y[n] is None) or (x[n] is not None and not same_bits(x[n], y[n]))]


def members(case, sl):
    """the case restricted to the members of a slice: every array has the members last"""
    def cut(a):
        return None if a is None else np.ascontiguousarray(a[..., sl])

    def cutd(d):
        return None if d is None else {k: cut(v) for k, v in d.items()}
    return dict(case, zint=cut(case["zint"]), out0=cutd(case["out0"]), steps=[(cutd(f), cutd(p), fac) for f, p, fac in case["steps"]])


def join(parts):
    return {x: (None if parts[0][x] is None else np.concatenate([p[x] for p in parts], axis=-1)) for x in OUT}


# ---- the named cases
CLEAR, THICK, THIN, PARTIAL = 0, 1, 2, 3
TARGET_P = {LOW: 85000.0, MED: 55000.0, HGH: 25000.0}     # +- 10 %: inside the class
CONDENSATE = ((True, True), (True, False), (False, True), (False, False))
PRECIP_FORMS = ("both", "liq", "ice", "neither", "no_table")
CLASS_SETS = {"only_low": (LOW,), "only_med": (MED,), "only_high": (HGH,), "low_med": (LOW, MED), "low_high": (LOW, HGH), "med_high": (MED, HGH)}
ABSENT = ["c%d_i%d_%s" % (int(c), int(i), p) for c, i in CONDENSATE for p in PRECIP_FORMS if not (c and i and p == "both")]
CASE_NAMES = tuple(["base"] + list(CLASS_SETS) + ["at_threshold", "ulp_above_threshold", "cldfrac"] + ABSENT +
                   ["nan_temp", "nan_rho_c", "nan_cldfrac", "neg_zero", "factor_zero", "factor_negative", "factor_third", "two_steps"])
FACTOR = 20.0 / 240.0
_CACHE, _REF = {}, {}


def column_kind(config):
    """(ny, nx, nens): cloud-free, thick (well above the threshold), thin (well below it) and scattered columns"""
    nz, ny, nx, nens = config
    return (np.arange(ny * nx).reshape(ny, nx, 1) + np.arange(nens)[None, None, :]) % 4


def cell_class(config):
    """(nz, ny, nx, nens): the class the base fields put a cell's pressure in -- it changes from level to level and from column to
    column, so that even a single level has all three"""
    nz, ny, nx, nens = config
    return 1 + (np.arange(nz)[:, None, None, None] + np.arange(ny * nx).reshape(1, ny, nx, 1) // 2 + np.arange(nens)[None, None, None, :]) % 3


def special_cell(config):
    """where the NaN cases put their one value: (k, j, i, e)"""
    nz, ny, nx, nens = config
    return nz // 2, ny // 2, nx // 2, nens // 2


def _zint(config, rng):
    """every member its own interfaces; the depths are multiples of 1/8 m, so that the interfaces and their differences are exact"""
    nz, nens = config[0], config[3]
    dz = np.round(rng.uniform(100.0, 500.0, (nz, nens)) * 8.0) / 8.0
    return np.concatenate([np.zeros((1, nens)), np.cumsum(dz, axis=0)], axis=0), dz


def _fields(config, rng):
    nz, ny, nx, nens = config
    shp = (nz, ny, nx, nens)
    cls = cell_class(config)
    temp = 290.0 - 6.0 * np.arange(nz)[:, None, None, None] + rng.normal(0.0, 1.5, shp)
    rho_v = 1.0e-2 * rng.uniform(0.3, 1.7, shp)
    target = np.select([cls == LOW, cls == MED, cls == HGH], [TARGET_P[LOW], TARGET_P[MED], TARGET_P[HGH]]) * rng.uniform(0.9, 1.1, shp)
    rho_d = (target - rho_v * PARAMS["R_v"] * temp) / (PARAMS["R_d"] * temp)
    kind = column_kind(config)[None]
    cloudy = (kind == THICK) | (kind == THIN) | ((kind == PARTIAL) & (rng.uniform(size=shp) < 0.5))
    scale = np.where(kind == THIN, 1.0e-3, 1.0)
    icy = rng.uniform(size=shp) < 0.5
    return {"temp": temp, "rho_d": rho_d, "rho_v": rho_v,
            "rho_c": np.where(cloudy & ~icy, 1.0e-4 * rng.uniform(0.1, 1.0, shp), 0.0) * scale,
            "rho_i": np.where(cloudy & icy, 3.0e-5 * rng.uniform(0.1, 1.0, shp), 0.0) * scale,
            "cldfrac": None}


def cases(config):
    """name -> case, built once per shape and shared (nobody writes to them: every backend copies what it changes)"""
    if config in _CACHE:
        return _CACHE[config]
    nz, ny, nx, nens = config
    rng = np.random.default_rng(11 + 1000 * nz + 100 * ny + 10 * nx + nens)
    zint, dz = _zint(config, rng)
    f = _fields(config, rng)
    cls = cell_class(config)
    assert np.array_equal(level_class(pressure(f, PARAMS), PARAMS), cls)
    shp = f["temp"].shape
    precip = {"precip_liq": rng.uniform(0.0, 1.0e-4, (ny, nx, nens)) * (rng.uniform(size=(ny, nx, nens)) < 0.6),
              "precip_ice": rng.uniform(0.0, 3.0e-5, (ny, nx, nens)) * (rng.uniform(size=(ny, nx, nens)) < 0.3)}

    def start(f, precip, fill=None):
        def one(there):
            if not there:
                return None
            return rng.normal(0.0, 1.0, nens) if fill is None else np.full(nens, fill)
        cloudy = f.get("rho_c") is not None or f.get("rho_i") is not None
        out = {x: one(cloudy) for x in COVERS}
        out.update(lwp=one(f.get("rho_c") is not None), iwp=one(f.get("rho_i") is not None), pw=one(True))
        for n in PRECIP:
            out[n] = one(precip is not None and precip.get(n) is not None)
        return out

    def case(fields, pr=precip, out0=None, steps=None, z=zint, factor=FACTOR, fill=0.0):
        return dict(zint=z, params=PARAMS, steps=steps or [(fields, pr, factor)], out0=out0 or start(fields, pr, fill))

    def changed(**kw):
        g = dict(f)
        g.update(kw)
        return g

    def poke(a, value, where=None):
        a = a.copy()
        a[where or special_cell(config)] = value
        return a

    out = {"base": case(f)}
    for name, keep in CLASS_SETS.items():
        m = np.isin(cls, keep)
        out[name] = case(changed(rho_c=np.where(m, f["rho_c"], 0.0), rho_i=np.where(m, f["rho_i"], 0.0)))
    # column (0, 0) of member 0: cloud water in its top level only, whose depth is 256 m, so that rho_c dz is exact
    z256 = dz.copy()
    z256[nz - 1, 0] = 256.0
    z256 = np.concatenate([np.zeros((1, nens)), np.cumsum(z256, axis=0)], axis=0)
    thr = PARAMS["cwp_threshold"]
    for name, path in (("at_threshold", thr), ("ulp_above_threshold", np.nextafter(thr, np.inf))):
        c, i = f["rho_c"].copy(), f["rho_i"].copy()
        c[:, 0, 0, 0], i[:, 0, 0, 0] = 0.0, 0.0
        c[nz - 1, 0, 0, 0] = path / 256.0
        out[name] = case(changed(rho_c=c, rho_i=i), z=z256)
    frac = rng.uniform(0.0, 1.0, shp) * (rng.uniform(size=shp) < 0.7)
    out["cldfrac"] = case(changed(cldfrac=frac))
    for has_c, has_i in CONDENSATE:
        for form in PRECIP_FORMS:
            if has_c and has_i and form == "both":
                continue
            g = changed(**({} if has_c else {"rho_c": None}), **({} if has_i else {"rho_i": None}))
            pr = None if form == "no_table" else {"precip_liq": precip["precip_liq"] if form in ("both", "liq") else None,
                                                  "precip_ice": precip["precip_ice"] if form in ("both", "ice") else None}
            out["c%d_i%d_%s" % (int(has_c), int(has_i), form)] = case(g, pr)
    k, j, i, e = special_cell(config)
    out["nan_temp"] = case(changed(temp=poke(f["temp"], np.nan), rho_c=poke(f["rho_c"], 2.0e-4)))
    out["nan_rho_c"] = case(changed(rho_c=poke(f["rho_c"], np.nan)))
    out["nan_cldfrac"] = case(changed(cldfrac=poke(frac, np.nan)))
    nzf = {n: (None if f[n] is None else np.full(shp, -0.0)) for n in FIELDS}
    nzp = {n: np.full((ny, nx, nens), -0.0) for n in PRECIP}
    out["neg_zero"] = case(nzf, nzp, fill=-0.0)
    for name, factor in (("factor_zero", 0.0), ("factor_negative", -0.25), ("factor_third", 1.0 / 3.0)):
        out[name] = case(f, factor=factor, out0=start(f, precip))
    g2 = changed(rho_v=f["rho_v"] * 1.1, rho_c=f["rho_c"] * 0.5)
    out["two_steps"] = case(f, out0=start(f, precip), steps=[(f, precip, FACTOR * 3.0), (g2, {n: a * 0.5 for n, a in precip.items()}, FACTOR)])
    assert tuple(out) == CASE_NAMES
    _CACHE[config] = out
    return out


def reference(config, name):
    """the restatement's result of a named case, computed once and shared"""
    key = (config, name)
    if key not in _REF:
        _REF[key] = run_case(RefBackend(), cases(config)[name])
    return _REF[key]
