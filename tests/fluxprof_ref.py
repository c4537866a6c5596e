"""The CRM flux profiles (convective mass fluxes by conditional sampling, cloud fraction profile, resolved vertical fluxes and resolved
turbulence kinetic energy): the numpy restatement of the contract (include/pam_amd_modules.h), the shapes, the named
cases and the mutants of the restatement.  TEST INFRASTRUCTURE ONLY.

The method is not part of the reference tree, so this restatement is the yardstick, and the device bodies (pam_amd/csrc/fluxprof_device.h,
under g++ in tests/emu/fluxprof_emu.cpp and under hipcc in modules_kernels.hip) are held to it bit for bit.  numpy's element-wise float64
arithmetic is IEEE and never contracted; every sum below is written out as a loop over rounds of 16 cells and over slots, so no numpy
reduction (pairwise order) takes part.

Fields are (nz, ny, nx, nens), members fastest; an output is (nz, nens).  A mutant is a deliberately wrong variant of ONE line of the
restatement, switched on by name; each must be caught by at least one named case (tests/test_fluxprof.py)."""
import numpy as np

NS = 16
FIELDS = ("rho_d", "rho_v", "rho_c", "rho_i", "temp", "uvel", "vvel", "wvel")
OUT = ("mcup", "mcdn", "mcuup", "mcudn", "cld", "flux_t", "flux_qt", "flux_u", "flux_v", "tke")
SAMPLED = ("mcup", "mcdn", "cld")                          # absent exactly where both condensates are
FLUXES = ("flux_t", "flux_qt", "flux_u", "flux_v")
MUTANTS = ("ge_threshold", "w_ge_zero", "shift_from_mean", "q_over_rho_d", "no_clamp", "all_classes_add", "slots_reversed")
QC = 1.0e-5

# (nz, ny, nx): 1, 5, 16, 17, 21 and 64 columns -- empty slots, one full round, one cell over, an odd count, four cells per slot;
# nens 1, 3 and 65 (across a member block)
GRIDS = ((1, 1, 1), (2, 1, 5), (7, 1, 16), (3, 1, 17), (5, 3, 7), (4, 8, 8))
NENS = (1, 3, 65)
CONFIGS = [g + (n,) for g in GRIDS for n in NENS]
# one line of 2 .. 15 columns each, so that every number of occupied slots from 1 to 16 occurs: the CPU tests take them
SLOT_CONFIGS = [(2, 1, n, 3) for n in range(2, 16)]


def config_id(config):
    return "%dx%dx%dx%d" % config


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- the contract

def level_mean(vals, mask=None, mutant=None):
    """M(vals)(e) of one level, vals (ncol, nens): cell c belongs to slot c % 16; a slot adds vals r (the product rounded first) over its
    cells in ascending c from 0.0 -- with a mask only where the mask holds --; the 16 slot sums are added in ascending slot order from 0.0"""
    ncol, nens = vals.shape
    r = 1.0 / ncol
    parts = np.zeros((NS, nens))
    for c0 in range(0, ncol, NS):                          # one round: the next cell of every slot
        n = min(NS, ncol - c0)
        new = parts[:n] + vals[c0:c0 + n] * r
        parts[:n] = new if mask is None else np.where(mask[c0:c0 + n], new, parts[:n])
    tot = np.zeros(nens)
    for s in (range(NS - 1, -1, -1) if mutant == "slots_reversed" else range(NS)):
        tot = tot + parts[s]
    return tot


def cell_values(f, k, qc, mutant=None):
    """the level's per-cell values (ncol, nens): the six quantities m, temp, q, uvel, vvel, wvel and the masks cloudy and up"""
    def lev(n):
        a = f.get(n)
        return None if a is None else a[k].reshape(-1, a.shape[-1])
    rho_d, rho_v, c, i, w = lev("rho_d"), lev("rho_v"), lev("rho_c"), lev("rho_i"), lev("wvel")
    rho = rho_d + rho_v
    wat = rho_v
    if c is not None:
        wat = wat + c
    if i is not None:
        wat = wat + i
    x = {"m": rho * w, "temp": lev("temp"), "q": wat / (rho_d if mutant == "q_over_rho_d" else rho), "uvel": lev("uvel"), "vvel": lev("vvel"),
         "wvel": w}
    if c is None and i is None:
        cloudy = np.zeros(w.shape, dtype=bool)
    else:
        cond = c + i if (c is not None and i is not None) else (c if c is not None else i)
        cloudy = (cond >= qc * rho) if mutant == "ge_threshold" else (cond > qc * rho)
    up = (w >= 0) if mutant == "w_ge_zero" else (w > 0)
    return x, cloudy, up


def level_values(f, k, qc, mutant=None, preclamp=None):
    """the ten values (nens) of level k; preclamp: a dict that receives B - A A of uvel, vvel, wvel before the clamp"""
    with np.errstate(all="ignore"):
        x, cloudy, up = cell_values(f, k, qc, mutant)
        classes = {"mcup": cloudy & up, "mcdn": cloudy & ~up, "mcuup": ~cloudy & up, "mcudn": ~cloudy & ~up}
        val = {n: level_mean(x["m"], None if mutant == "all_classes_add" else mask, mutant) for n, mask in classes.items()}
        val["cld"] = level_mean(np.ones(cloudy.shape), cloudy, mutant)
        if mutant == "shift_from_mean":
            d = {n: a - a.mean(axis=0)[None, :] for n, a in x.items()}
        else:
            d = {n: a - a[0][None, :] for n, a in x.items()}
        A = {n: level_mean(a, None, mutant) for n, a in d.items()}
        for name, n in zip(FLUXES, ("temp", "q", "uvel", "vvel")):
            val[name] = level_mean(d["m"] * d[n], None, mutant) - A["m"] * A[n]
        var = []
        for n in ("uvel", "vvel", "wvel"):
            v = level_mean(d[n] * d[n], None, mutant) - A[n] * A[n]
            if preclamp is not None:
                preclamp[n] = v
            var.append(v if mutant == "no_clamp" else np.where(v < 0, 0.0, v))
        val["tke"] = 0.5 * ((var[0] + var[1]) + var[2])
    return val


def profiles(f, qc, out, factor, mutant=None):
    """out_x = out_x + value factor, the product rounded, then the add -> new arrays (None stays None)"""
    nz = f["rho_d"].shape[0]
    has_cond = f.get("rho_c") is not None or f.get("rho_i") is not None
    new = {n: (None if a is None else a.copy()) for n, a in out.items()}
    for n in OUT:
        assert (new[n] is None) == (n in SAMPLED and not has_cond), n
    with np.errstate(all="ignore"):
        for k in range(nz):
            val = level_values(f, k, qc, mutant)
            for n in OUT:
                if new[n] is not None:
                    new[n][k] = new[n][k] + val[n] * factor
    return new


class RefBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def profiles(self, f, qc, out, factor):
        return profiles(f, qc, out, factor, self.mutant)


def run_case(backend, case):
    """the accumulations of the case's steps one after the other"""
    out = {x: (None if a is None else a.copy()) for x, a in case["out0"].items()}
    for f, factor in case["steps"]:
        out = backend.profiles(f, case["qc"], out, factor)
    return out


def results_differ(x, y):
    """names of what differs bitwise between two results of run_case"""
    return [n for n in OUT if (x[n] is None) != (y[n] is None) or (x[n] is not None and not same_bits(x[n], y[n]))]


def members(case, sl):
    """the case restricted to the members of a slice: every array has the members last"""
    def cut(a):
        return None if a is None else np.ascontiguousarray(a[..., sl])

    def cutd(d):
        return {k: cut(v) for k, v in d.items()}
    return dict(case, out0=cutd(case["out0"]), steps=[(cutd(f), fac) for f, fac in case["steps"]])


def join(parts):
    return {x: (None if parts[0][x] is None else np.concatenate([p[x] for p in parts], axis=-1)) for x in OUT}


# ---- the named cases
CONDENSATE = ((True, True), (True, False), (False, True), (False, False))
CASE_NAMES = ("base", "all_clear", "all_cloudy", "at_threshold", "ulp_above_threshold", "w_zero", "nan_w", "nan_rho_c", "nan_temp",
              "constant_level", "var_rounds_negative", "c1_i1", "c1_i0", "c0_i1", "c0_i0", "factor_third", "two_steps", "neg_zero")
FACTOR = 20.0 / 240.0
TINY = 5.0e-324                                            # the smallest subnormal
_CACHE, _REF = {}, {}
NEGATIVE_FOUND = {}                                        # config -> whether var_rounds_negative has B - A A < 0 somewhere


def special(config):
    """where the cases that change one level of one member, or one cell of it, put their values: (k, j, i, e)"""
    nz, ny, nx, nens = config
    return nz // 2, ny // 2, nx // 2, nens // 2


def base_fields(config, rng):
    """about 40 % cloudy cells, half of them liquid and half ice, and vertical velocities of both signs"""
    nz, ny, nx, nens = config
    shp = (nz, ny, nx, nens)
    cloudy = rng.uniform(size=shp) < 0.4
    icy = rng.uniform(size=shp) < 0.5
    return {"rho_d": 1.1 * np.exp(-np.arange(nz)[:, None, None, None] / 8.0) * rng.uniform(0.95, 1.05, shp),
            "rho_v": 1.0e-2 * rng.uniform(0.3, 1.7, shp),
            "rho_c": np.where(cloudy & ~icy, 1.0e-4 * rng.uniform(0.3, 1.0, shp), 0.0),
            "rho_i": np.where(cloudy & icy, 6.0e-5 * rng.uniform(0.5, 1.0, shp), 0.0),
            "temp": 290.0 - 6.0 * np.arange(nz)[:, None, None, None] + rng.normal(0.0, 1.5, shp),
            "uvel": rng.normal(5.0, 2.0, shp), "vvel": rng.normal(-1.0, 2.0, shp),
            "wvel": rng.normal(0.2, 1.0, shp) + np.where(cloudy, 0.5, 0.0)}


def _negative_variance_speed(f, qc):
    """uvel = 0 at a level's first cell and a elsewhere, a^2 a few subnormal units: d d and A A are then rounded to whole units, and for
    some a the one rounds down and the other up.  -> the first such a (searched on the restatement) with B - A A of two units or more below
    zero -- half of it times a factor of 1 is then still below zero in tke --, failing that the first with B - A A < 0, or None (one
    column: every d is 0)"""
    nz = f["rho_d"].shape[0]
    for bound in (-2 * TINY, -TINY):
        for j in range(1, 65):
            a = float(np.sqrt(j * TINY))
            u = np.full(f["uvel"].shape, a)
            u[:, 0, 0, :] = 0.0
            g = dict(f, uvel=u)
            for k in range(nz):
                pre = {}
                level_values(g, k, qc, preclamp=pre)
                if (pre["uvel"] <= bound).any():
                    return a
    return None


def cases(config):
    """name -> case, built once per shape and shared (nobody writes to them: every backend copies what it changes)"""
    if config in _CACHE:
        return _CACHE[config]
    nz, ny, nx, nens = config
    rng = np.random.default_rng(23 + 1000 * nz + 100 * ny + 10 * nx + nens)
    f = base_fields(config, rng)
    shp = f["temp"].shape
    sk, sj, si, se = special(config)

    def start(fields, fill=None):
        has_cond = fields.get("rho_c") is not None or fields.get("rho_i") is not None
        return {x: (None if (x in SAMPLED and not has_cond) else (rng.normal(0.0, 1.0, (nz, nens)) if fill is None else np.full((nz, nens), fill)))
                for x in OUT}

    def case(fields, out0=None, steps=None, factor=FACTOR, fill=0.0):
        return dict(qc=QC, steps=steps or [(fields, factor)], out0=out0 or start(fields, fill))

    def changed(**kw):
        g = dict(f)
        g.update(kw)
        return g

    def poke(a, value, where=None):
        a = a.copy()
        a[where or (sk, sj, si, se)] = value
        return a

    out = {"base": case(f)}
    out["all_clear"] = case(changed(rho_c=np.zeros(shp), rho_i=np.zeros(shp)))
    out["all_cloudy"] = case(changed(rho_c=np.full(shp, 1.0e-3)))
    # level sk of member se: liquid exactly at (one ulp above) the threshold in every cell, no ice
    thr = QC * (f["rho_d"] + f["rho_v"])
    for name, value in (("at_threshold", thr), ("ulp_above_threshold", np.nextafter(thr, np.inf))):
        c, i = f["rho_c"].copy(), f["rho_i"].copy()
        c[sk, :, :, se], i[sk, :, :, se] = value[sk, :, :, se], 0.0
        out[name] = case(changed(rho_c=c, rho_i=i))
    # level sk of member se: w is 0.0 and -0.0 in turn, so m is a zero of either sign and no cell is up; the special cell's infinite density
    # makes its m a NaN, which shows in whose sum the cell lands
    w = f["wvel"].copy()
    w[sk, :, :, se] = np.where(np.arange(ny * nx).reshape(ny, nx) % 2 == 0, 0.0, -0.0)
    out["w_zero"] = case(changed(wvel=w, rho_d=poke(f["rho_d"], np.inf)))
    out["nan_w"] = case(changed(wvel=poke(f["wvel"], np.nan)))
    out["nan_rho_c"] = case(changed(rho_c=poke(f["rho_c"], np.nan)))
    out["nan_temp"] = case(changed(temp=poke(f["temp"], np.nan)))
    const = {n: np.broadcast_to(a[:, :1, :1, :], shp).copy() for n, a in f.items()}
    const["rho_c"] = np.broadcast_to((2.0e-4 * ((np.arange(nz)[:, None] + np.arange(nens)[None, :]) % 2))[:, None, None, :], shp).copy()
    out["constant_level"] = case(const)
    a = _negative_variance_speed(f, QC)
    NEGATIVE_FOUND[config] = a is not None
    u = np.full(shp, a if a is not None else float(np.sqrt(2 * TINY)))
    u[:, 0, 0, :] = 0.0
    # vvel and wvel constant on every level, so that tke is half of uvel's variance alone, and a factor of 1
    out["var_rounds_negative"] = case(changed(uvel=u, vvel=const["vvel"], wvel=const["wvel"]), factor=1.0)
    for has_c, has_i in CONDENSATE:
        g = changed(**({} if has_c else {"rho_c": None}), **({} if has_i else {"rho_i": None}))
        out["c%d_i%d" % (int(has_c), int(has_i))] = case(g)
    out["factor_third"] = case(f, factor=1.0 / 3.0, out0=start(f))
    g2 = changed(wvel=f["wvel"] * -0.7, rho_c=f["rho_c"] * 0.5, temp=f["temp"] + 1.0)
    out["two_steps"] = case(f, out0=start(f), steps=[(f, FACTOR * 3.0), (g2, FACTOR)])
    nzf = {n: np.full(shp, 1.0 if n == "rho_d" else -0.0) for n in FIELDS}
    out["neg_zero"] = case(nzf, fill=-0.0)
    assert tuple(out) == CASE_NAMES
    _CACHE[config] = out
    return out


def reference(config, name):
    """the restatement's result of a named case, computed once and shared"""
    key = (config, name)
    if key not in _REF:
        _REF[key] = run_case(RefBackend(), cases(config)[name])
    return _REF[key]
