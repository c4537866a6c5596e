"""CRM variance transport: the numpy restatement of the contract (include/pam_amd_modules.h), the named cases and
the mutants of the restatement.  TEST INFRASTRUCTURE ONLY.

The method is not part of the reference tree, so this restatement is the yardstick, and the device bodies (pam_amd/csrc/vt_device.h,
under g++ in tests/emu/vt_emu.cpp and under hipcc in modules_kernels.hip) are held to it bit for bit.  numpy's element-wise float64
arithmetic is IEEE and never contracted (np.sqrt and / are correctly rounded); every sum below is written out as a loop over cells and
slots, so no numpy reduction (pairwise order) takes part.

Fields are (nz, ncol, nens), members fastest.  A mutant is a deliberately wrong variant of ONE line of the restatement, switched on
by name; each must be caught by at least one named case (tests/test_vt.py)."""
from fractions import Fraction

import numpy as np

import msa_ref

NS = 16
QUANTITIES = ("t", "q", "u")
FIELDS = ("temp", "water_vapor", "cloud", "ice", "uvel")
MUTANTS = ("slots_descending", "unshifted", "var_fma", "mean_form", "clamp_before_root", "cloud_incremented", "feedback_reciprocal")

NENS = (1, 3, 64, 65, 130)
# (nz, ny, nx): empty slots, 16k+1, uneven slots, even, C2's ncol, and the single column
GRIDS = ((4, 1, 5), (5, 1, 17), (3, 4, 5), (6, 8, 8), (2, 32, 32), (2, 1, 1))
SHAPES = [(g, n) for g in GRIDS for n in NENS]
LIMIT = 0.05


def shape_id(shape):
    (nz, ny, nx), nens = shape
    return "%dx%dx%d-e%d" % (nz, ny, nx, nens)


def quantities(use_u):
    return QUANTITIES if use_u else QUANTITIES[:2]


def quantity(st, x):
    """T, q = water_vapor + cloud + ice (left to right, an absent species skipped), U"""
    return msa_ref.quantity(st, x)


def level_stats(x, mutant=None):
    """-> mean, var (nz,nens) of x (nz,ncol,nens): ONE pass, shifted by the level's first cell"""
    nz, ncol, nens = x.shape
    r = 1.0 / ncol
    c = np.zeros((nz, nens)) if mutant == "unshifted" else x[:, 0, :]
    pa, pb = np.zeros((NS, nz, nens)), np.zeros((NS, nz, nens))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(ncol):
            d = x[:, i, :] - c
            pa[i % NS] = pa[i % NS] + d * r
            pb[i % NS] = pb[i % NS] + (d * d) * r
        A, B = np.zeros((nz, nens)), np.zeros((nz, nens))
        for s in (range(NS - 1, -1, -1) if mutant == "slots_descending" else range(NS)):
            A = A + pa[s]
            B = B + pb[s]
        mean = c + A
        if mutant == "var_fma":         # B - A A with ONE rounding
            v = np.array([[float(Fraction(b) - Fraction(a) * Fraction(a)) if np.isfinite(a) and np.isfinite(b) else b - a * a
                           for a, b in zip(ra, rb)] for ra, rb in zip(A.tolist(), B.tolist())]).reshape(nz, nens)
        else:
            v = B - A * A
        var = np.where(v < 0, 0.0, v)
    return mean, var


def diagnose(st, use_u, mutant=None):
    out = {x: level_stats(quantity(st, x), mutant) for x in quantities(use_u)}
    return {x: m for x, (m, _) in out.items()}, {x: v for x, (_, v) in out.items()}


def scale_of(var, tend, dt, lim, mutant=None):
    with np.errstate(all="ignore"):
        ratio = 1.0 + (dt * tend) / var
        lo, hi = 1.0 - lim, 1.0 + lim
        if mutant == "clamp_before_root":
            s = np.sqrt(np.where(ratio < lo, lo, np.where(ratio > hi, hi, ratio)))
        else:
            root = np.sqrt(np.where(ratio > 0, ratio, 0.0))
            s = np.where(root < lo, lo, np.where(root > hi, hi, root))
        return np.where(~(var > 0) | np.isnan(ratio), 1.0, s)


def forcing(st, use_u, tend, dt, lim, mutant=None):
    mean, var = diagnose(st, use_u, mutant)
    return mean, var, {x: scale_of(var[x], tend[x], dt, lim, mutant) for x in quantities(use_u)}


def vapor_levels(vp, on):
    """P, N, mode (nz,nens) of the stretched vapour; levels with on == False add nothing and are clean"""
    return msa_ref.vapor_levels(np.where(on[:, None, :], vp, 0.0))


def apply(st, use_u, mean, scale, mutant=None):
    """-> the new state (every array a copy; an array the call does not write is returned with the same bits)"""
    out = {k: (None if v is None else v.copy()) for k, v in st.items()}
    with np.errstate(all="ignore"):
        for x, name in (("t", "temp"), ("u", "uvel")):
            if x == "u" and not use_u:
                continue
            g, m = (scale[x] - 1.0)[:, None, :], mean[x][:, None, :]
            new = m + scale[x][:, None, :] * (st[name] - m) if mutant == "mean_form" else st[name] + g * (st[name] - m)
            out[name] = np.where(g != 0, new, st[name])
        g = scale["q"] - 1.0
        d = g[:, None, :] * (quantity(st, "q") - mean["q"][:, None, :])
        vp = st["water_vapor"] + d
        P, N, mode = vapor_levels(vp, g != 0)
        filled = np.where(vp > 0, vp, 0.0) * (1.0 + N / P)[:, None, :]
        m = mode[:, None, :]
        new = np.where(m == 0, vp, np.where(m == 1, filled, 0.0))
        out["water_vapor"] = np.where((g != 0)[:, None, :], new, st["water_vapor"])
        if mutant == "cloud_incremented" and st.get("cloud") is not None:
            out["cloud"] = st["cloud"] + np.where((g != 0)[:, None, :], d, 0.0)
    return out


def feedback(st, use_u, var_start, gcm_dt, mutant=None):
    mean, var = diagnose(st, use_u, mutant)
    with np.errstate(all="ignore"):
        if mutant == "feedback_reciprocal":
            fb = {x: (var[x] - var_start[x]) * (1.0 / gcm_dt) for x in quantities(use_u)}
        else:
            fb = {x: (var[x] - var_start[x]) / gcm_dt for x in quantities(use_u)}
    return mean, var, fb


class RefBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def diagnose(self, st, use_u):
        return diagnose(st, use_u, self.mutant)

    def forcing(self, st, use_u, tend, dt, lim):
        return forcing(st, use_u, tend, dt, lim, self.mutant)

    def apply(self, st, use_u, mean, scale):
        return apply(st, use_u, mean, scale, self.mutant)

    def feedback(self, st, use_u, var_start, gcm_dt):
        return feedback(st, use_u, var_start, gcm_dt, self.mutant)


def run_case(backend, case, scale_from=None):
    """a GCM step of one CRM step: diagnose on the state at the start, forcing and apply on the state after the CRM's modules, feedback
    on what the apply left.  scale_from: a result whose scale table the apply is fed in place of this backend's own"""
    u = case["use_u"]
    start_mean, var_start = backend.diagnose(case["start"], u)
    mean, var, scale = backend.forcing(case["now"], u, case["tend"], case["dt"], case["lim"])
    fields = backend.apply(case["now"], u, mean, scale if scale_from is None else scale_from["scale"])
    end_mean, end_var, fb = backend.feedback(fields, u, var_start, case["gcm_dt"])
    return dict(start_mean=start_mean, var_start=var_start, mean=mean, var=var, scale=scale, fields=fields, end_mean=end_mean,
                end_var=end_var, feedback=fb)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


TABLES = ("start_mean", "var_start", "mean", "var", "scale", "end_mean", "end_var", "feedback")


def results_differ(x, y, tables=TABLES):
    """names of what differs bitwise between two results of run_case"""
    bad = []
    for t in tables:
        if set(x[t]) != set(y[t]):
            bad.append(t)
            continue
        bad += [t + "_" + q for q in x[t] if not same_bits(x[t][q], y[t][q])]
    for f in FIELDS:
        a, b = x["fields"].get(f), y["fields"].get(f)
        if (a is None) != (b is None) or (a is not None and not same_bits(a, b)):
            bad.append(f)
    return bad


# ---- the named cases
def _states(shape):
    """the state vt_init sees and the state after a CRM step's modules.  The spread is drawn per (level, member), not per field:
    temperatures near 300 K with sigma from 0.01 to 3 K, log-normal moisture, mixed-sign winds about a mean of either sign"""
    (nz, ny, nx), nens = shape
    ncol = ny * nx
    rng = np.random.default_rng(7000 + 1000 * nz + 10 * ncol + nens)
    k = np.arange(nz)[:, None, None]
    full, lev = (nz, ncol, nens), (nz, 1, nens)
    sig_t = 10.0 ** rng.uniform(-2.0, 0.5, lev)
    sig_q = rng.uniform(0.05, 0.5, lev)
    sig_u = 10.0 ** rng.uniform(-2.0, 1.0, lev)
    start = {
        "temp": 300.0 - 6.5 * k + sig_t * rng.normal(0.0, 1.0, full),
        "water_vapor": 1.0e-2 * np.exp(-0.4 * k) * np.exp(sig_q * rng.normal(0.0, 1.0, full)),
        "cloud": 1.0e-4 * rng.uniform(0.0, 1.0, full) * (rng.uniform(size=full) < 0.4),
        "ice": 3.0e-5 * rng.uniform(0.0, 1.0, full) * (rng.uniform(size=full) < 0.3),
        "uvel": 5.0 * rng.normal(0.0, 1.0, lev) + sig_u * rng.normal(0.0, 1.0, full),
    }
    now = {
        "temp": start["temp"] + rng.uniform(-1.0, 1.0, lev) + 0.3 * sig_t * rng.normal(0.0, 1.0, full),
        "water_vapor": start["water_vapor"] * np.exp(0.3 * sig_q * rng.normal(0.0, 1.0, full)),
        "cloud": start["cloud"] * rng.uniform(0.5, 1.5, full),
        "ice": start["ice"] * rng.uniform(0.5, 1.5, full),
        "uvel": start["uvel"] + 0.3 * sig_u * rng.normal(0.0, 1.0, full),
    }
    return start, now, rng


CASE_NAMES = ("base", "clamp_low", "clamp_high", "ratio_negative", "tend_zero", "tend_nan", "tend_inf", "zero_variance_level",
              "nan_in_temp", "outlier_cell0", "dry_cells", "no_cloud", "no_ice", "vapour_only", "use_u_off")
DRY_KIND = ("filled", "zeroed", "clean")      # of level (k + e) % 3 in dry_cells
_CACHE = {}


def _tend(st, rate, dt, use_u=True):
    """the tendency that makes ratio = 1 + rate (up to rounding): rate var / dt"""
    _, var = diagnose(st, use_u)
    return {x: rate * var[x] / dt for x in var}


def cases(shape):
    """name -> case, built once per shape and shared (nobody writes to them: every backend copies what it changes)"""
    if shape in _CACHE:
        return _CACHE[shape]
    (nz, ny, nx), nens = shape
    ncol = ny * nx
    start, now, rng = _states(shape)
    dt, gcm_dt = 20.0, 240.0
    # both signs, scales strictly inside the clamp: sqrt(1 +- 0.08) lies in (0.959, 1.040)
    rate = rng.uniform(0.02, 0.08, (nz, nens)) * np.where(rng.uniform(size=(nz, nens)) < 0.5, -1.0, 1.0)

    def case(**kw):
        c = dict(start=start, now=now, use_u=True, dt=dt, gcm_dt=gcm_dt, lim=LIMIT)
        c.update(kw)
        if "tend" not in c:
            c["tend"] = _tend(c["now"], c.pop("rate", rate), dt, c["use_u"])
        return c

    def without(st, *names):
        return {k: (None if k in names else v) for k, v in st.items()}

    def changed(st, **kw):
        out = dict(st)
        out.update(kw)
        return out

    out = {"base": case()}
    base_tend = out["base"]["tend"]
    out["clamp_low"] = case(rate=-0.5)
    out["clamp_high"] = case(rate=0.5)
    out["ratio_negative"] = case(rate=-3.0)
    out["tend_zero"] = case(tend={x: np.zeros((nz, nens)) for x in QUANTITIES})
    kk, ee = nz // 2, nens // 2
    t_nan = {x: v.copy() for x, v in base_tend.items()}
    for x in QUANTITIES:
        t_nan[x][kk, ee] = np.nan
    out["tend_nan"] = case(tend=t_nan)
    t_inf = {x: v.copy() for x, v in base_tend.items()}
    for x in QUANTITIES:
        t_inf[x][0, 0] = np.inf
        t_inf[x][nz - 1, nens - 1] = -np.inf
    out["tend_inf"] = case(tend=t_inf)
    flat = now["temp"].copy()
    flat[0] = flat[0, :1, :]                       # level 0 is constant in every member
    out["zero_variance_level"] = case(now=changed(now, temp=flat), tend=base_tend)
    nan_t = now["temp"].copy()
    nan_t[kk, ncol // 2, ee] = np.nan
    out["nan_in_temp"] = case(now=changed(now, temp=nan_t), tend=base_tend)
    far = now["temp"].copy()
    if ncol > 1:                                                            # cell 0 ten sigma of the other cells above their mean
        far[:, 0, :] = far[:, 1:, :].mean(axis=1) + 10.0 * far[:, 1:, :].std(axis=1)
    out["outlier_cell0"] = case(now=changed(now, temp=far), start=changed(start, temp=far))
    # vapour below 5 % of a moist level's mean under the amplifying scale 1 + lim: v' = 1.05 v - 0.05 mean_q < 0.  Levels of kind
    # "filled" get a few such cells, levels of kind "zeroed" hold (unphysical) slightly negative vapour throughout, so that P + N <= 0
    dry = now["water_vapor"].copy()
    kind = (np.arange(nz)[:, None] + np.arange(nens)[None, :]) % 3
    dry[:, ::3, :] = np.where((kind == 0)[:, None, :], 0.001 * dry[:, ::3, :], dry[:, ::3, :])
    dry = np.where((kind == 1)[:, None, :], -1.0e-4 * dry, dry)
    out["dry_cells"] = case(now=changed(now, water_vapor=dry), rate=0.5)
    out["no_cloud"] = case(start=without(start, "cloud"), now=without(now, "cloud"))
    out["no_ice"] = case(start=without(start, "ice"), now=without(now, "ice"))
    out["vapour_only"] = case(start=without(start, "cloud", "ice"), now=without(now, "cloud", "ice"))
    out["use_u_off"] = case(start=without(start, "uvel"), now=without(now, "uvel"), use_u=False,
                            tend={x: base_tend[x] for x in QUANTITIES[:2]})
    assert tuple(out) == CASE_NAMES
    _CACHE[shape] = out
    return out


_REF = {}


def reference(shape, name):
    """the restatement's result of a named case, computed once and shared"""
    key = (shape, name)
    if key not in _REF:
        _REF[key] = run_case(RefBackend(), cases(shape)[name])
    return _REF[key]
