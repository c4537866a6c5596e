"""CRM mean-state acceleration: the numpy restatement of the contract (include/pam_amd_modules.h), the named
cases and the mutants of the restatement.  TEST INFRASTRUCTURE ONLY.

The method is not part of the reference tree, so this restatement is the yardstick, and the device bodies (pam_amd/csrc/msa_device.h,
under g++ in tests/emu/msa_emu.cpp and under hipcc in modules_kernels.hip) are held to it bit for bit.  numpy's element-wise float64
arithmetic is IEEE and never contracted; every sum below is written out as a loop over cells and slots, so no numpy reduction (pairwise
order) takes part.

Fields are (nz, ncol, nens), members fastest.  A mutant is a deliberately wrong variant of ONE line of the restatement, switched on
by name; each must be caught by at least one named case (tests/test_msa.py)."""
import numpy as np

NS = 16
QUANTITIES = ("t", "q", "u", "v")
FIELDS = ("temp", "water_vapor", "cloud", "ice", "uvel", "vvel")
MUTANTS = ("slots_descending", "scale_after_sum", "cease_ge", "cloud_incremented", "factor_minus")

NENS = (1, 3, 64, 65, 130)
GRIDS = ((4, 1, 5), (5, 1, 17), (3, 4, 5), (6, 8, 8), (2, 32, 32))      # (nz, ny, nx): empty slots, 16k+1, uneven slots, even, C2's ncol
SHAPES = [(g, n) for g in GRIDS for n in NENS]


def shape_id(shape):
    (nz, ny, nx), nens = shape
    return "%dx%dx%d-e%d" % (nz, ny, nx, nens)


def level_sum(f, r=None, mutant=None):
    """S(f)(k,e) (r None) or M(f)(k,e) (r = 1/ncol): cell c belongs to slot c % 16; a slot adds its cells in ascending c from 0.0, every
    product f r rounded before it is added; the 16 slot sums are added in ascending slot order from 0.0."""
    nz, ncol, nens = f.shape
    scale_in = r is not None and mutant != "scale_after_sum"
    parts = np.zeros((NS, nz, nens))
    for c in range(ncol):
        term = f[:, c, :] * r if scale_in else f[:, c, :]
        parts[c % NS] = parts[c % NS] + term
    tot = np.zeros((nz, nens))
    for s in (range(NS - 1, -1, -1) if mutant == "slots_descending" else range(NS)):
        tot = tot + parts[s]
    if r is not None and mutant == "scale_after_sum":
        tot = tot * r
    return tot


def level_mean(f, mutant=None):
    return level_sum(f, 1.0 / f.shape[1], mutant)


def quantity(st, x):
    """T, q = water_vapor + cloud + ice (left to right, an absent species skipped), U, V"""
    if x == "t":
        return st["temp"]
    if x == "u":
        return st["uvel"]
    if x == "v":
        return st["vvel"]
    q = st["water_vapor"]
    if st.get("cloud") is not None:
        q = q + st["cloud"]
    if st.get("ice") is not None:
        q = q + st["ice"]
    return q


def diagnose(st, mutant=None):
    return {x: level_mean(quantity(st, x), mutant) for x in QUANTITIES}


def tendencies(st, save, max_ttend, cease, mutant=None):
    """-> (tend, cease): the flag is sticky (left alone where nothing ceases)"""
    tend = {x: level_mean(quantity(st, x), mutant) - save[x] for x in QUANTITIES}
    with np.errstate(invalid="ignore"):
        a = np.abs(tend["t"])
        within = (a < max_ttend) if mutant == "cease_ge" else (a <= max_ttend)
    if not within.all():
        cease = 1
    return tend, cease


def vapor_levels(vp):
    """-> P, N, mode (nz,nens): 0 no negative value, 1 filled by 1 + N/P, 2 zeroed"""
    P = level_sum(np.where(vp > 0, vp, 0.0))
    N = level_sum(np.where(vp < 0, vp, 0.0))
    with np.errstate(invalid="ignore"):
        mode = np.where(~(N < 0), 0, np.where(P + N > 0, 1, 2))
    return P, N, mode


def apply(st, tend, a, accel_uv, cease, mutant=None):
    """-> the new state (every array a copy; an array the call does not write is returned with the same bits)"""
    out = {k: (None if v is None else v.copy()) for k, v in st.items()}
    if a == 0 or cease:
        return out
    d = {x: a * tend[x] for x in QUANTITIES}
    out["temp"] = st["temp"] + d["t"][:, None, :]
    if accel_uv:
        out["uvel"] = st["uvel"] + d["u"][:, None, :]
        out["vvel"] = st["vvel"] + d["v"][:, None, :]
    vp = st["water_vapor"] + d["q"][:, None, :]
    P, N, mode = vapor_levels(vp)
    with np.errstate(invalid="ignore", divide="ignore"):
        factor = (1.0 - N / P) if mutant == "factor_minus" else (1.0 + N / P)
        filled = np.where(vp > 0, vp, 0.0) * factor[:, None, :]
    m = mode[:, None, :]
    out["water_vapor"] = np.where(m == 0, vp, np.where(m == 1, filled, 0.0))
    if mutant == "cloud_incremented" and st.get("cloud") is not None:
        out["cloud"] = st["cloud"] + d["q"][:, None, :]
    return out


class RefBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def diagnose(self, st):
        return diagnose(st, self.mutant)

    def tendencies(self, st, save, max_ttend, cease):
        return tendencies(st, save, max_ttend, cease, self.mutant)

    def apply(self, st, tend, a, accel_uv, cease):
        return apply(st, tend, a, accel_uv, cease, self.mutant)


def run_case(backend, case):
    """diagnose on the state at the start of the step, tendencies and apply on the state at its end"""
    save = backend.diagnose(case["before"])
    tend, cease = backend.tendencies(case["after"], save, case["max_ttend"], case["cease_in"])
    fields = backend.apply(case["after"], tend, case["a"], case["accel_uv"], cease)
    return dict(save=save, tend=tend, cease=int(cease), fields=fields)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def results_differ(x, y):
    """names of what differs bitwise between two results of run_case"""
    bad = ["save_" + q for q in QUANTITIES if not same_bits(x["save"][q], y["save"][q])]
    bad += ["tend_" + q for q in QUANTITIES if not same_bits(x["tend"][q], y["tend"][q])]
    if x["cease"] != y["cease"]:
        bad.append("cease")
    for f in FIELDS:
        a, b = x["fields"].get(f), y["fields"].get(f)
        if (a is None) != (b is None) or (a is not None and not same_bits(a, b)):
            bad.append(f)
    return bad


# ---- the named cases
VAPOR_SCALE = (0.8, 0.3, 1.05)      # of level (k + e) % 3 over the step: filled by 1 + N/P, zeroed (P + N <= 0), no negative value


def _states(shape):
    """the state at the start and at the end of a CRM step: mixed-sign winds of wide range, a temperature change of about 1 K per
    level and member, vapour that dries by a factor set per (level, member) so that every branch of the hole filling is reached"""
    (nz, ny, nx), nens = shape
    ncol = ny * nx
    rng = np.random.default_rng(1000 * nz + 10 * ncol + nens)
    k = np.arange(nz)[:, None, None]
    e = np.arange(nens)[None, None, :]
    before = {
        "temp": 300.0 - 6.5 * k + rng.normal(0.0, 1.5, (nz, ncol, nens)),
        "water_vapor": 1.0e-2 * np.exp(-0.4 * k) * rng.uniform(0.3, 1.7, (nz, ncol, nens)),
        "cloud": 1.0e-4 * rng.uniform(0.0, 1.0, (nz, ncol, nens)) * (rng.uniform(size=(nz, ncol, nens)) < 0.4),
        "ice": 3.0e-5 * rng.uniform(0.0, 1.0, (nz, ncol, nens)) * (rng.uniform(size=(nz, ncol, nens)) < 0.3),
        "uvel": rng.normal(0.0, 1.0, (nz, ncol, nens)) * 10.0 ** rng.uniform(-3, 1.5, (nz, ncol, nens)),
        "vvel": rng.normal(0.0, 1.0, (nz, ncol, nens)) * 10.0 ** rng.uniform(-3, 1.5, (nz, ncol, nens)),
    }
    before["water_vapor"][:, 0, :] *= 0.01          # one nearly dry cell per level: it goes negative wherever the level dries
    scale = np.asarray(VAPOR_SCALE)[(k + e) % 3]
    after = {
        "temp": before["temp"] + rng.uniform(-1.0, 1.0, (nz, 1, nens)) + rng.normal(0.0, 0.2, (nz, ncol, nens)),
        "water_vapor": before["water_vapor"] * scale,
        "cloud": before["cloud"] * rng.uniform(0.5, 1.5, (nz, ncol, nens)),
        "ice": before["ice"] * rng.uniform(0.5, 1.5, (nz, ncol, nens)),
        "uvel": before["uvel"] + rng.normal(0.0, 0.3, (nz, ncol, nens)),
        "vvel": before["vvel"] + rng.normal(0.0, 0.3, (nz, ncol, nens)),
    }
    return before, after


CASE_NAMES = ("base", "ttend_equal", "ttend_one_ulp_above", "nan_in_temp", "no_cloud", "no_ice", "vapour_only", "accel_uv_off",
              "flag_already_set", "accel_factor_zero", "accel_factor_one")
_CACHE = {}


def cases(shape):
    """name -> case, built once per shape and shared (nobody writes to them: every backend copies what it changes)"""
    if shape in _CACHE:
        return _CACHE[shape]
    before, after = _states(shape)

    def case(**kw):
        c = dict(before=before, after=after, a=2.0, accel_uv=True, max_ttend=5.0, cease_in=0)
        c.update(kw)
        return c

    def without(st, *names):
        return {k: (None if k in names else v) for k, v in st.items()}

    out = {"base": case()}
    base_tend, _ = tendencies(after, diagnose(before), 5.0, 0)
    top = float(np.abs(base_tend["t"]).max())
    out["ttend_equal"] = case(max_ttend=top)                                   # |tend_T| == max_ttend somewhere: must not cease
    out["ttend_one_ulp_above"] = case(max_ttend=float(np.nextafter(top, 0.0)))  # that tendency is one ulp above: must cease
    nan_after = dict(after)
    nan_after["temp"] = after["temp"].copy()
    nan_after["temp"][after["temp"].shape[0] // 2, after["temp"].shape[1] // 2, shape[1] // 2] = np.nan
    out["nan_in_temp"] = case(after=nan_after)
    out["no_cloud"] = case(before=without(before, "cloud"), after=without(after, "cloud"))
    out["no_ice"] = case(before=without(before, "ice"), after=without(after, "ice"))
    out["vapour_only"] = case(before=without(before, "cloud", "ice"), after=without(after, "cloud", "ice"))
    out["accel_uv_off"] = case(accel_uv=False)
    out["flag_already_set"] = case(cease_in=1)
    out["accel_factor_zero"] = case(a=0.0)
    out["accel_factor_one"] = case(a=1.0)
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
