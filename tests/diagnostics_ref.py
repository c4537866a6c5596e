"""The field diagnostics (pam_amd_field_diagnostics, include/pam_amd_modules.h) restated in numpy, and the cases of its tests.

The sum is a CONTRACT, not "some sum": fold(v; W, K) below is the tree of the header, written with elementwise adds only (never np.sum,
whose pairwise order is numpy's own).  Whole field: W = 256, K = 8 over the flat index.  Per member: W = 4, K = 64 over the row index of
x[r*M + m], each member on its own.  The extremes: the least / greatest element that is no NaN, the lowest flat index among elements
that compare equal, and that element's own bits."""
import functools
import math

import numpy as np

FIELD_W, FIELD_K = 256, 8
MEMBER_W, MEMBER_K = 4, 64
KIND_DTYPES = [np.float64, np.float32]


def levels(n, W, K):
    """levels fold() takes for n entries"""
    out = 1
    n = -(-n // (W * K))
    while n > 1:
        n = -(-n // (W * K))
        out += 1
    return out


def fold(v, W, K):
    """v: (n, cols) float64, the columns independent.  Returns (cols,)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            n, cols = v.shape
            chunks = -(-n // (W * K))
            padded = np.full((chunks * W * K, cols), -0.0)          # a missing entry is -0.0, the identity of IEEE addition
            padded[:n] = v
            steps = padded.reshape(chunks, K, W, cols)              # entry e of a chunk: lane e % W, step e // W
            lane = steps[:, 0].copy()
            for s in range(1, K):                                   # a lane adds its K entries in ascending step order
                lane = lane + steps[:, s]
            d = W // 2
            while d >= 1:                                           # for d = W/2 .. 1: lane[l] += lane[l + d]
                lane[:, :d] = lane[:, :d] + lane[:, d:2 * d]
                d //= 2
            v = lane[:, 0]
            if chunks == 1:
                return v[0]


def tree_sum(a, members=0):
    a = np.asarray(a).reshape(-1).astype(np.float64)                # float32 -> float64 is exact
    if members == 0:
        return fold(a.reshape(-1, 1), FIELD_W, FIELD_K)[0]
    return fold(a.reshape(-1, members), MEMBER_W, MEMBER_K)


def diagnose(a, members=0):
    """dict of vmin, vmax, vsum (float64), argmin, argmax, nan_count (int64): scalars for members = 0, arrays of (members,) otherwise"""
    flat = np.asarray(a).reshape(-1)
    M = max(members, 1)
    x = flat.reshape(-1, M)
    nan = np.isnan(x)
    lo = np.where(nan, np.inf, x).min(axis=0)
    hi = np.where(nan, -np.inf, x).max(axis=0)
    rmin, rmax = (x == lo).argmax(axis=0), (x == hi).argmax(axis=0)          # the first row that compares equal; a NaN never does
    cols = np.arange(M)
    some = ~nan.all(axis=0)
    out = {
        "vmin": np.where(some, x[rmin, cols].astype(np.float64), np.inf),    # that element's own bits (-0.0 stays -0.0)
        "vmax": np.where(some, x[rmax, cols].astype(np.float64), -np.inf),
        "argmin": np.where(some, rmin * M + cols, -1).astype(np.int64),
        "argmax": np.where(some, rmax * M + cols, -1).astype(np.int64),
        "nan_count": nan.sum(axis=0).astype(np.int64),
        "vsum": np.atleast_1d(tree_sum(flat, members)),
    }
    return {k: v[0] for k, v in out.items()} if members == 0 else out


KEYS = ("vmin", "vmax", "vsum", "argmin", "argmax", "nan_count")

MEMBER_GROUP, EXTREME_BYTES, RESULT_BYTES = 4, 40, 48


def member_plan_bytes(sizes, members):
    """bytes of scratch a per-member call (members >= 1) of fields of these sizes plans: per field the level buffers of its sums and
    one extreme per (group of MEMBER_GROUP row chunks, member), every region 16-byte aligned, then one result per (field, member)
    (plan_field of diagnostics_device.h and the entry point's own sum over the list)"""
    chunk, at = MEMBER_W * MEMBER_K, 0
    for size in sizes:
        n1 = -(-(size // members) // chunk)
        entries, n = n1, n1
        while n > 1:
            n = -(-n // chunk)
            entries += n
        at = -(-(at + entries * members * 8) // 16) * 16
        at = -(-(at + -(-n1 // MEMBER_GROUP) * members * EXTREME_BYTES) // 16) * 16
    return at + len(sizes) * members * RESULT_BYTES


def bits(d):
    """a result as comparable bytes: the bit patterns of the values, except that every NaN sum is one NaN"""
    vsum = np.where(np.isnan(d["vsum"]), np.nan, d["vsum"])
    return b"".join(np.ascontiguousarray(np.asarray(v, dtype=t)).tobytes() for v, t in (
        (d["vmin"], np.float64), (d["vmax"], np.float64), (vsum, np.float64), (d["argmin"], np.int64), (d["argmax"], np.int64),
        (d["nan_count"], np.int64)))


def fold_members(d, M):
    """the whole-field extremes and NaN count from the per-member results, by the lexicographic (value, index) comparison"""
    out = {"nan_count": np.int64(d["nan_count"].sum())}
    for v, i, sign in (("vmin", "argmin", 1.0), ("vmax", "argmax", -1.0)):
        have = d[i] >= 0
        if not have.any():
            out[v], out[i] = np.float64(sign * np.inf), np.int64(-1)
            continue
        best = None
        for m in np.flatnonzero(have):
            key = (sign * d[v][m], d[i][m])
            if best is None or key < best[0]:
                best = (key, m)
        out[v], out[i] = d[v][best[1]], d[i][best[1]]
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the cases

FIELD_SIZES = [1, 2, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 3, 2048 ** 2 - 1, 2048 ** 2, 2048 ** 2 + 1]
MEMBER_SHAPES = [(1, 1), (1, 3), (255, 5), (256, 64), (257, 65), (513, 130), (65537, 2)]
BIG = 3.0e6                      # beyond every mixed value: |normal| * 10^[-3, 4)
SMALL_CASE = 3 * 2048            # up to here every planting; above, the two that reach the ends


def mixed(rng, n):
    """magnitudes over seven decades, both signs"""
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 4.0, n)


def _spots(rows):
    """first, head, middle, tail and last rows"""
    return sorted({0, 1, 3, rows // 2, rows - 4, rows - 2, rows - 1} & set(range(rows)))


def _plantings(rng, rows, M, every):
    """[(label, (rows, M) float64)]: the extremes planted at the spots -- the minimum twice, so that the lowest index must win --
    and the special values"""
    out = []
    spots = _spots(rows)
    picks = range(len(spots)) if every else (0, len(spots) - 1)
    for k in picks:
        a = mixed(rng, rows * M).reshape(rows, M)
        lo, again, hi = spots[k], spots[(k + 2) % len(spots)], spots[(k + 3) % len(spots)]
        a[lo] = -BIG
        a[again] = -BIG                        # the minimum a second time (a lower or a higher row: the lowest index wins)
        if hi not in (lo, again):
            a[hi] = BIG
            a[hi, ::2] = 2 * BIG              # the members differ in where their maximum is
            if rows > 1:
                a[(hi + 1) % rows, ::2] = np.where(a[(hi + 1) % rows, ::2] == -BIG, -BIG, BIG)
        out.append(("min_at%d" % lo, a))
    if every:
        a = np.zeros((rows, M))
        a[spots[len(spots) // 2]] = -0.0       # -0.0 beside +0.0: equal, so index 0 wins with ITS bits
        out.append(("zeros", a))
        a = np.zeros((rows, M))
        a[0] = -0.0
        out.append(("negzero_first", a))
        out.append(("all_negzero", np.full((rows, M), -0.0)))          # the sum keeps a lone -0.0
        a = mixed(rng, rows * M).reshape(rows, M)
        a[spots[0]] = np.nan
        a[spots[-1], ::2] = np.nan
        a[spots[len(spots) // 2], 0] = np.inf
        out.append(("nan_and_inf", a))
        a = mixed(rng, rows * M).reshape(rows, M)
        a[spots[-1]] = -np.inf
        out.append(("minus_inf", a))
        a = np.full((rows, M), np.nan)
        a[spots[-1], 0] = np.inf               # every element a NaN but one +inf: it is the minimum AND the maximum
        out.append(("nan_but_one_inf", a))
        a = mixed(rng, rows * M).reshape(rows, M)
        a[spots[0]] = np.inf
        a[spots[-1]] = -np.inf                 # inf - inf: the sum is a NaN
        out.append(("inf_minus_inf", a))
        out.append(("all_nan", np.full((rows, M), np.nan)))
    return out


@functools.lru_cache(maxsize=None)
def field_cases(kind):
    """[(label, 1-d array of the kind's dtype)]; never modified after this"""
    rng = np.random.default_rng(4100 + kind)
    out = []
    for n in FIELD_SIZES:
        for label, a in _plantings(rng, n, 1, n <= SMALL_CASE):
            out.append(("n%d_%s" % (n, label), a.reshape(-1).astype(KIND_DTYPES[kind])))
    for _, a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def member_cases(kind):
    """[(label, 1-d array, M)]"""
    rng = np.random.default_rng(4200 + kind)
    out = []
    for rows, M in MEMBER_SHAPES:
        for label, a in _plantings(rng, rows, M, rows * M <= 70000):
            out.append(("r%d_m%d_%s" % (rows, M, label), a.reshape(-1).astype(KIND_DTYPES[kind]), M))
    for _, a, _ in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def field_expected(kind):
    return [diagnose(a, 0) for _, a in field_cases(kind)]


@functools.lru_cache(maxsize=None)
def member_expected(kind):
    return [diagnose(a, M) for _, a, M in member_cases(kind)]


def gamma(n, W, K):
    """the bound of a summation tree of depth D on |error| / sum|x|: every element passes through D adds"""
    D = levels(n, W, K) * (K - 1 + int(math.log2(W)))
    u = 2.0 ** -53
    return D * u / (1.0 - D * u)
