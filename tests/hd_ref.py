"""Horizontal hyperdiffusion: the numpy restatement of the contract (include/pam_amd_modules.h), the named cases
and the mutants of the restatement.  TEST INFRASTRUCTURE ONLY.

The method is not part of the reference tree, so this restatement is the yardstick, and the device bodies (pam_amd/csrc/hd_device.h,
under g++ in tests/emu/hd_emu.cpp and under hipcc in modules_kernels.hip) are held to it bit for bit.  It is out of place: every
neighbour is a np.roll of the field as it was before the call.  numpy's element-wise float64 arithmetic is IEEE and never contracted;
the fill's sums are written out as loops over cells and slots (msa_ref.level_sum), so no numpy reduction takes part.

Fields are (nz, ny, nx, nens), members fastest.  A mutant is a deliberately wrong variant of ONE line of the restatement, switched on
by name; each must be caught by at least one named case (tests/test_hd.py)."""
from fractions import Fraction

import numpy as np

import msa_ref

MUTANTS = ("wrap_off_by_one", "inplace_x", "inplace_y", "stencil_form", "update_fma", "y_plus_x", "fill_clean_level", "slots_descending")

# (nz, ny, nx, nens): every nx, nz and nens with ny == 1 and with ny > 1, every ny.  The last three reuse the slots of the row ring
# (rows 2 .. ny-3 pass through six slots: ny = 11 wraps it once, 13 and 32 leave a ring length that is no multiple of six); the last two
# have a tail member block and more than 256 cells of a row per block (32 x 17 and 16 x 32)
SHAPES = ((1, 1, 5, 1), (3, 1, 6, 3), (1, 1, 7, 64), (3, 1, 8, 65), (1, 1, 16, 130), (3, 1, 17, 3), (1, 1, 33, 65),
          (1, 5, 5, 3), (3, 6, 6, 1), (1, 9, 7, 64), (3, 5, 8, 65), (1, 6, 16, 130), (3, 9, 17, 3), (1, 5, 33, 65), (3, 6, 8, 130),
          (1, 11, 6, 3), (2, 13, 17, 65), (1, 32, 32, 37))
DT, TAU = 20.0, 60.0


def shape_id(shape):
    return "%dx%dx%d-e%d" % shape


def coefficient(dt, tau):
    return dt / (16.0 * tau)


def _shift(f, s, axis, mutant=None):
    """f[i + s] along the axis, indices modulo n"""
    if mutant == "wrap_off_by_one" and s > 0:
        n = f.shape[axis]
        i = np.arange(n) + s
        return np.take(f, np.where(i >= n, (i - n + 1) % n, i), axis=axis)
    return np.roll(f, -s, axis=axis)


def d4(f, axis, mutant=None):
    """the fourth difference along one axis from the four first differences, every operation rounded separately"""
    m2, m1, p1, p2 = (_shift(f, s, axis, mutant) for s in (-2, -1, 1, 2))
    if mutant == "stencil_form":
        return (((m2 - 4.0 * m1) + 6.0 * f) - 4.0 * p1) + p2
    e1 = m1 - m2
    e2 = f - m1
    e3 = p1 - f
    e4 = p2 - p1
    return (e4 - e1) - 3.0 * (e3 - e2)


def _d4_in_place(f, axis, c, other):
    """the hazard: a walk along the axis that reads its neighbours from the field it is writing (other: the other axis' D4, original)"""
    g = np.moveaxis(f.copy(), axis, 0)
    o = None if other is None else np.moveaxis(other, axis, 0)
    n = g.shape[0]
    for i in range(n):
        m2, m1, v, p1, p2 = g[(i - 2) % n], g[(i - 1) % n], g[i], g[(i + 1) % n], g[(i + 2) % n]
        D = ((p2 - p1) - (m1 - m2)) - 3.0 * ((p1 - v) - (v - m1))
        if o is not None:
            D = D + o[i] if axis == 2 else o[i] + D
        g[i] = v - c * D
    return np.moveaxis(g, 0, axis)


def update(f, c, mutant=None):
    """f_new = f - c D4 of one field, before any fill"""
    with np.errstate(invalid="ignore", over="ignore"):
        with_y = f.shape[1] > 1
        if mutant == "inplace_x":
            return _d4_in_place(f, 2, c, d4(f, 1) if with_y else None)
        if mutant == "inplace_y" and with_y:
            return _d4_in_place(f, 1, c, d4(f, 2))
        D = d4(f, 2, mutant)
        if with_y:
            D = (d4(f, 1, mutant) + D) if mutant == "y_plus_x" else (D + d4(f, 1, mutant))
        if mutant == "update_fma":          # f - c D4 with ONE rounding
            flat = [float(Fraction(a) - Fraction(c) * Fraction(b)) if np.isfinite(a) and np.isfinite(b) else a - c * b
                    for a, b in zip(f.ravel().tolist(), D.ravel().tolist())]
            return np.array(flat).reshape(f.shape)
        return f - c * D


def fill_levels(fn, mutant=None):
    """-> P, N, mode (nz,nens) of a field (nz,ny,nx,nens): cell c = j nx + i in slot c % 16"""
    nz, ny, nx, nens = fn.shape
    flat = fn.reshape(nz, ny * nx, nens)
    m = "slots_descending" if mutant == "slots_descending" else None
    P = msa_ref.level_sum(np.where(flat > 0, flat, 0.0), mutant=m)
    N = msa_ref.level_sum(np.where(flat < 0, flat, 0.0), mutant=m)
    with np.errstate(invalid="ignore"):
        mode = np.where(~(N < 0), 0, np.where(P + N > 0, 1, 2))
    return P, N, mode


def fill(fn, mutant=None):
    """the level fill of mean-state acceleration with no increment: a clean (level, member) keeps its bits"""
    P, N, mode = fill_levels(fn, mutant)
    with np.errstate(invalid="ignore", divide="ignore"):
        factor = 1.0 + N / P
        filled = np.where(fn > 0, fn, 0.0) * factor[:, None, None, :]
    m = mode[:, None, None, :]
    clean = filled if mutant == "fill_clean_level" else fn      # the mutant fills a clean level too: -0.0 loses its sign, 0/0 appears
    return np.where(m == 0, clean, np.where(m == 1, filled, 0.0))


def hyperdiffusion(fields, positive, dt, tau, mutant=None):
    """-> the new fields (every array new)"""
    c = coefficient(dt, tau)
    out = []
    for f, pos in zip(fields, positive):
        fn = update(f, c, mutant)
        out.append(fill(fn, mutant) if pos else fn)
    return out


class RefBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def run(self, fields, positive, dt, tau):
        return hyperdiffusion(fields, positive, dt, tau, self.mutant)


def run_case(backend, case):
    return backend.run(case["fields"], case["positive"], case["dt"], case["tau"])


def same_bits(a, b, nan_by_place=False):
    """the same bits in every cell.  nan_by_place, for a comparison across hardware only: a NaN must stand where a NaN stands, but its
    sign and payload are not compared -- IEEE 754 leaves them to the implementation (a subtraction carried out as an add of the negated
    operand returns the NaN with its sign flipped: the MI355X gives 0xfff8... in some cells of a stencil where x86 gives 0x7ff8...), so
    they are no part of the contract.  The emulation runs the restatement's own arithmetic and is held to every bit."""
    if a.shape != b.shape:
        return False
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if not nan_by_place:
        return np.array_equal(a.view(np.uint64), b.view(np.uint64))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def results_differ(x, y, nan_by_place=False):
    """indices of the fields that differ bitwise between two results"""
    assert len(x) == len(y)
    return [i for i, (a, b) in enumerate(zip(x, y)) if not same_bits(a, b, nan_by_place)]


# ---- the named cases.  Three fields: temp (about 300 K, perturbations of 1e-3), a wind of mixed sign, a flagged tracer
FIELD_NAMES = ("temp", "wind", "tracer")
POSITIVE = (0, 0, 1)
CASE_NAMES = ("base", "spike", "edge", "all_negative", "constant", "checkerboard_x", "checkerboard_xy", "nan_cell", "neg_zero",
              "no_positive_fields", "dt_equals_tau")
_CACHE = {}


def _smooth(shape, rng):
    nz, ny, nx, nens = shape
    k = np.arange(nz)[:, None, None, None]
    j = np.arange(ny)[None, :, None, None]
    i = np.arange(nx)[None, None, :, None]
    e = np.arange(nens)[None, None, None, :]
    wave = np.sin(2 * np.pi * i / nx + 0.3 * e) * np.cos(2 * np.pi * j / ny + 0.1 * k)
    temp = 300.0 - 6.5 * k + 1.0e-3 * wave + 1.0e-3 * rng.normal(0.0, 1.0, shape)
    wind = 10.0 * wave + rng.normal(0.0, 1.0, shape) * 10.0 ** rng.uniform(-3, 1, shape)
    tracer = 1.0e-2 * np.exp(-0.4 * k) * (1.0 + 0.2 * wave) * rng.uniform(0.9, 1.1, shape)
    return [temp, wind, tracer]


def cases(shape):
    """name -> case, built once per shape and shared (nobody writes to them: every backend copies what it changes)"""
    if shape in _CACHE:
        return _CACHE[shape]
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(100000 * nz + 1000 * ny + 10 * nx + nens)
    base = _smooth(shape, rng)
    k = np.arange(nz)[:, None, None, None]
    j = np.arange(ny)[None, :, None, None]
    i = np.arange(nx)[None, None, :, None]
    e = np.arange(nens)[None, None, None, :]

    def case(fields, **kw):
        c = dict(fields=fields, positive=list(POSITIVE), dt=DT, tau=TAU)
        c.update(kw)
        return c

    out = {"base": case(base)}
    spike = np.zeros(shape)
    spike[:, ny // 2, nx // 2, :] = 1.0e-3 * rng.uniform(0.5, 1.5, (nz, nens))
    out["spike"] = case([base[0], base[1], spike])
    edge = np.where((i + np.zeros(shape)) < (nx + 1) // 2, 1.0e-3 * rng.uniform(0.9, 1.1, shape), 0.0)
    out["edge"] = case([base[0], base[1], edge])
    neg = base[2].copy()
    neg[0] = -1.0e-5 * rng.uniform(0.1, 1.0, (ny, nx, nens))
    out["all_negative"] = case([base[0], base[1], neg])
    const = [b[:, :1, :1, :] + np.zeros(shape) for b in base]
    out["constant"] = case(const)
    amp = 2.0 ** ((k + e) % 7 - 3) + np.zeros(shape)
    cx = amp * (1.0 - 2.0 * ((i + np.zeros(shape)) % 2))
    out["checkerboard_x"] = case([cx, -cx, cx], positive=[0, 0, 0], dt=TAU)
    cxy = amp * (1.0 - 2.0 * ((i + j + np.zeros(shape)) % 2))
    out["checkerboard_xy"] = case([cxy, -cxy, cxy], positive=[0, 0, 0], dt=TAU)
    nan = [b.copy() for b in (base[0], base[1], spike)]
    for f in nan:
        f[nz // 2, ny // 2, nx // 2, nens // 2] = np.nan
    out["nan_cell"] = case(nan)
    nz0 = base[2].copy()
    nz0[0] = -0.0
    nz0[-1, :, : nx // 2, :] = -0.0
    out["neg_zero"] = case([base[0], base[1], nz0])
    out["no_positive_fields"] = case([base[0], base[1], spike], positive=[0, 0, 0])
    out["dt_equals_tau"] = case([base[0], base[1], edge], dt=TAU)
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
