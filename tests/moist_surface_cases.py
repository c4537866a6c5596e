"""Named cases, state builders, gates and mutants for saturation_adjustment and surface_friction_init / compute_surface_friction cell by
cell (tests/test_moist_surface_cells.py; tests/test_moist_surface_modules.py and tests/p3_cases.py use the gates).  The float64
restatement and its mutants are in tests/moist_surface_ref.py.  TEST INFRASTRUCTURE ONLY.

Saturation adjustment: bit equality
-----------------------------------
In compute_adjusted_state the only operation that is not IEEE basic arithmetic is exp, and its value is used only in the comparisons
pv > svp and pv_loc > svp_loc.  Wherever the device's exp and glibc's take the same decisions, rho_v, rho_c and temp equal the float64
restatement in every bit.  The restatement records each cell's smallest relative decision margin |pv - svp| / svp; two exps of about an
ulp each differ by some 1e-16 relative, so a cell whose margin is >= MARGIN = 1e-12 is held to equality and only a cell below it keeps
the allowance of one flipped decision (2 tol in density, the matching dT).  Every committed state has a smallest margin >= MIN_MARGIN
= 1e-10 (a CPU test asserts it from the restatement alone), so no cell of a GPU test is exempt.

Surface friction: a per-cell gate in units of the cell's own scale
-------------------------------------------------------------------
The reference is surface_friction.h on the double inputs, evaluated in binary128 (tests/emu/moist_surface_quad_emu.cpp) and rounded
once to np.longdouble (friction_reference, z0_reference), with the np.longdouble restatement beside it (friction_reference_ld,
z0_reference_ld).  The level-0 means are NOT part of it: they are the float64 slot-order means the kernels form with IEEE operations only (product rounded, cell c in
slot c % 16, slots added in ascending order from 0.0) and are handed to the reference as exact inputs -- a wrong mean on the device is
a wrong flux in every cell of the member, and the gate need not cover the freedom of a summation order.  One unit of a flux is

    2^-53 (|u| + |u_mean|) / wnd  rho_mean ustar^2  |rho_sfc| / dz        (v likewise; wnd, ustar, rho_sfc the reference's)

and one unit of z0 is 2^-53 z0.  E_FLUX and E_Z0 are the worst errors, in units, of the float64 restatement at the same means over
every committed friction state (test_the_restatement_is_within_E_of_the_longdouble_reference measures them); the device is gated at
G = 4 E: its log / atan / exp are allowed 1 to 2 ulp where glibc stays under 1, and they enter through the same eight-iteration
recurrence as the restatement's own roundings.
"""
import collections
import ctypes as C
import functools
import math
import os

import numpy as np

import moist_surface_ref as ref
from pam_amd import idealized as idz
from tools.native_build import emu_library

R_V, CP_D, CP_V = 461.0, 1003.0, 1859.0            # the Kessler scheme's constants (pam_amd/micro.py)
TRACER_SETS = {"kessler": idz.TRACERS_KESSLER_SHOC, "p3": idz.TRACERS_P3_SHOC}
CONDENSATE = {"kessler": "cloud_liquid", "p3": "cloud_water"}
ADJUSTED = ("rho_v", "rho_c", "temp")
MARGIN = 1e-12          # below it a last-place difference of exp may flip a decision of the bisection
MIN_MARGIN = 1e-10      # the smallest margin a committed state may have
OLD_GATE = 1e-12        # the gate these tests replace: of the field's largest value
LD = np.longdouble
U = 2.0 ** -53
_DP = C.POINTER(C.c_double)


def same_bits(a, b):
    """NaN in the same places, every other element equal bit for bit (the signs of zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(np.where(np.isnan(a), 0.0, a).view(np.uint64), np.where(np.isnan(b), 0.0, b).view(np.uint64))


def differing(a, b):
    """mask of the elements same_bits would object to"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return (na != nb) | (np.where(na, 0.0, a).view(np.uint64) != np.where(nb, 0.0, b).view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------------------
# the host emulation of the device bodies (pam_amd/csrc/moist_surface_device.h under g++)

@functools.lru_cache(maxsize=None)
def emu():
    lib = C.CDLL(emu_library("moist_surface_emu"))
    lib.emu_saturation_adjustment.argtypes = [C.c_longlong, C.c_int] + [_DP] * 5 + [C.c_double] * 4 + [C.POINTER(C.c_int)]
    lib.emu_saturation_max_iter.restype = C.c_int
    lib.emu_surface_friction_z0.argtypes = [C.c_int] + [_DP] * 7
    lib.emu_surface_friction_cell.argtypes = [C.c_longlong] + [_DP] * 14
    return lib


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def emu_adjust(rho_d, massy, rv, rc, temp):
    """the device loop on the host, massy in the order given: (rho_v, rho_c, temp, iterations) as new flat arrays"""
    rho_d = np.ascontiguousarray(rho_d, dtype=np.float64).ravel()
    m = np.ascontiguousarray(np.stack([np.asarray(x).ravel() for x in massy])) if massy else np.zeros((1, rho_d.size))
    out = [np.array(np.asarray(x).ravel(), dtype=np.float64) for x in (rv, rc, temp)]
    it = np.zeros(rho_d.size, dtype=np.int32)
    emu().emu_saturation_adjustment(rho_d.size, len(massy), _p(rho_d), _p(m), _p(out[0]), _p(out[1]), _p(out[2]), R_V, CP_D, CP_V,
                                    ref.CP_L, it.ctypes.data_as(C.POINTER(C.c_int)))
    return out[0], out[1], out[2], it


def emu_saturation_adjustment(lib, f, tracers, micro):
    """the device loop on the host for a coupler state: returns (rho_v, rho_c, temp, iterations) as flat arrays"""
    return emu_adjust(f["density_dry"], [f[n] for n, _, m in tracers if m], f["water_vapor"], f[CONDENSATE[micro]], f["temp"])


# ------------------------------------------------------------------------------------------------------------------------------
# saturation adjustment: states

def moist_state(tracers, nens, nx, ny, nz, seed=0):
    """(nz,ny,nx,nens) fields whose cells are, at random, super-saturated (condensation), unsaturated with plenty of cloud (partial
    evaporation), unsaturated with a trace of cloud (complete evaporation) or unsaturated without cloud (untouched)"""
    rng = np.random.default_rng(seed)
    shape = (nz, ny, nx, nens)
    f = {"density_dry": 1.1 * np.exp(-np.arange(nz) / 20.0)[:, None, None, None] * (1 + 0.02 * rng.random(shape)),
         "temp": 250.0 + 50.0 * rng.random(shape)}
    tc = f["temp"] - 273.15
    rvs = 610.94 * np.exp(17.625 * tc / (243.04 + tc)) / (R_V * f["temp"])
    kind = rng.integers(0, 4, shape)
    ratio = np.choose(kind, [rng.uniform(1.02, 1.3, shape), rng.uniform(0.85, 0.99, shape), rng.uniform(0.3, 0.6, shape),
                             rng.uniform(0.5, 0.95, shape)])
    cloud = np.choose(kind, [rng.uniform(0, 1e-3, shape), rng.uniform(2e-2, 3e-2, shape), rng.uniform(1e-7, 1e-5, shape),
                             np.zeros(shape)])
    cond = {"kessler": "cloud_liquid", "p3": "cloud_water"}
    for name, _, mass in tracers:
        if name == "water_vapor":
            f[name] = rvs * ratio
        elif name in cond.values():
            f[name] = cloud
        elif mass:
            f[name] = rng.uniform(0, 1e-3, shape)
        else:
            f[name] = rng.uniform(1e5, 1e7, shape)       # number concentrations, tke: do not add mass
    for k in f:
        f[k] = np.ascontiguousarray(f[k], dtype=np.float64)
    return f


MODULE_SHAPES = [(70, 5, 4, 4), (3, 3, 2, 5), (1, 6, 1, 4)]   # (nens, nx, ny, nz): ragged nens with nx*ny >= 16, nx*ny < 16, one member
MODULE_SHAPE_IDS = ["ragged_nens_16cols", "small", "one_member"]
CELLS_SHAPE = (70, 5, 4, 4)                                   # of specials and massy_*: 22 workgroups of 256 cells, the last ragged
SatCase = collections.namedtuple("SatCase", "name via micro shape")
SATURATION = [SatCase("%s_%s" % (m, i), "module", m, s) for m in ("kessler", "p3") for s, i in zip(MODULE_SHAPES, MODULE_SHAPE_IDS)] + \
    [SatCase(m + "_order", "module", m, CELLS_SHAPE) for m in ("kessler", "p3")] + \
    [SatCase(n, "capi", None, CELLS_SHAPE) for n in ("specials", "massy_0", "massy_1", "massy_55")]
SATURATION_BY_NAME = {c.name: c for c in SATURATION}
SATURATION_IDS = [c.name for c in SATURATION]
MODULE_IDS = [c.name for c in SATURATION if c.via == "module"]
ORDER_IDS = [n for n in MODULE_IDS if n.endswith("_order")]     # the module path's own proof of the registration order
CAPI_IDS = [c.name for c in SATURATION if c.via == "capi"]
_WATER = [("water_vapor", True, True), ("cloud_liquid", True, True)]


def _saturation_density(temp):
    tc = temp - 273.15
    return 610.94 * np.exp(17.625 * tc / (243.04 + tc)) / (R_V * temp)


def specials_state():
    """a normal state with chosen cells overwritten, every special cell among ordinary ones of its wavefront.  Returns (rho_d, rv, rc,
    temp, names): names maps the flat index of a special cell to what it is.  rho = rho_d + rv + rc."""
    nens, nx, ny, nz = CELLS_SHAPE
    f = moist_state(_WATER, nens, nx, ny, nz, seed=41)
    rd, rv, rc, t = (f[k].reshape(-1) for k in ("density_dry", "water_vapor", "cloud_liquid", "temp"))
    nan, inf = math.nan, math.inf
    S = lambda temp, ratio: float(_saturation_density(np.float64(temp)) * ratio)        # vapour at `ratio` of saturation
    cells = [   # (what, rho_v, rho_c, temp)
        ("nan_rho_v", nan, 1e-3, 280.0),
        ("nan_rho_c_subsaturated", S(280.0, 0.7), nan, 280.0),            # NaN > 0 is false: untouched
        ("nan_rho_c_supersaturated", S(280.0, 1.2), nan, 280.0),          # condenses; the cloud and the temperature stay NaN
        ("nan_temp", 5e-3, 1e-3, nan),
        ("negative_zero_cloud_subsaturated", S(285.0, 0.8), -0.0, 285.0),  # -0.0 > 0 is false: untouched, the sign kept
        ("negative_zero_cloud_supersaturated", S(285.0, 1.1), -0.0, 285.0),
        ("negative_cloud_subsaturated", S(275.0, 0.8), -2e-4, 275.0),
        ("negative_cloud_supersaturated", S(275.0, 1.25), -2e-4, 275.0),   # max(0, rho_c + x) clamps while x < 2e-4
        ("negative_cloud_below_what_condenses", S(275.0, 1.02), -1e-2, 275.0),
        ("negative_vapour_with_cloud", -1e-4, 5e-3, 290.0),                # max(0, rho_v + x) clamps while x < 1e-4
        ("negative_vapour_without_cloud", -1e-4, 0.0, 290.0),
        ("evaporation_bracket_2tol", S(290.0, 0.5), 2e-6, 290.0),          # one iteration, exactly half
        ("evaporation_bracket_tol", S(290.0, 0.5), 1e-6, 290.0),
        ("evaporation_bracket_above_2tol", S(290.0, 0.5), 2.5e-6, 290.0),  # two iterations
        ("evaporation_bracket_1e-10", S(290.0, 0.5), 1e-10, 290.0),        # an adjustment of 5e-11
        ("evaporation_bracket_1e-13", S(300.0, 0.4), 1e-13, 300.0),
        ("condensation_bracket_tol_cold", 1e-6, 0.0, 180.0),               # saturation at 180 K is 1.3e-7
        ("condensation_bracket_2tol_cold", 2e-6, 1e-4, 182.0),
        ("condensation_bracket_above_2tol_cold", 3e-6, 0.0, 185.0),
        ("vapour_1e3", 1e3, 0.0, 290.0), ("vapour_1e6", 1e6, 1e-3, 270.0), ("vapour_1e9", 1e9, 0.0, 300.0),
        ("cloud_1e3", S(290.0, 0.5), 1e3, 290.0), ("cloud_1e6", S(270.0, 0.9), 1e6, 270.0), ("cloud_1e9", S(300.0, 0.2), 1e9, 300.0),
        ("inf_rho_v", inf, 1e-3, 290.0),                                   # ends at the 2048 cap
        ("inf_rho_c", S(290.0, 0.5), inf, 290.0),                          # likewise
    ]
    names = {}
    for k, (what, v, c, temp) in enumerate(cells):
        # spread over the workgroups of 256 cells, never two in one wavefront; the two cells that end at the cap lie in the ragged last
        # workgroup (cells 5376 .. 5599), one of them in its half-filled last wavefront
        i = {"inf_rho_v": 5400, "inf_rho_c": 5590}.get(what, 19 + 197 * k + (k % 5))
        assert i < rv.size and i not in names
        rv[i], rc[i], t[i] = v, c, temp
        names[i] = what
    return rd, rv, rc, t, names


def order_state(micro):
    """a coupler state in which the order of rho = rho_d + (the tracers that add mass, as registered) shows: thin air and cells far from
    saturation as in massy_55, the other tracers that add mass up to 1e-2.  With the three tracers of kessler the reversed order changes
    the bits of temp in 18 of 4137 adjusted cells, with the four of p3 in 21 (in none at the states of the three module shapes)."""
    tr = TRACER_SETS[micro]
    nens, nx, ny, nz = CELLS_SHAPE
    f = moist_state(tr, nens, nx, ny, nz, seed=77)
    cn = CONDENSATE[micro]
    f["density_dry"] = np.ascontiguousarray(0.15 * f["density_dry"])
    rv, rc = f["water_vapor"], f[cn]
    f["water_vapor"] = np.ascontiguousarray(np.where(rv > _saturation_density(f["temp"]), 4.0 * rv, np.where(rc > 1e-2, 0.25 * rv, rv)))
    for n, _, m in tr:
        if m and n not in ("water_vapor", cn):
            f[n] = np.ascontiguousarray(10.0 * f[n])
    return f


def massy_state(n):
    """(rho_d, rv, rc, temp, massy): massy lists n arrays in the order they are summed.  n = 55: the vapour at position 17, the
    condensate at 41, the other 53 of magnitudes spread log-uniformly over 1e-9 .. 1e-2 -- in thin air, 0.15 of the other states'
    dry density, and far from saturation: the super-saturated cells hold four times the vapour of the other states, the cloudy ones a
    quarter.  The order of the sum shows in the last places of rho in one cell of seven, and from there in temp only where the
    temperature change x Lv / (rho cp) is large enough for 1e-16 of it to move a rounding of temp (an ulp of 280 K is 5.7e-14): with
    changes of 10 K at the median the reversed list changes the bits of temp in 93 of 4111 adjusted cells; with the moisture and the
    density of the other states (changes of 0.6 K) in 2."""
    nens, nx, ny, nz = CELLS_SHAPE
    f = moist_state(_WATER, nens, nx, ny, nz, seed=50 + n)
    rd, rv, rc, t = (f[k].reshape(-1) for k in ("density_dry", "water_vapor", "cloud_liquid", "temp"))
    if n == 0:
        return rd, rv, rc, t, []
    if n == 1:
        # 24 of the trace clouds are 1e-14 .. 4e-14: their complete evaporation moves rho_c by half of that, below 1e-12 of the field's
        # largest value (3e-14), and temp by 1e-10 of a kelvin at most
        trace = np.flatnonzero((rc > 0) & (rc < 1e-5))[:24]
        rc[trace] = 1e-14 * (1 + np.arange(24) % 4)
        return rd, rv, rc, t, [rv]
    rng = np.random.default_rng(5500 + n)
    rd = np.ascontiguousarray(0.15 * rd)
    rv = np.ascontiguousarray(np.where(rv > _saturation_density(t), 4.0 * rv, np.where(rc > 1e-2, 0.25 * rv, rv)))
    mag = 10.0 ** rng.permutation(np.linspace(-9.0, -2.0, n - 2))
    others = [np.ascontiguousarray(m * rng.uniform(0.5, 1.5, rd.size)) for m in mag]
    massy = others[:17] + [rv] + others[17:40] + [rc] + others[40:]
    assert len(massy) == n and massy[17] is rv and massy[41] is rc
    return rd, rv, rc, t, massy


def _restate_cells(rd, massy, rv, rc, t, skip=None, mutant=None):
    """the restatement on flat arrays; the cells of `skip` (those that end at the iteration cap, where it raises) are left out.
    Returns ((rho_v, rho_c, temp), info)"""
    keep = np.ones(rd.size, bool) if skip is None else ~skip
    out = {"water_vapor": np.array(rv[keep]), "cond": np.array(rc[keep]), "temp": np.array(t[keep])}
    o, part = ref.adjust_cells(out, np.ascontiguousarray(rd[keep]), [np.ascontiguousarray(m[keep]) for m in massy], "cond", R_V, CP_D, CP_V,
                               ref.CP_L, mutant)
    res = [np.array(rv), np.array(rc), np.array(t)]
    for a, k in zip(res, ("water_vapor", "cond", "temp")):
        a[keep] = o[k]
    info = {"branch": np.zeros(rd.size, np.int8), "iters": np.zeros(rd.size, np.int32), "margin": np.full(rd.size, np.inf),
            "amount": np.zeros(rd.size)}
    for k in info:
        info[k][keep] = part[k]
    return dict(zip(ADJUSTED, res)), info


@functools.lru_cache(maxsize=None)
def saturation_case(name):
    """computed once per session and never written to: the state (fields and tracers for a module case; rho_d, before, massy for every
    case), the expected state `want` and the restatement's `info`"""
    c = SATURATION_BY_NAME[name]
    nens, nx, ny, nz = c.shape
    d = dict(case=c, capped=None, special=None)
    if c.via == "module":
        tr = TRACER_SETS[c.micro]
        f = order_state(c.micro) if name.endswith("_order") else moist_state(tr, nens, nx, ny, nz, seed=10 + nens)
        d.update(fields=f, tracers=tr)
        rd, rv, rc, t = (f[k].reshape(-1) for k in ("density_dry", "water_vapor", CONDENSATE[c.micro], "temp"))
        massy = [f[n].reshape(-1) for n, _, m in tr if m]
    elif name == "specials":
        rd, rv, rc, t, special = specials_state()
        massy = [rv, rc]
        d["special"] = special
        d["capped"] = np.isinf(rv) | np.isinf(rc)
    else:
        rd, rv, rc, t, massy = massy_state(int(name.split("_")[1]))
    want, info = _restate_cells(rd, massy, rv, rc, t, skip=d["capped"])
    if d["capped"] is not None:
        # the restatement raises at the cap: these cells come from the host emulation (the restatement bit for bit on every other
        # cell: test_the_emulation_is_the_restatement_bit_for_bit).  Their decisions compare inf and NaN: no last place takes part.
        e = emu_adjust(rd, massy, rv, rc, t)
        for k, a in zip(ADJUSTED, e[:3]):
            want[k][d["capped"]] = a[d["capped"]]
        info["iters"][d["capped"]] = e[3][d["capped"]]
        info["branch"][d["capped"]] = np.where(np.isinf(rv), 1, 2)[d["capped"]]
    d.update(rho_d=rd, massy=massy, before=dict(zip(ADJUSTED, (rv, rc, t))), want=want, info=info)
    for a in [rd, rv, rc, t] + list(massy) + list(want.values()) + list(info.values()):
        a.setflags(write=False)
    return d


def saturation_mutant(name, mutant):
    """(rho_v, rho_c, temp) of the restatement with one deliberate error, on a committed case"""
    d = saturation_case(name)
    got, _ = _restate_cells(d["rho_d"], d["massy"], *[d["before"][k] for k in ADJUSTED], skip=d["capped"], mutant=mutant)
    if d["capped"] is not None:
        for k in ADJUSTED:
            got[k][d["capped"]] = d["want"][k][d["capped"]]
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# saturation adjustment: gates

def _allowance(k, rho_min):
    """what one flipped decision may move: 2 tol in density; Lv / (rho cp) bounds the temperature change per unit of density moved"""
    return 2 * ref.TOL if k != "temp" else 2 * ref.TOL * 2.6e6 / (rho_min * CP_D)


def assert_adjusted_bits(got, want, info, before, rho_min=0.05):
    """got, want, before: dicts of rho_v, rho_c, temp (any shape); info: the restatement's.  A cell in neither branch equals `before` bit
    for bit (NaNs and the signs of zeros included); an adjusted cell with a decision margin >= MARGIN equals `want` bit for bit; an
    adjusted cell below MARGIN keeps the allowance of one flipped decision.  Returns the number of cells below MARGIN."""
    branch, margin = np.asarray(info["branch"]).reshape(-1), np.asarray(info["margin"]).reshape(-1)
    none = branch == 0
    exempt = (~none) & (margin < MARGIN)
    held = (~none) & (~exempt)
    for k in ADJUSTED:
        g, w, b = (np.asarray(x[k]).reshape(-1) for x in (got, want, before))
        bad = differing(g[none], b[none])
        assert not bad.any(), "%s: %d cells in neither branch were written, the first at %d" % (k, bad.sum(), np.flatnonzero(none)[bad][0])
        bad = differing(g[held], w[held])
        if bad.any():
            i = np.flatnonzero(held)[bad][0]
            raise AssertionError("%s: %d of %d adjusted cells differ from the restatement, the first at %d: %r against %r (margin %.3g)"
                                 % (k, bad.sum(), held.sum(), i, g[i], w[i], margin[i]))
        assert np.all(np.abs(g[exempt] - w[exempt]) <= _allowance(k, rho_min)), k
    return int(exempt.sum())


def old_gate_accepts(got, want, info):
    """the gate this one replaces: 1e-12 of the field's largest value on every cell with a margin >= 1e-12 (no cap on the others)"""
    keep = np.asarray(info["margin"]).reshape(-1) >= MARGIN
    for k in ADJUSTED:
        g, w = np.asarray(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1)
        with np.errstate(invalid="ignore"):
            if not np.all(np.abs(g[keep] - w[keep]) <= OLD_GATE * np.abs(w).max()):
                return False
    return True


# ------------------------------------------------------------------------------------------------------------------------------
# surface friction: states

FrictionCase = collections.namedtuple("FrictionCase", "name nens nx ny")
FRICTION = [
    FrictionCase("ragged", 70, 5, 4),               # 64 + 6 members, one chunk, every slot used
    FrictionCase("few_columns", 3, 3, 2),           # fewer columns than the 16 slots, a block of 3 x 16 threads
    FrictionCase("one_member", 1, 6, 1),
    FrictionCase("three_chunks", 5, 12, 12),        # 144 columns in three chunks of 48
    FrictionCase("uneven_chunks", 5, 13, 5),        # 65 columns in chunks of 33 and 32
    FrictionCase("capped_chunks", 70, 3277, 5),     # 16385 columns, two member blocks: 256 chunks of 65, chunk 252 holds 5, 253-255 none
]
FRICTION_BY_NAME = {c.name: c for c in FRICTION}
FRICTION_IDS = [c.name for c in FRICTION]
SMALL_FRICTION_IDS = [c.name for c in FRICTION if c.nx * c.ny * c.nens < 10000]     # the ones the scalar Python restatement can walk
NZ = 3
DENORMAL = 5e-324


def chunks(nens, ncol):
    """the launch arithmetic of pam_amd_surface_friction_compute: (member blocks, column chunks, columns per chunk)"""
    ME = nens if nens < 64 else 64                  # slot_block_shape
    nblk = (nens + ME - 1) // ME
    nchunk = (512 + nblk - 1) // nblk               # ~512 workgroups in all
    nchunk = min(nchunk, (ncol + 63) // 64)         # each chunk at least 64 columns
    nchunk = max(nchunk, 1)
    return nblk, nchunk, (ncol + nchunk - 1) // nchunk


def last_chunk_start(nens, ncol):
    """the first column of the last chunk that holds any"""
    chunk = chunks(nens, ncol)[2]
    return (ncol - 1) // chunk * chunk


def friction_state(nens, nx, ny, seed=0, zero_mean_u="some"):
    """the inputs of both entry points, nz = 3.  Per member: z0 log-uniform in [1e-5, 1] with both ends present, tau log-uniform in
    [1e-3, 0.5] with the smallest on the last members, bflx zero for a third of the members and of mixed sign in the others, its own
    interface heights.  Level-0 winds: a member mean plus perturbations of 1e-4 .. 10, so that u - u_mean spans decades.  In the
    members of `zero_mean_u` ("some": e % 4 == 1 and e >= 64; "all") the mean of u is zero but for rounding: the perturbations come in
    pairs c, c + ncol/2 of opposite sign.  Calm cells (|u|, |v| << 1: the wind clamp) are every fifth column of the first half, their
    partners, and the partners of the last chunk's columns: in a zero-mean member their |u| + |u_mean| is 1e-4 of the member's
    typical wind, which is where an error of the mean shows.
    Conditioning: with a positive buoyancy flux above some 0.002 and a wind below 1.5 m/s the eight iterations of diag_ustar do not
    settle (ustar oscillates), and a rounding grows to several hundred ulps of ustar^2 in the worst of a million cells.  So every
    second member with a positive flux carries a strong one (0.005 .. 0.05) and a v of 4 .. 6 m/s in every cell, the calm ones too
    (their u stays small); the others a weak one (2e-4 .. 2e-3) and the full range of winds.  Negative and zero fluxes need no care."""
    rng = np.random.default_rng([seed, nens, nx, ny])
    ncol = nx * ny
    e = np.arange(nens)
    shp = (NZ, ncol, nens)
    half = ncol // 2
    d = {"rho_d": 1.1 * np.exp(-np.arange(NZ) / 20.0)[:, None, None] * (1 + 0.02 * rng.random(shp)),
         "rho_v": rng.uniform(0.005, 0.015, shp)}
    zero = np.ones(nens, bool) if zero_mean_u == "all" else ((e % 4 == 1) | (e >= 64))
    calm = np.zeros(ncol, bool)
    calm[:half:5] = True
    if ncol - last_chunk_start(nens, ncol) < ncol // 10:                 # a small last chunk: all of it calm
        calm[last_chunk_start(nens, ncol) - half:half] = True
        calm[2 * half:] = True
    calm[half:2 * half] = calm[:half]
    strong = (e % 3 == 1) & ((e // 3) % 2 == 0)                          # a strong positive buoyancy flux: v of 4 .. 6 m/s everywhere
    wind = {}
    means = {"u": np.where(zero, 0.0, rng.normal(4.0, 3.0, nens)),
             "v": np.where(strong, rng.choice([-1.0, 1.0], nens) * rng.uniform(4.5, 5.5, nens),
                           np.where(zero, 0.05, 1.0) * rng.normal(0.0, 3.0, nens))}
    for name, mean in means.items():
        amp = 10.0 ** rng.uniform(-4.0, 1.0, (ncol, nens)) * rng.choice([-1.0, 1.0], (ncol, nens))
        amp[calm] = 1e-3 * rng.uniform(-1.0, 1.0, (int(calm.sum()), nens))
        if name == "u":
            amp[half:2 * half, zero] = -amp[:half, zero]
            amp[2 * half:, zero] = 0.0                                   # the odd column out: at rest
            lull = calm[:, None] & ~zero[None, :]
        else:
            amp[:, strong] *= 0.05
            lull = calm[:, None] & ~zero[None, :] & ~strong[None, :]
        wind[name] = np.where(lull, 0.01, 1.0) * mean[None, :] + amp     # a calm cell of a member with a mean wind: |mean| / 100
    if nens >= 70 and zero_mean_u != "all":
        # the last member: a uniform calm wind but for 1e-11 -- its fluxes are 1e-11 of the others'
        wind["u"][:, -1] = 0.3 + 1e-11 * rng.uniform(-1.0, 1.0, ncol)
        wind["v"][:, -1] = -0.2 + 1e-11 * rng.uniform(-1.0, 1.0, ncol)
    for name, key in (("u", "uvel"), ("v", "vvel")):
        full = rng.normal(0.0, 5.0, shp)                                 # levels 1 and 2 are never read
        full[0] = wind[name]
        d[key] = full
    dz = 40.0 * (1.0 + 2.0 * ((e * 0.618034) % 1.0))                     # 40 .. 120 m, member by member
    d["zint"] = np.stack([0.0 * dz, dz, 2.2 * dz, 3.6 * dz])
    d["zmid"] = 0.5 * (d["zint"][:-1] + d["zint"][1:])
    d["gcm_uvel"], d["gcm_vvel"] = rng.normal(3.0, 4.0, (NZ, nens)), rng.normal(0.0, 3.0, (NZ, nens))
    d["gcm_uvel"][0, ::7], d["gcm_vvel"][0, ::7] = 0.3, -0.2             # a calm GCM wind: max(1, |u|)
    z0 = 10.0 ** rng.uniform(-5.0, 0.0, nens)
    if nens >= 3:
        z0[1], z0[2] = 1e-5, 1.0                                         # the values the init's clamps produce
    d["z0"] = z0
    d["tau"] = np.sort(10.0 ** rng.uniform(-3.0, np.log10(0.5), nens))[::-1].copy()
    sign = np.where(e % 3 == 1, 1.0, -1.0)
    d["bflx"] = np.where(e % 3 == 0, 0.0, sign * rng.uniform(0.005, 0.05, nens) * np.where((e % 3 == 1) & ~strong, 0.04, 1.0))
    if nens >= 70:
        d["bflx"][7] = DENORMAL          # -bflx * 0.4 rounds to -0.0: the one zeta that is zero inside diag_ustar's loop
    out = {}
    for k, v in d.items():
        v = np.ascontiguousarray(v, dtype=np.float64)
        out[k] = v.reshape(NZ, ny, nx, nens) if v.shape == shp else v
    return out


def module_friction_state(nens, nx, ny, nz, seed):
    """the state test_gpu_surface_friction_matches_restatement runs through the coupler: (tracers, fields, tau, bflx, zint)"""
    rng = np.random.default_rng(seed)
    tr = TRACER_SETS["kessler"]
    f = moist_state(tr, nens, nx, ny, nz, seed)
    shape = (nz, ny, nx, nens)
    f["uvel"] = rng.normal(4, 4, shape)
    f["vvel"] = rng.normal(-1, 4, shape)
    f["uvel"][0, 0, 0], f["vvel"][0, 0, 0] = 0.2, -0.1        # calm cells: max(1, |u|)
    f["water_vapor"] = rng.uniform(0.005, 0.015, shape)
    f["gcm_uvel"] = rng.normal(5, 4, (nz, nens))
    f["gcm_vvel"] = rng.normal(0, 4, (nz, nens))
    tau = rng.uniform(1e-3, 0.4, nens)
    bflx = np.where(np.arange(nens) % 3 == 0, 0.0, rng.uniform(-0.03, 0.03, nens))   # bflx = 0: diag_ustar does not iterate
    zi = idz.stretched_interfaces(nz, 12000.0)[:, None] * (1 + 0.01 * np.arange(nens))[None, :]
    for k in f:
        f[k] = np.ascontiguousarray(f[k])
    return tr, f, tau, bflx, zi


MODULE_FRICTION_SHAPES = MODULE_SHAPES + [(5, 12, 12, 3)]
MODULE_FRICTION_IDS = MODULE_SHAPE_IDS + ["column_chunks"]


def module_friction_inputs(shape):
    """module_friction_state in the layout of friction_state; z0 is the float64 restatement's (the module test hands the gate the
    device's own z0 once that has passed its gate)"""
    nens, nx, ny, nz = shape
    tr, f, tau, bflx, zi = module_friction_state(nens, nx, ny, nz, seed=20 + nens)
    d = dict(rho_d=f["density_dry"], rho_v=f["water_vapor"], uvel=f["uvel"], vvel=f["vvel"], zint=np.ascontiguousarray(zi),
             zmid=np.ascontiguousarray(0.5 * (zi[:-1] + zi[1:])), gcm_uvel=f["gcm_uvel"], gcm_vvel=f["gcm_vvel"], tau=tau, bflx=bflx)
    d["z0"] = z0_f64(d)
    return d


@functools.lru_cache(maxsize=None)
def friction_case(name):
    """the inputs of a named case, or of "module_<id>", built once and never written to"""
    if name.startswith("module_"):
        d = module_friction_inputs(MODULE_FRICTION_SHAPES[MODULE_FRICTION_IDS.index(name[7:])])
    else:
        c = FRICTION_BY_NAME[name]
        d = friction_state(c.nens, c.nx, c.ny, zero_mean_u="all" if name == "capped_chunks" else "some")
    for a in d.values():
        a.setflags(write=False)
    return d


ALL_FRICTION_STATES = FRICTION_IDS + ["module_" + i for i in MODULE_FRICTION_IDS]


# ------------------------------------------------------------------------------------------------------------------------------
# surface friction: the level-0 means and the float64 side

def slot_means(d):
    """(u_mean, v_mean, rho_mean), each (nens): the float64 means in the kernels' order"""
    return ref.level0_means_slot([d["uvel"][0], d["vvel"][0], d["rho_d"][0] + d["rho_v"][0]], d["rho_d"].shape[-1])


def serial_means(d):
    """the same in the order of a serial loop over the columns (np.cumsum adds one after the other)"""
    nens = d["rho_d"].shape[-1]
    r = 1.0 / (d["rho_d"].shape[1] * d["rho_d"].shape[2])
    return [np.cumsum(a.reshape(-1, nens) * r, axis=0)[-1] for a in (d["uvel"][0], d["vvel"][0], d["rho_d"][0] + d["rho_v"][0])]


def exact_means(d):
    """the means of the real numbers, to 2^-64: longdouble sums of longdouble products"""
    nens = d["rho_d"].shape[-1]
    ncol = d["rho_d"].shape[1] * d["rho_d"].shape[2]
    return [a.reshape(-1, nens).astype(LD).sum(axis=0) / LD(ncol) for a in (d["uvel"][0], d["vvel"][0], d["rho_d"][0] + d["rho_v"][0])]


BODY_MUTANTS = ("seven_iterations", "zeta_ge", "m_pi", "no_wind_clamp", "rho_sfc_two_levels")     # change surface_friction_cell itself


def cell_inputs(d, z0=None, mutant=None):
    """the twelve arguments of surface_friction_cell for every cell, each (ncol, nens) float64, as the kernel hands them over.  The
    mutants that are not in the cell's own arithmetic change what it is handed."""
    nens = d["rho_d"].shape[-1]
    ncol = d["rho_d"].shape[1] * d["rho_d"].shape[2]
    um, vm, rm = serial_means(d) if mutant == "serial_means" else slot_means(d)
    z0 = np.array(d["z0"] if z0 is None else z0, dtype=np.float64)
    if mutant == "last_member_z0" and nens > 1:
        z0[-1] = z0[-2]
    dz = d["zint"][1] - d["zint"][0]
    if mutant == "dz_member0":
        dz = np.full(nens, dz[0])
    rho = (d["rho_d"] + d["rho_v"]).reshape(-1, ncol, nens)
    row = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64)[None, :], (ncol, nens))
    um = row(um)
    if mutant == "last_chunk_zero_umean":
        um = np.array(um)
        um[last_chunk_start(nens, ncol):] = 0.0
    args = [d["uvel"][0].reshape(ncol, nens), d["vvel"][0].reshape(ncol, nens), um, row(vm), row(rm), row(d["zmid"][0]), row(d["bflx"]),
            row(z0), rho[0], rho[1], rho[2], row(dz)]
    return [np.ascontiguousarray(a) for a in args]


def fluxes_f64(d, z0=None, mutant=None):
    """(sfc_mom_flx_u, sfc_mom_flx_v), each (ny, nx, nens): the float64 restatement at the slot-order means.  Without a mutant of the
    cell's own arithmetic the cells go through the host emulation, which is the restatement bit for bit
    (test_the_emulation_is_the_restatement_bit_for_bit); with one, through the scalar Python restatement."""
    args = cell_inputs(d, z0, mutant)
    shape = d["rho_d"].shape[1:]
    n = args[0].size
    if mutant in BODY_MUTANTS:
        out = np.array([ref.surface_friction_cell(*a, mutant=mutant) for a in zip(*[x.ravel().tolist() for x in args])])
        return out[:, 0].reshape(shape), out[:, 1].reshape(shape)
    fu, fv = np.zeros(n), np.zeros(n)
    emu().emu_surface_friction_cell(n, *[_p(a) for a in args], _p(fu), _p(fv))
    return fu.reshape(shape), fv.reshape(shape)


def fluxes_python(d, z0=None):
    """the scalar Python restatement at the slot-order means (small cases)"""
    args = cell_inputs(d, z0)
    out = np.array([ref.surface_friction_cell(*a) for a in zip(*[x.ravel().tolist() for x in args])])
    shape = d["rho_d"].shape[1:]
    return out[:, 0].reshape(shape), out[:, 1].reshape(shape)


def z0_f64(d, python=False):
    """z0 (nens) of surface_friction_init: the float64 restatement at the slot-order mean density"""
    nens = d["rho_d"].shape[-1]
    (rm,) = ref.level0_means_slot([d["rho_d"][0] + d["rho_v"][0]], nens)
    args = [np.ascontiguousarray(a, dtype=np.float64) for a in (d["zmid"][0], d["bflx"], d["gcm_uvel"][0], d["gcm_vvel"][0], d["tau"], rm)]
    if python:
        return np.array([ref.surface_friction_z0(*a) for a in zip(*[x.tolist() for x in args])])
    z0 = np.zeros(nens)
    emu().emu_surface_friction_z0(nens, *[_p(a) for a in args], _p(z0))
    return z0


# ------------------------------------------------------------------------------------------------------------------------------
# surface friction: the reference (longdouble here, binary128 in tests/emu/moist_surface_quad_emu.cpp).  Every constant is the double the
# code holds (PI = 3.14159), taken as an exact number.

VONK, EPS, AM, BM, PI = (LD(x) for x in (ref.VONK, ref.EPS, ref.AM, ref.BM, ref.PI))
C1 = PI / 2 - 3 * np.log(LD(2))


def _psi1(zeta):
    x = np.sqrt(np.sqrt(1 - BM * zeta))
    return 2 * np.log(1 + x) + np.log(1 + x * x) - 2 * np.arctan(x) + C1


def diag_ustar_ld(z, bflx, wnd, z0):
    """surface_friction.h:44-63 on longdouble arrays of one shape"""
    lnz = np.log(z / z0)
    ustar = wnd * (VONK / lnz)
    it = np.flatnonzero(bflx != 0)
    if it.size:
        z, bflx, wnd, lnz, u = z[it], bflx[it], wnd[it], lnz[it], ustar[it]
        for _ in range(8):
            zeta = np.minimum(LD(1), z * (-bflx * VONK / (u * u * u + EPS)))
            st = zeta > 0
            new = np.empty_like(u)
            new[st] = VONK * wnd[st] / (lnz[st] + AM * zeta[st])
            un = ~st
            new[un] = wnd[un] * VONK / (lnz[un] - _psi1(zeta[un]))
            u = new
        ustar[it] = u
    return ustar


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """friction_reference and z0_reference of a named state, computed once and shared: dict(fu, fv, unit_u, unit_v, z0_raw, z0)"""
    d = friction_case(name)
    r = friction_reference(d)
    r["z0_raw"], r["z0"] = z0_reference(d)
    for a in r.values():
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def quad():
    """tests/emu/moist_surface_quad_emu.cpp: the formulas in binary128, linked against gcc's libquadmath"""
    lib = C.CDLL(emu_library("moist_surface_quad_emu", libs=("quadmath", "pthread")))
    lib.quad_surface_friction_cells.argtypes = [C.c_longlong, C.c_int] + [_DP] * 12 + [C.c_void_p] * 2 + [_DP] * 2
    lib.quad_surface_friction_cells.restype = None
    lib.quad_surface_friction_z0.argtypes = [C.c_int] + [_DP] * 6 + [C.c_void_p] * 2
    lib.quad_surface_friction_z0.restype = None
    return lib


def friction_reference(d, z0=None):
    """the fluxes of compute_surface_friction at the float64 slot-order means, and one unit of each: dict(fu, fv (longdouble), unit_u,
    unit_v (float64)), each (ny, nx, nens).  Evaluated in binary128 and rounded once to longdouble: np.longdouble's own 64 bits leave
    5e-3 of a unit after the eight iterations of diag_ustar (friction_reference_ld, kept as a cross-check of the two restatements)."""
    args = cell_inputs(d, z0)
    n = args[0].size
    shape = d["rho_d"].shape[1:]
    fu, fv = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    unit_u, unit_v = np.zeros(n), np.zeros(n)
    assert fu.itemsize == 16 and np.finfo(LD).nmant == 63            # the x87 long double of the C side
    quad().quad_surface_friction_cells(n, min(8, os.cpu_count() or 1), *[_p(a) for a in args], fu.ctypes.data_as(C.c_void_p), fv.ctypes.data_as(C.c_void_p),
                                       _p(unit_u), _p(unit_v))
    return dict(fu=fu.reshape(shape), fv=fv.reshape(shape), unit_u=unit_u.reshape(shape), unit_v=unit_v.reshape(shape))


def friction_reference_ld(d, z0=None):
    """the same in np.longdouble, vectorised over the cells"""
    a = [x.ravel().astype(LD) for x in cell_inputs(d, z0)]
    u, v, um, vm, rm, zm0, bflx, z0, r0, r1, r2, dz = a
    wnd = np.maximum(LD(1), np.sqrt(u * u + v * v))
    ustar = diag_ustar_ld(zm0, bflx, wnd, z0)
    tau00 = rm * ustar * ustar
    rho_sfc = 2 * ((r0 + r1) / 2) - (r1 + r2) / 2
    k = tau00 / wnd * rho_sfc / dz
    shape = d["rho_d"].shape[1:]
    s = np.abs(k)
    return dict(fu=(-(u - um) * k).reshape(shape), fv=(-(v - vm) * k).reshape(shape),
                unit_u=(U * (np.abs(u) + np.abs(um)) * s).astype(np.float64).reshape(shape),
                unit_v=(U * (np.abs(v) + np.abs(vm)) * s).astype(np.float64).reshape(shape))


def z0_reference(d):
    """z0 of surface_friction_init at the float64 slot-order mean density: (z0 before the clamps, z0), longdouble.  Evaluated in
    binary128 and rounded once to longdouble, like the fluxes (z0_reference_ld is the np.longdouble restatement beside it)."""
    nens = d["rho_d"].shape[-1]
    (rm,) = ref.level0_means_slot([d["rho_d"][0] + d["rho_v"][0]], nens)
    args = [np.ascontiguousarray(a, dtype=np.float64) for a in (d["zmid"][0], d["bflx"], d["gcm_uvel"][0], d["gcm_vvel"][0], d["tau"], rm)]
    raw, z0 = np.zeros(nens, dtype=LD), np.zeros(nens, dtype=LD)
    assert raw.itemsize == 16 and np.finfo(LD).nmant == 63
    quad().quad_surface_friction_z0(nens, *[_p(a) for a in args], raw.ctypes.data_as(C.c_void_p), z0.ctypes.data_as(C.c_void_p))
    return raw, z0


def z0_reference_ld(d):
    """the same in np.longdouble: z0 of surface_friction_init at the float64 slot-order mean density: (z0 before the clamps, z0)"""
    nens = d["rho_d"].shape[-1]
    (rm,) = ref.level0_means_slot([d["rho_d"][0] + d["rho_v"][0]], nens)
    z, bflx, gu, gv, tau, rm = (np.asarray(x, dtype=np.float64).astype(LD) for x in
                                (d["zmid"][0], d["bflx"], d["gcm_uvel"][0], d["gcm_vvel"][0], d["tau"], rm))
    wnd = np.maximum(LD(1), np.sqrt(gu * gu + gv * gv))
    ustar = np.sqrt(tau / rm)
    zeta = np.minimum(LD(1), z * (-bflx * VONK / (ustar * ustar * ustar + EPS)))
    psi1 = np.where(zeta >= 0, -AM * zeta, _psi1(np.minimum(zeta, LD(0))))
    lnz = np.maximum(LD(0), VONK * wnd / (ustar + EPS) + psi1)
    raw = z * np.exp(-lnz)
    return raw, np.maximum(LD(0.00001), np.minimum(LD(1), raw))


# ------------------------------------------------------------------------------------------------------------------------------
# surface friction: gates

E_FLUX, E_Z0 = 44.0, 43.0       # measured 43.5 and 42.5: test_the_restatement_is_within_E_of_the_longdouble_reference
G_FLUX, G_Z0 = 4 * E_FLUX, 4 * E_Z0


def flux_errors(got_u, got_v, r):
    """the errors of two flux arrays in units, per cell: (of u, of v); a cell whose unit is zero counts 0 if it is exact, inf if not"""
    out = []
    for g, w, unit in ((got_u, r["fu"], r["unit_u"]), (got_v, r["fv"], r["unit_v"])):
        err = np.abs(np.asarray(g).astype(LD) - w).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf)))
    return out


def assert_fluxes_within(got_u, got_v, r, gate=None):
    """every cell of both fluxes within `gate` (G_FLUX) units of the reference r (friction_reference).  Returns the worst, in units."""
    gate = G_FLUX if gate is None else gate
    worst = 0.0
    for name, e in zip(("sfc_mom_flx_u", "sfc_mom_flx_v"), flux_errors(got_u, got_v, r)):
        assert np.isfinite(np.asarray(got_u)).all() and np.isfinite(np.asarray(got_v)).all()
        bad = ~(e <= gate)
        if bad.any():
            i = np.unravel_index(np.argmax(np.where(bad, e, 0)), e.shape)
            raise AssertionError("%s: %d of %d cells beyond %g units, the worst %g at (j, i, member) = %s" % (name, bad.sum(), e.size, gate, e[i], i))
        worst = max(worst, float(e.max()))
    return worst


def z0_errors(got, raw, want):
    """per member, in units of 2^-53 z0"""
    return (np.abs(np.asarray(got).astype(LD) - want) / (U * want)).astype(np.float64)


def assert_z0_within(got, raw, want, gate=None):
    """every member within `gate` (G_Z0) units; a member the clamps pin to 1e-5 or 1.0 must hold that literal exactly, unless the value
    before the clamps is itself within the gate of the literal.  Returns the worst, in units."""
    gate = G_Z0 if gate is None else gate
    got = np.asarray(got)
    e = z0_errors(got, raw, want)
    assert np.all(e <= gate), (float(e.max()), int(np.argmax(e)))
    for lit, pinned in ((0.00001, raw < LD(0.00001)), (1.0, raw > LD(1))):
        clear = pinned & ((np.abs(raw - LD(lit)) / (U * LD(lit))).astype(np.float64) > gate)
        assert np.array_equal(got[clear], np.full(int(clear.sum()), lit)), lit
    return float(e.max())


def old_flux_gate_accepts(got_u, got_v, want_u, want_v):
    """the gate this one replaces: 1e-12 of the field's largest value"""
    return all(np.abs(g - w).max() <= OLD_GATE * np.abs(w).max() for g, w in ((got_u, want_u), (got_v, want_v)))
