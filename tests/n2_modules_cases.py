"""Named cases, state builders and mutants for sponge_layer, perturb_temperature and broadcast_initial_gcm_column cell by cell
(tests/test_n2_modules_cells.py; the restatements and the gates are in tests/n2_modules_ref.py).

Sponge states (sponge_state): every field varies horizontally on every level, and every field's level mean depends on the member --
    uvel, vvel      change sign; |mean| (0.3 .. 1.5) well below the spread (10)
    temp, rho_d     mean (250 .. 280 K; 0.3 .. 0.42) far above the spread (2 K; 0.005)
    wvel            mean 2.0 .. 2.8, spread 1: relaxing it to its mean instead of to zero moves every cell
    tracers         tracer t has magnitude 10^-(2t % 9): positive in some cells of a level and exactly zero in others
and every member has its own stretch ratio and its own model top, so the relaxation factor on a level differs from member to member
(a census test asserts by more than 1e-3 relative).  The state the other sponge tests share (tests/test_modules.py: _case) is
horizontally uniform in the sponge but for wvel, its tracers are zero there and its members' grids are multiples of one another, which
leaves the factor the same for all of them.

No case has more than 25 000 cells per field.
"""
import collections
import functools

import numpy as np

import n2_modules_ref as nr
from pam_amd import idealized as idz

# ---- sponge_layer -----------------------------------------------------------------------------------------------------------------

SpongeCase = collections.namedtuple("SpongeCase", "name nens nx ny nz ntr num_layers time_scale dt via")
# num_layers None: the options are absent, the module's defaults (5 layers, 60 s) hold.  via: "coupler" (PamCoupler.run_module) or
# "capi" (pam_amd_sponge_layer called directly: the coupler's field dump needs at least one tracer).
#   ncol: 1 (15 empty slots), 5 (2-D), 15, 16, 17, 33.   nens: 1, 3, 5, 64, 65, 70, 130 (three member blocks, the last ragged).
#   num_layers: 1 (F = 0 on the only level), 2, nz, absent.   fields: 5, 6, 9, 55 (the whole pointer table).   factor above 1: dt > ts.
SPONGE = [
    SpongeCase("n3_1x1x6_L2_f9", 3, 1, 1, 6, 4, 2, 30.0, 2.0, "coupler"),
    SpongeCase("n1_5x1x8_L4_f6", 1, 5, 1, 8, 1, 4, 30.0, 2.0, "coupler"),
    SpongeCase("n64_5x3x7_L3_f6", 64, 5, 3, 7, 1, 3, 20.0, 2.0, "coupler"),
    SpongeCase("n65_4x4x6_Lnz_f9", 65, 4, 4, 6, 4, 6, 30.0, 3.0, "coupler"),
    SpongeCase("n130_17x1x6_Ldefault_f6", 130, 17, 1, 6, 1, None, None, 2.0, "coupler"),
    SpongeCase("n3_11x3x8_L1_f9", 3, 11, 3, 8, 4, 1, 30.0, 2.0, "coupler"),
    SpongeCase("n70_11x3x7_L4_f9_factor_above_1", 70, 11, 3, 7, 4, 4, 30.0, 45.0, "coupler"),
    SpongeCase("n3_5x1x6_L3_f55", 3, 5, 1, 6, 50, 3, 30.0, 2.0, "coupler"),
    SpongeCase("n5_3x2x6_L2_f5_capi", 5, 3, 2, 6, 0, 2, 30.0, 2.0, "capi"),
    SpongeCase("n3_5x1x6_L3_f55_capi", 3, 5, 1, 6, 50, 3, 30.0, 2.0, "capi"),
]
SPONGE_BY_NAME = {c.name: c for c in SPONGE}
SPONGE_IDS = [c.name for c in SPONGE]
SPONGE_RAGGED = "n70_11x3x7_L4_f9_factor_above_1"        # 64 + 6 members: determinism and member shards run on this one


def layers_and_scale(case):
    return (5, 60.0) if case.num_layers is None else (case.num_layers, case.time_scale)


def member_grids(nens, nz):
    """(nz+1, nens) interfaces and (nz, nens) midpoints: member e has its own stretch ratio (1.0 .. 1.15) and its own top (12 .. 15.6
    km).  The midpoints are formed as PamCoupler.set_grid forms them."""
    e = np.arange(nens)
    ratio = 1.0 + 0.15 * ((e * 0.618034) % 1.0)
    ztop = 12000.0 * (1.0 + 0.3 * ((e * 0.377) % 1.0))
    zi = np.ascontiguousarray(np.stack([idz.stretched_interfaces(nz, ztop[m], ratio[m]) for m in range(nens)], axis=1))
    return zi, np.ascontiguousarray(0.5 * (zi[:-1] + zi[1:]))


def sponge_state(nens, nx, ny, nz, ntr, seed=0):
    """X (5 + ntr, nz, ny, nx, nens), zint, zmid: see the module docstring"""
    rng = np.random.default_rng([seed, nens, nx, ny, nz, ntr])
    shp = (nz, ny, nx, nens)
    e = np.arange(nens)
    X = np.empty((5 + ntr,) + shp)
    X[0] = 0.3 + 0.01 * (e % 13) + rng.uniform(-0.005, 0.005, shp)
    X[1] = 0.3 * (1 + e % 5) + 10.0 * rng.standard_normal(shp)
    X[2] = -0.3 * (1 + e % 4) + 10.0 * rng.standard_normal(shp)
    X[3] = 2.0 + 0.1 * (e % 9) + rng.standard_normal(shp)
    X[4] = 250.0 + 3.0 * (e % 11) + rng.uniform(-2.0, 2.0, shp)
    ncol = ny * nx
    if ncol > 1:           # both signs of u and v on every level of every member, however few the cells
        for f in (1, 2):
            flat = X[f].reshape(nz, ncol, nens)
            for k in range(nz):
                flat[k, k % ncol] = -1.0 - np.abs(flat[k, k % ncol])
                flat[k, (k + 1) % ncol] = 1.0 + np.abs(flat[k, (k + 1) % ncol])
    for t in range(ntr):
        a = 10.0 ** -(2 * t % 9) * (1.0 + 0.05 * (e % 7)) * rng.uniform(0.5, 1.5, shp) * (rng.random(shp) > 0.4)
        flat = a.reshape(nz, ncol, nens)
        if ncol > 1:       # on every level of every member one cell that is certainly zero and one that is certainly not
            for k in range(nz):
                flat[k, (k + t) % ncol] = 0.0
                flat[k, (k + t + 1) % ncol] = 10.0 ** -(2 * t % 9) * (1.0 + 0.05 * (e % 7))
        X[5 + t] = a
    zi, zm = member_grids(nens, nz)
    return X, zi, zm


@functools.lru_cache(maxsize=None)
def sponge_reference(name):
    """computed once per session and never written to: state, restatement with its gate, the oracle's result and the slot-order
    emulation's"""
    from oracle import awfl_oracle as ao
    c = SPONGE_BY_NAME[name]
    L, ts = layers_and_scale(c)
    X, zi, zm = sponge_state(c.nens, c.nx, c.ny, c.nz, c.ntr)
    ref = nr.sponge(X, zi, zm, c.dt, L, ts)
    f = nr.unstack(X.copy())
    ao.sponge_layer(f, zi, zm, c.dt, num_layers=L, time_scale=ts)
    emu = nr.sponge_slot_emulation(X, zi, zm, c.dt, L, ts)
    for a in (X, zi, zm, ref["r"], ref["tol"], emu):
        a.setflags(write=False)
    return dict(case=c, X=X, zint=zi, zmid=zm, ref=ref, oracle=nr.stack(f), emulation=emu, num_layers=L, time_scale=ts)


# A mutant is an error put into the RESTATEMENT (never into a kernel): name -> the cases meant to catch it.  Every one of them needs a
# level with F > 0, i.e. num_layers >= 2, but the last.
def _relaxes(c):
    return layers_and_scale(c)[0] >= 2


SPONGE_MUTANTS = {
    # the members' grids differ
    "member0_heights": lambda c: _relaxes(c) and c.nens > 1,
    "factor_from_level_above": _relaxes,
    "factor_halved": _relaxes,
    "w_to_its_mean": _relaxes,
    # the cells beyond 16 * floor(ncol / 16): there are some
    "mean_drops_ragged_tail": lambda c: _relaxes(c) and (c.nx * c.ny) % 16 != 0,
    # slot 15 owns a cell
    "mean_drops_slot_15": lambda c: _relaxes(c) and c.nx * c.ny >= 16,
    # (a level of one cell is its own mean: the sponge leaves every field but w as it is)
    "last_tracer_skipped": lambda c: _relaxes(c) and c.ntr >= 1 and c.nx * c.ny >= 2,
    "tracer_means_swapped": lambda c: _relaxes(c) and c.ntr >= 2,
    # (e + 64) % nens is another member
    "mean_from_member_plus_64": lambda c: _relaxes(c) and 64 % c.nens != 0,
    "one_cell_1e-9": lambda c: True,
}


# ---- perturb_temperature ------------------------------------------------------------------------------------------------------------

PerturbCase = collections.namedtuple("PerturbCase", "name nens nx ny nz magnitude ids")
I31 = 2 ** 31 - 1
#   nz: 3 (nz/4 = 0: nothing may change), 4, 7, 8, 17.   ncol: 1 (the rescale restores the cell), 2, 15, 40.
#   nens: 1, 3, 33 with two levels (66 threads: across a wavefront's edge), 64, 65, 70.
#   ids: 0, duplicates across members, negative, 2^31 - 1 (times nl * ncol: the seed needs 64 bits)
PERTURB = [
    PerturbCase("n3_2x1x3_noop", 3, 2, 1, 3, 30.0, "count"),
    PerturbCase("n1_1x1x4_id0", 1, 1, 1, 4, 30.0, "zero"),
    PerturbCase("n3_1x1x8_one_column", 3, 1, 1, 8, 30.0, "count"),
    PerturbCase("n33_2x1x8_duplicate_ids", 33, 2, 1, 8, 30.0, "pairs"),
    PerturbCase("n64_5x3x7_negative_ids", 64, 5, 3, 7, 0.25, "negative"),
    PerturbCase("n65_8x5x4_ids_at_int_max", 65, 8, 5, 4, 30.0, "large"),
    PerturbCase("n70_5x3x17_mixed_ids", 70, 5, 3, 17, 30.0, "mixed"),
    PerturbCase("n3_5x1x17_small_magnitude", 3, 5, 1, 17, 0.25, "count"),
]
PERTURB_BY_NAME = {c.name: c for c in PERTURB}
PERTURB_IDS = [c.name for c in PERTURB]
PERTURB_RAGGED = "n70_5x3x17_mixed_ids"


def perturb_ids(kind, nens):
    e = np.arange(nens, dtype=np.int64)
    ids = {"zero": 0 * e, "count": 3 * e + 11, "pairs": e // 2, "negative": -5 * e - 3, "large": I31 - e,
           "mixed": np.where(e % 4 == 0, 0, np.where(e % 4 == 1, I31 - e, np.where(e % 4 == 2, -e, e // 8)))}[kind]
    return np.ascontiguousarray(ids.astype(np.int32))


def perturb_state(nens, nx, ny, nz, seed=0):
    """temperature: 250 .. 280 K by member, +- 20 K from cell to cell"""
    rng = np.random.default_rng([seed, nens, nx, ny, nz, 77])
    shp = (nz, ny, nx, nens)
    base = 250.0 + 3.0 * (np.arange(nens) % 11)
    T = np.ascontiguousarray(base + rng.uniform(-20.0, 20.0, shp))
    if nx * ny > 1:        # the whole range on every level of every member, however few the cells
        flat = T.reshape(nz, ny * nx, nens)
        for k in range(nz):
            flat[k, k % (ny * nx)] = base - 20.0
            flat[k, (k + 1) % (ny * nx)] = base + 20.0
    return T


@functools.lru_cache(maxsize=None)
def perturb_reference(name):
    from oracle import awfl_oracle as ao
    c = PERTURB_BY_NAME[name]
    T = perturb_state(c.nens, c.nx, c.ny, c.nz)
    ids = perturb_ids(c.ids, c.nens)
    ref = nr.perturb(T, ids, c.magnitude)
    oracle = T.copy()
    ao.perturb_temperature(oracle, ids, c.magnitude)
    emu = nr.perturb_serial_emulation(T, ids, c.magnitude)
    for a in (T, ids, ref["r"], ref["tol"], oracle, emu):
        a.setflags(write=False)
    return dict(case=c, T=T, ids=ids, ref=ref, oracle=oracle, emulation=emu)


def _perturbs(c):       # a level is perturbed, and the level has more than the one cell the rescale restores
    return c.nz // 4 >= 1 and c.nx * c.ny >= 2


def _ids_differ_from_the_member_before(c):
    ids = perturb_ids(c.ids, c.nens)
    return bool((ids != np.roll(ids, 1)).any())


PERTURB_MUTANTS = {
    "seed_without_level": lambda c: _perturbs(c) and c.nz // 4 >= 2,
    "seed_member_fastest": lambda c: _perturbs(c) and c.nens > 1,
    "scaling_of_level_above": _perturbs,
    "rescale_inverted": _perturbs,
    "id_of_member_before": lambda c: _perturbs(c) and _ids_differ_from_the_member_before(c),
    "hmean1_of_next_member": lambda c: c.nz // 4 >= 1 and c.nens > 1,
}


# ---- broadcast_initial_gcm_column ---------------------------------------------------------------------------------------------------

#   ncell = nens * nx * ny * nz against the 256 threads of a workgroup: below, an exact multiple, just past one; nens 1 and 70
BROADCAST = [(1, 3, 2, 5), (1, 8, 4, 8), (1, 1, 1, 257), (70, 3, 1, 1), (70, 8, 4, 4), (70, 11, 1, 5)]
BROADCAST_IDS = ["n%d_%dx%dx%d" % s for s in BROADCAST]
SPECIALS = np.array([0x8000000000000000,      # -0.0
                     0x0000000000000003,      # a denormal
                     0x7FF0000000000000,      # +inf
                     0xFFF0000000000000,      # -inf
                     0x7FF8000000ABCDEF,      # a quiet NaN with a payload
                     0xFFF80000DEADBEEF], dtype=np.uint64)


def broadcast_state(nens, nx, ny, nz, seed=0):
    """(crm, gcm): six (nz, ny, nx, nens) fields of canaries, distinct per field and per cell, and six (nz, nens) columns of ordinary
    numbers with the special bit patterns strewn in, every field at other places"""
    rng = np.random.default_rng([seed, nens, nx, ny, nz, 99])
    n = nz * ny * nx * nens
    crm = [np.ascontiguousarray(((f + 1) * 1.0e6 + np.arange(n, dtype=np.float64)).reshape(nz, ny, nx, nens)) for f in range(6)]
    gcm = []
    for f in range(6):
        g = np.ascontiguousarray(rng.uniform(-1.5, 1.5, (nz, nens)) * 10.0 ** (f - 2))
        flat = nr.bits(g).reshape(-1)
        for s in range(len(SPECIALS)):      # (a column too short for all of them keeps other ones in every field)
            flat[(f + 7 * s) % flat.size] = SPECIALS[(s + f) % len(SPECIALS)]
        gcm.append(g)
    return crm, gcm
