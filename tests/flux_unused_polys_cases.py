"""Cases and runs shared by tests/test_flux_unused_polys.py and tests/golden/make_flux_unused_polys_golden.py: one sub-step of the host
emulation (tests/emu/awfl_emu.cpp) on small grids, in every way the y/z flux sweeps can be scheduled.  TEST INFRASTRUCTURE ONLY.

A PHYSICS case (grid, tracers, dry air, vertical tables) fixes the numbers; a SCHEDULE (member or flat lanes, the z sweep whole or cut
into two spans, the y differences folded into the z sweep or not, fused or three-kernel stage) must not change them.  The golden file
holds one set of arrays per physics case, recorded from the parent commit's emulation on the plain schedule; every schedule is compared
with it."""
import copy

import numpy as np

from pam_amd import idealized as idz
from parity_cases import build_inputs

NENS = 2            # member lanes need two members; flat lanes run on the same fields
DT = 0.5            # one sub-step: crm_dt == dt_dyn

# (nx, ny, nz): every remainder of the five-trip rounds in y and z, the shortest periodic line (ny = 3), and a 2-D grid (no y sweep)
# physics variants per grid: (NT, carve_dry_air zeros, per-member vertical tables) -- all eight combinations occur, the larger grids
# carry one each (the golden file has to stay below the size limit of a committed file)
GRIDS = {
    (5, 3, 6): [(1, 0, 0), (4, 0, 1), (1, 1, 1)],
    (5, 4, 7): [(4, 1, 0), (1, 0, 1)],
    (5, 5, 9): [(4, 1, 1)],
    (5, 6, 10): [(4, 0, 0)],
    (5, 7, 11): [(1, 0, 1)],
    (5, 11, 12): [(1, 1, 0)],
    (5, 1, 8): [(1, 1, 1), (4, 0, 0), (1, 0, 1), (4, 1, 0)],
}
PHYSICS = [(g, v) for g in GRIDS for v in GRIDS[g]]
# dx != dy with the sounding's shear along y (a third element: options of parity_cases.build_inputs).  The golden file has none of
# these: tests/test_flux_unused_polys.py holds their plain schedule to the oracle and every other schedule to the plain one's bits.
ANISO_PHYSICS = [((5, 7, 9), (4, 1, 1), dict(dxy=500.0, dy=800.0, flow="y")),
                 ((6, 5, 8), (1, 1, 0), dict(dxy=800.0, dy=500.0, flow="y")),
                 ((5, 6, 10), (4, 0, 0), dict(dxy=1000.0, dy=250.0, flow="y"))]
# (lanes, z spans, fold, fused)
SCHEDULES = [(lanes, spans, fold, fused) for fused in (True, False) for lanes in ("member", "flat") for spans in (1, 2) for fold in (False, True)
             if not (fold and (lanes == "flat" or not fused)) and not (lanes == "flat" and not fused)]
PLAIN = ("member", 1, False, True)
FIELDS = ("density_dry", "uvel", "vvel", "wvel", "temp", "tracers")


def physics_id(p):
    (nx, ny, nz), (nt, carve, perens) = p[:2]
    return "%dx%dx%d_nt%d%s%s" % (nx, ny, nz, nt, "_carved" if carve else "", "_perens" if perens else "") + (
        "_dx%g_dy%g_flow%s" % (p[2]["dxy"], p[2]["dy"], p[2]["flow"]) if len(p) > 2 else "")


def schedule_id(s):
    lanes, spans, fold, fused = s
    return "%s_%s%s%s" % ("fused" if fused else "three", lanes, "_cut" if spans == 2 else "", "_fold" if fold else "")


def applies(p, s):
    (nx, ny, nz) = p[0]
    return not (s[2] and ny == 1)          # nothing to fold on a 2-D grid


def make_fields(p):
    (nx, ny, nz), (nt, carve, perens) = p[:2]
    tr = idz.TRACERS_NONE if nt == 1 else idz.TRACERS_KESSLER_SHOC
    assert len(tr) == nt
    zint = idz.stretched_interfaces(nz, 12000.0)
    f, xlen, ylen, _, _ = build_inputs(NENS, nx, ny, nz, tr, zint, mag=0.5, **(p[2] if len(p) > 2 else {}))
    # wind through every face, vertical motion next to both walls, and members that differ
    k, j, i, e = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), np.arange(NENS), indexing="ij")
    f["uvel"] = f["uvel"] - 25.0 + 3.0 * np.sin(1.3 * i + 0.7 * k + e)
    f["vvel"] = f["vvel"] - 2.0 + 14.0 * np.cos(1.1 * j + 1.3 * i + 0.8 * k + 2.0 * e) * (ny > 1)     # both signs at every j
    f["wvel"] = f["wvel"] + 2.0 * np.sin(0.9 * k + 1.7 * j + 0.6 * i + e + 0.5)
    if carve:
        idz.carve_dry_air(f, tr, moist_every=0)
    zi = np.asarray(zint)[:, None] * np.ones((1, NENS))
    if perens:
        zi = zi * (1 + 0.03 * np.arange(NENS))[None, :]
    return f, tr, zi, xlen, ylen


def written(p, name, fused):
    """mask of the entries of a flux array that the stage writes (the rest keeps what the buffer held before)"""
    (nx, ny, nz), (nt, _, _) = p[:2]
    if name == "flux_y":
        m = np.ones((5 + nt, nz, ny, nx, NENS), dtype=bool)
    else:
        m = np.ones((5 + nt, nz + 1, ny, nx, NENS), dtype=bool)
        if fused:
            m[1:5, nz] = False              # differences of cells: nz levels
    if fused and ny == 1:
        m[2] = False                        # 2-D: v has no tendency, the fused stage does not advect it
    return m


def run(emu_harness, p, s):
    """one sub-step of schedule s on physics case p -> {name: 1-D array of the written entries}"""
    (nx, ny, nz), (nt, carve, perens) = p[:2]
    lanes, spans, fold, fused = s
    f, tr, zi, xlen, ylen = make_fields(p)
    f = copy.deepcopy(f)
    names, pos, mass, idwv = idz.tracer_flags(tr)
    d = emu_harness.EmuDycore(NENS, nx, ny, nz, xlen, ylen, np.diff(zi, axis=0), pos, mass, idwv)
    assert d.vz_per_ens == bool(perens)
    d.set_fused(fused)
    d.set_lane_mapping(lanes == "flat", False)
    d.set_yz_fold(fold)
    d.set_span((nz + 2) // 2 if spans == 2 else 0)        # nz + 1 faces in two spans: one starts at a wall, the other ends at one
    d.declare_current_profile_as_hydrostatic(f)
    ncyc, dt = d.time_step(f, DT, DT)
    assert ncyc == 1 and dt == DT
    out = {}
    for name in ("flux_y", "flux_z"):
        if name == "flux_y" and ny == 1:
            continue
        m = written(p, name, fused)
        a = d.buffer(name, m.shape).copy()
        if fold:                              # the z sweep stores the y+z part of the divergence: not the recorded differences
            if name == "flux_z":
                m[1:5] = False
        out[name] = (a, m)
    for k in FIELDS:
        out[k] = (f[k], np.ones(f[k].shape, dtype=bool))
    return out


def key(p, fused, name):
    return "%s__%s__%s" % (physics_id(p), "fused" if fused else "three", name)
