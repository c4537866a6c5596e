"""The named oracle cases of tests/test_gpu_parity.py, built without torch or a device: their inputs, vertical grids, the oracle
that checks them, its run and its noise floor (tests/parity_gate.py).  A plain helper module: the GPU tests load the same inputs into
the device, the CPU tests (tests/test_parity_gate.py) hold the gate itself against the oracle."""
import copy

import numpy as np

from oracle import awfl_oracle as ao
from pam_amd import idealized as idz
from parity_gate import noise_floor

CASES = {
    # name: (nens, nx, ny, nz, tracers, zint, kwargs, mode_a, nsteps)
    "2d_nt1_uniform_A": (3, 8, 1, 10, idz.TRACERS_NONE, idz.uniform_interfaces(10, 10000.0), {}, True, 2),
    "2d_nt4_stretched_A": (2, 9, 1, 11, idz.TRACERS_KESSLER_SHOC, idz.stretched_interfaces(11, 12000.0), {}, True, 2),
    "3d_nt1_stretched_A": (2, 7, 5, 9, idz.TRACERS_NONE, idz.stretched_interfaces(9, 12000.0), {}, True, 2),
    "3d_nt4_stretched_B": (2, 6, 6, 8, idz.TRACERS_KESSLER_SHOC, idz.stretched_interfaces(8, 12000.0), {}, False, 2),
    # mode B (balance_hydrostasis_with_gravity = false, Dycore.h:313-314,562,678-681) with ONE tracer: the NT=1 tail kernels
    "3d_nt1_stretched_B": (2, 7, 5, 9, idz.TRACERS_NONE, idz.stretched_interfaces(9, 12000.0), {}, False, 2),
    # water_vapor as the only tracer AND limited in every stage (exact zeros beside moist air, wind across the edges): the
    # x-sweep's own-multiplier store + row flags and the work branch of awfl_trfix_kernel over several timeSteps, with a member
    # count that makes every wavefront one whole flag row (64) and a ragged one (70); mode A and mode B
    "3d_nt1_vapour_limited_nens64": (64, 6, 4, 8, idz.TRACERS_NONE, idz.stretched_interfaces(8, 12000.0), dict(dry_air=True), True, 2),
    "3d_nt1_vapour_limited_nens70_ragged": (70, 6, 4, 8, idz.TRACERS_NONE, idz.stretched_interfaces(8, 12000.0), dict(dry_air=True), True, 2),
    "3d_nt1_vapour_limited_B": (5, 6, 4, 8, idz.TRACERS_NONE, idz.stretched_interfaces(8, 12000.0), dict(dry_air=True), False, 2),
    "2d_nt1_vapour_limited": (66, 9, 1, 10, idz.TRACERS_NONE, idz.stretched_interfaces(10, 12000.0), dict(dry_air=True), True, 2),
    "3d_nt10_perens_A_p3": (3, 6, 4, 8, idz.TRACERS_P3_SHOC, idz.stretched_interfaces(8, 12000.0),
                            dict(per_ens=True, consts=idz.CONSTS_P3), True, 2),
    # per-member vertical grids with MEMBER lanes (64+ members: awfl_fluxz_pe_kernel, tables staged in LDS): whole blocks; a ragged
    # block (130 = 2 x 64 + 2) with 15 columns (not a multiple of the workgroup's four)
    "3d_nt4_perens_nens64_member_lanes": (64, 6, 4, 8, idz.TRACERS_KESSLER_SHOC, idz.stretched_interfaces(8, 12000.0),
                                          dict(per_ens="mod16"), True, 2),
    "3d_nt1_perens_nens130_ragged_B": (130, 5, 3, 7, idz.TRACERS_NONE, idz.stretched_interfaces(7, 9000.0), dict(per_ens="mod16"), False, 1),
    "2d_bubble_A": (2, 16, 1, 20, idz.TRACERS_NONE, idz.uniform_interfaces(20, 10000.0),
                    dict(supercell=False, crm_dt=1.0), True, 3),
    # ragged sizes: nens not a multiple of 64 but > 64, line lengths not multiples of the segment
    "3d_ragged_nens70": (70, 5, 3, 7, idz.TRACERS_NONE, idz.stretched_interfaces(7, 9000.0), {}, True, 1),
    # smallest legal grid: one member, 3 cells per direction (the periodic stencil wraps the whole line twice)
    "3d_minimal_1x3x3x3": (1, 3, 3, 3, idz.TRACERS_NONE, idz.uniform_interfaces(3, 3000.0), dict(gate_factor=4.0), True, 2),
    # BASELINE configs at their true grid (32 x {32,1} x 60, L60 levels; the 61-face column is swept as two spans) with few
    # members so that the oracle finishes in seconds: C1 exactly (dry bubble, nens=2), C2's grid, C3's and C4's tracer sets
    # (the theta = 300 K bubble atmosphere ends at cp*theta/g = 30.7 km: C1 uses the reference's 20 km box, uniform levels)
    "c1_bubble_32x32x60_20km_nens2": (2, 32, 32, 60, idz.TRACERS_NONE, idz.uniform_interfaces(60, 20000.0),
                                      dict(supercell=False, dxy=625.0), True, 1),
    "c2_grid_32x32x60_L60_nens2": (2, 32, 32, 60, idz.TRACERS_NONE, idz.l60_interfaces(), {}, True, 1),
    "c3_grid_32x1x60_L60_nt4": (66, 32, 1, 60, idz.TRACERS_KESSLER_SHOC, idz.l60_interfaces(), {}, True, 1),
    "c4_grid_32x1x60_L60_nt10": (5, 32, 1, 60, idz.TRACERS_P3_SHOC, idz.l60_interfaces(), dict(consts=idz.CONSTS_P3), True, 1),
    # the reference's maximum tracer count (pam_const.h:24 max_fields = 50): water_vapor + 49 more, mixed flags
    "2d_nt50_max_tracers": (2, 6, 1, 6, [("t%02d" % i, i % 3 != 0, i % 4 == 0) for i in range(20)] +
                            [("water_vapor", True, True)] + [("u%02d" % i, i % 2 == 0, False) for i in range(29)],
                            idz.stretched_interfaces(6, 9000.0), {}, True, 1),
}
# every case above has dx == dy, and apart from the noise and the 7 m/s of the dry_air cases no flow along y
# (tests/test_anisotropy_census.py keeps the record).  The cases below have dx != dy in both orders of the ratio, nx != ny, and the
# sounding's shear along y or along both: one per kernel family, at the smallest shape that selects it.
ISOTROPIC_CASES = tuple(sorted(CASES))
_Z8 = idz.stretched_interfaces(8, 12000.0)
CASES.update({
    # flat lanes + tile kernels: 2 x 8 x 5 (a row of 8 cells x 2 members: the shuffle exchange is possible) and 5 x 6 x 7 (LDS exchange)
    "aniso_500x800_flat_2x8x5_nt1_A_flowy": (2, 8, 5, 8, idz.TRACERS_NONE, _Z8, dict(dxy=500.0, dy=800.0, flow="y"), True, 2),
    "aniso_800x500_flat_2x8x5_nt4_B_diag": (2, 8, 5, 8, idz.TRACERS_KESSLER_SHOC, _Z8, dict(dxy=800.0, dy=500.0, flow="diag"), False, 2),
    "aniso_1000x250_flat_5x6x7_nt1_B_flowy": (5, 6, 7, 8, idz.TRACERS_NONE, _Z8, dict(dxy=1000.0, dy=250.0, flow="y"), False, 2),
    "aniso_500x800_flat_5x6x7_nt4_A_diag": (5, 6, 7, 8, idz.TRACERS_KESSLER_SHOC, _Z8, dict(dxy=500.0, dy=800.0, flow="diag"), True, 2),
    # member lanes, a whole block and a ragged one, the limiter acting on vapour across the dry rows in y: NT = 1 (tail fusion), NT = 4
    "aniso_800x500_nens64_nt1_vapour_limited_flowy": (64, 6, 5, 8, idz.TRACERS_NONE, _Z8,
                                                      dict(dxy=800.0, dy=500.0, flow="y", dry_air=True), True, 2),
    "aniso_500x800_nens70_ragged_nt4_vapour_limited_flowy_B": (70, 5, 7, 8, idz.TRACERS_KESSLER_SHOC, _Z8,
                                                               dict(dxy=500.0, dy=800.0, flow="y", dry_air=True), False, 2),
    # per-member vertical grids with member lanes
    "aniso_500x800_perens_nens64_nt4_diag": (64, 6, 5, 8, idz.TRACERS_KESSLER_SHOC, _Z8,
                                             dict(dxy=500.0, dy=800.0, flow="diag", per_ens="mod16"), True, 2),
    # NT = 10
    "aniso_800x500_nt10_p3_flowy": (3, 6, 5, 8, idz.TRACERS_P3_SHOC, _Z8,
                                    dict(dxy=800.0, dy=500.0, flow="y", consts=idz.CONSTS_P3), True, 2),
})
ANISOTROPIC_CASES = tuple(sorted(set(CASES) - set(ISOTROPIC_CASES)))
FLOOR_SEED = 0             # the seed of the named cases' twins


FLOWS = ("x", "y", "diag")


def _turn_wind(f, flow, dry_air, ny):
    """the sounding's shear (u(z), v = 0: idealized.supercell_column) along x (today's inputs), along y, or along both at once with
    different values and signs; with dry_air, the mean wind that carries the vapour across the carved edges"""
    su = f["uvel"].copy()
    if flow == "y":          # the shear along y, a fifth of it left along x
        f["vvel"] = su
        f["uvel"] = 0.2 * su
    elif flow == "diag":     # u in [-9, 15], v in [-14, 4] m/s
        f["uvel"] = 0.8 * su + 3.0
        f["vvel"] = -0.6 * su - 5.0
    elif flow != "x":
        raise ValueError("flow must be one of %s" % (FLOWS,))
    if dry_air:
        if flow == "x":
            f["uvel"] -= 25.0
            f["vvel"] += 7.0 if ny > 1 else 0.0
        elif flow == "y":    # the x case turned: 25 m/s across the dry rows in y, 7 m/s across the slabs in x
            f["vvel"] -= 25.0
            f["uvel"] += 7.0
        else:                # as strong along y as along x
            f["uvel"] -= 20.0
            f["vvel"] += 20.0


def _add_turned_tracer_blobs(f, tracers, xlen, ylen, zint, rel=1.0e-3):
    """idealized.add_tracer_blobs turned into y: the blob centres spread along y (off the y centre line, where that one puts every
    blob) at one x off the x centre line, and the two horizontal half-widths swapped.  No half-width is less than 0.75 cells (of the thickest
    level, in z), so that at any dx/dy and on the coarsest grids every blob still holds a cell centre."""
    nt, nz, ny, nx, nens = f["tracers"].shape
    zmid = 0.5 * (zint[:-1] + zint[1:])
    dx, dy = xlen / nx, ylen / ny
    Z, Y, X = np.meshgrid(zmid, (np.arange(ny) + 0.5) * dy, (np.arange(nx) + 0.5) * dx, indexing="ij")
    ztop = zint[-1]
    rho = f["density_dry"]
    for t, (name, _, _) in enumerate(tracers):
        if name == "water_vapor":
            continue
        y0 = ylen * (0.2 + 0.6 * ((t * 0.37) % 1.0))
        z0 = ztop * (0.05 + 0.25 * ((t * 0.61) % 1.0))
        blob = idz.sample_ellipse_cosine(1.0, X, Y, Z, xlen * 0.35, y0, z0, max(ylen * 0.15, 0.75 * dx), max(xlen * 0.15, 0.75 * dy),
                                         max(ztop * 0.06, 0.75 * np.diff(zint).max()))
        if name == "tke":
            f["tracers"][t] = rho * (0.1 * blob[..., None] + 0.0)
        else:
            f["tracers"][t] = rho * (rel * (1.0 + 0.1 * t)) * blob[..., None] * (1.0 + 0.01 * np.arange(nens))
    return f


def build_inputs(nens, nx, ny, nz, tr, zint, consts=idz.CONSTS_DEFAULT, supercell=True, per_ens=False, mag=0.5, dxy=500.0,
                 dry_air=False, dy=None, flow="x", id0=0):
    """the seeded input fields of a case and its grid: (fields, xlen, ylen, interfaces (nz+1, nens), dz (nz, nens)).  `dxy` is the
    spacing in x and, unless `dy` is given, in y; `flow` is the direction of the sounding's shear and of the tracer blobs' spread
    (FLOWS; "x" is the supercell state as pam_amd.idealized builds it); `id0` is the seed offset of the temperature noise."""
    if flow != "x" and (ny == 1 or not supercell):
        raise ValueError("flow=%r needs a 3-D supercell case" % flow)
    xlen = nx * dxy
    ylen = ny * (dxy if dy is None else dy) if ny > 1 else xlen
    if supercell:
        f = idz.supercell_fields(nens, nx, ny, nz, zint, consts=consts, tracers=tr, magnitude=mag, id0=id0)
        (idz.add_tracer_blobs if flow == "x" else _add_turned_tracer_blobs)(f, tr, xlen, ylen, zint)
        _turn_wind(f, flow, dry_air, ny)
        if dry_air:      # exact zeros in the vapour beside moist air + a mean wind across the edges: the limiter acts on water_vapor
            idz.carve_dry_air(f, tr)
    else:
        f = idz.dry_bubble_fields(nens, nx, ny, nz, xlen, ylen, zint, consts=consts, tracers=tr)
    zi = np.asarray(zint)[:, None] * np.ones((1, nens))
    if per_ens == "mod16":
        zi = zi * (1 + 0.01 * (np.arange(nens) % 16) + 1.0e-4 * (np.arange(nens) // 16))[None, :]
    elif per_ens:
        zi = zi * (1 + 0.01 * np.arange(nens))[None, :]
    return f, xlen, ylen, zi, np.diff(zi, axis=0)


class OracleCase:
    """a case as the oracle sees it: `fields` (the inputs), `run(f)` (declare the hydrostatic profile of `f`, then `nsteps`
    timeSteps of `crm_dt`, in place; returns the sub-step count) and `floor()` (parity_gate.noise_floor of that run)"""

    def __init__(self, nens, nx, ny, nz, tr, zint, consts=idz.CONSTS_DEFAULT, supercell=True, per_ens=False, mag=0.5, crm_dt=2.0,
                 dxy=500.0, dry_air=False, mode_a=True, nsteps=1, gate_factor=1.0, dy=None, flow="x"):
        self.dims = (nens, nx, ny, nz)
        self.flow, self.dry_air = flow, dry_air
        self.tracers, self.consts, self.crm_dt, self.mode_a, self.nsteps, self.gate_factor = tr, consts, crm_dt, mode_a, nsteps, gate_factor
        self.names, self.pos, self.mass, self.idwv = idz.tracer_flags(tr)
        self.fields, self.xlen, self.ylen, self.zi, self.dz = build_inputs(nens, nx, ny, nz, tr, zint, consts, supercell, per_ens,
                                                                           mag, dxy, dry_air, dy, flow)
        self.dx, self.dy = self.xlen / nx, self.ylen / ny

    def oracle(self, consts=None, ylen=None):
        """the case's oracle; `ylen` replaces the case's own (tests/test_anisotropy_census.py: the grid a dy -> dx slip would see)"""
        nens, nx, ny, nz = self.dims
        o = ao.OracleDycore(nens, nx, ny, nz, self.xlen, self.ylen if ylen is None else ylen, self.dz, self.pos, self.mass, self.idwv,
                            consts=self.consts if consts is None else consts)
        if not self.mode_a:
            o.set_grav_balance(False)
        return o

    def run(self, f, consts=None, ylen=None):
        o = self.oracle(consts, ylen)
        o.declare_current_profile_as_hydrostatic(f)
        return sum(o.time_step(f, self.crm_dt)[0] for _ in range(self.nsteps))

    def floor(self, base=None, seed=FLOOR_SEED):
        return noise_floor(self.run, self.fields, self.names, seed, base=base)

    def inputs(self):
        return copy.deepcopy(self.fields)


def named_case(name):
    nens, nx, ny, nz, tr, zint, kw, mode_a, nsteps = CASES[name]
    return OracleCase(nens, nx, ny, nz, tr, zint, mode_a=mode_a, nsteps=nsteps, **kw)
