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
FLOOR_SEED = 0             # the seed of the named cases' twins


def build_inputs(nens, nx, ny, nz, tr, zint, consts=idz.CONSTS_DEFAULT, supercell=True, per_ens=False, mag=0.5, dxy=500.0,
                 dry_air=False):
    """the seeded input fields of a case and its grid: (fields, xlen, ylen, interfaces (nz+1, nens), dz (nz, nens))"""
    xlen = nx * dxy
    ylen = ny * dxy if ny > 1 else xlen
    if supercell:
        f = idz.supercell_fields(nens, nx, ny, nz, zint, consts=consts, tracers=tr, magnitude=mag)
        idz.add_tracer_blobs(f, tr, xlen, ylen, zint)
        if dry_air:      # exact zeros in the vapour beside moist air + a mean wind across the edges: the limiter acts on water_vapor
            f["uvel"] -= 25.0
            f["vvel"] += 7.0 if ny > 1 else 0.0
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
                 dxy=500.0, dry_air=False, mode_a=True, nsteps=1, gate_factor=1.0):
        self.dims = (nens, nx, ny, nz)
        self.tracers, self.consts, self.crm_dt, self.mode_a, self.nsteps, self.gate_factor = tr, consts, crm_dt, mode_a, nsteps, gate_factor
        self.names, self.pos, self.mass, self.idwv = idz.tracer_flags(tr)
        self.fields, self.xlen, self.ylen, self.zi, self.dz = build_inputs(nens, nx, ny, nz, tr, zint, consts, supercell, per_ens,
                                                                           mag, dxy, dry_air)

    def oracle(self, consts=None):
        nens, nx, ny, nz = self.dims
        o = ao.OracleDycore(nens, nx, ny, nz, self.xlen, self.ylen, self.dz, self.pos, self.mass, self.idwv,
                            consts=self.consts if consts is None else consts)
        if not self.mode_a:
            o.set_grav_balance(False)
        return o

    def run(self, f, consts=None):
        o = self.oracle(consts)
        o.declare_current_profile_as_hydrostatic(f)
        return sum(o.time_step(f, self.crm_dt)[0] for _ in range(self.nsteps))

    def floor(self, base=None, seed=FLOOR_SEED):
        return noise_floor(self.run, self.fields, self.names, seed, base=base)

    def inputs(self):
        return copy.deepcopy(self.fields)


def named_case(name):
    nens, nx, ny, nz, tr, zint, kw, mode_a, nsteps = CASES[name]
    return OracleCase(nens, nx, ny, nz, tr, zint, mode_a=mode_a, nsteps=nsteps, **kw)
