"""The two time-step limits that are a device minimum over every cell of the ensemble -- the dycore's CFL step (awfl_cfl_kernel / cfl_body)
and Kessler's sedimentation limit (kessler_limit_kernel / kessler_limit_column) -- BY VALUE, with the minimum planted in one chosen cell.

A reduction that drops a cell returns a step that is too long and nothing else in a run notices; on a smooth state thousands of cells
sit within a fraction of a percent of the minimum, so a comparison of the minimum alone does not notice either.  Here the state is quiet
and ONE cell is made the limiter by a wide margin: its limit is at most half of every other cell's (asserted on the reference array,
time_step_limits_ref.undercuts), so a lane, wavefront, workgroup, tail, grid-stride pass or dealt level that is skipped is a factor-2
error.  The planted positions are the edges of the launch: flat index 0, 63, 64, 255, 256, the first and last lane of each of a
workgroup's four wavefronts, the partial last workgroup, the first and last cell of the second grid-stride pass (above 2048 x 256 cells),
the last member of a ragged ensemble at the top level; for Kessler the same columns at level 0, level nz-2 and a level that a workgroup
reaches in its second round of dealt levels.  test_planted_positions_reach_every_class checks that list against the launch geometry.

References: tests/time_step_limits_ref.py (numpy.longdouble, one value per cell), tied on the CPU to the oracle -- which
test_reference_pin.py pins to the reference model bit for bit -- and to the host emulation of the same device bodies.

Gates.  CFL: 1e-14 relative, the gate of test_gpu_parity.  Kessler: 1e-14 relative as well -- pow_pos_fast is within 0.55 ulp
(test_pow_pos.py), division and sqrt are correctly rounded and there are fewer than ten rounded operations, so the device is a few ulp
(~1e-15) from the longdouble value.  Both tests print the worst ratio they saw, and in how many plants the device gave the bits of the
host emulation (not asserted); docs/experiments.md has the figures measured on the device: 2.2e-16 (CFL) and 2.3e-16 (Kessler).

Not covered: the 64-bit index path of cfl_body (above 2^32 cells: out of reach of a test of seconds) and the all-reduce across
processes (test_sharding_*)."""
import functools
import os
import re

import numpy as np
import pytest

import kessler_cases as kc
import time_step_limits_ref as ref
from emu_harness import EmuDycore
from oracle import awfl_oracle as ao
from pam_amd import idealized as idz
from pam_amd.micro import Microphysics
from test_kessler_emu import emu_dt_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
GATE = 1e-14
CONSTS = idz.derived_constants(idz.CONSTS_DEFAULT)
R_D, R_V, GAMMA = CONSTS["R_d"], CONSTS["R_v"], CONSTS["gamma_d"]
TR = idz.TRACERS_NONE
DX, DY = 500.0, 700.0          # dx != dy: an x-limited and a y-limited cell give different values
WG, WAVE, MAX_WG = 256, 64, 2048      # awfl_cfl_kernel: lanes per workgroup and wavefront, the cap of launch_cfl
PASS = WG * MAX_WG                   # 524 288: the first cell of the second grid-stride pass


def _rel(got, exp):
    return float(abs(LD(got) - exp) / exp)


# ==============================================================================================================================
# CFL

# (nens, nx, ny, nz): below one workgroup (2-D); a ragged ensemble of 64 + 6 members, 7350 cells = 28 workgroups + 182 cells = 114
# wavefronts + 54 cells (3-D; two member ranges are 64 + 6); 532 480 cells = one full pass of 2048 workgroups + 8192 cells (two member
# ranges are 128 + 2)
CFL_SHAPES = {"small": (3, 5, 1, 4), "ragged": (70, 5, 3, 7), "two_pass": (130, 32, 8, 16)}
KINDS = ("u", "v", "w", "temp")
FIELD_OF = {"u": "uvel", "v": "vvel", "w": "wvel", "temp": "temp", "rho_d": "density_dry"}
LIMITER_OF = {"u": "x", "v": "y", "w": "z", "temp": "x"}     # (dx is the shortest of dx, dy and every dz of these grids)


class CflCase:
    """a quiet state on a per-member grid (member e's levels are 1 + 0.01 e times member 0's), its per-cell limits, and the plants.
    thin = (k, e): dz of that one (level, member) entry is 100 m, a fifth of dx and less of every other dz"""

    def __init__(self, nens, nx, ny, nz, thin=None):
        self.dims, self.shape, self.ncell = (nens, nx, ny, nz), (nz, ny, nx, nens), nz * ny * nx * nens
        zint = idz.stretched_interfaces(nz, 15000.0)
        dz = np.diff(zint[:, None] * (1 + 0.01 * np.arange(nens))[None, :], axis=0)
        if thin is not None:
            dz[thin] = 100.0
        self.zi = np.concatenate([np.zeros((1, nens)), np.cumsum(dz, axis=0)])
        self.dz = np.diff(self.zi, axis=0)            # as set_grid takes it: interface differences in double
        self.xlen, self.ylen = nx * DX, ny * DY
        self.f = idz.supercell_fields(nens, nx, ny, nz, zint, tracers=TR, magnitude=0.5)
        self.rebase()

    def rebase(self, f=None):
        """the per-cell reference of the state `f` (default: the case's own)"""
        if f is not None:
            self.f = f
        self.lim, self.dirn = ref.cfl_limits(self.f, 0, DX, DY, self.dz, R_D, R_V, GAMMA)
        self.argmin, self.base_min, self.second = ref.two_smallest(self.lim)

    def oracle(self):
        nens, nx, ny, nz = self.dims
        names, pos, mass, idwv = idz.tracer_flags(TR)
        return ao.OracleDycore(nens, nx, ny, nz, self.xlen, self.ylen, self.dz, pos, mass, idwv, consts=idz.CONSTS_DEFAULT)

    def emu(self):
        nens, nx, ny, nz = self.dims
        names, pos, mass, idwv = idz.tracer_flags(TR)
        return EmuDycore(nens, nx, ny, nz, self.xlen, self.ylen, self.dz, pos, mass, idwv, consts=idz.CONSTS_DEFAULT)

    def cell_values(self, cell):
        v = {k: self.f[name].reshape(-1)[cell] for k, name in FIELD_OF.items()}
        v["rho_v"] = self.f["tracers"][0].reshape(-1)[cell]
        return v

    def plant(self, kind, cell, target=None):
        """make `cell` (flat index, nens fastest) the limiter through `kind`: a wind against the axis (u, v, w < 0: the kernel takes
        |.|) that brings the cell's limit to `target` (default: a quarter of the state's minimum), or 25 times its temperature (five
        times its speed of sound).  Returns (field, value to store, expected minimum, limiting direction); the margin is asserted"""
        k, j, i, e = np.unravel_index(cell, self.shape)
        v = self.cell_values(cell)
        dz = self.dz[k, e]
        if target is None:
            target = self.base_min / 4
        if kind == "temp":
            v["temp"] = v["temp"] * 25.0
        else:
            cs = LD(0.8) * LD(DX) / ref.cfl_cell(dx=DX, dy=DY, dz=dz, R_d=R_D, R_v=R_V, gamma=GAMMA, **v)[0] - abs(LD(v["u"]))
            v[kind] = -float(LD(0.8) * LD({"u": DX, "v": DY, "w": dz}[kind]) / target - cs)
        three = ref.cfl_cell(dx=DX, dy=DY, dz=dz, R_d=R_D, R_v=R_V, gamma=GAMMA, **v)
        exp, d = min(three), int(np.argmin(three))
        others = self.second if cell == self.argmin else self.base_min
        assert exp * 2 <= others, (kind, cell, exp, others)            # the planting condition (module docstring)
        assert ref.DIRECTIONS[d] == LIMITER_OF[kind], (kind, cell, three)
        return FIELD_OF[kind], float(v[kind]), exp, ref.DIRECTIONS[d]

    def stored(self, field):
        return self.f["tracers"][0] if field == "water_vapor" else self.f[field]

    def planted_fields(self, field, cell, value):
        f = {k: a.copy() for k, a in self.f.items()}
        (f["tracers"][0] if field == "water_vapor" else f[field]).reshape(-1)[cell] = value
        return f

    def emulated(self, field, cell, value):
        """cfl_body on the host (g++), reduced by a plain loop, for the state with `value` planted: what the device's bits are
        compared with.  Kept: the tests of both chunk settings ask for the same plants"""
        if not hasattr(self, "_emu"):
            self._emu, self._emulated = self.emu(), {}
        key = (field, cell, value)
        if key not in self._emulated:
            self._emulated[key] = self._emu.compute_time_step(self.planted_fields(field, cell, value))
        return self._emulated[key]


def cfl_positions(nens, nx, ny, nz):
    """the planted flat indices of a shape, by name"""
    ncell, sz = nens * nx * ny * nz, nens * nx * ny
    pos = {"cell_%d" % c: c for c in (0, 63, 64, 255, 256)}
    for wave in range(4):                     # the second workgroup: no lane of it is cell 0
        pos["wg1_wave%d_first" % wave] = WG + WAVE * wave
        pos["wg1_wave%d_last" % wave] = WG + WAVE * wave + WAVE - 1
    pos["last_cell"] = ncell - 1
    pos["last_workgroup_first"] = (ncell - 1) // WG * WG
    pos["top_level_last_member"] = (nz - 1) * sz + nens - 1
    pos["first_pass_last"] = PASS - 1
    pos["second_pass_first"] = PASS
    for wave in range(4):
        pos["second_pass_wave%d_last" % wave] = PASS + WAVE * wave + WAVE - 1
    return {n: c for n, c in pos.items() if 0 <= c < ncell}


@functools.lru_cache(maxsize=None)
def cfl_case(name):
    return CflCase(*CFL_SHAPES[name])


@functools.lru_cache(maxsize=None)
def cfl_plants(name):
    """[(position name, kind, cell, field, value, expected, direction)]: every kind at every position; on the large shape the kinds
    take turns over the positions (each is there several times) -- a reference of 532 480 longdoubles per plant is not free"""
    case, out = cfl_case(name), []
    for n, (pname, cell) in enumerate(sorted(cfl_positions(*CFL_SHAPES[name]).items(), key=lambda p: p[1])):
        for kind in (KINDS if name != "two_pass" else (KINDS[n % 4],)):
            out.append((pname, kind, cell) + case.plant(kind, cell))
    return out


# (level, member) whose dz is thinned, on the ragged shape: the first entry, the last (top level, last member of the ragged range), and
# the first member of the second block of 64 in a middle level
THIN = [(0, 0), (6, 69), (3, 64)]


@functools.lru_cache(maxsize=None)
def thin_case(k, e):
    return CflCase(*CFL_SHAPES["ragged"], thin=(k, e))


def thin_plants(k, e):
    """a thinned dz[k, e] makes the whole row (k, :, :, e) the smallest limits of the state; an updraft in ONE cell of the row then
    undercuts the row by four.  A kernel that takes another entry of dz for that cell gives four times the expected value."""
    case = thin_case(k, e)
    nens, nx, ny, nz = case.dims
    rows = ref.cfl_limits(case.f, 0, DX, DY, case.dz, R_D, R_V, GAMMA)[0][k, :, :, e]
    assert case.base_min == rows.min() and case.dirn.reshape(-1)[case.argmin] == 2      # the thin row limits the quiet state, through z
    out = []
    for j, i in ((0, 0), (ny - 1, nx - 1)):
        cell = int(np.ravel_multi_index((k, j, i, e), case.shape))
        out.append(("thin_dz_%d_%d_cell_%d_%d" % (k, e, j, i), "w", cell) + case.plant("w", cell))
    return case, out


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement against the oracle and the emulated cfl_body, the margins, the position list

@pytest.mark.parametrize("name", sorted(CFL_SHAPES))
def test_cfl_reference_matches_the_oracle(name):
    """the minimum of the per-cell longdouble array against oracle.compute_time_step, on the quiet state and with every kind planted.
    Both evaluate the same dozen operations, the oracle with a rounding of 2^-53 after each: 4e-15 covers them several times over"""
    case, o = cfl_case(name), cfl_case(name).oracle()
    assert _rel(o.compute_time_step(case.f), case.base_min) <= 4e-15
    seen = set()
    for pname, kind, cell, field, value, exp, d in cfl_plants(name):
        if kind in seen and pname != "top_level_last_member":
            continue
        seen.add(kind)
        f = case.planted_fields(field, cell, value)
        lim, dirn = ref.cfl_limits(f, 0, DX, DY, case.dz, R_D, R_V, GAMMA)
        assert lim.min() == exp and int(lim.argmin()) == cell and ref.undercuts(lim, cell), (pname, kind)     # the one-cell update
        assert ref.DIRECTIONS[dirn.reshape(-1)[cell]] == d
        assert _rel(o.compute_time_step(f), exp) <= 4e-15, (pname, kind)
    assert seen == set(KINDS)


@pytest.mark.parametrize("k,e", THIN)
def test_cfl_reference_matches_the_oracle_on_a_thin_dz_entry(k, e):
    case, plants = thin_plants(k, e)
    o = case.oracle()
    assert _rel(o.compute_time_step(case.f), case.base_min) <= 4e-15
    for pname, kind, cell, field, value, exp, d in plants:
        assert d == "z"
        assert _rel(o.compute_time_step(case.planted_fields(field, cell, value)), exp) <= 4e-15, pname


@pytest.mark.parametrize("name", ["small", "ragged"])
def test_emulated_cfl_body_gives_every_planted_minimum(name):
    """cfl_body as g++ compiles it (its 32-bit shortcut to dz[k, e] included), reduced by a plain loop: every plant of the two
    small shapes and of the thinned grids"""
    cases = [(cfl_case(name), cfl_plants(name))] + ([thin_plants(k, e) for k, e in THIN] if name == "ragged" else [])
    worst = 0.0
    for case, plants in cases:
        g = case.emu()
        assert _rel(g.compute_time_step(case.f), case.base_min) <= GATE
        for pname, kind, cell, field, value, exp, d in plants:
            got = g.compute_time_step(case.planted_fields(field, cell, value))
            worst = max(worst, _rel(got, exp))
            assert _rel(got, exp) <= GATE, (pname, kind, got, exp)
    print("emulated cfl_body, %s: worst |emu - ref| / ref = %.3g" % (name, worst))


def test_emulated_cfl_body_on_the_two_pass_shape():
    """the cells on both sides of 2048 x 256 and the last one, through the emulated body (one plant per position)"""
    case, g = cfl_case("two_pass"), cfl_case("two_pass").emu()
    for pname, kind, cell, field, value, exp, d in cfl_plants("two_pass"):
        if pname in ("first_pass_last", "second_pass_first", "last_cell", "top_level_last_member"):
            assert _rel(g.compute_time_step(case.planted_fields(field, cell, value)), exp) <= GATE, (pname, kind)


def unusable_values(v):
    """[(field, value)] that make a cell (its values: v) unusable: a NaN temperature; a NaN, zero or negative dry density; vapour so
    negative that the total density is (rho_d > 0 with p and rho both negative: a real speed of sound); a negative temperature.
    With each of the negative ones the reference formula gives a real, positive limit or a NaN: the answer has to be "no step" """
    return [("temp", float("nan")), ("density_dry", -v["rho_d"]), ("density_dry", 0.0), ("density_dry", float("nan")),
            ("water_vapor", -2.0 * v["rho_d"]), ("temp", -v["temp"])]


def test_emulated_cfl_body_refuses_densities_and_temperatures_that_are_not_positive():
    """rho_d = -|rho_d|, or rho_v < -rho_d, makes both the pressure and the density negative: the speed of sound comes out real and the
    cell looked healthy"""
    case, g = cfl_case("small"), cfl_case("small").emu()
    for cell in (0, case.ncell - 1):
        v = case.cell_values(cell)
        with np.errstate(invalid="ignore"):
            looks_healthy = [min(ref.cfl_cell(dx=DX, dy=DY, dz=100.0, R_d=R_D, R_v=R_V, gamma=GAMMA, **dict(v, **{k: val})))
                             for k, val in (("rho_d", -v["rho_d"]), ("rho_v", -2.0 * v["rho_d"]))]
        assert all(x > 0 for x in looks_healthy), looks_healthy          # the formula alone lets these two through
        for field, value in unusable_values(v):
            assert np.isnan(g.compute_time_step(case.planted_fields(field, cell, value))), (cell, field, value)


def launch_classes(ncell):
    """what a wrong awfl_cfl_kernel could leave out, as sets of flat indices: {class name: predicate of the flat index}"""
    nwg = min((ncell + WG - 1) // WG, MAX_WG)
    cls = {"lane_%d" % l: (lambda c, l=l: c % WAVE == l) for l in (0, WAVE - 1) if l < ncell}
    cls.update({"wave_%d" % w: (lambda c, w=w: c % WG // WAVE == w) for w in range(4) if w * WAVE < ncell})
    if ncell % WG:
        cls["partial_last_workgroup"] = lambda c: c // WG == ncell // WG
    if ncell > nwg * WG:
        cls["second_pass"] = lambda c: c >= nwg * WG
    cls["last_cell"] = lambda c: c == ncell - 1
    return cls


def test_planted_positions_reach_every_class():
    """every class of cells that a lane, a wavefront's LDS word, the tail or a grid-stride pass stands for holds a planted position,
    and the three shapes are what the module says they are"""
    n = {name: np.prod(s) for name, s in CFL_SHAPES.items()}
    assert n["small"] < WG and n["ragged"] % WAVE and n["ragged"] % WG and n["ragged"] > 4 * WG
    assert PASS < n["two_pass"] <= PASS + 8192 and CFL_SHAPES["ragged"][0] % 64
    for name, shape in CFL_SHAPES.items():
        cells = set(cfl_positions(*shape).values())
        for cname, inside in launch_classes(int(n[name])).items():
            assert any(inside(c) for c in cells), (name, cname)
    assert "second_pass" in launch_classes(int(n["two_pass"])) and "partial_last_workgroup" in launch_classes(int(n["ragged"]))
    assert {k for _, k, *_ in cfl_plants("two_pass")} == set(KINDS)
    assert {d for *_, d in cfl_plants("ragged")} | {"z"} == set(ref.DIRECTIONS)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU

def _gpu_cfl(case):
    from pam_amd import Dycore, PamCoupler
    nens, nx, ny, nz = case.dims
    coupler = PamCoupler("cuda:0")
    coupler.set_option("crm_dt", 2.0)
    for k, v in idz.CONSTS_DEFAULT.items():
        coupler.set_option(k, v)
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(case.xlen, case.ylen, case.zi)
    for n, p, m in TR:
        coupler.add_tracer(n, "", p, m)
    dycore = Dycore()
    dycore.init(coupler)
    if nens >= 64:      # a ragged ensemble below 128 members runs flat lanes by default, and those take one member range only
        dycore.set_lane_mapping("member", "sweep")
    coupler.load_fields(case.f)
    assert np.array_equal(coupler.dm.get("vertical_cell_dz", readonly=True).cpu().numpy(), case.dz)
    return coupler, dycore


@pytest.fixture(scope="module")
def gpu_cfl():
    """one coupler and dycore per shape, shared by the tests below: each leaves the state as it found it"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _gpu_cfl(cfl_case(name))
        return made[name]
    yield get
    for coupler, dycore in made.values():
        dycore.finalize(coupler)


def _set(coupler, field, cell, value):
    coupler.dm.get(field).view(-1)[cell] = value


def _set_ranges(dycore, chunks, small=False):
    """ask for `chunks` member ranges and check what the handle made of it: one range runs the copy-free form of the reduction, two
    the copying one.  (Flat lanes and tile kernels -- ensembles below 64 members, the small shape -- take the whole ensemble as one
    range whatever is asked.)"""
    dycore.set_ensemble_chunks(chunks)
    assert dycore.get_ensemble_ranges() == (1 if small else chunks), (chunks, dycore.get_ensemble_ranges(), dycore.get_lane_mapping())


def _run_plants(coupler, dycore, case, plants, what, compare=None):
    """compare: the position names whose device value is also compared, bit for bit, with the host emulation's (None: all of them);
    printed, not asserted"""
    bad, worst, same, compared = [], 0.0, 0, 0
    assert _rel(dycore.compute_time_step(coupler), case.base_min) <= GATE
    try:
        for pname, kind, cell, field, value, exp, d in plants:
            old = case.f[field].reshape(-1)[cell]
            _set(coupler, field, cell, value)
            got = dycore.compute_time_step(coupler)
            _set(coupler, field, cell, old)
            worst = max(worst, _rel(got, exp))
            if not _rel(got, exp) <= GATE:
                bad.append((pname, kind, cell, d, got, float(exp)))
            if compare is None or pname in compare:
                compared += 1
                same += got == case.emulated(field, cell, value)
    finally:
        coupler.load_fields(case.f)            # whatever happened, the shared coupler holds the quiet state again
    assert _rel(dycore.compute_time_step(coupler), case.base_min) <= GATE      # and the state is what it was
    print("%s: %d plants, worst |device - ref| / ref = %.3g; same bits as the host emulation in %d of %d compared"
          % (what, len(plants), worst, same, compared))
    assert not bad, bad


# the large shape's plants that are also run through the host emulation (532 480 cells each): those of the CPU test above
TWO_PASS_COMPARED = ("cell_0", "first_pass_last", "second_pass_first", "last_cell", "top_level_last_member")


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("name", sorted(CFL_SHAPES))
def test_gpu_cfl_returns_the_planted_minimum(gpu_cfl, name, chunks):
    """every position x every way of planting (x-, y- and z-limited, a hot cell), in the copy-free form (one member range) and the
    copying one (two)"""
    coupler, dycore = gpu_cfl(name)
    _set_ranges(dycore, chunks, small=name == "small")
    _run_plants(coupler, dycore, cfl_case(name), cfl_plants(name), "cfl %s, %d member range(s)" % (name, chunks),
                compare=TWO_PASS_COMPARED if name == "two_pass" else None)


@pytest.mark.gpu
@pytest.mark.parametrize("k,e", THIN)
def test_gpu_cfl_limited_by_one_entry_of_dz(k, e):
    """the limit hangs on dz of ONE (level, member) of a per-member grid: the 32-bit shortcut (c / sz) * nens + c % nens"""
    case, plants = thin_plants(k, e)
    coupler, dycore = _gpu_cfl(case)
    try:
        for chunks in (1, 2):
            _set_ranges(dycore, chunks)
            _run_plants(coupler, dycore, case, plants, "cfl thin dz[%d, %d], %d member range(s)" % (k, e, chunks))
    finally:
        dycore.finalize(coupler)


SEQUENCES = {"lean": (1, 1, 1, 1), "copying": (2, 2, 2, 2), "alternating": (1, 2, 1, 2, 1), "alternating_from_2": (2, 1, 2, 1, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "two_pass"])
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
def test_gpu_cfl_rising_minima_on_one_handle(gpu_cfl, name, seq):
    """minima m, 2m, 4m, 8m (, 16m) planted in turn, each in another cell, on one handle: every call returns its own.  A word that a
    launch failed to put +inf back into hands the next but one call the smaller minimum of this one."""
    coupler, dycore = gpu_cfl(name)
    case = cfl_case(name)
    cells = [3, case.ncell - 2, WG + 130, 2 * WG + 64, 77][:len(SEQUENCES[seq])]
    m = case.base_min / 40                                                # the largest is 16 m = 0.4 x the quiet minimum
    plants = [case.plant("u", c, m * 2 ** n) for n, c in enumerate(cells)]
    current, got = None, []
    try:
        for (field, value, exp, d), cell, chunks in zip(plants, cells, SEQUENCES[seq]):
            if chunks != current:
                _set_ranges(dycore, chunks)
                current = chunks
            _set(coupler, field, cell, value)
            got.append(dycore.compute_time_step(coupler))
            _set(coupler, field, cell, case.f[field].reshape(-1)[cell])
    finally:
        coupler.load_fields(case.f)
    assert all(_rel(g, p[2]) <= GATE for g, p in zip(got, plants)), (got, [float(p[2]) for p in plants])
    assert _rel(dycore.compute_time_step(coupler), case.base_min) <= GATE


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 2])
def test_gpu_cfl_words_survive_a_time_step_in_between(chunks):
    """timeStep takes its own CFL minimum through the same words: a planted call, a timeStep of the quiet state (which must sub-cycle
    on ITS minimum, not on the planted one before it), then planted calls that return their own, larger, minima"""
    import torch
    case = CflCase(*CFL_SHAPES["ragged"])
    coupler, dycore = _gpu_cfl(case)
    try:
        _set_ranges(dycore, chunks)
        dycore.declare_current_profile_as_hydrostatic(coupler)
        crm_dt = coupler.get_option("crm_dt")

        def planted_call(cell, target):
            field, value, exp, d = case.plant("u", cell, target)
            _set(coupler, field, cell, value)
            got = dycore.compute_time_step(coupler)
            _set(coupler, field, cell, case.f[field].reshape(-1)[cell])
            assert _rel(got, exp) <= GATE, (cell, got, exp)

        planted_call(5, case.base_min / 20)
        for step in range(2):
            n = dycore.timeStep(coupler)
            assert n == int(np.ceil(crm_dt / float(case.base_min))) and dycore.last_dt_dyn == crm_dt / n, (step, n, case.base_min)
            torch.cuda.synchronize()
            case.rebase(coupler.dump_fields())          # the reference of the state the device now holds
            assert _rel(dycore.compute_time_step(coupler), case.base_min) <= GATE
            planted_call(case.ncell - 7 - step, case.base_min / 10 * (step + 1))
    finally:
        dycore.finalize(coupler)


def _unusable_cells(ncell):
    return [c for c in (0, ncell - 1, PASS) if c < ncell]


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("name", ["ragged", "two_pass"])
def test_gpu_cfl_reports_an_unusable_cell_as_zero_and_recovers(gpu_cfl, name, chunks):
    """a NaN temperature, and a dry density, a total density or a temperature that is not positive (unusable_values), in the first cell,
    the last one and the first of the second pass: exactly 0.0 (the host refuses it); with the cell put right the next call returns
    the clean minimum"""
    coupler, dycore = gpu_cfl(name)
    _set_ranges(dycore, chunks)
    case = cfl_case(name)
    bad = []
    try:
        for cell in _unusable_cells(case.ncell):
            for field, value in unusable_values(case.cell_values(cell)):
                _set(coupler, field, cell, value)
                got = dycore.compute_time_step(coupler)
                _set(coupler, field, cell, case.stored(field).reshape(-1)[cell])
                clean = dycore.compute_time_step(coupler)
                if not (got == 0.0 and _rel(clean, case.base_min) <= GATE):
                    bad.append((cell, field, value, got, clean))
    finally:
        coupler.load_fields(case.f)
    assert not bad, bad


# ==============================================================================================================================
# Kessler

K_DT = 5.0
# (nens, nx, ny, nz): one workgroup, a workgroup per level; 29 120 columns = 113 workgroups + 192 columns, which leaves fewer workgroups
# than levels in y; two levels, of which only level 0 counts (1050 columns = 4 workgroups + 26)
K_SHAPES = {"small": (3, 5, 2, 6), "dealt": (130, 32, 7, 40), "two_levels": (70, 5, 3, 2)}
GRID_RULE = """const long long nxb = (ncol + 255) / 256; long long nyb = (4096 + nxb - 1) / nxb; if (nyb > nz - 1) nyb = nz - 1;
if (nyb < 1) nyb = 1; return dim3((unsigned)nxb, (unsigned)nyb);"""


def kessler_limit_grid(ncol, nz):
    """(gridDim.x, gridDim.y) of kessler_limit_kernel: GRID_RULE restated.  Skips the calling test when modules_kernels.hip no
    longer deals the levels by that rule: the shapes here were chosen by it."""
    with open(os.path.join(ROOT, "pam_amd", "csrc", "modules_kernels.hip")) as fh:
        body = re.search(r"dim3 kessler_limit_grid\(long long ncol, int nz\) \{(.*?)\n\}", fh.read(), re.S)
    if body is None or " ".join(body.group(1).split()) != " ".join(GRID_RULE.split()):
        pytest.skip("kessler_limit_grid of modules_kernels.hip is no longer the rule restated in this module: restate it and choose "
                    "the shapes again")
    nxb = (ncol + 255) // 256
    return nxb, max(1, min((4096 + nxb - 1) // nxb, nz - 1))


class KesslerCase:
    """a quiet state with a trace of rain in every cell (1e-12 kg/kg: every cell has a limit of its own, hundreds of seconds), a dry
    density that differs from column to column, and a per-member grid; its per-cell limits"""

    def __init__(self, nens, nx, ny, nz):
        self.dims, self.shape, self.ncol = (nens, nx, ny, nz), (nz, ny, nx, nens), ny * nx * nens
        zint = idz.stretched_interfaces(nz, 15000.0)
        self.zi = zint[:, None] * (1 + 0.01 * np.arange(nens))[None, :]
        self.zm = np.ascontiguousarray(0.5 * (self.zi[:-1] + self.zi[1:]))
        f = idz.supercell_fields(nens, nx, ny, nz, zint, magnitude=0.0)
        rng = np.random.default_rng(12345 + nz)
        rho = np.ascontiguousarray(f["density_dry"] * rng.uniform(0.97, 1.03, self.shape))
        zero = np.zeros(self.shape)
        self.s = dict(rho_v=zero.copy(), rho_c=zero.copy(), rho_r=1e-12 * rho, rho_dry=rho, temp=np.ascontiguousarray(f["temp"]))
        self.lim = ref.kessler_limits(self.s["rho_r"], rho, self.zm, K_DT)
        self.argmin, self.base_min, self.second = ref.two_smallest(self.lim)

    def plant(self, k, col, zm=None, lim=None):
        """heavy rain in cell (k, col) that brings its limit to a quarter of the state's minimum: (rho_r to store, expected limit)"""
        nens = self.dims[0]
        zm = self.zm if zm is None else zm
        argmin, base_min, second = (self.argmin, self.base_min, self.second) if lim is None else ref.two_smallest(lim)
        rho, rho0 = (LD(self.s["rho_dry"].reshape(self.shape[0], -1)[kk, col]) for kk in (k, 0))
        gap = LD(zm[k + 1, col % nens]) - LD(zm[k, col % nens])
        velqr = LD(0.8) * gap / (base_min / 4)
        qr = (velqr / (LD(36.34) * np.sqrt(rho0 / rho))) ** (1 / LD(0.1364)) / (LD(0.001) * rho)
        value = float(qr * rho)
        exp = _kessler_cell(value, rho, rho0, gap)
        others = second if k * self.ncol + col == argmin else base_min
        assert exp * 2 <= others, (k, col, exp, others)                # the planting condition
        return value, exp

    def planted_state(self, k, col, value):
        s = dict(self.s, rho_r=self.s["rho_r"].copy())
        s["rho_r"].reshape(self.shape[0], -1)[k, col] = value
        return s


def _kessler_cell(rho_r, rho, rho0, gap):
    """the limit of one rainy cell from its values, as time_step_limits_ref.kessler_limits has it"""
    velqr = LD(36.34) * (LD(rho_r) / rho * LD(0.001) * rho) ** LD(0.1364) * np.sqrt(rho0 / rho)
    return LD(0.8) * gap / velqr


def kessler_positions(name):
    """{name: (level, column)}: the columns at the edges of wavefronts and workgroups x level 0, the last level looked at, and -- where
    there are fewer workgroups than levels -- the first and last level of the second round"""
    nens, nx, ny, nz = K_SHAPES[name]
    ncol = nens * nx * ny
    nxb, nyb = kessler_limit_grid(ncol, nz)
    cols = sorted({c for c in (0, 63, 64, 255, 256, ncol - 1, (ncol - 1) // 256 * 256, nens - 1) if c < ncol})
    levels = sorted({0, nz - 2} | ({nyb, nz - 2} if nyb < nz - 1 else set()))
    return {"level%d_col%d" % (k, c): (k, c) for k in levels for c in cols}


@functools.lru_cache(maxsize=None)
def kessler_case(name):
    return KesslerCase(*K_SHAPES[name])


def kessler_plants(name):
    case = kessler_case(name)
    return [(pname, k, col) + case.plant(k, col) for pname, (k, col) in kessler_positions(name).items()]


def test_kessler_shapes_are_what_the_dispatch_rule_makes_of_them():
    for name, (nens, nx, ny, nz) in K_SHAPES.items():
        nxb, nyb = kessler_limit_grid(nens * nx * ny, nz)
        if name == "dealt":
            assert nyb < nz - 1 <= 2 * nyb and (nens * nx * ny) % 256, (nxb, nyb)     # a second round, and no third
            assert any(k >= nyb for k, _ in kessler_positions(name).values())
        else:
            assert nyb == nz - 1
    assert K_SHAPES["two_levels"][3] == 2


def test_kessler_reference_cell_formula_is_the_array_formula():
    """KesslerCase.plant evaluates one cell; kessler_limits the array: the same numbers, and the margin holds on the whole array"""
    for name in ("small", "two_levels"):
        case = kessler_case(name)
        for pname, k, col, value, exp in kessler_plants(name):
            s = case.planted_state(k, col, value)
            lim = ref.kessler_limits(s["rho_r"], s["rho_dry"], case.zm, K_DT)
            assert lim.min() == exp and int(lim.argmin()) == k * case.ncol + col and ref.undercuts(lim, k * case.ncol + col), pname


@pytest.mark.parametrize("i", range(len(kc.NAMED)), ids=kc.NAMED_IDS)
def test_kessler_reference_and_emulation_on_the_named_cases(i):
    """the minimum of the per-cell array gives the oracle's sub-cycle count, and the emulated limit agrees with it BY VALUE however the
    levels are dealt (the count is 1 in most cases: a fall speed wrong by tens of percent leaves it unchanged)"""
    zi, zm, s, dt, _ = kc.named_state(kc.NAMED[i])
    lim = ref.kessler_limits(s["rho_r"], s["rho_dry"], zm, dt)
    _, n_ref = kc.run_oracle(s, zm, dt)
    assert Microphysics.rainsplit_for(dt, float(lim.min())) == n_ref
    worst = 0.0
    for level_step in (1, 3, s["temp"].shape[0] - 1):
        rc, dt_max = emu_dt_max(s, zm, dt, level_step)
        worst = max(worst, _rel(dt_max, lim.min()))
        assert rc == 0 and _rel(dt_max, lim.min()) <= GATE, (level_step, dt_max, lim.min())
    print("emulated kessler limit, %s: worst |emu - ref| / ref = %.3g" % (kc.NAMED_IDS[i], worst))


@pytest.mark.parametrize("name", sorted(K_SHAPES))
def test_emulated_kessler_limit_gives_every_planted_minimum(name):
    """the emulated column body with the levels dealt as the launch deals them: every plant, rain at the top level alone, no rain"""
    case = kessler_case(name)
    nens, nx, ny, nz = case.dims
    nxb, nyb = kessler_limit_grid(case.ncol, nz)
    rc, dt_max = emu_dt_max(case.s, case.zm, K_DT, nyb)
    assert rc == 0 and _rel(dt_max, case.base_min) <= GATE
    for pname, k, col, value, exp in kessler_plants(name):
        rc, dt_max = emu_dt_max(case.planted_state(k, col, value), case.zm, K_DT, nyb)
        assert rc == 0 and _rel(dt_max, exp) <= GATE, (pname, dt_max, exp)
    for s in _rain_free_variants(case):
        assert emu_dt_max(s, case.zm, K_DT, nyb) == (0, K_DT)


def _rain_free_variants(case):
    """no rain at all; heavy rain in every column of the top level alone, which the limit leaves out on purpose"""
    none = dict(case.s, rho_r=np.zeros(case.shape))
    top = dict(case.s, rho_r=np.zeros(case.shape))
    top["rho_r"][-1] = 5e-3 * case.s["rho_dry"][-1]
    assert (ref.kessler_limits(top["rho_r"], top["rho_dry"], case.zm, K_DT) == K_DT).all()
    return none, top


def _thin_gap(case, k, e):
    """zmid with the gap between levels k and k+1 of member e at a quarter: the whole row (k, :, :, e) undercuts the state"""
    zm = case.zm.copy()
    zm[k + 1:, e] -= 0.75 * (zm[k + 1, e] - zm[k, e])
    lim = ref.kessler_limits(case.s["rho_r"], case.s["rho_dry"], zm, K_DT)
    return zm, lim


def _thin_gap_cases(name):
    nens, nx, ny, nz = K_SHAPES[name]
    nxb, nyb = kessler_limit_grid(nens * nx * ny, nz)
    return [(0, 0), (nz - 2, nens - 1)] + ([(nyb, 64)] if nyb < nz - 1 else [])


@pytest.mark.parametrize("name", ["small", "dealt"])
def test_emulated_kessler_limit_hangs_on_one_gap_of_zmid(name):
    case = kessler_case(name)
    nens, nx, ny, nz = case.dims
    nxb, nyb = kessler_limit_grid(case.ncol, nz)
    for k, e in _thin_gap_cases(name):
        zm, lim = _thin_gap(case, k, e)
        col = (case.ncol - nens) + e                     # the last horizontal cell's column of that member
        value, exp = case.plant(k, col, zm, lim)
        rc, dt_max = emu_dt_max(case.planted_state(k, col, value), zm, K_DT, nyb)
        assert rc == 0 and _rel(dt_max, exp) <= GATE, (k, e, dt_max, exp)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU

@pytest.fixture(scope="module")
def gpu_kessler():
    import test_micro_kessler as tk
    made = {}

    def get(name):
        if name not in made:
            case = kessler_case(name)
            made[name] = tk._gpu_setup(case.s, case.zi, *case.dims, K_DT)
        return made[name]
    yield get
    for coupler, micro, dm in made.values():
        micro.finalize(coupler)


def _set_rain(dm, case, k, col, value):
    dm.get("precip_liquid").view(case.shape[0], -1)[k, col] = value


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(K_SHAPES))
def test_gpu_kessler_limit_returns_the_planted_minimum(gpu_kessler, name):
    """heavy rain in one cell at every position, and one thinned gap of zmid per (level, member) class, against the longdouble value;
    prints the worst ratio and whether device and host emulation gave the same bits"""
    import torch
    coupler, micro, dm = gpu_kessler(name)
    case = kessler_case(name)
    nens, nx, ny, nz = case.dims
    nxb, nyb = kessler_limit_grid(case.ncol, nz)
    bad, worst, same_bits, compared = [], 0.0, 0, 0
    # (the large shape's emulation walks 1.1 million cells a call: compared at the first and the last column of every planted level)
    compare = {pname for pname, k, col, *_ in kessler_plants(name) if name != "dealt" or col in (0, case.ncol - 1)}
    got = micro.max_stable_dt(coupler)
    assert _rel(got, case.base_min) <= GATE, (got, case.base_min)
    plants = kessler_plants(name)
    for pname, k, col, value, exp in plants:
        _set_rain(dm, case, k, col, value)
        got = micro.max_stable_dt(coupler)
        _set_rain(dm, case, k, col, case.s["rho_r"].reshape(nz, -1)[k, col])
        worst = max(worst, _rel(got, exp))
        if pname in compare:
            compared += 1
            same_bits += got == emu_dt_max(case.planted_state(k, col, value), case.zm, K_DT, nyb)[1]
        if not _rel(got, exp) <= GATE:
            bad.append((pname, got, float(exp)))
    zmid = dm.get("vertical_midpoint_height")
    for k, e in _thin_gap_cases(name) if name != "two_levels" else []:
        zm, lim = _thin_gap(case, k, e)
        col = (case.ncol - nens) + e
        value, exp = case.plant(k, col, zm, lim)
        zmid.copy_(torch.from_numpy(zm))
        _set_rain(dm, case, k, col, value)
        got = micro.max_stable_dt(coupler)
        _set_rain(dm, case, k, col, case.s["rho_r"].reshape(nz, -1)[k, col])
        zmid.copy_(torch.from_numpy(case.zm))
        worst = max(worst, _rel(got, exp))
        if not _rel(got, exp) <= GATE:
            bad.append(("thin_gap_%d_%d" % (k, e), got, float(exp)))
    assert _rel(micro.max_stable_dt(coupler), case.base_min) <= GATE
    print("kessler limit %s: %d plants, worst |device - ref| / ref = %.3g; same bits as the host emulation in %d of %d compared"
          % (name, len(plants), worst, same_bits, compared))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(K_SHAPES))
def test_gpu_kessler_limit_without_rain_below_the_top_is_dt_exactly(gpu_kessler, name):
    import torch
    coupler, micro, dm = gpu_kessler(name)
    case = kessler_case(name)
    rr = dm.get("precip_liquid")
    try:
        for s in _rain_free_variants(case):
            rr.copy_(torch.from_numpy(s["rho_r"]))
            assert micro.max_stable_dt(coupler) == K_DT
    finally:
        rr.copy_(torch.from_numpy(case.s["rho_r"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "dealt"])
def test_gpu_kessler_refuses_unusable_rain_wherever_it_is(gpu_kessler, name):
    """NaN and negative rain in the first column, the last column and (where the levels are dealt) a level of the second round: both
    entry points raise PAM_AMD_ESTATE and every coupler array is bit for bit what it was -- the assertion of
    test_gpu_kessler_refuses_an_unusable_state_and_touches_nothing, at these positions"""
    import torch
    from pam_amd.capi import PamAmdError
    coupler, micro, dm = gpu_kessler(name)
    case = kessler_case(name)
    nens, nx, ny, nz = case.dims
    nxb, nyb = kessler_limit_grid(case.ncol, nz)
    where = [(0, 0), (1, case.ncol - 1), (nz - 2, case.ncol - 1)] + ([(nyb, 300), (nz - 2, 0)] if nyb < nz - 1 else [])
    names = ["water_vapor", "cloud_liquid", "precip_liquid", "density_dry", "temp", "precl"]
    for k, col in where:
        for value in (float("nan"), -1e-6):
            _set_rain(dm, case, k, col, value)
            before = {n: dm.get(n).clone() for n in names}
            for call in (lambda: micro.timeStep(coupler), lambda: micro.max_stable_dt(coupler)):
                with pytest.raises(PamAmdError, match="sedimentation time-step limit is not positive") as err:
                    call()
                assert "[code -4]" in str(err.value), (k, col, value)
                torch.cuda.synchronize()
                for n in names:
                    assert torch.equal(dm.get(n).view(torch.int64), before[n].view(torch.int64)), (k, col, value, n)
            _set_rain(dm, case, k, col, case.s["rho_r"].reshape(nz, -1)[k, col])
    assert _rel(micro.max_stable_dt(coupler), case.base_min) <= GATE
