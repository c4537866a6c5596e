"""States, per-level scale and gate of the GCM forcing tests (tests/test_gcm_forcing_cells.py).  No GPU, no test of its own.

state(): a CRM with a real column's dynamic range -- water falls off with height by four decades, ice rises with it -- whose cloud and
ice are exactly zero in 40 % of the cells, drawn cell by cell: a cloud-free cell beside a cloudy one goes negative under any negative
tendency, so the level pass of fill_holes (pam_core/modules/gcm_forcing.h:243-250) runs on every application, as it does in a real run.
Scenarios are dealt to the members round-robin and touch that member's columns only; between them they send every species through
the level pass and through the whole-CRM fallback (:252-272), alone and together, and the number concentrations into their clamps
(:391-393).

The gate is per (field, level, member).  Every error term of the module is a rounding of something the level holds or is relaxed to:
the horizontal mean of the level, the GCM value, the mass the level's cells pay for its holes.  So a cell of a water, number, density
or wind field is held to tol x S, S[k,e] = max(max over the level's cells of |input|, the same of the oracle's output, |gcm[k,e]|);
temp element-wise and relative; each of the 14 tendencies per (level, member) to tol x max(|gcm value|, |level mean|) / dt_gcm of its
OWN field (a mixing ratio for qv, ql, qi, their sum for qtot; the level means before and after the application for the three density
tendencies, which apply diagnoses from the updated cells).  Where a scale is zero the device's value must be exactly zero.  tol =
parity_gate.floor_gate(floor, 1e-11) = 4 x floor, not below 1e-12: the form and factor of tests/kessler_cases.py; floor = the oracle's
own response, in the same units, to three twins of the case whose ten CRM fields carry one ulp of noise (two seeded +-1 ulp draws per
cell, and every value one ulp away from zero).  An exact zero stays zero in a twin: a cloud-free cell is a fact of the state, not a
rounded number.  On top of the gate, exactly: the hole-filling mask of every application, and the set of water cells that are zero
after it -- yakl_max(0, ...) and the `< 0` clamps are decisions, not roundings.  The bound this replaces, 1e-12 x max|field|, lets a
relative error of 1e-8 through in a level that holds 1e-4 of the field's maximum; tests/test_gcm_forcing_cells.py shows it."""
import copy
import functools

import numpy as np

import parity_gate as pg
from oracle import awfl_oracle as ao

CRM, GCM, TEND = ao.GCM_FORCING_CRM, ao.GCM_FORCING_GCM, ao.GCM_FORCING_TEND
WATER = ("water_vapor", "cloud_water", "ice")
GCM_WATER = ("gcm_water_vapor", "gcm_cloud_water", "gcm_cloud_ice")
NUM = ("cloud_water_num", "ice_num", "rain_num")
GCM_NUM = ("gcm_num_liq", "gcm_num_ice", "gcm_num_rain")
T = "gcm_forcing_tend_"
DIAGNOSED = tuple(T + n for n in ("rho_v", "rho_l", "rho_i"))       # written by apply; the other eleven by compute
COMPUTED = tuple(n for n in TEND if n not in DIAGNOSED)
DT_GCM, CRM_DT, NAPP = 1200.0, 300.0, 4
TOL_CAP = 1e-11            # the base of the curve of parity_gate.tol_noise_fields
FLOOR_MAX = 2.5e-13        # a named case whose oracle floor is above this amplifies noise: rejected as an input (4 x = 1e-12)

MIXED = ("plain", "level0", "glob1", "level2", "numclamp", "glob2", "level1", "glob0", "level_all", "glob_all")
SINGLES = ("plain", "level0", "level1", "level2", "glob0", "glob1", "glob2", "level_all", "glob_all", "numclamp")


def state(nens, nx, ny, nz, seed, scenarios):
    """crm (dict name -> (nz,ny,nx,nens)), gcm (dict name -> (nz,nens)) and dz (nz,nens).  prof[k] = exp(-9 k/(nz-1)):
      density_dry 1.2 prof^0.25 x U(0.95, 1.05); temp 300 -> 240 K + N(0, 1); uvel, vvel N(0, 8)
      vapour 0.015 prof x U(0.5, 1.5); cloud 1e-3 prof x U(0.5, 1.5); ice 1e-4 prof reversed in height x U(0.5, 1.5);
      cloud and ice zeroed in 40 % of the cells, each cell on its own; the number fields 1e8, 1e5, 1e4 x prof x U(0, 2)
    The GCM columns are the CRM's level means x U(0.9, 1.1).  Member e plays scenarios[e % len(scenarios)]:
      plain      nothing more: only the cloud-free cells go negative
      level<s>   every other x-column of species s x 0.02 and its GCM column x 0.5: the poor columns go negative, the level can pay
      glob<s>    the species' GCM value at level nz//3 x -0.2 (-0.02 for vapour): the level cannot pay, the whole-CRM fallback runs
      level_all, glob_all   all three species at once
      numclamp   the three GCM number columns x 0.3: cells below 0.7 of their level's mean end below zero"""
    rng = np.random.default_rng(seed)
    sh = (nz, ny, nx, nens)
    prof = np.exp(-np.arange(nz) * (9.0 / max(nz - 1, 1)))[:, None, None, None]
    crm = {"density_dry": 1.2 * prof ** 0.25 * rng.uniform(0.95, 1.05, sh), "uvel": rng.normal(0, 8, sh), "vvel": rng.normal(0, 8, sh),
           "temp": 300 - 60 * (1 - prof ** 0.25) + rng.normal(0, 1, sh)}
    crm["water_vapor"] = 0.015 * prof * rng.uniform(0.5, 1.5, sh)
    crm["cloud_water"] = 1e-3 * prof * rng.uniform(0.5, 1.5, sh) * (rng.random(sh) < 0.6)
    crm["ice"] = 1e-4 * prof[::-1] * rng.uniform(0.5, 1.5, sh) * (rng.random(sh) < 0.6)
    for n, m in zip(NUM, (1e8, 1e5, 1e4)):
        crm[n] = m * prof * rng.uniform(0.0, 2.0, sh)
    gcm = {g: crm[c].mean(axis=(1, 2)) * rng.uniform(0.9, 1.1, (nz, nens)) for g, c in zip(GCM, CRM)}
    dz = rng.uniform(50.0, 400.0, (nz, nens))
    for e in range(nens):
        s = scenarios[e % len(scenarios)]
        for sp, (w, g) in enumerate(zip(WATER, GCM_WATER)):
            if s in ("level%d" % sp, "level_all"):
                crm[w][:, :, ::2, e] *= 0.02
                gcm[g][:, e] *= 0.5
            if s in ("glob%d" % sp, "glob_all"):
                gcm[g][nz // 3, e] *= -0.2 if sp else -0.02
        if s == "numclamp":
            for g in GCM_NUM:
                gcm[g][:, e] *= 0.3
    return ({k: np.ascontiguousarray(crm[k]) for k in CRM}, {k: np.ascontiguousarray(gcm[k]) for k in GCM}, np.ascontiguousarray(dz))


def declared_mask(scenarios, ncol):
    """the union of the hole-filling masks over the NAPP applications that a scenario list stands for: bit s = species s filled
    holes, bit 4+s = its whole-CRM fallback ran.  With more than one column per level the cloud-free and ice-free cells alone put
    liquid and ice through the level pass; a one-column level has no cell beside the empty one."""
    m = 0b110 if ncol > 1 else 0
    for s in scenarios:
        for sp in range(3):
            if s in ("level%d" % sp, "level_all"):
                m |= 1 << sp
            if s in ("glob%d" % sp, "glob_all"):
                m |= (1 << sp) | (16 << sp)
    return m


# The named cases: (name, (nens, nx, ny, nz), seed, scenario list).  nens: one lane, a few, one full block of members, one more, the
# suite's usual 70, two blocks and two; ny*nx = 1, 5, 6 and 7 (below the 8 slots of the averages kernel or the 16 of the apply
# kernel, so that some slots own no cell), 18 and 25.  Every case is below 25 000 cells.  A seed is moved where the case would not
# do what its scenarios declare, or where a cell's clamp would flip under one ulp of noise (tests/test_gcm_forcing_cells.py).
SHAPES = [(1, 5, 1, 6), (3, 1, 1, 5), (10, 3, 2, 6), (64, 3, 2, 8), (65, 7, 1, 8), (70, 6, 3, 9), (130, 5, 5, 7)]
SEEDS = {"n64_3x2x8_mixed": 4, "n130_5x5x7_mixed": 5}     # seed 3 there: a wind level mean so near zero that its floor is > FLOOR_MAX
NAMED = []
for _sh in ((70, 6, 3, 9), (1, 5, 1, 6)):
    NAMED += [("n%d_%dx%dx%d_%s" % (_sh + (_s,)), _sh, (_s,)) for _s in SINGLES]
NAMED += [("n%d_%dx%dx%d_mixed" % _sh, _sh, MIXED) for _sh in SHAPES if _sh[0] >= len(MIXED)]
NAMED += [("n3_1x1x5_glob%d" % _s, (3, 1, 1, 5), ("glob%d" % _s,)) for _s in range(3)]
NAMED.append(("n3_1x1x5_glob012", (3, 1, 1, 5), ("glob0", "glob1", "glob2")))
NAMED = [(_n, _sh, SEEDS.get(_n, 3), _sc) for _n, _sh, _sc in NAMED]
NAMED_IDS = [c[0] for c in NAMED]
BY_NAME = {c[0]: c for c in NAMED}


def named_state(name):
    _, shape, seed, scenarios = BY_NAME[name]
    return state(*shape, seed=seed, scenarios=scenarios)


def hazard_state():
    """the mixed ensemble at (12, 5, 3, 8) with member 0 turned into a clear sky whose GCM column agrees: no liquid in any cell, none
    asked for.  Other members send liquid into the whole-CRM fallback, which then runs on every member of the call; member 0 has no
    liquid to pay with and none to pay for, 0 dz / 0 (gcm_forcing.h:270), and yakl_max(0, NaN) hands the NaN on."""
    crm, gcm, dz = state(12, 5, 3, 8, seed=3, scenarios=MIXED)
    crm["cloud_water"][..., 0] = 0.0
    gcm["gcm_cloud_water"][:, 0] = 0.0
    return crm, gcm, dz


def grid_dz(dz):
    """the layer depths as a coupler stores them: set_grid takes interfaces, so dz makes a cumsum round trip"""
    zint = np.concatenate([np.zeros((1, dz.shape[1])), np.cumsum(dz, axis=0)], axis=0)
    return np.ascontiguousarray(np.diff(zint, axis=0))


def members(crm, gcm, dz, lo, hi):
    """the members lo..hi-1 of a state, as a state of their own"""
    return ({k: np.ascontiguousarray(v[..., lo:hi]) for k, v in crm.items()},
            {k: np.ascontiguousarray(v[:, lo:hi]) for k, v in gcm.items()}, np.ascontiguousarray(dz[:, lo:hi]))


def run_oracle(crm, gcm, dz):
    """compute, then NAPP applications, by the oracle on a copy of `crm` with the layer depths `dz` as given.  Returns a run:
    dict(computed = the eleven tendencies of compute, steps = per application dict(crm, tend = the three diagnosed ones, mask))"""
    crm = copy.deepcopy(crm)
    tend = ao.compute_gcm_forcing_tendencies(crm, gcm, DT_GCM)
    run = dict(computed={n: tend[n].copy() for n in COMPUTED}, steps=[])
    for _ in range(NAPP):
        mask = ao.apply_gcm_forcing_tendencies(crm, gcm, tend, dz, CRM_DT, DT_GCM)
        run["steps"].append(dict(crm=copy.deepcopy(crm), tend={n: tend[n].copy() for n in DIAGNOSED}, mask=mask))
    return run


def masks(run):
    return [s["mask"] for s in run["steps"]]


def zero_sets(run):
    """per application, the water cells that are exactly zero after it"""
    return [np.stack([s["crm"][w] == 0.0 for w in WATER]) for s in run["steps"]]


def same_bits(a, b, with_masks=True):
    """two runs equal bit for bit (NaN equal to NaN) in the computed tendencies and, after every application, in all fields, the
    diagnosed tendencies and (with_masks) the mask; returns the first name that differs, or None"""
    for n in COMPUTED:
        if not np.array_equal(a["computed"][n], b["computed"][n], equal_nan=True):
            return n
    for i, (sa, sb) in enumerate(zip(a["steps"], b["steps"])):
        if with_masks and sa["mask"] != sb["mask"]:
            return "mask of application %d: %d, %d" % (i, sa["mask"], sb["mask"])
        for grp in ("crm", "tend"):
            for n in sa[grp]:
                if not np.array_equal(sa[grp][n], sb[grp][n], equal_nan=True):
                    return "%s after application %d" % (n, i)
    return None


def run_members(run, lo, hi):
    """the members lo..hi-1 of a run (its masks stay the whole call's)"""
    return dict(computed={n: v[:, lo:hi] for n, v in run["computed"].items()},
                steps=[dict(crm={n: v[..., lo:hi] for n, v in s["crm"].items()}, tend={n: v[:, lo:hi] for n, v in s["tend"].items()},
                            mask=s["mask"]) for s in run["steps"]])


# ---- the scale ------------------------------------------------------------------------------------------------------------------

def level_max(a):
    return np.abs(a).max(axis=(1, 2))


def field_scale(crm_in, gcm, crm_out):
    """S per field, (nz,nens): the most the level holds in the case's input or in the oracle's output, or the GCM asks for"""
    return {c: np.maximum(np.maximum(level_max(crm_in[c]), level_max(crm_out[c])), np.abs(gcm[g])) for c, g in zip(CRM, GCM)}


def _mixing_ratios(f, names, dry, vap):
    den = f[dry] + f[vap]
    return [f[n] / den for n in names]


def computed_scale(crm_in, gcm):
    """per computed tendency, (nz,nens): max(|gcm value|, |level mean|) / dt_gcm of its own field"""
    mean = {c: np.abs(crm_in[c].mean(axis=(1, 2))) for c in CRM}
    s = {T + t: np.maximum(np.abs(gcm[g]), mean[c]) for t, c, g in
         (("rho_d", "density_dry", "gcm_density_dry"), ("uvel", "uvel", "gcm_uvel"), ("vvel", "vvel", "gcm_vvel"),
          ("temp", "temp", "gcm_temp"), ("nc", NUM[0], GCM_NUM[0]), ("ni", NUM[1], GCM_NUM[1]), ("nr", NUM[2], GCM_NUM[2]))}
    q_crm = _mixing_ratios(crm_in, WATER, "density_dry", "water_vapor")
    q_gcm = _mixing_ratios(gcm, GCM_WATER, "gcm_density_dry", "gcm_water_vapor")
    for t, qc, qg in zip(("qv", "ql", "qi"), q_crm, q_gcm):
        s[T + t] = np.maximum(np.abs(qg), np.abs(qc.mean(axis=(1, 2))))
    s[T + "qtot"] = np.maximum(np.abs(sum(q_gcm)), np.abs(sum(q_crm).mean(axis=(1, 2))))
    return {k: v / DT_GCM for k, v in s.items()}


def diagnosed_scale(crm_before, crm_after, gcm):
    """the same for the three density tendencies apply writes: the level mean of the cells before and after the application"""
    return {t: np.maximum(np.abs(gcm[g]), np.maximum(np.abs(crm_before[w].mean(axis=(1, 2))), np.abs(crm_after[w].mean(axis=(1, 2)))))
            / DT_GCM for t, w, g in zip(DIAGNOSED, WATER, GCM_WATER)}


def _worst(err, scale):
    """max of err/scale; a non-zero error where the scale is zero is infinitely wrong"""
    pos = scale > 0
    w = float((err[pos] / scale[pos]).max()) if pos.any() else 0.0
    return float("inf") if np.any(err[~pos] != 0) else w


def run_errors(got, exp, crm_in, gcm):
    """per field and tendency, the worst error of the run `got` against the oracle's `exp` in the gate's units, over all applications"""
    worst = {n: _worst(np.abs(got["computed"][n] - exp["computed"][n]), s) for n, s in computed_scale(crm_in, gcm).items()}
    before = crm_in
    for sg, se in zip(got["steps"], exp["steps"]):
        S = field_scale(crm_in, gcm, se["crm"])
        for c in CRM:
            if c == "temp":
                e = float(np.abs((sg["crm"][c] - se["crm"][c]) / se["crm"][c]).max())
            else:
                e = _worst(np.abs(sg["crm"][c] - se["crm"][c]), np.broadcast_to(S[c][:, None, None, :], se["crm"][c].shape))
            worst[c] = max(worst.get(c, 0.0), e)
        for n, s in diagnosed_scale(before, se["crm"], gcm).items():
            worst[n] = max(worst.get(n, 0.0), _worst(np.abs(sg["tend"][n] - se["tend"][n]), s))
        before = se["crm"]
    return worst


# ---- floor, tolerance, gate -----------------------------------------------------------------------------------------------------

def perturbed_twins(crm, seed):
    """three twins of the CRM state, in the manner of parity_gate.perturbed_twins but over all ten fields (temp alone does not feed the
    water path): two seeded draws of +-1 ulp per cell, and every value one ulp away from zero.  Exact zeros stay."""
    rng = np.random.default_rng(seed)
    twins = []
    for _ in range(2):
        twins.append({k: v * (1.0 + rng.integers(-1, 2, size=v.shape) * 1.1e-16) for k, v in crm.items()})
    twins.append({k: np.where(v != 0.0, np.nextafter(v, np.where(v > 0, np.inf, -np.inf)), 0.0) for k, v in crm.items()})
    return twins


def oracle_floor(crm, gcm, dz, base, seed=0):
    """(floor per field and tendency in run_errors' units, problems): the oracle's own response to the perturbed twins, and what the
    noise changed that it must not change -- a mask or the zero set of an application"""
    floor, problems = {}, []
    for i, twin in enumerate(perturbed_twins(crm, seed)):
        run = run_oracle(twin, gcm, dz)
        if masks(run) != masks(base):
            problems.append("twin %d: masks %s, not %s" % (i, masks(run), masks(base)))
        for a, (z, zb) in enumerate(zip(zero_sets(run), zero_sets(base))):
            if not np.array_equal(z, zb):
                problems.append("twin %d: %d water cells change between zero and non-zero in application %d" % (i, (z != zb).sum(), a))
        for k, e in run_errors(run, base, crm, gcm).items():
            floor[k] = max(floor.get(k, 0.0), e)
    return floor, problems


def tolerances(floor):
    return {k: pg.floor_gate(v, TOL_CAP) for k, v in floor.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """everything a test needs of a named case, computed once and shared (read only): the state, the oracle's run on the layer depths
    the coupler stores, its floor with what the twins must leave alone, and the gate"""
    crm, gcm, dz = named_state(name)
    base = run_oracle(crm, gcm, grid_dz(dz))
    floor, problems = oracle_floor(crm, gcm, grid_dz(dz), base)
    return dict(crm=crm, gcm=gcm, dz=dz, run=base, floor=floor, problems=problems, tol=tolerances(floor))


def gate(got, exp, crm_in, gcm, tol, what="", case=None, floor=None):
    """the run `got` against the oracle's `exp`: everything finite, the mask and the zero set of every application exactly the
    oracle's, every field and tendency within tol of it in run_errors' units.  `case`: a name under which the worst errors, the floor
    and the gate go to the parity record (PAM_AMD_PARITY_RECORD, parity_gate.record)."""
    assert masks(got) == masks(exp), (what, masks(got), masks(exp))
    for n in COMPUTED:
        assert np.isfinite(exp["computed"][n]).all() and np.isfinite(got["computed"][n]).all(), (what, n)
    for a, (sg, se) in enumerate(zip(got["steps"], exp["steps"])):
        for grp in ("crm", "tend"):
            for n in se[grp]:
                assert np.isfinite(se[grp][n]).all() and np.isfinite(sg[grp][n]).all(), (what, n, a)
        for w in WATER:
            assert np.array_equal(sg["crm"][w] == 0.0, se["crm"][w] == 0.0), (what, w, "zero set of application %d" % a)
    worst = run_errors(got, exp, crm_in, gcm)
    if case is not None:
        pg.record(case, dict(worst=worst, floor=floor, gate=tol))
    for k in worst:
        assert worst[k] <= tol[k], (what, k, worst[k], tol[k])
    return worst
