"""The multi-step parity gate of every HIP-vs-oracle comparison (tests, the C++ driver tests, __graft_entry__.smoke()).

north_star: prognostic fields within rtol 1e-12 (fp64).  rho_d, T (max-norm and element-wise) and water vapour keep 1e-12 however
many sub-steps were run.  The small, noise-dominated fields (u, v, w, tracers other than water vapour) are gated at the case's OWN
noise floor: noise_floor() runs the oracle on three twins of the inputs whose T carries one ulp of noise (two seeded +-1 ulp draws per
cell and one np.nextafter(T, inf)) and takes, per field, the largest departure from the unperturbed run -- the flow's own sensitivity
to rounding, which is all a correct kernel may add.  compare(..., floor=floor) then holds every noise field to

    min(tol_noise_fields(nsub, factor), max(1e-12, 4 * floor[k]))

so it is never looser than the global curve it replaces and, for most cases, 10-50x tighter (DESIGN.md section 4 has the per-case
table, profiles/r07_parity_worst.json the record).  The device sits within ~3.3x of the floor in every named case; the 4 leaves room
for its rounding (FMA contraction, v_rcp_f64 + Newton reciprocals, device pow) without letting a wrong constant of 1e-11 through.  A
field that is identically zero in the oracle (2-D v) must stay exactly zero, whatever its twins do.  rho_d, T and vapour stay at
1e-12: their twin floor is ~2e-15, but the device's own rounding adds up to ~1e-14 there directly, which a floor gate does not fit.

tol_noise_fields(nsub) = 1e-11 (1 + nsub/3) is the measured error curve of round 3 (profiles/r03_error_growth_c1.txt: C1's u, v, w
at 4.5e-13 ... 6.8e-12 over 3 ... 30 sub-steps, fitted to the noisiest case).  With floor=None it is the gate on its own, as before
(smoke() calls it that way).  `factor`: the degenerate 3 x 3 x 3 grid (the periodic stencil wraps every line twice; w is 1e-3 m/s
of noise there), gated at 4x the curve.  Under PAM_AMD_PARITY_RECORD=<file> every named comparison writes its worst errors, the
floor and the per-field gate to <file>; a relative perturbation of 1e-10 injected into one field turns a case red
(tests/test_gpu_parity.py), and a gravity constant off by 1e-11 or 1e-12 turns named cases red (tests/test_parity_gate.py)."""
import copy
import json
import os

import numpy as np

TOL_TIGHT = 1e-12
FLOOR_MIN = 1e-12          # the floor gate never goes below the north_star bar
FLOOR_K = 4.0              # how many times the oracle's own noise response a noise field may reach
TIGHT_FIELDS = ("density_dry", "temp", "water_vapor")
_RECORD = {}


def tol_noise_fields(nsub, factor=1.0):
    return factor * 1.0e-11 * (1.0 + nsub / 3.0)


def worst_errors(got, exp, names):
    worst = {}
    for k in ("density_dry", "temp", "uvel", "vvel", "wvel"):
        scale = max(np.abs(exp[k]).max(), 1e-300)
        worst[k] = float(np.abs(got[k] - exp[k]).max() / scale)
    for t, n in enumerate(names):
        scale = max(np.abs(exp["tracers"][t]).max(), 1e-300)
        worst[n] = float(np.abs(got["tracers"][t] - exp["tracers"][t]).max() / scale)
    for k in ("density_dry", "temp"):   # bounded away from zero: also ELEMENT-WISE
        worst[k + "_elementwise"] = float(np.abs((got[k] - exp[k]) / exp[k]).max())
    return worst


def is_tight(k):
    return k.split("_elementwise")[0] in TIGHT_FIELDS


def _field(f, names, k):
    return f["tracers"][names.index(k)] if k in names else f[k]


def perturbed_twins(fields, seed):
    """the three twins of noise_floor(): T with a seeded +-1 ulp per cell (two draws, as test_fuzz_parity always did) and
    T one ulp up everywhere"""
    rng = np.random.default_rng(seed)
    twins = []
    for _ in range(2):
        t = copy.deepcopy(fields)
        t["temp"] = t["temp"] * (1.0 + rng.integers(-1, 2, size=t["temp"].shape) * 1.1e-16)
        twins.append(t)
    t = copy.deepcopy(fields)
    t["temp"] = np.nextafter(t["temp"], np.inf)
    twins.append(t)
    return twins


def noise_floor(run_oracle, fields, names, seed, base=None):
    """Per field, the oracle's own response to one ulp of noise in T: the largest worst_errors() of three perturbed twins
    (perturbed_twins) against the unperturbed run.  `run_oracle(f)` advances the input dict `f` in place through the same oracle
    sequence the device ran; `fields` are the inputs (left untouched); `base`, if given, is run_oracle's output on `fields`
    (saves one run)."""
    if base is None:
        base = copy.deepcopy(fields)
        run_oracle(base)
    floor = {}
    for twin in perturbed_twins(fields, seed):
        run_oracle(twin)
        for k, e in worst_errors(twin, base, names).items():
            floor[k] = max(floor.get(k, 0.0), e)
    return floor


def floor_gate(floor_k, cap):
    """the gate of one noise field: FLOOR_K x its floor, not below FLOOR_MIN, never above `cap` (the bound it replaces)"""
    return min(cap, max(FLOOR_MIN, FLOOR_K * floor_k))


def gates(exp, names, nsub, factor=1.0, floor=None, cap=None):
    """per-field tolerance of compare(): TOL_TIGHT for rho_d, T, vapour; the curve or, with a floor, floor_gate(floor, curve) for
    the noise fields, and 0 for a noise field that is identically zero in the oracle.  `cap` (per noise field) replaces the curve
    where a caller's bound of today is another one (test_fuzz_parity: the curve or 4x the floor)."""
    curve = tol_noise_fields(nsub, factor)
    out = {}
    for k in ["density_dry", "temp", "uvel", "vvel", "wvel"] + list(names) + ["density_dry_elementwise", "temp_elementwise"]:
        if is_tight(k):
            out[k] = TOL_TIGHT
        elif floor is None:
            out[k] = curve
        elif not np.any(_field(exp, names, k)):
            out[k] = 0.0
        else:
            out[k] = floor_gate(floor[k], curve if cap is None else cap[k])
    return out


def record(case, entry):
    """one named comparison into the record (PAM_AMD_PARITY_RECORD=<json file>, merged with what the file holds)"""
    _RECORD[case] = entry
    path = os.environ.get("PAM_AMD_PARITY_RECORD")
    if path:
        old = {}
        if os.path.exists(path):
            try:
                old = json.load(open(path))
            except Exception:
                old = {}
        old.update(_RECORD)
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)


def compare(got, exp, names, nsub, case=None, factor=1.0, floor=None, cap=None):
    """rho_d, T (max-norm and element-wise) and water vapour within 1e-12; the noise-dominated fields within tol_noise_fields(nsub)
    or, given the case's noise_floor(), within min(curve, max(1e-12, 4 floor)) (and exactly zero where the oracle's field is).
    `got` / `exp`: dicts with density_dry, temp, uvel, vvel, wvel (arrays) and tracers (sequence in the order of `names`)."""
    worst = worst_errors(got, exp, names)
    gate = gates(exp, names, nsub, factor, floor, cap)
    if case is not None:
        entry = dict(worst, nsub=nsub, gate_noise_fields=tol_noise_fields(nsub, factor))
        if floor is not None:
            entry.update(floor=floor, gate=gate)
        record(case, entry)
    for k, e in worst.items():
        assert e <= gate[k], (k, e, gate[k], worst)
    return worst
