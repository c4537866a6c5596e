"""States, per-cell scale and gate of the Kessler tests (tests/test_kessler_emu.py on the CPU, tests/test_micro_kessler.py on the GPU).
No GPU, no test of its own.

state(): every cell of every member draws its vapour, cloud and rain category on its own, so that one column kernel run meets every
branch of the scheme (physics/micro/kessler/Microphysics.h:346-457) and a wavefront -- 64 consecutive columns at one level -- holds
rainy and rain-free lanes side by side.  The oracle's census (oracle.awfl_oracle.kessler_census) counts the branches;
tests/test_kessler_emu.py asserts that every named case reaches all of them.

The gate is per cell.  Water only moves down, and every error term of the scheme is a rounding of water that is in the cell or can
fall into it (cond = max(prod, -qc), ern <= qr, sed is a difference of the fluxes of the cell and the one above).  So the three
water densities are held, cell by cell, to tol x S, S[k] = max over k' >= k of (rho_v + rho_c + rho_r) of the column's INPUT state;
temp element-wise and relative; precl per column to tol x the precl the column would have if all of S[0] were rain at the ground
(36.34 (0.001 S0)^0.1364 S0 / 1000).  tol = min(1e-11, max(1e-12, 4 x floor)): the form and the factor of parity_gate.floor_gate,
floor = the oracle's own response, in the same per-cell units, to the three parity_gate.perturbed_twins of the case, run at the base
run's sub-cycle count.  The floors are ~1e-14, so the gate comes out at 1e-12 -- of the cell's own scale, where
the bound it joins (1e-12 x max|field|) lets a relative error of 1e-6 through in a cell that holds 1e-6 of the field's maximum."""
import copy

import numpy as np

import parity_gate as pg
from oracle import awfl_oracle as ao
from pam_amd import idealized as idz

C0 = dict(idz.CONSTS_DEFAULT, cp_d=1003.0, cp_v=1859.0)   # the scheme's own constants (Microphysics.h:66-71)
WATER = ("rho_v", "rho_c", "rho_r")
FIELDS = WATER + ("temp", "precl")
TOL_CAP = 1e-11            # the base of the curve of parity_gate.tol_noise_fields
FLOOR_MAX = 2.5e-13        # a named case whose oracle floor is above this amplifies noise: rejected as an input (4 x = 1e-12)


def state(nens, nx, ny, nz, seed, rain="mixed"):
    """zi (nz+1,nens), zm (nz,nens) and the dict rho_v, rho_c, rho_r, rho_dry, temp, each (nz,ny,nx,nens).  rho_d and T are the
    supercell sounding's; the water of every cell is drawn on its own, as mixing ratios:
      vapour  qvs x U(0.3, 1.3), or (p = 0.2) just below saturation, qvs x U(0.97, 0.9999): with a little cloud and some rain that is
              where rain evaporation ends at saturation (tmp2) instead of at its own rate or at the rain present
      rain    none (0.5), trace 10^U(-14,-8) (0.15), moderate 10^U(-5,-3) (0.15), heavy U(2e-3, 8e-3) (0.1), 1e-95 (0.1: a fall speed
              of ~1e-12 m/s, the dt2d = dt branch of the time-step limit)
      cloud   none (0.4), trace 10^U(-9,-6) (0.2), below the autoconversion threshold U(1e-4, 9e-4) (0.2), above it U(1.2e-3, 3e-3) (0.2);
              in half of the nearly saturated cells instead U(0.9, 1.3) x what would saturate the cell
    qvs = 3.8 / p_hPa exp(17.27 (T - 273) / (T - 36)), the scheme's own formula, at the dry pressure.
    rain="slow": none or 1e-95 only -- every fall speed is <= 1e-10."""
    rng = np.random.default_rng(7919 * seed + 11)
    zint = idz.stretched_interfaces(nz, 15000.0)
    zi = zint[:, None] * (1 + 0.01 * np.arange(nens))[None, :]
    zm = 0.5 * (zi[:-1] + zi[1:])
    f = idz.supercell_fields(nens, nx, ny, nz, zint, magnitude=1.0)
    rho_d, T = np.ascontiguousarray(f["density_dry"]), np.ascontiguousarray(f["temp"])
    shape = rho_d.shape
    qvs = 3.8 / (C0["R_d"] * rho_d * T / 100.0) * np.exp(17.27 * (T - 273.0) / (T - 36.0))
    near = rng.random(shape) < 0.2
    qv = qvs * np.where(near, rng.uniform(0.97, 0.9999, shape), rng.uniform(0.3, 1.3, shape))
    kind = rng.choice(5, size=shape, p=[0.5, 0.15, 0.15, 0.1, 0.1])
    qr = np.choose(kind, [np.zeros(shape), 10.0 ** rng.uniform(-14, -8, shape), 10.0 ** rng.uniform(-5, -3, shape),
                          rng.uniform(2e-3, 8e-3, shape), np.full(shape, 1e-95)])
    if rain == "slow":
        qr = np.where(kind >= 3, 1e-95, 0.0)
    kind = rng.choice(4, size=shape, p=[0.4, 0.2, 0.2, 0.2])
    qc = np.choose(kind, [np.zeros(shape), 10.0 ** rng.uniform(-9, -6, shape), rng.uniform(1e-4, 9e-4, shape),
                          rng.uniform(1.2e-3, 3e-3, shape)])
    # half of the cells just below saturation hold about the cloud that fills their deficit (-prod of :422: what evaporates until
    # the cell is saturated), a little less once accretion has taken its share: tmp2 = -prod - qc is then small and positive
    deficit = (qvs - qv) / (1.0 + qvs * (4093.0 * 2.5e6 / C0["cp_d"]) / (T - 36.0) ** 2)
    fill = near & (rng.random(shape) < 0.5)
    qc = np.where(fill, deficit * rng.uniform(0.9, 1.3, shape), qc)
    s = dict(rho_v=qv * rho_d, rho_c=qc * rho_d, rho_r=qr * rho_d, rho_dry=rho_d, temp=T)
    return zi, zm, {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in s.items()}


# The named cases: (nens, nx, ny, nz, state seed) x the three step variants.  nens covers one lane, a few, one full wavefront, one
# lane more, the suite's usual 70 and several wavefronts per row; ny 2-D and 3-D; every case is below 150 000 cells.
SHAPES = [(1, 48, 3, 30, 1), (3, 33, 1, 41, 2), (64, 6, 3, 30, 3), (65, 5, 1, 24, 4), (70, 6, 3, 30, 5), (200, 4, 3, 60, 6)]
VARIANTS = [("dt5", 5.0, 0), ("dt60", 60.0, 0), ("dt60_forced1", 60.0, 1)]      # (name, dt, forced rainsplit or 0)
NAMED = [("n%d_%dx%dx%d_%s" % (sh[0], sh[1], sh[2], sh[3], v[0]), sh, v) for sh in SHAPES for v in VARIANTS]
NAMED_IDS = [c[0] for c in NAMED]


def named_state(case):
    _, (nens, nx, ny, nz, seed), (_, dt, forced) = case
    zi, zm, s = state(nens, nx, ny, nz, seed)
    return zi, zm, s, dt, forced


def run_oracle(s, zm, dt, rainsplit=0, census=False):
    """a copy of `s` advanced by the oracle: (outputs with precl, rainsplit[, census])"""
    o = copy.deepcopy(s)
    if census:
        precl, n, cen = ao.kessler_census(o["rho_v"], o["rho_c"], o["rho_r"], o["rho_dry"], o["temp"], zm, dt, C0, rainsplit=rainsplit)
    else:
        precl, n = ao.kessler(o["rho_v"], o["rho_c"], o["rho_r"], o["rho_dry"], o["temp"], zm, dt, C0, rainsplit=rainsplit)
    o["precl"] = precl
    return (o, n, cen) if census else (o, n)


def cell_scale(s_in):
    """S (nz,ny,nx,nens): the most water any cell at or above holds in the INPUT state"""
    tot = s_in["rho_v"] + s_in["rho_c"] + s_in["rho_r"]
    return np.maximum.accumulate(tot[::-1], axis=0)[::-1]


def precl_scale(S):
    """(ny,nx,nens): the column's precl if all of S[0] were rain at the ground (:397 with rho = rho0, so rhalf = 1)"""
    return 36.34 * (0.001 * S[0]) ** 0.1364 * S[0] / 1000.0


def cell_errors(got, exp, S):
    """the worst error of every field in the gate's units: water per cell over S, temp element-wise relative, precl over precl_scale"""
    e = {k: float((np.abs(got[k] - exp[k]) / S).max()) for k in WATER}
    e["temp"] = float(np.abs((got["temp"] - exp["temp"]) / exp["temp"]).max())
    e["precl"] = float((np.abs(got["precl"] - exp["precl"]) / precl_scale(S)).max())
    return e


def oracle_floor(s_in, zm, dt, base, n, seed=0):
    """per field, the oracle's own response to one ulp of noise in T, in cell_errors' units: the three parity_gate.perturbed_twins
    of the inputs, run at the base run's sub-cycle count `n`, against the base run's outputs `base`"""
    S = cell_scale(s_in)
    floor = dict.fromkeys(FIELDS, 0.0)
    for twin in pg.perturbed_twins(s_in, seed):
        out, _ = run_oracle(twin, zm, dt, rainsplit=n)
        for k, e in cell_errors(out, base, S).items():
            floor[k] = max(floor[k], e)
    return floor


def tolerances(floor):
    return {k: pg.floor_gate(floor[k], TOL_CAP) for k in FIELDS}


def gate(got, exp, s_in, tol, what="", case=None, floor=None):
    """every output finite and within tol[k] of the oracle's in cell_errors' units.  `case`: a name under which the worst errors,
    the floor and the gate go to the parity record (PAM_AMD_PARITY_RECORD, parity_gate.record)."""
    for k in FIELDS:
        assert np.isfinite(exp[k]).all() and np.isfinite(got[k]).all(), (what, k)
    worst = cell_errors(got, exp, cell_scale(s_in))
    if case is not None:
        pg.record(case, dict(worst=worst, floor=floor, gate=tol))
    for k in FIELDS:
        assert worst[k] <= tol[k], (what, k, worst[k], tol[k], worst)
    return worst


def gate_against_oracle(got, s_in, zm, dt, n, what="", case=None):
    """the whole comparison of one run: the oracle at `n` sub-cycles, its floor, the per-cell gate.  Returns (oracle outputs, worst)"""
    exp, n_ref = run_oracle(s_in, zm, dt, rainsplit=n)
    assert n_ref == n
    floor = oracle_floor(s_in, zm, dt, exp, n)
    return exp, gate(got, exp, s_in, tolerances(floor), what, case, floor)


def mixed_wavefront_fraction(rho_r):
    """of all (level, 64 consecutive columns) groups -- the wavefronts of the column kernel --, the fraction that holds both rainy and
    rain-free columns"""
    nz = rho_r.shape[0]
    rainy = (rho_r.reshape(nz, -1) != 0.0)
    mixed = total = 0
    for c0 in range(0, rainy.shape[1], 64):
        g = rainy[:, c0:c0 + 64]
        mixed += int((g.any(axis=1) & ~g.all(axis=1)).sum())
        total += nz
    return mixed / total
