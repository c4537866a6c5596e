"""The native grey two-stream longwave radiation scheme: the numpy restatement of the contract (include/pam_amd_modules.h at
pam_amd_radiation_gray) and the mutants of the restatement.  TEST INFRASTRUCTURE ONLY.

numpy's element-wise float64 arithmetic is IEEE and never contracted, no numpy reduction takes part, and the exponential is the
contract's own (sgs_moist_ref.exp_c), so no libm takes part either: the device bodies are held to this file bit for bit.  A mutant is a
deliberately wrong variant of ONE line, switched on by name; each must be caught by a named case (tests/grayrad_cases.py)."""
import numpy as np

from sgs_moist_ref import exp_c
from sgs_ref import same_bits, results_differ, shape_id      # noqa: F401

MUTANTS = ("sweeps_swapped", "one_minus_t_dropped", "rho_d_alone", "surface_at_level_1")
SIGMA = 5.670374419e-8
OUTPUTS = ("temp", "rad_heating", "rad_olr", "rad_lw_down_sfc", "rad_lw_up_sfc")


def table_sum(case, names, like):
    """0.0 of an empty table, else left to right"""
    if not names:
        return np.zeros_like(like)
    s = case["fields"][names[0]]
    for n in names[1:]:
        s = s + case["fields"][n]
    return s


def radiation(case, mutant=None, internals=False):
    """-> dict of OUTPUTS; internals: also t (nz,...), D and U (nz+1,...) and the heat capacity c (nz,...)"""
    F = case["fields"]
    temp, rho_d, rho_v = F["temp"], F["density_dry"], F["water_vapor"]
    nz = temp.shape[0]
    zint = case["zint"]
    dz = (zint[1:] - zint[:-1])[:, None, None, :]
    L, I = table_sum(case, case["liquid"], temp), table_sum(case, case["ice"], temp)
    c = case["k_d"] * rho_d + case["k_v"] * rho_v
    c = c + case["k_l"] * L
    c = c + case["k_i"] * I
    dtau = c * dz
    t = exp_c(-dtau)
    t2 = temp * temp
    B = case["sigma"] * (t2 * t2)
    e = B if mutant == "one_minus_t_dropped" else B * (1.0 - t)
    ts = case["sfc_temp"] if case.get("sfc_temp") is not None else temp[1 if (mutant == "surface_at_level_1" and nz > 1) else 0]
    ts2 = ts * ts
    D, U = np.empty((nz + 1,) + temp.shape[1:]), np.empty((nz + 1,) + temp.shape[1:])
    top, ground = np.full(temp.shape[1:], case["lw_down_top"]), case["sigma"] * (ts2 * ts2)
    if mutant == "sweeps_swapped":           # the downward recurrence climbs from the ground and the upward one descends from the top
        D[0], U[nz] = top, ground
        for k in range(nz):
            D[k + 1] = D[k] * t[k] + e[k]
        for k in range(nz - 1, -1, -1):
            U[k] = U[k + 1] * t[k] + e[k]
    else:
        D[nz], U[0] = top, ground
        for k in range(nz - 1, -1, -1):
            D[k] = D[k + 1] * t[k] + e[k]
        for k in range(nz):
            U[k + 1] = U[k] * t[k] + e[k]
    rho = rho_d if mutant == "rho_d_alone" else rho_d + rho_v
    cap = (case["cp_d"] * rho) * dz
    heating = ((D[1:] - D[:-1]) + (U[:-1] - U[1:])) / cap
    out = dict(temp=temp.copy() if case["dt"] == 0 else temp + heating * case["dt"], rad_heating=heating, rad_olr=U[nz].copy(),
               rad_lw_down_sfc=D[0].copy(), rad_lw_up_sfc=U[0].copy())
    if internals:
        out.update(t=t, D=D, U=U, cap=cap)
    return out


class RefBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def run(self, case):
        return radiation(case, self.mutant)
