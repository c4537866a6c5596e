"""The native grey two-stream shortwave radiation scheme: the numpy restatement of the contract (include/pam_amd_modules.h at
pam_amd_radiation_gray_sw) and the mutants of the restatement.  TEST INFRASTRUCTURE ONLY.

numpy's element-wise float64 arithmetic is IEEE and never contracted, no numpy reduction takes part, and the exponential is the
contract's own (sgs_moist_ref.exp_c, taken as tests/grayrad_ref.py takes it), so no libm takes part either: the device bodies are held
to this file bit for bit.  The day branch is evaluated for every member and the night members are replaced afterwards, which gives a day
member the same bits whatever its neighbours are.  A mutant is a deliberately wrong variant of ONE line, switched on by name; each must
be caught by a named case (tests/grayrad_sw_cases.py)."""
import numpy as np

from sgs_moist_ref import exp_c
from sgs_ref import same_bits, results_differ, shape_id      # noqa: F401
from grayrad_ref import table_sum

MUTANTS = ("r_from_b", "trt_other_way", "m_before_dz", "night_not_positive", "fu_from_rb_above")
OUTPUTS = ("temp", "rad_sw_heating", "rad_sw_down_sfc", "rad_sw_up_sfc", "rad_sw_up_top")
SCALARS = ("solar_constant", "a_d", "a_v", "a_l", "a_i", "s_l", "s_i", "albedo", "cp_d", "dt")


def radiation(case, mutant=None, internals=False):
    """-> dict of OUTPUTS; internals: also ta, b, da, q and the heat capacity cap (nz,...), Fd and Fu (nz+1,...), as the day branch gives
    them for every member, and night (nens)"""
    F = case["fields"]
    temp, rho_d, rho_v = F["temp"], F["density_dry"], F["water_vapor"]
    nz = temp.shape[0]
    zint, mu0 = case["zint"], np.asarray(case["coszen"], dtype=np.float64)
    night = ~(mu0 > 0.0) if mutant == "night_not_positive" else mu0 <= 0.0
    with np.errstate(all="ignore"):
        m = 1.0 / mu0
        dz = (zint[1:] - zint[:-1])[:, None, None, :]
        L, I = table_sum(case, case["liquid"], temp), table_sum(case, case["ice"], temp)
        a = case["a_d"] * rho_d + case["a_v"] * rho_v
        a = a + case["a_l"] * L
        a = a + case["a_i"] * I
        da = (a * m) * dz if mutant == "m_before_dz" else (a * dz) * m
        ta = exp_c(-da)
        s = case["s_l"] * L + case["s_i"] * I
        b = (s * m) * dz if mutant == "m_before_dz" else (s * dz) * m
        tr = 1.0 / (1.0 + b)
        r = b / (1.0 + b) if mutant == "r_from_b" else 1.0 - tr
        R, T = r * ta, tr * ta
        col = temp.shape[1:]
        Rb, Fd, Fu = np.empty((nz + 1,) + col), np.empty((nz + 1,) + col), np.empty((nz + 1,) + col)
        Rb[0] = case["sfc_albedo"] if case.get("sfc_albedo") is not None else np.full(col, case["albedo"])
        q = np.empty((nz,) + col)
        for k in range(nz):
            q[k] = 1.0 - Rb[k] * R[k]
            # the other association: T (Rb T) has the bits of (T Rb) T, a product being commutative, so the one that differs is (T T) Rb
            n = (T[k] * T[k]) * Rb[k] if mutant == "trt_other_way" else (T[k] * Rb[k]) * T[k]
            Rb[k + 1] = R[k] + n / q[k]
        Fd[nz] = np.broadcast_to(case["solar_constant"] * mu0, col)
        Fu[nz] = Rb[nz] * Fd[nz]
        for k in range(nz - 1, -1, -1):
            Fd[k] = (T[k] * Fd[k + 1]) / q[k]
            Fu[k] = (Rb[k + 1] if mutant == "fu_from_rb_above" else Rb[k]) * Fd[k]
        cap = (case["cp_d"] * (rho_d + rho_v)) * dz
        heating = ((Fd[1:] - Fd[:-1]) + (Fu[:-1] - Fu[1:])) / cap
        new_temp = temp.copy() if case["dt"] == 0 else temp + heating * case["dt"]
    out = dict(temp=np.where(night, temp, new_temp), rad_sw_heating=np.where(night, 0.0, heating), rad_sw_down_sfc=np.where(night, 0.0, Fd[0]),
               rad_sw_up_sfc=np.where(night, 0.0, Fu[0]), rad_sw_up_top=np.where(night, 0.0, Fu[nz]))
    if internals:
        out.update(ta=ta, b=b, da=da, q=q, Fd=Fd, Fu=Fu, cap=cap, night=night)
    return out


class RefBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def run(self, case):
        return radiation(case, self.mutant)
