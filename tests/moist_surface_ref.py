"""CPU restatement of two coupler modules of the reference, the checker of tests/test_moist_surface_modules.py.  TEST INFRASTRUCTURE.

Written from the reference's text -- pam_core/modules/saturation_adjustment.h and pam_core/modules/surface_friction.h -- as scalar
Python: math.exp / log / atan / sqrt are glibc's, every expression keeps the reference's operation order (Python evaluates left to
right with C's precedence), and no product is fused with a sum.  It shares no code with the HIP path (pam_amd/csrc).

The only addition to the reference is bookkeeping: the iteration count of each bisection and the smallest relative margin
|pv_loc - svp_loc| / svp_loc of its decisions, which tells a comparison where a last-place difference of exp may flip a decision.

A `mutant=` argument switches on ONE deliberate error by name (SATURATION_MUTANTS, FRICTION_MUTANTS): the proof that a gate bites
(tests/moist_surface_cases.py, tests/test_moist_surface_cells.py).  With mutant=None every function is the reference's.
"""
import math

import numpy as np

TOL = 1.e-6          # saturation_adjustment.h:33
CP_L = 4188.0        # :141
MAX_ITER = 2048      # the cap of the HIP path; the restatement raises if a state it is given would need more
NS = 16              # slots of the device's horizontal sums (pam_amd/csrc/modules_kernels.hip: MOD_NS)

SATURATION_MUTANTS = ("rho_reversed", "cp_reassociated", "temp_fused", "skip_below_1e-9", "lv_at_temp_loc", "tol_2e-6")
FRICTION_MUTANTS = ("seven_iterations", "zeta_ge", "m_pi", "no_wind_clamp", "dz_member0", "rho_sfc_two_levels", "serial_means",
                    "last_member_z0", "last_chunk_zero_umean")


def _yakl_max(a, b):
    return a if a > b else b


def _std_min(a, b):
    return b if b < a else a


def _std_max(a, b):
    return b if a < b else a


def saturation_vapor_pressure(temp):                                     # :9-12
    tc = temp - 273.15
    return 610.94 * _exp(17.625 * tc / (243.04 + tc))


def _margin(diff, svp):
    """|pv - svp| / svp; where svp is 0 or inf (exp under- or overflowed) or the difference is NaN no last place decides: inf, but
    for a tie"""
    if math.isnan(diff):
        return math.inf
    if svp == 0.0 or math.isinf(svp):
        return math.inf if diff != 0.0 else 0.0
    return abs(diff) / svp


def _exp(x):
    """C's exp: +inf on overflow, where math.exp raises"""
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def latent_heat_condensation(temp):                                      # :15-18
    tc = temp - 273.15
    return (2500.8 - 2.36 * tc + 0.0016 * tc * tc - 0.00006 * tc * tc * tc) * 1000


def cp_moist(rho_d, rho_v, rho_c, cp_d, cp_v, cp_l, mutant=None):       # :21-25
    rho = rho_d + rho_v + rho_c
    if mutant == "cp_reassociated":
        return (rho_d * cp_d + rho_v * cp_v + rho_c * cp_l) / rho
    return rho_d / rho * cp_d + rho_v / rho * cp_v + rho_c / rho * cp_l


def condensed_state(amount, rho, rho_d, rho_v, rho_c, temp, R_v, cp_d, cp_v, cp_l, mutant=None):
    """one iteration of the condensation loop (:52-59) for rho_cond = amount: (rv_loc, rc_loc, temp_loc, pv_loc - svp_loc, svp_loc)"""
    rv_loc = _yakl_max(0.0, rho_v - amount)
    rc_loc = _yakl_max(0.0, rho_c + amount)
    Lv = latent_heat_condensation(temp)
    cp = cp_moist(rho_d, rv_loc, rc_loc, cp_d, cp_v, cp_l, mutant)
    temp_loc = temp + amount * Lv / (rho * cp)
    if mutant == "lv_at_temp_loc":
        temp_loc = temp + amount * latent_heat_condensation(temp_loc) / (rho * cp)
    if mutant == "temp_fused":          # the product, the quotient and the sum rounded once
        L = np.longdouble
        temp_loc = float(L(temp) + L(amount) * L(Lv) / L(rho * cp))
    svp_loc = saturation_vapor_pressure(temp_loc)
    pv_loc = rv_loc * R_v * temp_loc
    return rv_loc, rc_loc, temp_loc, pv_loc - svp_loc, svp_loc


def evaporated_state(amount, rho, rho_d, rho_v, rho_c, temp, R_v, cp_d, cp_v, cp_l, mutant=None):
    """one iteration of the evaporation loop (:89-96) for rho_evap = amount"""
    rv_loc = _yakl_max(0.0, rho_v + amount)
    rc_loc = _yakl_max(0.0, rho_c - amount)
    Lv = latent_heat_condensation(temp)
    cp = cp_moist(rho_d, rv_loc, rc_loc, cp_d, cp_v, cp_l, mutant)
    temp_loc = temp - amount * Lv / (rho * cp)
    if mutant == "lv_at_temp_loc":
        temp_loc = temp - amount * latent_heat_condensation(temp_loc) / (rho * cp)
    if mutant == "temp_fused":          # the product, the quotient and the sum rounded once
        L = np.longdouble
        temp_loc = float(L(temp) - L(amount) * L(Lv) / L(rho * cp))
    svp_loc = saturation_vapor_pressure(temp_loc)
    pv_loc = rv_loc * R_v * temp_loc
    return rv_loc, rc_loc, temp_loc, pv_loc - svp_loc, svp_loc


def compute_adjusted_state(rho, rho_d, rho_v, rho_c, temp, R_v, cp_d, cp_v, cp_l, mutant=None):
    """:28-113.  Returns (rho_v, rho_c, temp, branch, iterations, margin, amount); branch 'cond', 'evap' or None (untouched)."""
    svp = saturation_vapor_pressure(temp)
    pv = rho_v * R_v * temp
    margin = _margin(pv - svp, svp)
    if pv > svp:
        step, branch, lo, hi = condensed_state, "cond", 0.0, rho_v
    elif pv < svp and rho_c > 0:
        step, branch, lo, hi = evaporated_state, "evap", 0.0, rho_c
    else:
        return rho_v, rho_c, temp, None, 0, margin, 0.0
    it = 0
    tol = 2.e-6 if mutant == "tol_2e-6" else TOL
    while True:
        it += 1
        if it > MAX_ITER:
            raise RuntimeError("bisection needs more than %d iterations" % MAX_ITER)
        amount = (lo + hi) / 2
        rv_loc, rc_loc, temp_loc, diff, svp_loc = step(amount, rho, rho_d, rho_v, rho_c, temp, R_v, cp_d, cp_v, cp_l, mutant)
        margin = min(margin, _margin(diff, svp_loc))
        # condensation: still super-saturated -> condense more; evaporation: still unsaturated -> evaporate more
        if (diff > 0) if branch == "cond" else (diff < 0):
            lo = amount
        else:
            hi = amount
        if abs(hi - lo) <= tol:
            if mutant == "skip_below_1e-9" and amount < 1.e-9:
                return rho_v, rho_c, temp, None, it, margin, amount
            return rv_loc, rc_loc, temp_loc, branch, it, margin, amount


def saturation_adjustment(fields, tracers, micro, R_v, cp_d, cp_v, cp_l=CP_L, mutant=None):
    """modules::saturation_adjustment (:116-147) on numpy (nz,ny,nx,nens) arrays.
    fields: dict with density_dry, temp and one array per tracer name; tracers: (name, positive, adds_mass) in registration order.
    Returns (new fields, info) -- info: per-cell arrays branch (0 none, 1 cond, 2 evap), iters, margin, amount."""
    cond_name = {"kessler": "cloud_liquid", "p3": "cloud_water"}.get(micro)
    if cond_name is None:
        raise ValueError("saturation_adjustment.h only currently supports kessler and p3 microphysics")
    out = {k: np.array(v, dtype=np.float64, copy=True) for k, v in fields.items()}
    rho_d = fields["density_dry"].ravel()
    massy = [fields[n].ravel() for n, _, m in tracers if m]
    return adjust_cells(out, rho_d, massy, cond_name, R_v, cp_d, cp_v, cp_l, mutant)


def adjust_cells(out, rho_d, massy, cond_name, R_v, cp_d, cp_v, cp_l=CP_L, mutant=None):
    """the loop of :142-146 over the cells of out["water_vapor"], out[cond_name], out["temp"] (written in place); massy: the flat
    arrays that add mass, in the order they are summed onto rho_d"""
    if mutant == "rho_reversed":
        massy = massy[::-1]
    rv, rc, tt = out["water_vapor"].reshape(-1), out[cond_name].reshape(-1), out["temp"].reshape(-1)
    n = rho_d.size
    info = {"branch": np.zeros(n, np.int8), "iters": np.zeros(n, np.int32), "margin": np.zeros(n), "amount": np.zeros(n)}
    for i in range(n):
        rho = float(rho_d[i])
        for m in massy:
            rho += float(m[i])
        v, c, t, br, it, mg, amt = compute_adjusted_state(rho, float(rho_d[i]), float(rv[i]), float(rc[i]), float(tt[i]), R_v, cp_d,
                                                          cp_v, cp_l, mutant)
        if br is not None:
            rv[i], rc[i], tt[i] = v, c, t
        info["branch"][i] = {None: 0, "cond": 1, "evap": 2}[br]
        info["iters"][i], info["margin"][i], info["amount"][i] = it, mg, amt
    return out, info


# ---------------------------------------------------------------------------------------------------------------------------
# surface_friction.h
VONK, EPS, AM, BM, PI = 0.4, 1.0e-10, 4.8, 19.3, 3.14159                 # :8-12 (pi as written there)


def z0_est(z, bflx, wnd, ustar):                                         # :16-31
    c1 = PI / 2.0 - 3.0 * math.log(2.0)
    rlmo = -bflx * VONK / (ustar * ustar * ustar + EPS)
    zeta = _std_min(1.0, z * rlmo)
    if zeta >= 0.0:
        psi1 = -AM * zeta
    else:
        x = math.sqrt(math.sqrt(1.0 - BM * zeta))
        psi1 = 2.0 * math.log(1.0 + x) + math.log(1.0 + x * x) - 2.0 * math.atan(x) + c1
    lnz = _std_max(0.0, VONK * wnd / (ustar + EPS) + psi1)
    return z * math.exp(-lnz)


def diag_ustar(z, bflx, wnd, z0, mutant=None):                           # :44-63
    lnz = math.log(z / z0)
    klnz = VONK / lnz
    c1 = (math.pi if mutant == "m_pi" else PI) / 2.0 - 3.0 * math.log(2.0)
    ustar = wnd * klnz
    if bflx != 0.0:
        for _ in range(7 if mutant == "seven_iterations" else 8):
            rlmo = -bflx * VONK / (ustar * ustar * ustar + EPS)
            zeta = _std_min(1.0, z * rlmo)
            if (zeta >= 0.0) if mutant == "zeta_ge" else (zeta > 0.0):
                ustar = VONK * wnd / (lnz + AM * zeta)
            else:
                x = math.sqrt(math.sqrt(1.0 - BM * zeta))
                psi1 = 2.0 * math.log(1.0 + x) + math.log(1.0 + x * x) - 2.0 * math.atan(x) + c1
                ustar = wnd * VONK / (lnz - psi1)
    return ustar


def _level0_means(arrs, nens):
    """per-member horizontal means of level-0 slices (ny,nx,nens), every sample times r_nx_ny, summed from zero in (j,i) order"""
    ny, nx = arrs[0].shape[0], arrs[0].shape[1]
    r_nx_ny = 1.0 / (nx * ny)
    means = []
    for a in arrs:
        m = [0.0] * nens
        for e in range(nens):
            s = 0.0
            for j in range(ny):
                for i in range(nx):
                    s += float(a[j, i, e]) * r_nx_ny
            m[e] = s
        means.append(m)
    return means


def level0_means_slot(arrs, nens):
    """the same means in the order of the HIP path: cell c = j * nx + i belongs to slot c % 16; a slot adds its products in ascending
    c from 0.0, and the 16 slot sums are added in ascending slot order from 0.0 (tests/msa_ref.py: level_sum).  One array (nens)
    per input."""
    ny, nx = arrs[0].shape[0], arrs[0].shape[1]
    r_nx_ny = 1.0 / (nx * ny)
    means = []
    for a in arrs:
        f = np.asarray(a, dtype=np.float64).reshape(ny * nx, nens)
        parts = np.zeros((NS, nens))
        for c in range(ny * nx):
            parts[c % NS] = parts[c % NS] + f[c] * r_nx_ny
        tot = np.zeros(nens)
        for s in range(NS):
            tot = tot + parts[s]
        means.append(tot)
    return means


def surface_friction_z0(zmid0, bflx, gcm_u0, gcm_v0, tau, rho_horz_mean):
    """:96-103 for one member"""
    wnd_spd = _std_max(1.0, math.sqrt(gcm_u0 * gcm_u0 + gcm_v0 * gcm_v0))
    ustar = math.sqrt(tau / rho_horz_mean)
    z0 = z0_est(zmid0, bflx, wnd_spd, ustar)
    return _std_max(0.00001, _std_min(1.0, z0))


def surface_friction_init(rho_d, rho_v, zmid, gcm_u, gcm_v, tau, bflx, means=_level0_means):
    """:66-104.  rho_d, rho_v (nz,ny,nx,nens); zmid, gcm_u, gcm_v (nz,nens); tau, bflx (nens).  The mean density starts from zero.
    means: _level0_means (the order of a serial loop) or level0_means_slot (the HIP path's).
    Returns z0, sfc_bflx (nens) and the zeroed fluxes (ny,nx,nens)."""
    nz, ny, nx, nens = rho_d.shape
    (rho_mean,) = means([rho_d[0] + rho_v[0]], nens)
    z0 = np.array([surface_friction_z0(float(zmid[0, e]), float(bflx[e]), float(gcm_u[0, e]), float(gcm_v[0, e]), float(tau[e]),
                                       rho_mean[e]) for e in range(nens)])
    zeros = np.zeros((ny, nx, nens))
    return z0, np.array(bflx, dtype=np.float64, copy=True), zeros, zeros.copy()


def surface_friction_cell(u, v, u_mean, v_mean, rho_mean, zmid0, bflx, z0, rho_mid0, rho_mid1, rho_mid2, dz, mutant=None):
    """:147-166 for one cell: (sfc_mom_flx_u, sfc_mom_flx_v) in [m2/s2]"""
    u2 = u * u
    v2 = v * v
    wnd_spd = _std_max(1.0, math.sqrt(u2 + v2))
    if mutant == "no_wind_clamp":
        wnd_spd = math.sqrt(u2 + v2)
    ustar = diag_ustar(zmid0, bflx, wnd_spd, z0, mutant)
    tau00 = rho_mean * ustar * ustar
    fu = -(u - u_mean) / wnd_spd * tau00
    fv = -(v - v_mean) / wnd_spd * tau00
    rho_int0 = (rho_mid0 + rho_mid1) / 2
    rho_int1 = (rho_mid1 + rho_mid2) / 2
    rho_sfc = 2.0 * rho_int0 - rho_int1
    if mutant == "rho_sfc_two_levels":
        rho_sfc = rho_int0
    return fu * rho_sfc / dz, fv * rho_sfc / dz


def compute_surface_friction(rho_d, rho_v, uvel, vvel, zmid, zint, z0, sfc_bflx, means=_level0_means, mutant=None):
    """:107-167.  Returns sfc_mom_flx_u, sfc_mom_flx_v (ny,nx,nens).  means: as for surface_friction_init; mutant: one of the
    per-cell FRICTION_MUTANTS (the others change what a cell is handed: tests/moist_surface_cases.py)."""
    nz, ny, nx, nens = rho_d.shape
    rho = rho_d[:3] + rho_v[:3]          # (rho_d + rho_v of a cell: one rounding, as in the reference)
    u_mean, v_mean, rho_mean = means([uvel[0], vvel[0], rho[0]], nens)
    fu, fv = np.zeros((ny, nx, nens)), np.zeros((ny, nx, nens))
    for e in range(nens):
        dz = float(zint[1, e]) - float(zint[0, e])
        for j in range(ny):
            for i in range(nx):
                fu[j, i, e], fv[j, i, e] = surface_friction_cell(
                    float(uvel[0, j, i, e]), float(vvel[0, j, i, e]), u_mean[e], v_mean[e], rho_mean[e], float(zmid[0, e]),
                    float(sfc_bflx[e]), float(z0[e]), float(rho[0, j, i, e]), float(rho[1, j, i, e]), float(rho[2, j, i, e]), dz,
                    mutant)
    return fu, fv
