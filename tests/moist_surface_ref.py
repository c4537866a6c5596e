"""CPU restatement of two coupler modules of the reference, the checker of tests/test_moist_surface_modules.py.  TEST INFRASTRUCTURE.

Written from the reference's text -- pam_core/modules/saturation_adjustment.h and pam_core/modules/surface_friction.h -- as scalar
Python: math.exp / log / atan / sqrt are glibc's, every expression keeps the reference's operation order (Python evaluates left to
right with C's precedence), and no product is fused with a sum.  It shares no code with the HIP path (pam_amd/csrc).

The only addition to the reference is bookkeeping: the iteration count of each bisection and the smallest relative margin
|pv_loc - svp_loc| / svp_loc of its decisions, which tells a comparison where a last-place difference of exp may flip a decision.
"""
import math

import numpy as np

TOL = 1.e-6          # saturation_adjustment.h:33
CP_L = 4188.0        # :141
MAX_ITER = 2048      # the cap of the HIP path; the restatement raises if a state it is given would need more


def _yakl_max(a, b):
    return a if a > b else b


def _std_min(a, b):
    return b if b < a else a


def _std_max(a, b):
    return b if a < b else a


def saturation_vapor_pressure(temp):                                     # :9-12
    tc = temp - 273.15
    return 610.94 * math.exp(17.625 * tc / (243.04 + tc))


def latent_heat_condensation(temp):                                      # :15-18
    tc = temp - 273.15
    return (2500.8 - 2.36 * tc + 0.0016 * tc * tc - 0.00006 * tc * tc * tc) * 1000


def cp_moist(rho_d, rho_v, rho_c, cp_d, cp_v, cp_l):                    # :21-25
    rho = rho_d + rho_v + rho_c
    return rho_d / rho * cp_d + rho_v / rho * cp_v + rho_c / rho * cp_l


def condensed_state(amount, rho, rho_d, rho_v, rho_c, temp, R_v, cp_d, cp_v, cp_l):
    """one iteration of the condensation loop (:52-59) for rho_cond = amount: (rv_loc, rc_loc, temp_loc, pv_loc - svp_loc, svp_loc)"""
    rv_loc = _yakl_max(0.0, rho_v - amount)
    rc_loc = _yakl_max(0.0, rho_c + amount)
    Lv = latent_heat_condensation(temp)
    cp = cp_moist(rho_d, rv_loc, rc_loc, cp_d, cp_v, cp_l)
    temp_loc = temp + amount * Lv / (rho * cp)
    svp_loc = saturation_vapor_pressure(temp_loc)
    pv_loc = rv_loc * R_v * temp_loc
    return rv_loc, rc_loc, temp_loc, pv_loc - svp_loc, svp_loc


def evaporated_state(amount, rho, rho_d, rho_v, rho_c, temp, R_v, cp_d, cp_v, cp_l):
    """one iteration of the evaporation loop (:89-96) for rho_evap = amount"""
    rv_loc = _yakl_max(0.0, rho_v + amount)
    rc_loc = _yakl_max(0.0, rho_c - amount)
    Lv = latent_heat_condensation(temp)
    cp = cp_moist(rho_d, rv_loc, rc_loc, cp_d, cp_v, cp_l)
    temp_loc = temp - amount * Lv / (rho * cp)
    svp_loc = saturation_vapor_pressure(temp_loc)
    pv_loc = rv_loc * R_v * temp_loc
    return rv_loc, rc_loc, temp_loc, pv_loc - svp_loc, svp_loc


def compute_adjusted_state(rho, rho_d, rho_v, rho_c, temp, R_v, cp_d, cp_v, cp_l):
    """:28-113.  Returns (rho_v, rho_c, temp, branch, iterations, margin, amount); branch 'cond', 'evap' or None (untouched)."""
    svp = saturation_vapor_pressure(temp)
    pv = rho_v * R_v * temp
    margin = abs(pv - svp) / svp
    if pv > svp:
        step, branch, lo, hi = condensed_state, "cond", 0.0, rho_v
    elif pv < svp and rho_c > 0:
        step, branch, lo, hi = evaporated_state, "evap", 0.0, rho_c
    else:
        return rho_v, rho_c, temp, None, 0, margin, 0.0
    it = 0
    while True:
        it += 1
        if it > MAX_ITER:
            raise RuntimeError("bisection needs more than %d iterations" % MAX_ITER)
        amount = (lo + hi) / 2
        rv_loc, rc_loc, temp_loc, diff, svp_loc = step(amount, rho, rho_d, rho_v, rho_c, temp, R_v, cp_d, cp_v, cp_l)
        margin = min(margin, abs(diff) / svp_loc)
        # condensation: still super-saturated -> condense more; evaporation: still unsaturated -> evaporate more
        if (diff > 0) if branch == "cond" else (diff < 0):
            lo = amount
        else:
            hi = amount
        if abs(hi - lo) <= TOL:
            return rv_loc, rc_loc, temp_loc, branch, it, margin, amount


def saturation_adjustment(fields, tracers, micro, R_v, cp_d, cp_v, cp_l=CP_L):
    """modules::saturation_adjustment (:116-147) on numpy (nz,ny,nx,nens) arrays.
    fields: dict with density_dry, temp and one array per tracer name; tracers: (name, positive, adds_mass) in registration order.
    Returns (new fields, info) -- info: per-cell arrays branch (0 none, 1 cond, 2 evap), iters, margin, amount."""
    cond_name = {"kessler": "cloud_liquid", "p3": "cloud_water"}.get(micro)
    if cond_name is None:
        raise ValueError("saturation_adjustment.h only currently supports kessler and p3 microphysics")
    out = {k: np.array(v, dtype=np.float64, copy=True) for k, v in fields.items()}
    rho_d = fields["density_dry"].ravel()
    massy = [fields[n].ravel() for n, _, m in tracers if m]
    rv, rc, tt = out["water_vapor"].reshape(-1), out[cond_name].reshape(-1), out["temp"].reshape(-1)
    n = rho_d.size
    info = {"branch": np.zeros(n, np.int8), "iters": np.zeros(n, np.int32), "margin": np.zeros(n), "amount": np.zeros(n)}
    for i in range(n):
        rho = float(rho_d[i])
        for m in massy:
            rho += float(m[i])
        v, c, t, br, it, mg, amt = compute_adjusted_state(rho, float(rho_d[i]), float(rv[i]), float(rc[i]), float(tt[i]), R_v, cp_d,
                                                          cp_v, cp_l)
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


def diag_ustar(z, bflx, wnd, z0):                                        # :44-63
    lnz = math.log(z / z0)
    klnz = VONK / lnz
    c1 = PI / 2.0 - 3.0 * math.log(2.0)
    ustar = wnd * klnz
    if bflx != 0.0:
        for _ in range(8):
            rlmo = -bflx * VONK / (ustar * ustar * ustar + EPS)
            zeta = _std_min(1.0, z * rlmo)
            if zeta > 0.0:
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


def surface_friction_z0(zmid0, bflx, gcm_u0, gcm_v0, tau, rho_horz_mean):
    """:96-103 for one member"""
    wnd_spd = _std_max(1.0, math.sqrt(gcm_u0 * gcm_u0 + gcm_v0 * gcm_v0))
    ustar = math.sqrt(tau / rho_horz_mean)
    z0 = z0_est(zmid0, bflx, wnd_spd, ustar)
    return _std_max(0.00001, _std_min(1.0, z0))


def surface_friction_init(rho_d, rho_v, zmid, gcm_u, gcm_v, tau, bflx):
    """:66-104.  rho_d, rho_v (nz,ny,nx,nens); zmid, gcm_u, gcm_v (nz,nens); tau, bflx (nens).  The mean density starts from zero.
    Returns z0, sfc_bflx (nens) and the zeroed fluxes (ny,nx,nens)."""
    nz, ny, nx, nens = rho_d.shape
    (rho_mean,) = _level0_means([rho_d[0] + rho_v[0]], nens)
    z0 = np.array([surface_friction_z0(float(zmid[0, e]), float(bflx[e]), float(gcm_u[0, e]), float(gcm_v[0, e]), float(tau[e]),
                                       rho_mean[e]) for e in range(nens)])
    zeros = np.zeros((ny, nx, nens))
    return z0, np.array(bflx, dtype=np.float64, copy=True), zeros, zeros.copy()


def surface_friction_cell(u, v, u_mean, v_mean, rho_mean, zmid0, bflx, z0, rho_mid0, rho_mid1, rho_mid2, dz):
    """:147-166 for one cell: (sfc_mom_flx_u, sfc_mom_flx_v) in [m2/s2]"""
    u2 = u * u
    v2 = v * v
    wnd_spd = _std_max(1.0, math.sqrt(u2 + v2))
    ustar = diag_ustar(zmid0, bflx, wnd_spd, z0)
    tau00 = rho_mean * ustar * ustar
    fu = -(u - u_mean) / wnd_spd * tau00
    fv = -(v - v_mean) / wnd_spd * tau00
    rho_int0 = (rho_mid0 + rho_mid1) / 2
    rho_int1 = (rho_mid1 + rho_mid2) / 2
    rho_sfc = 2.0 * rho_int0 - rho_int1
    return fu * rho_sfc / dz, fv * rho_sfc / dz


def compute_surface_friction(rho_d, rho_v, uvel, vvel, zmid, zint, z0, sfc_bflx):
    """:107-167.  Returns sfc_mom_flx_u, sfc_mom_flx_v (ny,nx,nens)."""
    nz, ny, nx, nens = rho_d.shape
    rho = rho_d[:3] + rho_v[:3]          # (rho_d + rho_v of a cell: one rounding, as in the reference)
    u_mean, v_mean, rho_mean = _level0_means([uvel[0], vvel[0], rho[0]], nens)
    fu, fv = np.zeros((ny, nx, nens)), np.zeros((ny, nx, nens))
    for e in range(nens):
        dz = float(zint[1, e]) - float(zint[0, e])
        for j in range(ny):
            for i in range(nx):
                fu[j, i, e], fv[j, i, e] = surface_friction_cell(
                    float(uvel[0, j, i, e]), float(vvel[0, j, i, e]), u_mean[e], v_mean[e], rho_mean[e], float(zmid[0, e]),
                    float(sfc_bflx[e]), float(z0[e]), float(rho[0, j, i, e]), float(rho[1, j, i, e]), float(rho[2, j, i, e]), dz)
    return fu, fv
