"""The P3 coupling layer (physics/micro/p3/Microphysics.h:342-409 pack with the saturation adjustment of :769-852, :680-717 unpack) and
the stand-in for p3_main in numpy, written from the reference's loops and from the stand-in's description, independently of
pam_amd/csrc/p3_device.h.  Layout 0 throughout: P3 arrays are (lev, col) with lev = k (not flipped), col_location (3, col), p3_tend_out
(plane, lev, col).  numpy's float64 arithmetic rounds every operation (no fma), so the order of the expressions below is the result's
bits; exp and pow are the C library's, called cell by cell (numpy's vectorised exp is not glibc's).  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

# Microphysics.h:75-87
CONSTS = dict(R_d=287.042, cp_d=1004.64, R_v=461.505, cp_v=1859.0, p0=1.0e5, grav=9.80616, cp_l=4188.0)
CONSTS["cv_d"] = CONSTS["cp_d"] - CONSTS["R_d"]
TOL, MAX_ITER = 1.e-6, 2048           # :772; the cap of the HIP path: the restatement raises if a state would need more
TRACERS = ("cloud_water_num", "rain", "rain_num", "ice", "ice_num", "ice_rime", "ice_rime_vol")       # the order of pam_amd_p3_pack
STATE_4D = ("rho_d", "rho_v", "rho_c", "temp", "nccn_prescribed", "nc_nuceat_tend", "ni_activated", "q_prev", "t_prev")
INOUT = ("qc", "nc", "qr", "nr", "th_atm", "qv", "qi", "qm", "ni", "bm")
PACKED = INOUT + ("pres", "dz", "nc_nuceat_tend", "nccn_prescribed", "ni_activated", "inv_qc_relvar", "dpres", "inv_exner", "cld_frac_r",
                  "cld_frac_l", "cld_frac_i", "q_prev", "t_prev", "col_location", "exner")
UNPACKED = ("rho_c", "rho_v", "temp", "q_prev", "t_prev", "liq_ice_exchange_out", "vap_liq_exchange_out", "vap_ice_exchange_out",
            "precip_liq_surf_out", "precip_ice_surf_out")


def libm_pow(x, y):
    """the C library's pow, element by element: what the reference calls"""
    def one(v):
        try:
            return math.pow(v, y)
        except (ValueError, OverflowError):         # a negative base: the C library returns NaN
            return math.nan
    return np.array([one(float(v)) for v in np.asarray(x, dtype=np.float64).reshape(-1)]).reshape(np.shape(x))


def std_max(a, b):
    """std::max(a, b) = (a < b) ? b : a"""
    return np.where(np.less(a, b), b, a)


def _smax(a, b):
    return b if a < b else a


def columns(f):
    """(nz, ny, nx, nens) -> (nz, ncol): dm.get_lev_col"""
    return np.ascontiguousarray(f, dtype=np.float64).reshape(f.shape[0], -1)


# ---------------------------------------------------------------------------------------------------------------------------
# :745-852, one cell

def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def saturation_vapor_pressure(temp):                                     # :746-749
    tc = temp - 273.15
    return 610.94 * _exp(17.625 * tc / (243.04 + tc))


def latent_heat_condensation(temp):                                      # :753-756
    tc = temp - 273.15
    return (2500.8 - 2.36 * tc + 0.0016 * tc * tc - 0.00006 * tc * tc * tc) * 1000


def cp_moist(rho_d, rho_v, rho_c, cp_d, cp_v, cp_l):                    # :760-764
    rho = rho_d + rho_v + rho_c
    return rho_d / rho * cp_d + rho_v / rho * cp_v + rho_c / rho * cp_l


def compute_adjusted_state(rho, rho_d, rho_v, rho_c, temp, R_v, cp_d, cp_v, cp_l):
    """:769-852.  Returns (rho_v, rho_c, temp, branch, iterations, margin); branch 'cond', 'evap' or None (untouched).  margin: the
    smallest relative distance of a bisection decision (pv against svp) from the tie, the measure the device gate exempts cells by."""
    svp = saturation_vapor_pressure(temp)
    pv = rho_v * R_v * temp
    margin = abs(pv - svp) / svp
    if pv > svp:
        cond, lo, hi = True, 0.0, rho_v
    elif pv < svp and rho_c > 0:
        cond, lo, hi = False, 0.0, rho_c
    else:
        return rho_v, rho_c, temp, None, 0, margin
    it = 0
    while True:
        it += 1
        if it > MAX_ITER:
            raise RuntimeError("bisection needs more than %d iterations" % MAX_ITER)
        x = (lo + hi) / 2
        if cond:
            rv_loc = _smax(0.0, rho_v - x)
            rc_loc = _smax(0.0, rho_c + x)
        else:
            rv_loc = _smax(0.0, rho_v + x)
            rc_loc = _smax(0.0, rho_c - x)
        Lv = latent_heat_condensation(temp)
        cp = cp_moist(rho_d, rv_loc, rc_loc, cp_d, cp_v, cp_l)
        temp_loc = temp + x * Lv / (rho * cp) if cond else temp - x * Lv / (rho * cp)
        svp_loc = saturation_vapor_pressure(temp_loc)
        pv_loc = rv_loc * R_v * temp_loc
        margin = min(margin, abs(pv_loc - svp_loc) / svp_loc)
        if (pv_loc > svp_loc) if cond else (pv_loc < svp_loc):
            lo = x
        else:
            hi = x
        if abs(hi - lo) <= TOL:
            return rv_loc, rc_loc, temp_loc, ("cond" if cond else "evap"), it, margin


def adjust(rho_d, rho_v, rho_c, temp, consts=CONSTS):
    """:344-348 on (nz, ncol) arrays.  Returns (rho_v, rho_c, temp, info); info: branch (0 none, 1 cond, 2 evap), iters, margin"""
    rv, rc, tt = (np.array(a, dtype=np.float64, copy=True) for a in (rho_v, rho_c, temp))
    n = rv.size
    info = {"branch": np.zeros(n, np.int8), "iters": np.zeros(n, np.int32), "margin": np.zeros(n)}
    fd, fv, fc, ft = rho_d.reshape(-1), rv.reshape(-1), rc.reshape(-1), tt.reshape(-1)
    for i in range(n):
        d, v, c, t = float(fd[i]), float(fv[i]), float(fc[i]), float(ft[i])
        v2, c2, t2, br, it, mg = compute_adjusted_state(d + v, d, v, c, t, consts["R_v"], consts["cp_d"], consts["cp_v"], consts["cp_l"])
        if br is not None:
            fv[i], fc[i], ft[i] = v2, c2, t2
        info["branch"][i] = {None: 0, "cond": 1, "evap": 2}[br]
        info["iters"][i], info["margin"][i] = it, mg
    for k in info:
        info[k] = info[k].reshape(rv.shape)
    return rv, rc, tt, info


# ---------------------------------------------------------------------------------------------------------------------------

def pack(state, tracers, zint, do_adjust, first_step, consts=CONSTS, pow=libm_pow):
    """:273-409.  state: the STATE_4D arrays (nz,ny,nx,nens); tracers: the seven of TRACERS.  Returns (P3 inputs in layout 0, the coupler's
    (rho_v, rho_c, temp) after the adjustment as (nz,ny,nx,nens), info of the adjustment or None)"""
    shape = state["rho_d"].shape
    nz, ny, nx, nens = shape
    ncol = ny * nx * nens
    R_d, R_v, cp_d, p0, grav = (consts[k] for k in ("R_d", "R_v", "cp_d", "p0", "grav"))
    s = {k: columns(state[k]) for k in STATE_4D}
    q = [columns(x) for x in tracers]
    zi = np.tile(np.asarray(zint, dtype=np.float64), (1, ny * nx))           # column c has member c % nens
    rho_d, rho_v, rho_c, temp, info = s["rho_d"], s["rho_v"], s["rho_c"], s["temp"], None
    if do_adjust:
        rho_v, rho_c, temp, info = adjust(rho_d, rho_v, rho_c, temp, consts)
    with np.errstate(all="ignore"):
        o = {"qc": rho_c / rho_d, "nc": q[0] / rho_d, "qr": q[1] / rho_d, "nr": q[2] / rho_d, "qi": q[3] / rho_d, "ni": q[4] / rho_d,
             "qm": q[5] / rho_d, "bm": q[6] / rho_d, "qv": rho_v / rho_d}
        pd = R_d * rho_d * temp
        pressure = pd + R_v * rho_v * temp
        o["pres"] = pd
        o["exner"] = pow(pressure / p0, R_d / cp_d)
        o["inv_exner"] = 1. / o["exner"]
        o["th_atm"] = temp * o["inv_exner"]
        o["dz"] = zi[1:] - zi[:-1]
        o["dpres"] = rho_d * grav * o["dz"]
        o["col_location"] = np.ones((3, ncol))
        if first_step:
            o["q_prev"], o["t_prev"] = o["qv"].copy(), temp.copy()
        else:
            o["q_prev"], o["t_prev"] = s["q_prev"] / rho_d, s["t_prev"].copy()
    for k in ("cld_frac_l", "cld_frac_i", "cld_frac_r", "inv_qc_relvar"):
        o[k] = np.ones((nz, ncol))
    for k in ("nc_nuceat_tend", "nccn_prescribed", "ni_activated"):
        o[k] = s[k].copy()
    return o, tuple(a.reshape(shape) for a in (rho_v, rho_c, temp)), info


def standin(packed, num_tend_out=0):
    """the stand-in for p3_main as pam_amd/csrc/p3_device.h describes it, on the layout-0 set: returns the set after it"""
    a = {k: np.array(v, copy=True) for k, v in packed.items()}
    nz, ncol = a["qc"].shape
    with np.errstate(all="ignore"):
        acc = np.zeros(ncol)
        for r in range(3):
            acc = acc + a["col_location"][r] * (r + 1.0)
        weights = (("pres", 0.00001), ("dz", 0.001), ("nc_nuceat_tend", 3.0), ("nccn_prescribed", 5.0), ("ni_activated", 7.0),
                   ("inv_qc_relvar", 0.5), ("dpres", 0.0001), ("inv_exner", 0.25), ("cld_frac_r", 0.125), ("cld_frac_l", 0.0625),
                   ("cld_frac_i", 0.03125), ("q_prev", 11.0), ("t_prev", 0.001))
        for k in range(nz):
            t = None
            for name, w in weights:
                t = a[name][k] * w if t is None else t + a[name][k] * w
            acc = acc + (1.0 + k * 0.0625) * t
        a["precip_liq_surf"] = acc
        a["precip_ice_surf"] = acc * -0.25
        m = {}
        for j, name in enumerate(INOUT):
            x = packed[name]
            lo, hi = np.concatenate([x[:1], x[:-1]]), np.concatenate([x[1:], x[-1:]])
            m[name] = (0.25 * lo + 0.5 * x) + 0.25 * hi
            neg = (packed["ni_activated"] < 0) if (j & 1) else (packed["nc_nuceat_tend"] < 0)
            a[name] = m[name] if name == "th_atm" else np.where(neg, -m[name], m[name])
        a["diag_eff_radius_qc"] = a["dz"] * 0.001
        a["diag_eff_radius_qi"] = a["dpres"] * 0.001
        a["diag_eff_radius_qr"] = a["inv_exner"] * 0.01
        a["bulk_qi"] = a["q_prev"] * 2.0
        a["precip_total_tend"] = a["t_prev"] * 0.001
        a["nevapr"] = (a["cld_frac_l"] * 0.5 + a["cld_frac_i"] * 0.25) + a["cld_frac_r"] * 0.125
        a["qr_evap_tend"] = a["inv_qc_relvar"] * 3.0
        a["qv2qi_depos_tend"] = a["nccn_prescribed"] * 0.5
        a["mu_c"] = a["nc_nuceat_tend"] * 0.25
        a["lamc"] = a["ni_activated"] * 0.125
        a["liq_ice_exchange"] = m["qc"] * 0.5
        a["vap_liq_exchange"] = m["qv"] * 0.25
        a["vap_ice_exchange"] = m["qi"] * -0.5
        a["p3_tend_out"] = np.stack([a["pres"] * 0.000001 + p for p in range(num_tend_out)]) if num_tend_out else np.zeros((0, nz, ncol))
        kk = np.arange(nz + 1, dtype=np.float64)[:, None]
        a["precip_liq_flux"] = np.concatenate([a["pres"], a["pres"][-1:]]) * 0.00001 + kk
        a["precip_ice_flux"] = np.concatenate([a["dz"][:1], a["dz"]]) * 0.01 - kk
    return a


def unpack(after, rho_d, temp_old, tracers_shape, consts=CONSTS):
    """:680-717.  after: the layout-0 set after p3_main; rho_d, temp_old (nz,ny,nx,nens): the coupler's (temp_old after the adjustment).
    Returns (dict of the UNPACKED arrays, list of the seven tracers)"""
    shape = rho_d.shape
    nz, ny, nx, nens = shape
    rd, told = columns(rho_d), columns(temp_old)
    cv_d, cp_d = consts["cv_d"], consts["cp_d"]
    with np.errstate(all="ignore"):
        c = lambda name: std_max(after[name] * rd, 0.0).reshape(shape)
        out = {"rho_c": c("qc"), "rho_v": c("qv")}
        q = [c(n) for n in ("nc", "qr", "nr", "qi", "ni", "qm", "bm")]
        temp_new = after["th_atm"] * after["exner"]
        temp = told + (temp_new - told) * cv_d / cp_d
    out["temp"] = temp.reshape(shape)
    out["q_prev"] = out["rho_v"].copy()
    out["t_prev"] = out["temp"].copy()
    for k in ("liq_ice", "vap_liq", "vap_ice"):
        out[k + "_exchange_out"] = after[k + "_exchange"].reshape(shape).copy()
    out["precip_liq_surf_out"] = after["precip_liq_surf"].reshape(ny, nx, nens).copy()
    out["precip_ice_surf_out"] = after["precip_ice_surf"].reshape(ny, nx, nens).copy()
    return out, q


def to_layout1(arrays):
    """the layout-0 set as layout 1: (col, lev) with lev = nlev-1-k; col_location (col, 3) not flipped; p3_tend_out (col, plane, lev)"""
    out = {}
    for n, v in arrays.items():
        if n == "col_location":
            out[n] = np.ascontiguousarray(v.T)
        elif v.ndim == 1:
            out[n] = v.copy()
        elif v.ndim == 2:
            out[n] = np.ascontiguousarray(v[::-1].T)
        else:
            out[n] = np.ascontiguousarray(v[:, ::-1].transpose(2, 0, 1))
    return out
