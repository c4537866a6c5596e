"""The SHOC coupling layer (physics/sgs/shoc/SGS.h:254-411 pack, :718-756 unpack) and the stand-in for shoc_main in numpy, written from the
reference's loops and from the stand-in's description, independently of pam_amd/csrc/shoc_device.h.  Layout 0 throughout: SHOC arrays are
(lev, col), hwind (2, lev, col), qtracers (tr, lev, col), wtracer_sfc (tr, col); SHOC's level s = nz-1-k (cells), nz-k (interfaces).
numpy's float64 arithmetic rounds every operation (no fma), so the order of the expressions below is the result's bits.
TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

# SGS.h:60-80
CONSTS = dict(R_d=287.042, cp_d=1004.64, R_v=461.505, p0=1.0e5, grav=9.80616, latvap=2501000.0)
CONSTS["cv_d"] = CONSTS["cp_d"] - CONSTS["R_d"]
# the coupler's options R_d, R_v, which compute_pressure_array reads (pam_coupler.h:375-376): the Kessler microphysics' values
CONSTS["pres_R_d"], CONSTS["pres_R_v"] = 287.0, 461.0
KESSLER_TRACERS = ("precip_liquid",)
P3_TRACERS = ("cloud_water_num", "rain", "rain_num", "ice", "ice_num", "ice_rime", "ice_rime_vol")     # SGS.h:243-249
STATE_4D = ("rho_d", "rho_v", "rho_c", "uvel", "vvel", "wvel", "temp", "tke", "wthv_sec", "tk", "tkh", "cldfrac")
CELL_ARRAYS = ("thv", "zt_grid", "pres", "pdel", "w_field", "inv_exner", "host_dse", "tke", "thetal", "qw", "wthv_sec", "tk", "ql", "cldfrac",
               "mix", "isotropy", "w_sec", "wqls_sec", "brunt", "ql2", "tkh", "exner")
EDGE_ARRAYS = ("zi_grid", "presi", "thl_sec", "qw_sec", "qwthl_sec", "wthl_sec", "wqw_sec", "wtke_sec", "uw_sec", "vw_sec", "w3")
COLUMN_ARRAYS = ("host_dx", "host_dy", "wthl_sfc", "wqw_sfc", "uw_sfc", "vw_sfc", "phis", "pblh", "ustar", "obklen")
PACKED = ("host_dx", "host_dy", "thv", "zt_grid", "zi_grid", "pres", "presi", "pdel", "wthl_sfc", "wqw_sfc", "uw_sfc", "vw_sfc", "wtracer_sfc",
          "w_field", "inv_exner", "phis", "host_dse", "tke", "thetal", "qw", "hwind", "qtracers", "wthv_sec", "tk", "ql", "cldfrac", "tkh", "exner")


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


def std_min(a, b):
    """std::min(a, b) = (b < a) ? b : a"""
    return np.where(np.less(b, a), b, a)


def columns(f):
    """(nz, ny, nx, nens) -> (nz, ncol): dm.get_lev_col"""
    return np.ascontiguousarray(f, dtype=np.float64).reshape(f.shape[0], -1)


def pack(state, qtracers, sfc_mom_flx_u, sfc_mom_flx_v, zint, zmid, xlen, ylen, consts=CONSTS, pow=libm_pow):
    """SGS.h:254-411.  state: the STATE_4D arrays (nz,ny,nx,nens); qtracers: list of (nz,ny,nx,nens); zint (nz+1,nens), zmid (nz,nens)"""
    nz, ny, nx, nens = state["rho_d"].shape
    ncol = ny * nx * nens
    p0, grav, R_d, cp_d, latvap = (consts[k] for k in ("p0", "grav", "R_d", "cp_d", "latvap"))
    pres_R_d, pres_R_v = consts["pres_R_d"], consts["pres_R_v"]   # the coupler's options, not the SGS class's constants
    s = {k: columns(state[k]) for k in STATE_4D}
    q = [columns(x) for x in qtracers]
    zi = np.tile(np.asarray(zint, dtype=np.float64), (1, ny * nx))           # zint_tmp(k,j,i,iens) = zint_pam(k,iens): column c has member c % nens
    zm = np.tile(np.asarray(zmid, dtype=np.float64), (1, ny * nx))
    crm_dx = xlen / nx
    crm_dy = crm_dx if ny == 1 else ylen / ny
    A = {"host_dx": np.full(ncol, crm_dx), "host_dy": np.full(ncol, crm_dy), "wthl_sfc": np.zeros(ncol), "wqw_sfc": np.zeros(ncol),
         "uw_sfc": np.asarray(sfc_mom_flx_u, dtype=np.float64).reshape(-1).copy(),
         "vw_sfc": np.asarray(sfc_mom_flx_v, dtype=np.float64).reshape(-1).copy(), "phis": zi[0] * grav,
         "wtracer_sfc": np.zeros((len(q), ncol))}
    with np.errstate(all="ignore"):
        pmid = s["rho_d"] * pres_R_d * s["temp"] + s["rho_v"] * pres_R_v * s["temp"]          # pam_coupler.h:375-390
        rho_total = s["rho_d"] + s["rho_v"]
        z = zm
        dz = zi[1:] - zi[:-1]
        t = s["temp"]
        qv = std_max(0.0, s["rho_v"]) / rho_total
        ql = std_max(0.0, s["rho_c"]) / rho_total
        exner = pow(pmid / p0, R_d / cp_d)
        theta = t / exner
        theta_v = theta * (1 + 0.61 * qv - ql)
        theta_l = theta - (1 / exner) * (latvap / cp_d) * ql
        zt = z - zi[0]
        cell = {"ql": ql, "qw": qv + ql, "zt_grid": zt, "pres": pmid, "pdel": grav * rho_total * dz, "thv": theta_v, "w_field": s["wvel"],
                "exner": exner, "inv_exner": 1.0 / exner, "host_dse": cp_d * t + grav * zt + A["phis"], "thetal": theta_l,
                "wthv_sec": s["wthv_sec"], "tke": std_max(0.004, s["tke"] / rho_total), "tk": s["tk"], "tkh": s["tkh"], "cldfrac": s["cldfrac"]}
        for k, v in cell.items():
            A[k] = np.ascontiguousarray(v[::-1])                                 # k_shoc = nz-1-k
        A["hwind"] = np.stack([s["uvel"][::-1], s["vvel"][::-1]])
        A["qtracers"] = np.stack([std_max(0.0, x / rho_total)[::-1] for x in q]) if q else np.zeros((0, nz, ncol))
        half = grav * rho_total * dz / 2
        pint = np.empty((nz + 1, ncol))
        pint[0] = pmid[0] + half[0]
        pint[nz] = pmid[nz - 1] - half[nz - 1]
        for k in range(1, nz):
            pint[k] = 0.5 * (pmid[k - 1] - half[k - 1] + pmid[k] + half[k])
        A["zi_grid"] = np.ascontiguousarray((zi - zi[0])[::-1])                  # k_shoc = nz-k
        A["presi"] = np.ascontiguousarray(pint[::-1])
    return A


def standin(A):
    """the test double of shoc_main (pam_amd/csrc/shoc_device.h: standin_column describes it), on a layout-0 set; returns the set after it"""
    A = {k: np.array(v, dtype=np.float64, copy=True) for k, v in A.items()}
    nlev, ncol = A["thv"].shape
    ntr = A["qtracers"].shape[0]
    with np.errstate(all="ignore"):
        acc = np.zeros(ncol)
        for name, w in (("host_dx", 0.0009765625), ("host_dy", 0.00048828125), ("wthl_sfc", 3.0), ("wqw_sfc", 5.0), ("uw_sfc", 7.0),
                        ("vw_sfc", 11.0), ("phis", 0.00390625)):
            acc = acc + A[name] * w
        for tr in range(ntr):
            acc = acc + A["wtracer_sfc"][tr] * (13.0 + tr)
        for s in range(nlev):
            t = A["thv"][s] * 0.001
            for name, w in (("zt_grid", 0.0002), ("pres", 0.00003), ("pdel", 0.0004), ("w_field", 0.5), ("inv_exner", 0.7)):
                t = t + A[name][s] * w
            acc = acc + (1.0 + s * 0.0625) * t
        for s in range(nlev + 1):
            t = A["zi_grid"][s] * 0.0003
            t = t + A["presi"][s] * 0.00002
            acc = acc + (1.0 + s * 0.03125) * t
        A["pblh"], A["ustar"], A["obklen"] = acc, acc * 0.5, acc * -0.25

        def mixed(x):
            lo = np.concatenate([x[:1], x[:-1]])
            hi = np.concatenate([x[1:], x[-1:]])
            return 0.25 * lo + 0.5 * x + 0.25 * hi
        flip, dry, cf = A["tk"] < 0, A["wthv_sec"] < 0, A["cldfrac"].copy()
        m = {k: mixed(A[k]) for k in ("host_dse", "tke", "thetal", "qw", "wthv_sec", "tk", "ql", "cldfrac")}
        A["hwind"] = np.stack([mixed(A["hwind"][0]), mixed(A["hwind"][1])])
        A["qtracers"] = np.stack([np.where(flip, -mixed(x), mixed(x)) for x in A["qtracers"]]) if ntr else A["qtracers"]
        for k in ("host_dse", "tke", "thetal", "wthv_sec", "tk"):
            A[k] = m[k]
        A["qw"] = np.where(flip, -m["qw"], m["qw"])
        qn = np.where(dry, 0.0, m["ql"])
        A["ql"] = qn
        A["cldfrac"] = 3.0 * m["cldfrac"] - 1.0
        q2 = qn * qn
        A["ql2"] = np.where(cf < 0.2, 0.0, np.where(cf < 0.4, q2 * 2048.0, np.where(cf < 0.7, q2 * 2.0, q2 * 0.0078125)))
        A["mix"] = A["zt_grid"] * 0.5
        A["isotropy"] = A["pres"] * 0.0009765625
        A["w_sec"] = A["pdel"] * 0.001
        A["wqls_sec"] = A["w_field"] * 0.25
        A["brunt"] = A["inv_exner"] * 0.01
        A["tkh"] = m["tk"] * 2.0
        p = A["presi"] * 0.000244140625
        for j, name in enumerate(EDGE_ARRAYS[2:]):
            A[name] = A["zi_grid"] * (j + 1.0) + p
    return A


def unpack(A, state, qtracers, consts=CONSTS):
    """SGS.h:718-756.  Returns (state after, tracers after) with the shapes of the inputs; "inv_qc_relvar" is added to the state"""
    shape = state["rho_d"].shape
    cp_d, cv_d, latvap = consts["cp_d"], consts["cv_d"], consts["latvap"]
    up = lambda x: x[::-1]                                                       # k_shoc = nz-1-k
    out = {k: np.array(v, dtype=np.float64, copy=True) for k, v in state.items()}
    with np.errstate(all="ignore"):
        qw, ql = up(A["qw"]), up(A["ql"])
        qv = qw - ql
        temp_old = columns(state["temp"])
        rho_d = columns(state["rho_d"])
        temp_new = up(A["thetal"]) * up(A["exner"]) + (latvap / cp_d) * ql
        new = {"temp": temp_old + (temp_new - temp_old) * cv_d / cp_d}
        new["rho_v"] = std_max(0.0, qv * rho_d / (1 - qv))
        rho_total = rho_d + new["rho_v"]
        new["rho_c"] = std_max(0.0, ql * rho_total)
        new["uvel"], new["vvel"] = up(A["hwind"][0]), up(A["hwind"][1])
        new["tke"] = up(A["tke"]) * rho_total
        for k in ("wthv_sec", "tk", "tkh"):
            new[k] = up(A[k])
        new["cldfrac"] = std_max(0.0, std_min(1.0, up(A["cldfrac"])))
        q_out = [std_max(0.0, up(x) * rho_total).reshape(shape) for x in A["qtracers"]]
        rcm, rcm2 = ql, up(A["ql2"])
        new["inv_qc_relvar"] = np.where((rcm != 0) & (rcm2 != 0), std_min(10.0, std_max(0.001, rcm * rcm / rcm2)), 1.0)
    for k, v in new.items():
        out[k] = np.ascontiguousarray(v).reshape(shape)
    assert len(q_out) == len(qtracers)
    return out, q_out


def to_layout1(A):
    """the layout-0 set as SCREAM's C++ layout: (col, lev), hwind (col, 2, lev), qtracers (col, tr, lev), wtracer_sfc (col, tr)"""
    out = {}
    for k, v in A.items():
        if v.ndim == 1:
            out[k] = v.copy()
        elif k in ("hwind", "qtracers"):
            out[k] = np.ascontiguousarray(v.transpose(2, 0, 1))
        else:
            out[k] = np.ascontiguousarray(v.T)
    return out


def shoc_index(layout, col, s, ncol, nlev, comp=0, ncomp=1):
    """the flat index of (col, s[, comp]) in python integers"""
    return (comp * nlev + s) * ncol + col if layout == 0 else (col * ncomp + comp) * nlev + s
