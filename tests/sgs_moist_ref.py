"""The moist branch of the Smagorinsky SGS closure and the surface fluxes of heat and vapour in its solve: the numpy restatement of the
contract (include/pam_amd_modules.h at pam_amd_sgs_smag_coefficients_moist and pam_amd_sgs_smag_diffuse_fluxes),
its scalar-loop twin, the named cases and the mutants of the restatement.  TEST INFRASTRUCTURE ONLY.

What is unchanged comes from sgs_ref (the differences, the rows, the Thomas algorithm, the shapes, the constants).  As there, numpy's
element-wise float64 arithmetic is IEEE and never contracted, no numpy reduction takes part, and every function works in the dtype of its
inputs.  The exponential is part of the contract (exp_c), so no libm takes part either, and the device bodies are held to this file bit
for bit.  A mutant is a deliberately wrong variant of ONE line, switched on by name; each must be caught by a named case."""
import math

import numpy as np

import sgs_ref as ref
from sgs_ref import WINDS, same_bits, results_differ, shape_id, SHAPES      # noqa: F401

MUTANTS = ("branch_ge", "qs_without_rho", "loading_dropped", "dqt_dropped", "second_cloud_ignored_in_sat", "branch_on_upper_neighbour",
           "exp_degree_12", "shf_without_rho", "lhf_divided_by_rho", "flux_at_top")
R_D, R_V, LATVAP = 287.042, 461.505, 2501000.0
LOG2E, LN2_HI, LN2_LO = 1.44269504088896338700, 6.93147180369123816490e-01, 1.90821492927058770002e-10


# ---- 1. the exponential

def exp_c(x, degree=13):
    """n = floor(x log2(e) + 0.5); r = (x - n ln2_hi) - n ln2_lo; Horner with 1 / k!; ldexp(p, n).  NaN -> NaN, x < -700 -> 0, x > 700 ->
    +inf, none of which reaches the integer conversion"""
    x = np.asarray(x)
    T = x.dtype.type
    nan, lo, hi = np.isnan(x), x < -700, x > 700
    s = np.where(nan | lo | hi, T(0.0), x)
    n = np.floor(s * T(LOG2E) + T(0.5))
    r = (s - n * T(LN2_HI)) - n * T(LN2_LO)
    p = T(1.0) / T(math.factorial(degree)) + 0 * r
    for k in range(degree - 1, -1, -1):
        p = p * r + T(1.0) / T(math.factorial(k))
    y = np.ldexp(p, n.astype(np.int64))
    y = np.where(lo, T(0.0), y)
    y = np.where(hi, T(np.inf), y)
    return np.where(nan, x, y)


def scalar_exp_c(x):
    if x != x:
        return x
    if x < -700.0:
        return 0.0
    if x > 700.0:
        return math.inf
    n = math.floor(x * LOG2E + 0.5)
    r = (x - n * LN2_HI) - n * LN2_LO
    p = 1.0 / math.factorial(13)
    for k in range(12, -1, -1):
        p = p * r + 1.0 / math.factorial(k)
    return math.ldexp(p, n)


def latent_heat(temp):
    T = temp.dtype.type
    tc = temp - T(273.15)
    return (T(2500.8) - T(2.36) * tc + T(0.0016) * tc * tc - T(0.00006) * tc * tc * tc) * T(1000.0)


def saturation_ratio(temp, rho, R_v, mutant=None):
    """qs = (es / (R_v temp)) / rho, es = 610.94 exp_c((17.625 tc) / (243.04 + tc))"""
    T = temp.dtype.type
    tc = temp - T(273.15)
    es = T(610.94) * exp_c((T(17.625) * tc) / (T(243.04) + tc), 12 if mutant == "exp_degree_12" else 13)
    a = es / (R_v * temp)
    return a if mutant == "qs_without_rho" else a / rho


# ---- 2. the coefficients

def thermo(case, F, mutant=None):
    """-> trho, qt, c (None without a cloud table), rho of every cell"""
    T = F["temp"].dtype.type
    rho = F["density_dry"] + F["water_vapor"]
    qv = F["water_vapor"] / rho
    c = None
    for n in case["cloud"]:
        c = F[n] if c is None else c + F[n]
    load = c
    for n in case["precip"]:
        load = F[n] if load is None else load + F[n]
    f = T(1.0) + T(0.608) * qv
    qt = qv
    if load is not None:
        ql = load / rho
        if mutant != "loading_dropped":
            f = f - ql
        qt = qv + ql
    return F["temp"] * f, qt, c, rho


def stability(case, mutant=None, dtype=np.float64):
    """-> N2 as the coefficients use it, the unsaturated N2, the saturated N2 (None without a cloud table), sat (likewise)"""
    T = dtype
    F = {n: np.asarray(a, dtype=dtype) for n, a in case["fields"].items()}
    zmid = np.asarray(case["zmid"], dtype=dtype)
    grav, cp_d, R_d, R_v, thr = (T(case[n]) for n in ("grav", "cp_d", "R_d", "R_v", "cloud_threshold"))
    gc, eps = grav / cp_d, R_d / R_v
    temp = F["temp"]
    nz = temp.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        trho, qt, c, rho = thermo(case, F, mutant)
        unsat = (grav / trho) * (ref._ddz(trho, zmid) + gc)
        if c is None:
            return unsat, unsat, None, None
        cs = F[case["cloud"][0]] if mutant == "second_cloud_ignored_in_sat" else c
        sat = cs >= thr * rho if mutant == "branch_ge" else cs > thr * rho
        qs = saturation_ratio(temp, rho, R_v, mutant)
        lv = latent_heat(temp)
        a1 = T(1.0) + (lv * qs) / (R_d * temp)
        a2 = T(1.0) + (((eps * lv) * lv) * qs) / (((cp_d * R_d) * temp) * temp)
        b = (ref._ddz(temp, zmid) + gc) / temp + (lv / (cp_d * temp)) * ref._ddz(qs, zmid)
        m = (a1 / a2) * b
        satn2 = grav * m if mutant == "dqt_dropped" else grav * (m - ref._ddz(qt, zmid))
        pick = sat[np.minimum(np.arange(nz) + 1, nz - 1)] if mutant == "branch_on_upper_neighbour" else sat
        return np.where(pick, satn2, unsat), unsat, satn2, sat


def deformation(case, dtype=np.float64):
    """Def2, exactly as sgs_ref.coefficients forms it"""
    T = dtype
    u, v, w = (np.asarray(case["fields"][n], dtype=dtype) for n in WINDS)
    zmid = np.asarray(case["zmid"], dtype=dtype)
    two_dx, two_dy = T(2.0) * T(case["dx"]), T(2.0) * T(case["dy"])
    with_y = u.shape[1] > 1
    ux, vx, wx = (ref._ddh(f, 2, two_dx) for f in (u, v, w))
    uz, vz, wz = (ref._ddz(f, zmid) for f in (u, v, w))
    a = ux * ux
    if with_y:
        uy, vy, wy = (ref._ddh(f, 1, two_dy) for f in (u, v, w))
        a = a + vy * vy
    a = a + wz * wz
    d = T(2.0) * a
    s = uy + vx if with_y else vx
    d = d + s * s
    s = uz + wx
    d = d + s * s
    s = vz + wy if with_y else vz
    return d + s * s


def coefficients(case, mutant=None, dtype=np.float64, with_arg=False):
    """-> tk, tkh (and arg = Def2 - N2 / prandtl with with_arg)"""
    T = dtype
    zint = np.asarray(case["zint"], dtype=dtype)
    cs, pr = T(case["cs"]), T(case["prandtl"])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = deformation(case, dtype)
        n2 = stability(case, mutant, dtype)[0]
        l = cs * (zint[1:] - zint[:-1])
        l2 = (l * l)[:, None, None, :]
        arg = d - n2 / pr
        tk = l2 * np.sqrt(np.where(arg < 0, T(0.0), arg))
        tkh = tk / pr
    return (tk, tkh, arg) if with_arg else (tk, tkh)


# ---- 3. the solve

def diffuse(case, tk, tkh, mutant=None, dtype=np.float64):
    """sgs_ref.diffuse with row 0 of temp and of the vapour taking the surface fluxes of heat and vapour"""
    T = dtype
    F = {n: np.asarray(a, dtype=dtype) for n, a in case["fields"].items()}
    zint, zmid = np.asarray(case["zint"], dtype=dtype), np.asarray(case["zmid"], dtype=dtype)
    tk, tkh = np.asarray(tk, dtype=dtype), np.asarray(tkh, dtype=dtype)
    dt, cp_d, latvap = T(case["dt"]), T(case["cp_d"]), T(case["latvap"])
    gc = T(case["grav"]) / cp_d
    shf, lhf = (None if case.get(n) is None else np.asarray(case[n], dtype=dtype) for n in ("sfc_shf", "sfc_lhf"))
    assert lhf is None or "water_vapor" in case["tracers"]
    row = -1 if mutant == "flux_at_top" else 0
    out = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rho = F["density_dry"] + F["water_vapor"]
        lower, diag, upper, dzf_m, dzf_p, dz = ref.rows("momentum", rho, tk, zint, zmid, dt)
        for n, sfc in zip(WINDS, (case.get("sfc_flx_u"), case.get("sfc_flx_v"), None)):
            r = F[n].copy()
            if sfc is not None:
                r[0] = r[0] + (dt * np.asarray(sfc, dtype=dtype)) / dz[0]
            out[n] = ref.thomas(lower, diag, upper, r)
        lower, diag, upper, dzf_m, dzf_p, dz = ref.rows("heat", rho, tkh, zint, zmid, dt)
        r = F["temp"] + gc * (upper * dzf_p - lower * dzf_m)
        if shf is not None:
            s = shf / cp_d if mutant == "shf_without_rho" else shf / (cp_d * rho[0])
            r[row] = r[row] + (dt * s) / dz[row]
        out["temp"] = ref.thomas(lower, diag, upper, r)
        if case["tracers"]:
            lower, diag, upper, dzf_m, dzf_p, dz = ref.rows("tracer", rho, tkh, zint, zmid, dt)
            for n in case["tracers"]:
                r = F[n]
                if n == "water_vapor" and lhf is not None:
                    r = r.copy()
                    s = (lhf / latvap) / rho[0] if mutant == "lhf_divided_by_rho" else lhf / latvap
                    r[row] = r[row] + (dt * s) / dz[row]
                out[n] = ref.thomas(lower, diag, upper, r)
    return out


# ---- the scalar-loop twin: one cell, one (column, member) at a time in Python floats

_div = ref._div


def _scalar_cell(case, k, j, i, e):
    """-> trho, temp, qs, qt, sat of one cell"""
    F = case["fields"]
    at = lambda n: float(F[n][k, j, i, e])
    temp, rho = at("temp"), at("density_dry") + at("water_vapor")
    qv = _div(at("water_vapor"), rho)
    c = load = None
    for n in case["cloud"]:
        c = at(n) if c is None else c + at(n)
    load = c
    for n in case["precip"]:
        load = at(n) if load is None else load + at(n)
    f, qt = 1.0 + 0.608 * qv, qv
    if load is not None:
        ql = _div(load, rho)
        f, qt = f - ql, qv + ql
    sat, qs = False, 0.0
    if c is not None:
        sat = c > case["cloud_threshold"] * rho
        tc = temp - 273.15
        es = 610.94 * scalar_exp_c(_div(17.625 * tc, 243.04 + tc))
        qs = _div(_div(es, case["R_v"] * temp), rho)
    return temp * f, temp, qs, qt, sat


def scalar_coefficients(case):
    F = case["fields"]
    nz, ny, nx, nens = F["temp"].shape
    zint, zmid = case["zint"], case["zmid"]
    grav, cp_d, R_d, pr = case["grav"], case["cp_d"], case["R_d"], case["prandtl"]
    gc, eps = grav / cp_d, R_d / case["R_v"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = deformation(case)                      # Def2 is sgs_ref's, and sgs_ref's own twin covers it
    tk, tkh = np.zeros(F["temp"].shape), np.zeros(F["temp"].shape)
    for j in range(ny):
        for i in range(nx):
            for e in range(nens):
                cells = [_scalar_cell(case, k, j, i, e) for k in range(nz)]
                for k in range(nz):
                    ku, kd = min(k + 1, nz - 1), max(k - 1, 0)
                    span = float(zmid[ku, e]) - float(zmid[kd, e])
                    dd = [_div(cells[ku][q] - cells[kd][q], span) for q in range(4)]
                    trho, temp, qs, qt, sat = cells[k]
                    if sat:
                        tc = temp - 273.15
                        lv = (2500.8 - 2.36 * tc + 0.0016 * tc * tc - 0.00006 * tc * tc * tc) * 1000.0
                        a1 = 1.0 + _div(lv * qs, R_d * temp)
                        a2 = 1.0 + _div(((eps * lv) * lv) * qs, ((cp_d * R_d) * temp) * temp)
                        b = _div(dd[1] + gc, temp) + _div(lv, cp_d * temp) * dd[2]
                        n2 = grav * (_div(a1, a2) * b - dd[3])
                    else:
                        n2 = _div(grav, trho) * (dd[0] + gc)
                    l = case["cs"] * (float(zint[k + 1, e]) - float(zint[k, e]))
                    arg = float(d[k, j, i, e]) - n2 / pr
                    m = 0.0 if arg < 0 else arg
                    tk[k, j, i, e] = (l * l) * float(np.sqrt(np.float64(m)))
                    tkh[k, j, i, e] = tk[k, j, i, e] / pr
    return tk, tkh


def scalar_diffuse(case, tk, tkh):
    """sgs_ref's column solve, handed the flux as the row takes it: shf / (cp_d rho(0)) for temp, lhf / latvap for the vapour"""
    F = case["fields"]
    nz, ny, nx, nens = F["temp"].shape
    dt, gc = case["dt"], case["grav"] / case["cp_d"]
    out = {n: np.zeros(F["temp"].shape) for n in WINDS + ("temp",) + tuple(case["tracers"])}
    for j in range(ny):
        for i in range(nx):
            for e in range(nens):
                col = (slice(None), j, i, e)
                rho = [float(a) + float(b) for a, b in zip(F["density_dry"][col], F["water_vapor"][col])]
                zi, zm = case["zint"][:, e].tolist(), case["zmid"][:, e].tolist()
                for n, sfc in zip(WINDS, (case.get("sfc_flx_u"), case.get("sfc_flx_v"), None)):
                    s = None if sfc is None else float(sfc[j, i, e])
                    out[n][col] = ref._scalar_column_solve("momentum", rho, tk[col].tolist(), zi, zm, dt, gc, F[n][col].tolist(), s)
                s = None if case.get("sfc_shf") is None else _div(float(case["sfc_shf"][j, i, e]), case["cp_d"] * rho[0])
                out["temp"][col] = ref._scalar_column_solve("heat", rho, tkh[col].tolist(), zi, zm, dt, gc, F["temp"][col].tolist(), s)
                for n in case["tracers"]:
                    s = None
                    if n == "water_vapor" and case.get("sfc_lhf") is not None:
                        s = float(case["sfc_lhf"][j, i, e]) / case["latvap"]
                    out[n][col] = ref._scalar_column_solve("tracer", rho, tkh[col].tolist(), zi, zm, dt, gc, F[n][col].tolist(), s)
    return out


# ---- backends: .coefficients(case) -> tk, tkh; .diffuse(case, tk, tkh) -> name -> field

class RefBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def coefficients(self, case):
        return coefficients(case, self.mutant)

    def diffuse(self, case, tk, tkh):
        return diffuse(case, tk, tkh, self.mutant)


class ScalarBackend:
    def coefficients(self, case):
        return scalar_coefficients(case)

    def diffuse(self, case, tk, tkh):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            return scalar_diffuse(case, tk, tkh)


def run_case(backend, case):
    """-> dict: tk, tkh of the moist coefficient call, and the fields of the flux solve on the restatement's coefficients (so a backend's
    solve is judged on the same coefficients whatever its own coefficient call gave)"""
    tk, tkh = backend.coefficients(case)
    out = dict(backend.diffuse(case, *coefficients(case)))
    out["tk"], out["tkh"] = tk, tkh
    return out


def members(case, idx):
    """the case on a selection of members (members are independent)"""
    sub = dict(case, fields={n: np.ascontiguousarray(a[..., idx]) for n, a in case["fields"].items()},
               zint=np.ascontiguousarray(case["zint"][:, idx]), zmid=np.ascontiguousarray(case["zmid"][:, idx]))
    for n in ("sfc_flx_u", "sfc_flx_v", "sfc_shf", "sfc_lhf"):
        if case.get(n) is not None:
            sub[n] = np.ascontiguousarray(case[n][..., idx])
    return sub


# ---- the named cases
CASE_NAMES = ("kessler_set", "p3_set", "cloud_only", "precip_only", "empty_tables", "threshold_positive", "nan_cell", "fluxes_both", "shf_only",
              "lhf_only", "vapour_last_with_lhf", "downward_lhf")
CONDENSATE = ("cloud_liquid", "precip_liquid", "cloud_water", "ice", "rain")
EXTRA = ("tracer_a", "tracer_b", "tracer_c")
THRESHOLD = 1.0e-4
_CACHE, _REF = {}, {}


def cases(shape):
    """name -> case, built once per shape and shared (nobody writes to them).  Temperatures run from 303, 290 or 278 K at the ground (by member) to about
    195 K at the top, through pairs of unstable and of stable layers, so that either branch has levels it mixes and levels it does not; every cloud species is exactly zero in about half of the cells,
    cell by cell at random, so cloudy and clear cells are neighbours in all three directions; (0, 0, 0, 0) and (nz-1, ny-1, nx-1, nens-1)
    are cloudy in every species"""
    if shape in _CACHE:
        return _CACHE[shape]
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(9000000 + 100000 * nz + 1000 * ny + 10 * nx + nens)
    zint, zmid = ref.grid(nz, nens)
    z = zmid[:, None, None, :] + np.zeros(shape)
    j = np.arange(ny)[None, :, None, None]
    i = np.arange(nx)[None, None, :, None]
    e = np.arange(nens)[None, None, None, :]
    wave = np.sin(2 * np.pi * i / nx + 0.3 * e) * np.cos(2 * np.pi * j / ny + 0.7) + np.zeros(shape)
    gc = ref.GRAV / ref.CP_D
    gamma = np.array([1.35 * gc, 1.35 * gc, 0.001, 0.001])[np.arange(nz) % 4]      # the layer below level k: unstable and stable in pairs
    temp = np.empty(shape)
    temp[0] = 303.0 - 12.5 * (e[0] % 3)
    for k in range(1, nz):
        temp[k] = temp[k - 1] - gamma[k] * (z[k] - z[k - 1])
    temp = temp + 1.0e-3 * rng.normal(0.0, 1.0, shape)
    fields = dict(uvel=10.0 * z / 12000.0 + 2.0 * wave + 0.1 * rng.normal(0.0, 1.0, shape),
                  vvel=-3.0 * np.sqrt(z / 12000.0) + wave + 0.1 * rng.normal(0.0, 1.0, shape),
                  wvel=0.5 * wave * np.sin(np.pi * z / 12000.0) + 0.01 * rng.normal(0.0, 1.0, shape),
                  temp=temp, density_dry=1.2 * np.exp(-z / 8000.0) * rng.uniform(0.99, 1.01, shape),
                  water_vapor=0.012 * np.exp(-z / 2500.0) * (1.0 + 0.2 * wave) * rng.uniform(0.9, 1.1, shape))
    m = rng.uniform(0.0, 1.0, shape)                  # one draw places the cloud: the first species below 0.35, the second in 0.25 .. 0.5
    for n, lo, hi in (("cloud_liquid", 0.0, 0.5), ("cloud_water", 0.0, 0.35), ("ice", 0.25, 0.5)):
        fields[n] = np.where((m >= lo) & (m < hi), 1.0e-3 * np.exp(-z / 6000.0) * rng.uniform(0.02, 1.0, shape), 0.0)
        fields[n][0, 0, 0, 0] = fields[n][nz - 1, ny - 1, nx - 1, nens - 1] = 2.5e-4
    for n in ("precip_liquid", "rain") + EXTRA:
        fields[n] = np.where(rng.uniform(0.0, 1.0, shape) < 0.3, 0.0, 2.0e-3 * np.exp(-z / 5000.0) * rng.uniform(0.0, 1.0, shape))
    sfc_u = -0.05 * fields["uvel"][0] * rng.uniform(0.5, 1.5, shape[1:])
    sfc_v = -0.05 * fields["vvel"][0] * rng.uniform(0.5, 1.5, shape[1:])
    shf = 80.0 * rng.uniform(-0.25, 1.0, shape[1:])
    lhf = 300.0 * rng.uniform(0.0, 1.0, shape[1:])
    kessler, p3 = ("water_vapor", "cloud_liquid", "precip_liquid"), ("cloud_water", "ice", "rain", "water_vapor", "tracer_a")

    def case(tracers, cloud, precip, **kw):
        c = dict(fields=fields, tracers=tuple(tracers), cloud=tuple(cloud), precip=tuple(precip), zint=zint, zmid=zmid, dx=ref.DX, dy=ref.DY,
                 grav=ref.GRAV, cp_d=ref.CP_D, cs=ref.CS, prandtl=ref.PRANDTL, dt=ref.DT, R_d=R_D, R_v=R_V, latvap=LATVAP, cloud_threshold=0.0,
                 sfc_flx_u=sfc_u, sfc_flx_v=sfc_v, sfc_shf=None, sfc_lhf=None)
        c.update(kw)
        return c

    out = {"kessler_set": case(kessler, ("cloud_liquid",), ("precip_liquid",))}
    out["p3_set"] = case(p3, ("cloud_water", "ice"), ("rain",))
    out["cloud_only"] = case(kessler, ("cloud_liquid",), ())
    out["precip_only"] = case(kessler, (), ("precip_liquid",))
    out["empty_tables"] = case(kessler, (), ())
    # the threshold lies inside the range of the cloud, and one cell holds c == threshold rho exactly: unsaturated
    thr = {n: a.copy() for n, a in fields.items()}
    at = (0, ny // 2, nx // 2, nens // 3)              # at the ground, where neither branch is clamped, so the choice shows in tk
    thr["cloud_water"][at] = THRESHOLD * (thr["density_dry"][at] + thr["water_vapor"][at])
    thr["ice"][at] = 0.0
    out["threshold_positive"] = case(p3, ("cloud_water", "ice"), ("rain",), fields=thr, cloud_threshold=THRESHOLD)
    nan = {n: a.copy() for n, a in fields.items()}
    nan["temp"][nz // 2, ny // 2, nx // 2, nens // 2] = np.nan
    nan["cloud_liquid"][nz - 1, 0, 0, 0] = np.nan
    out["nan_cell"] = case(kessler, ("cloud_liquid",), ("precip_liquid",), fields=nan, sfc_shf=shf, sfc_lhf=lhf)
    out["fluxes_both"] = case(kessler, ("cloud_liquid",), ("precip_liquid",), sfc_shf=shf, sfc_lhf=lhf)
    out["shf_only"] = case(kessler, ("cloud_liquid",), ("precip_liquid",), sfc_shf=shf)
    out["lhf_only"] = case(p3, ("cloud_water", "ice"), ("rain",), sfc_lhf=lhf)
    # the vapour beyond the fields a thread keeps in registers, where the other loop of the solve adds the flux
    out["vapour_last_with_lhf"] = case(("cloud_water", "ice", "rain", "tracer_a", "tracer_b", "tracer_c", "water_vapor"), ("cloud_water", "ice"),
                                       ("rain",), sfc_shf=shf, sfc_lhf=lhf, sfc_flx_u=None, sfc_flx_v=None)
    # a downward flux of between half and twice the vapour the lowest level holds: the vapour goes negative in some columns
    dz0 = (zint[1] - zint[0])[None, None, :]
    down = -(fields["water_vapor"][0] * dz0 * LATVAP / ref.DT) * rng.uniform(0.5, 2.0, shape[1:])
    out["downward_lhf"] = case(kessler, ("cloud_liquid",), ("precip_liquid",), sfc_lhf=down)
    assert tuple(out) == CASE_NAMES
    _CACHE[shape] = out
    return out


def reference(shape, name):
    """the restatement's result of a named case, computed once and shared"""
    key = (shape, name)
    if key not in _REF:
        _REF[key] = run_case(RefBackend(), cases(shape)[name])
    return _REF[key]
