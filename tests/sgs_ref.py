"""The native Smagorinsky SGS closure: the numpy restatement of the contract (include/pam_amd_modules.h), its
scalar-loop twin, the named cases and the mutants of the restatement.  TEST INFRASTRUCTURE ONLY.

The method is not part of the reference tree, so this restatement is the yardstick, and the device bodies (pam_amd/csrc/sgs_device.h,
under g++ in tests/emu/sgs_emu.cpp and under hipcc in modules_kernels.hip) are held to it bit for bit.  numpy's element-wise float64
arithmetic is IEEE and never contracted; no numpy reduction takes part: the only sums are the recurrences over levels, written out as
loops.  Every function works in the dtype of its inputs, so the same restatement evaluated in np.longdouble measures the float64
restatement's own rounding error (tests/test_sgs_smag.py).

Fields are (nz, ny, nx, nens), members fastest; zint (nz+1, nens), zmid (nz, nens).  A mutant is a deliberately wrong variant of ONE
line of the restatement, switched on by name; each must be caught by at least one named case."""
import numpy as np

MUTANTS = ("face_swapped", "tracer_rho_k", "n2_no_lapse", "heat_no_lapse", "one_sided_wrong_place")
WINDS = ("uvel", "vvel", "wvel")
# both boundaries adjacent; nx of 1 and 2; ny of 1 and > 1; a partial wavefront, more than one wavefront, a whole one
SHAPES = ((2, 1, 1, 1), (3, 1, 2, 65), (5, 1, 4, 130), (7, 3, 5, 130), (6, 4, 3, 64))
GRAV, CP_D, DX, DY, CS, PRANDTL, DT = 9.80616, 1004.64, 500.0, 750.0, 0.2, 1.0 / 3.0, 10.0


def shape_id(shape):
    return "%dx%dx%d-e%d" % shape


# ---- 1. the coefficients

def _ddh(f, axis, two_d):
    return (np.roll(f, -1, axis=axis) - np.roll(f, 1, axis=axis)) / two_d


def _ddz(f, zmid, mutant=None):
    nz = f.shape[0]
    k = np.arange(nz)
    ku, kd = np.minimum(k + 1, nz - 1), np.maximum(k - 1, 0)
    if mutant == "one_sided_wrong_place":
        kd = np.where(k == 1, 1, kd)
    span = zmid[ku] - zmid[kd]
    return (f[ku] - f[kd]) / span[:, None, None, :]


def virtual_temp(temp, rho_d, rho_v):
    c = temp.dtype.type(0.608)
    rho = rho_d + rho_v
    return temp * (1.0 + c * (rho_v / rho))


def coefficients(case, mutant=None, dtype=np.float64):
    """-> tk, tkh"""
    F = {n: np.asarray(a, dtype=dtype) for n, a in case["fields"].items()}
    zint, zmid = np.asarray(case["zint"], dtype=dtype), np.asarray(case["zmid"], dtype=dtype)
    T = dtype
    grav, cp_d, cs, pr = T(case["grav"]), T(case["cp_d"]), T(case["cs"]), T(case["prandtl"])
    two_dx, two_dy = T(2.0) * T(case["dx"]), T(2.0) * T(case["dy"])
    u, v, w = (F[n] for n in WINDS)
    with_y = u.shape[1] > 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ux, vx, wx = (_ddh(f, 2, two_dx) for f in (u, v, w))
        uz, vz, wz = (_ddz(f, zmid, mutant) for f in (u, v, w))
        a = ux * ux
        if with_y:
            uy, vy, wy = (_ddh(f, 1, two_dy) for f in (u, v, w))
            a = a + vy * vy
        a = a + wz * wz
        d = T(2.0) * a
        s = uy + vx if with_y else vx
        d = d + s * s
        s = uz + wx
        d = d + s * s
        s = vz + wy if with_y else vz
        d = d + s * s
        tv = virtual_temp(F["temp"], F["density_dry"], F["water_vapor"])
        gc = grav / cp_d
        b = _ddz(tv, zmid, mutant)
        if mutant != "n2_no_lapse":
            b = b + gc
        n2 = (grav / tv) * b
        dz = zint[1:] - zint[:-1]
        l = cs * dz
        l2 = (l * l)[:, None, None, :]
        arg = d - n2 / pr
        m = np.where(arg < 0, T(0.0), arg)
        tk = l2 * np.sqrt(m)
        tkh = tk / pr
    return tk, tkh


# ---- 2. the solve

def thomas(lower, diag, upper, r):
    """-lower x(k-1) + diag x(k) - upper x(k+1) = r along axis 0; lower[0] and upper[-1] are 0.0"""
    nz = r.shape[0]
    cp = np.zeros_like(r)
    x = np.zeros_like(r)
    cprev = np.zeros_like(r[0])
    dprev = np.zeros_like(r[0])
    for k in range(nz):
        den = diag[k] - lower[k] * cprev
        cp[k] = upper[k] / den
        x[k] = (r[k] + lower[k] * dprev) / den
        cprev, dprev = cp[k], x[k]
    for k in range(nz - 2, -1, -1):
        x[k] = x[k] + cp[k] * x[k + 1]
    return x


def rows(cls, rho, K, zint, zmid, dt, mutant=None):
    """-> lower, diag, upper, dzf_below, dzf_above of one class, (nz, ny, nx, nens) each (dzf: (nz, 1, 1, nens))"""
    T = rho.dtype.type
    nz = rho.shape[0]
    dz = (zint[1:] - zint[:-1])[:, None, None, :]
    dzf = (zmid[1:] - zmid[:-1])[:, None, None, :]
    half = T(0.5)
    g = ((dt * (half * (rho[:-1] + rho[1:]))) * (half * (K[:-1] + K[1:]))) / dzf          # faces 1/2 .. nz - 3/2
    zero = np.zeros_like(rho[:1])
    g_m, g_p = np.concatenate([zero, g]), np.concatenate([g, zero])
    if mutant == "face_swapped":
        g_m, g_p = g_p, g_m
    rdz = rho * dz
    diag = T(1.0) + (g_m + g_p) / rdz
    if cls == "tracer" and mutant != "tracer_rho_k":
        rho_m, rho_p = np.concatenate([rho[:1], rho[:-1]]), np.concatenate([rho[1:], rho[-1:]])
        lower, upper = g_m / (rho_m * dz), g_p / (rho_p * dz)
    else:
        lower, upper = g_m / rdz, g_p / rdz
    lower[0] = 0.0
    upper[nz - 1] = 0.0
    z1 = np.zeros_like(dzf[:1])
    return lower, diag, upper, np.concatenate([z1, dzf]), np.concatenate([dzf, z1]), dz


def diffuse(case, tk, tkh, mutant=None, dtype=np.float64):
    """-> name -> new field, for the winds, temp and every tracer"""
    T = dtype
    F = {n: np.asarray(a, dtype=dtype) for n, a in case["fields"].items()}
    zint, zmid = np.asarray(case["zint"], dtype=dtype), np.asarray(case["zmid"], dtype=dtype)
    tk, tkh = np.asarray(tk, dtype=dtype), np.asarray(tkh, dtype=dtype)
    dt, gc = T(case["dt"]), T(case["grav"]) / T(case["cp_d"])
    out = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rho = F["density_dry"] + F["water_vapor"]
        lower, diag, upper, dzf_m, dzf_p, dz = rows("momentum", rho, tk, zint, zmid, dt, mutant)
        for n, sfc in zip(WINDS, (case.get("sfc_flx_u"), case.get("sfc_flx_v"), None)):
            r = F[n].copy()
            if sfc is not None:
                r[0] = r[0] + (dt * np.asarray(sfc, dtype=dtype)) / dz[0]
            out[n] = thomas(lower, diag, upper, r)
        lower, diag, upper, dzf_m, dzf_p, dz = rows("heat", rho, tkh, zint, zmid, dt, mutant)
        r = F["temp"]
        if mutant != "heat_no_lapse":
            r = r + gc * (upper * dzf_p - lower * dzf_m)
        out["temp"] = thomas(lower, diag, upper, r)
        if case["tracers"]:
            lower, diag, upper, dzf_m, dzf_p, dz = rows("tracer", rho, tkh, zint, zmid, dt, mutant)
            for n in case["tracers"]:
                out[n] = thomas(lower, diag, upper, F[n])
    return out


# ---- the scalar-loop twin: one (column, member) at a time in Python floats (IEEE doubles, never contracted)

def _scalar_column_solve(cls, rho, K, zint, zmid, dt, gc, f, sfc):
    nz = len(rho)
    x, cp = [0.0] * nz, [0.0] * nz
    cprev = dprev = 0.0
    for k in range(nz):
        first, last = k == 0, k == nz - 1
        dz = zint[k + 1] - zint[k]
        dzf_m = 0.0 if first else zmid[k] - zmid[k - 1]
        dzf_p = 0.0 if last else zmid[k + 1] - zmid[k]
        g_m = 0.0 if first else ((dt * (0.5 * (rho[k - 1] + rho[k]))) * (0.5 * (K[k - 1] + K[k]))) / dzf_m
        g_p = 0.0 if last else ((dt * (0.5 * (rho[k] + rho[k + 1]))) * (0.5 * (K[k] + K[k + 1]))) / dzf_p
        rdz = rho[k] * dz
        diag = 1.0 + (g_m + g_p) / rdz
        if cls == "tracer":
            lower = 0.0 if first else g_m / (rho[k - 1] * dz)
            upper = 0.0 if last else g_p / (rho[k + 1] * dz)
        else:
            lower = 0.0 if first else g_m / rdz
            upper = 0.0 if last else g_p / rdz
        r = f[k]
        if cls == "heat":
            r = r + gc * (upper * dzf_p - lower * dzf_m)
        if first and sfc is not None:
            r = r + (dt * sfc) / dz
        den = diag - lower * cprev
        cp[k] = upper / den
        x[k] = (r + lower * dprev) / den
        cprev, dprev = cp[k], x[k]
    for k in range(nz - 2, -1, -1):
        x[k] = x[k] + cp[k] * x[k + 1]
    return x


def _div(a, b):
    """IEEE division of two Python floats (Python raises where IEEE gives an infinity or a NaN)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return float(np.float64(a) / np.float64(b))


def scalar_coefficients(case):
    F = case["fields"]
    u, v, w, temp, rd, rv = (F[n] for n in WINDS + ("temp", "density_dry", "water_vapor"))
    nz, ny, nx, nens = u.shape
    zint, zmid = case["zint"], case["zmid"]
    grav, cs, pr = case["grav"], case["cs"], case["prandtl"]
    gc, two_dx, two_dy = grav / case["cp_d"], 2.0 * case["dx"], 2.0 * case["dy"]
    tk, tkh = np.zeros(u.shape), np.zeros(u.shape)

    def tv(k, j, i, e):
        d, q = float(rd[k, j, i, e]), float(rv[k, j, i, e])
        return float(temp[k, j, i, e]) * (1.0 + 0.608 * _div(q, d + q))

    for k in range(nz):
        ku, kd = min(k + 1, nz - 1), max(k - 1, 0)
        for j in range(ny):
            jp, jm = (j + 1) % ny, (j - 1) % ny
            for i in range(nx):
                ip, im = (i + 1) % nx, (i - 1) % nx
                for e in range(nens):
                    span = float(zmid[ku, e]) - float(zmid[kd, e])
                    dx_ = [(float(f[k, j, ip, e]) - float(f[k, j, im, e])) / two_dx for f in (u, v, w)]
                    dz_ = [_div(float(f[ku, j, i, e]) - float(f[kd, j, i, e]), span) for f in (u, v, w)]
                    a = dx_[0] * dx_[0]
                    if ny > 1:
                        dy_ = [(float(f[k, jp, i, e]) - float(f[k, jm, i, e])) / two_dy for f in (u, v, w)]
                        a = a + dy_[1] * dy_[1]
                    a = a + dz_[2] * dz_[2]
                    d = 2.0 * a
                    s = dy_[0] + dx_[1] if ny > 1 else dx_[1]
                    d = d + s * s
                    s = dz_[0] + dx_[2]
                    d = d + s * s
                    s = dz_[1] + dy_[2] if ny > 1 else dz_[1]
                    d = d + s * s
                    n2 = _div(grav, tv(k, j, i, e)) * (_div(tv(ku, j, i, e) - tv(kd, j, i, e), span) + gc)
                    l = cs * (float(zint[k + 1, e]) - float(zint[k, e]))
                    arg = d - n2 / pr
                    m = 0.0 if arg < 0 else arg
                    tk[k, j, i, e] = (l * l) * float(np.sqrt(np.float64(m)))
                    tkh[k, j, i, e] = tk[k, j, i, e] / pr
    return tk, tkh


def scalar_diffuse(case, tk, tkh):
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
                    out[n][col] = _scalar_column_solve("momentum", rho, tk[col].tolist(), zi, zm, dt, gc, F[n][col].tolist(), s)
                out["temp"][col] = _scalar_column_solve("heat", rho, tkh[col].tolist(), zi, zm, dt, gc, F["temp"][col].tolist(), None)
                for n in case["tracers"]:
                    out[n][col] = _scalar_column_solve("tracer", rho, tkh[col].tolist(), zi, zm, dt, gc, F[n][col].tolist(), None)
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
    """-> dict: tk, tkh of the coefficient call, and the fields of the diffuse call on the case's hand-set tk / tkh where it has them and
    on the restatement's otherwise (so a backend's solve is judged on the same coefficients whatever its own coefficient call gave)"""
    tk, tkh = backend.coefficients(case)
    if "tk" in case:
        k1, k2 = case["tk"], case["tkh"]
    else:
        k1, k2 = coefficients(case)
    out = dict(backend.diffuse(case, k1, k2))
    out["tk"], out["tkh"] = tk, tkh
    return out


def same_bits(a, b, nan_by_place=False):
    """the same bits in every cell; nan_by_place (a comparison across hardware only): a NaN where a NaN stands, sign and payload not
    compared, as in hd_ref.same_bits"""
    if a.shape != b.shape:
        return False
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if not nan_by_place:
        return np.array_equal(a.view(np.uint64), b.view(np.uint64))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def results_differ(x, y, nan_by_place=False):
    """names of the arrays that differ bitwise between two results"""
    assert set(x) == set(y), (sorted(x), sorted(y))
    return sorted(n for n in x if not same_bits(x[n], y[n], nan_by_place))


# ---- the named cases
CASE_NAMES = ("base", "vapour_middle", "vapour_last", "no_surface_flux", "no_tracers", "zero_k_faces", "nan_cell")
EXTRA = ("cloud_water", "rain", "tracer_a", "tracer_b", "tracer_c")
_CACHE, _REF = {}, {}


def grid(nz, nens, per_member=True):
    """stretched interfaces up to 12 km, every member's column scaled a little differently"""
    s = (np.arange(nz + 1) / nz) ** 1.5 * 12000.0
    scale = 1.0 + (0.02 * (np.arange(nens) % 5) if per_member else np.zeros(nens))
    zint = s[:, None] * scale[None, :]
    return zint, 0.5 * (zint[:-1] + zint[1:])


def cases(shape):
    """name -> case, built once per shape and shared (nobody writes to them: every backend copies what it changes)"""
    if shape in _CACHE:
        return _CACHE[shape]
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(7000000 + 100000 * nz + 1000 * ny + 10 * nx + nens)
    zint, zmid = grid(nz, nens)
    z = zmid[:, None, None, :] + np.zeros(shape)
    j = np.arange(ny)[None, :, None, None]
    i = np.arange(nx)[None, None, :, None]
    e = np.arange(nens)[None, None, None, :]
    wave = np.sin(2 * np.pi * i / nx + 0.3 * e) * np.cos(2 * np.pi * j / ny + 0.7) + np.zeros(shape)
    # lapse rates by level: unstable, unstable, neutral, stable in turn, so one column holds all three (and level 1 is never calm)
    gc = GRAV / CP_D
    gamma = np.array([1.5 * gc, 1.5 * gc, gc, 0.003])[np.arange(nz) % 4]
    temp = np.empty(shape)
    temp[0] = 300.0
    for k in range(1, nz):
        temp[k] = temp[k - 1] - gamma[k] * (z[k] - z[k - 1])
    temp = temp + 1.0e-3 * rng.normal(0.0, 1.0, shape)
    fields = dict(uvel=10.0 * z / 12000.0 + 2.0 * wave + 0.1 * rng.normal(0.0, 1.0, shape),
                  vvel=-3.0 * np.sqrt(z / 12000.0) + wave + 0.1 * rng.normal(0.0, 1.0, shape),
                  wvel=0.5 * wave * np.sin(np.pi * z / 12000.0) + 0.01 * rng.normal(0.0, 1.0, shape),
                  temp=temp, density_dry=1.2 * np.exp(-z / 8000.0) * rng.uniform(0.99, 1.01, shape),
                  water_vapor=0.012 * np.exp(-z / 2500.0) * (1.0 + 0.2 * wave) * rng.uniform(0.9, 1.1, shape))
    for n in EXTRA:
        blob = 1.0e-3 * np.exp(-((z - rng.uniform(1000.0, 9000.0)) / 2500.0) ** 2) * rng.uniform(0.0, 1.0, shape)
        fields[n] = np.where(rng.uniform(0.0, 1.0, shape) < 0.3, 0.0, blob)
    sfc_u = -0.05 * fields["uvel"][0] * rng.uniform(0.5, 1.5, shape[1:])
    sfc_v = -0.05 * fields["vvel"][0] * rng.uniform(0.5, 1.5, shape[1:])

    def case(tracers, **kw):
        c = dict(fields=fields, tracers=tuple(tracers), zint=zint, zmid=zmid, dx=DX, dy=DY, grav=GRAV, cp_d=CP_D, cs=CS, prandtl=PRANDTL,
                 dt=DT, sfc_flx_u=sfc_u, sfc_flx_v=sfc_v)
        c.update(kw)
        return c

    out = {"base": case(("water_vapor", "cloud_water", "rain"))}
    out["vapour_middle"] = case(("cloud_water", "rain", "water_vapor", "tracer_a", "tracer_b", "tracer_c"))
    out["vapour_last"] = case(("cloud_water", "rain", "tracer_a", "tracer_b", "tracer_c", "water_vapor"))
    out["no_surface_flux"] = case(("water_vapor", "cloud_water", "rain"), sfc_flx_u=None, sfc_flx_v=None)
    out["no_tracers"] = case(())
    # hand-set coefficients: three zero levels at the ground, so level 1 (level 0 at nz == 2) lies between two zero-K faces
    tk = 50.0 * rng.uniform(0.0, 1.0, shape)
    tk[: min(3, nz)] = 0.0
    out["zero_k_faces"] = case(("water_vapor", "cloud_water", "rain", "tracer_a", "tracer_b"), tk=tk, tkh=tk / PRANDTL)
    nan = {n: a.copy() for n, a in fields.items()}
    nan["temp"][nz // 2, ny // 2, nx // 2, nens // 2] = np.nan
    nan["rain"][nz - 1, 0, 0, 0] = np.nan
    out["nan_cell"] = case(("water_vapor", "cloud_water", "rain"), fields=nan)
    assert tuple(out) == CASE_NAMES
    _CACHE[shape] = out
    return out


def reference(shape, name):
    """the restatement's result of a named case, computed once and shared"""
    key = (shape, name)
    if key not in _REF:
        _REF[key] = run_case(RefBackend(), cases(shape)[name])
    return _REF[key]
