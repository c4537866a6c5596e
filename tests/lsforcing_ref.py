"""Large-scale forcing (subsidence, uniform tendencies, nudging of the level means, Coriolis): the numpy restatement of the contract
(include/pam_amd_modules.h at pam_amd_ls_forcing), operation for operation.  TEST INFRASTRUCTURE ONLY.

numpy's element-wise float64 arithmetic is IEEE and never contracted and no numpy reduction takes part (the level means are
msa_ref.level_mean, a loop over the cells in the slot order), so the device bodies are held to this file bit for bit.  Both upwind
branches are evaluated through one selection per element, which gives an element the same bits whatever its neighbours are.

A case is a dict:
  fields    uvel, vvel, temp, density_dry and every tracer, (nz,ny,nx,nens); the vapour is the tracer "water_vapor"
  tracers   the names of the tracer table, in its order; positive: their flags
  zmid      (nz,nens)
  wsub, temp_tend, qv_tend, ug, vg   (nz,nens) or None;  fcor (nens) or None
  target, rate   dicts over QUANTITIES of (nz,nens) arrays or None (rate["u"] is rate["v"]: one profile serves both winds)
  dt, grav, cp_d"""
import numpy as np

import msa_ref
from sgs_ref import same_bits, results_differ      # noqa: F401

QUANTITIES = ("t", "q", "u", "v")
STATE = ("uvel", "vvel", "temp")
PROFILES = ("wsub", "temp_tend", "qv_tend", "ug", "vg")
VAPOUR = "water_vapor"
MUTANTS = ("downwind", "wrong_dz_upper", "temp_without_adiabat", "nudge_cells", "euler_coriolis", "clamp_unflagged")


def shape_id(shape):
    return "%dx%dx%d-e%d" % shape


def level_mean(f):
    """M(f)(k,e) of a (nz,ny,nx,nens) field, in MSA's slot order"""
    nz, ny, nx, nens = f.shape
    return msa_ref.level_mean(f.reshape(nz, ny * nx, nens))


def nudged_quantity(F, x):
    if x == "t":
        return F["temp"]
    if x == "u":
        return F["uvel"]
    if x == "v":
        return F["vvel"]
    return F[VAPOUR] / (F["density_dry"] + F[VAPOUR])


def nudging(case, mutant=None):
    """-> {x: inc_x (nz,nens), or None where the target is absent}.  mutant nudge_cells: (nz,ny,nx,nens), every cell towards the target"""
    F, dt = case["fields"], np.float64(case["dt"])
    out = {}
    with np.errstate(all="ignore"):
        for x in QUANTITIES:
            tgt = (case.get("target") or {}).get(x)
            if tgt is None:
                out[x] = None
                continue
            rate = case["rate"][x]
            if mutant == "nudge_cells":
                out[x] = (dt * rate)[:, None, None, :] * (tgt[:, None, None, :] - nudged_quantity(F, x))
            else:
                out[x] = (dt * rate) * (tgt - level_mean(nudged_quantity(F, x)))
    return out


def _col(p):
    """a (nz,nens) profile or increment against the fields (an increment of the nudge_cells mutant is a field already)"""
    return p if p.ndim == 4 else p[:, None, None, :]


def subsidence(g, w, zmid, dt, mutant=None):
    """-> dg, active: the upwind increment of g (nz,ny,nx,nens) and where the term exists (nz,1,1,nens)"""
    nz = g.shape[0]
    W, Z = _col(w), _col(zmid)
    below = lambda a: np.concatenate([a[:1], a[:-1]])
    above = lambda a: np.concatenate([a[1:], a[-1:]])
    from_below = W > 0.0
    side = (W < 0.0) if mutant == "downwind" else from_below          # whose difference is taken
    d = np.where(side, g - below(g), above(g) - g)
    dz_up = (Z - below(Z)) if mutant == "wrong_dz_upper" else (above(Z) - Z)
    dz = np.where(side, Z - below(Z), dz_up)
    adv = (W * d) / dz
    dg = -(dt * adv)
    k = np.arange(nz)[:, None, None, None]
    nan = np.isnan(W)
    active = (from_below & (k > 0)) | ((W < 0.0) & (k < nz - 1)) | nan
    return np.where(nan, W, dg), active


def _uniform(dt, tend, inc):
    """d = dt tend + inc, an absent addend absent; None where both are"""
    if tend is None and inc is None:
        return None
    if tend is None:
        return _col(inc)
    t = dt * _col(tend)
    return t if inc is None else t + _col(inc)


def _sum(dg, active, d):
    """dg + d where the subsidence term exists, else d; -> (the sum, where there is one)"""
    if dg is None:
        return d, np.True_
    if d is None:
        return dg, active
    return np.where(active, dg + d, d), np.True_


def forcing(case, inc=None, mutant=None, census=None):
    """-> the new uvel, vvel, temp and tracers.  inc: what nudging() gave (None: no nudging).  census: a dict that takes the counts"""
    F = case["fields"]
    dt, gc = np.float64(case["dt"]), np.float64(case["grav"]) / np.float64(case["cp_d"])
    inc = inc or {x: None for x in QUANTITIES}
    w, zmid = case.get("wsub"), case["zmid"]
    out = {n: F[n].copy() for n in STATE + tuple(case["tracers"])}
    with np.errstate(all="ignore"):
        rho = F["density_dry"] + F[VAPOUR]

        def advect(g):
            return (None, None) if w is None else subsidence(g, w, zmid, dt, mutant)

        # temp
        g = F["temp"] if mutant == "temp_without_adiabat" else F["temp"] + gc * _col(zmid)
        dg, active = advect(g)
        s, there = _sum(dg, active, _uniform(dt, case.get("temp_tend"), inc["t"]))
        if s is not None:
            out["temp"] = np.where(there, F["temp"] + s, F["temp"])
        # the winds
        for n, x in (("uvel", "u"), ("vvel", "v")):
            dg, active = advect(F[n])
            s, there = _sum(dg, active, None if inc[x] is None else _col(inc[x]))
            if s is not None:
                out[n] = np.where(there, F[n] + s, F[n])
        # the tracers
        clamped = 0
        for n, flag in zip(case["tracers"], case["positive"]):
            dg, active = advect(F[n] / rho)
            d_q = _uniform(dt, case.get("qv_tend"), inc["q"]) if n == VAPOUR else None
            s, there = _sum(dg, active, d_q)
            if s is None:
                continue
            r = F[n] + rho * s
            if flag or mutant == "clamp_unflagged":
                clamped += int((there & (r < 0.0)).sum())
                r = np.where(r < 0.0, 0.0, r)
            out[n] = np.where(there, r, F[n])
        # Coriolis, on the updated winds
        if case.get("fcor") is not None:
            fd = case["fcor"] * dt
            ug, vg = _col(case["ug"]), _col(case["vg"])
            du, dv = out["uvel"] - ug, out["vvel"] - vg
            if mutant == "euler_coriolis":
                out["uvel"], out["vvel"] = out["uvel"] + fd * dv, out["vvel"] - fd * du
            else:
                a = 0.5 * fd
                aa = a * a
                c1, c2, den = 1.0 - aa, 2.0 * a, 1.0 + aa
                out["uvel"] = ug + ((c1 * du) + (c2 * dv)) / den
                out["vvel"] = vg + ((c1 * dv) - (c2 * du)) / den
    if census is not None:
        census["clamped"] = census.get("clamped", 0) + clamped
    return out


def ls_forcing(case, mutant=None, census=None):
    """the nudging increments from the state at entry, then the forcing: what the layers above the C ABI do"""
    inc = nudging(case, mutant)
    if all(v is None for v in inc.values()):
        inc = None
    return forcing(case, inc, mutant, census)


def members(case, idx):
    """the case on a selection of members (members are independent)"""
    sub = dict(case, fields={n: np.ascontiguousarray(a[..., idx]) for n, a in case["fields"].items()},
               zmid=np.ascontiguousarray(case["zmid"][:, idx]))
    for n in PROFILES:
        if case.get(n) is not None:
            sub[n] = np.ascontiguousarray(case[n][:, idx])
    if case.get("fcor") is not None:
        sub["fcor"] = np.ascontiguousarray(case["fcor"][idx])
    for table in ("target", "rate"):
        if case.get(table):
            sub[table] = {x: None if a is None else np.ascontiguousarray(a[:, idx]) for x, a in case[table].items()}
    return sub


class RefBackend:
    def run(self, case):
        return ls_forcing(case)
