"""One-moment ice microphysics (micro = "ice1m"): the numpy restatement of the contract (include/pam_amd_modules.h at
pam_amd_ice1m_time_step), operation for operation.  TEST INFRASTRUCTURE ONLY.

numpy's element-wise float64 arithmetic, division and square root are IEEE and never contracted, the exponential is the contract's own
exp_c (sgs_moist_ref), and no numpy reduction takes part, so the device bodies are held to this file bit for bit.  Every branch is
evaluated for every element and chosen by one selection, which gives an element the same bits whatever its neighbours are.

Why whole arrays may stand where the kernel walks a column: within a sub-cycle the flux F(k) is formed from level k before level k is
written (the pass marches upward and carries F(k + 1) from the still-old level above), so every flux of a pass comes from the state the
pass began with; and the local processes of a cell read that cell alone, after its last sedimentation, while no later flux of the pass
reads anything they write (rho of a level above uses that level's own vapour; rho(0) is the one of entry).  So a pass is one array
expression masked by the columns that still have sub-cycles left, and the local processes follow once.

A case is a dict:
  fields   water_vapor, cloud_liquid, cloud_ice, precip_liquid, precip_ice, density_dry, temp, (nz,ny,nx,nens)
  zint     (nz + 1, nens)
  dt, R_v, cp_d

The census (a dict of counters filled by the same body) names every branch the contract has; tests/ice1m_cases.py is held to reaching
each of them.

The rounding bounds of the two budgets are derived here from the number of rounded operations, with u = 2^-53:

  water: a column's M = sum_k dz (rv + rc + ri + rr + rs) against 1000 dt (precl + preci).  All quantities are non-negative and mass only
  moves down or out, so at any time the cells of a column hold at most W = M at entry between them, and a flux times dts is at most
  0.8 of the cell it leaves.  A sub-cycle does, per cell and falling species, five rounded operations on such quantities (dts / dz, the
  flux product, the flux difference, its product with q, the addition) whose operands belong to the cell or the cell above: 3 x 5 x 2 W u
  per sub-cycle, and 3 more for the two surface rates.  The local processes do fewer than 40 rounded additions and subtractions on a
  cell's species.  The test forms M with math.fsum over the rounded products dz r (one rounding each, before and after: 2 W u) and the
  precipitation term with four operations.  So |dM + 1000 dt (precl + preci)| <= (33 nsub + 46) W u.

  heat: per cell, cp_d rd dT against Lv d(rc + rr) + Ls d(ri + rs) over the local processes.  T is added to at most six times (melt,
  freeze, adjust, riming, rain, snow), each with the rounding u |T| of the sum and two more of the increment itself, which is smaller:
  8 u |T| (cp_d rd) covers them and the product with cp_d rd.  The species take fewer than 40 rounded operations, each at most u times
  the cell's water w (the greater of before and after), weighted by at most Ls: 40 u Ls w.  So the bound is u (8 cp_d rd Tmax + 40 Ls w)."""
import math

import numpy as np

from sgs_moist_ref import exp_c
from sgs_ref import same_bits, results_differ      # noqa: F401

SPECIES = ("water_vapor", "cloud_liquid", "cloud_ice", "precip_liquid", "precip_ice")
FALLING = ("precip_liquid", "precip_ice", "cloud_ice")
WRITTEN = SPECIES + ("temp",)
OUTPUTS = WRITTEN + ("precl", "preci")
MUTANTS = ("melt_order_swapped", "evaporate_ice_first", "unclipped_fall_speed", "global_nsub")
T0, TH, TW = 273.16, 233.16, 253.16
LV, LS = 2.5e6, 2.834e6
LF = LS - LV
CFL, MAX_SUB = 0.8, 64
U = 2.0 ** -53
COUNTERS = ("melt_by_ice", "melt_by_heat", "freeze_by_liquid", "freeze_by_heat", "w_zero", "w_one", "w_between", "condensation",
            "cloud_evaporation_limited", "cloud_evaporation_unlimited", "auto_liquid_above", "auto_liquid_below", "auto_ice_above",
            "auto_ice_below", "riming", "rain_limit_all", "rain_limit_half", "rain_limit_rate", "snow_limit_all", "snow_limit_half",
            "snow_limit_rate", "clipped_fall_speed", "nsub_1", "nsub_2_8", "nsub_64", "wavefront_unequal_nsub", "both_surface_rates")

f8 = np.float64


def shape_id(shape):
    return "%dx%dx%d-e%d" % shape


def count(census, name, mask):
    if census is not None:
        census[name] = census.get(name, 0) + int(np.count_nonzero(mask))


def s8(x):
    return np.sqrt(np.sqrt(np.sqrt(x)))


def s16(x):
    return np.sqrt(s8(x))


def pos(x):
    return np.where(x < 0.0, 0.0, x)


def least(a, b):
    return np.where(b < a, b, a)


def p875(q):
    return np.where(q == 0.0, 0.0, q / s8(q))


def p8125(q):
    t = s16(q)
    return np.where(q == 0.0, 0.0, q / ((t * t) * t))


def speeds(rr, rs, ri, rd, rv, rho0):
    rho = rd + rv
    fac = np.sqrt(rho0 / rho)
    return (f8(13.1) * s8(rr)) * fac, (f8(1.7) * s16(rs)) * fac, np.where(ri > 0.0, 0.4, 0.0)


def sub_cycles(case, census=None):
    """-> nsub (ny,nx,nens) from the state at entry"""
    F, dt = case["fields"], f8(case["dt"])
    zint = np.asarray(case["zint"], dtype=f8)
    dz = (zint[1:] - zint[:-1])[:, None, None, :]
    rho0 = F["density_dry"][0] + F["water_vapor"][0]
    v = speeds(F["precip_liquid"], F["precip_ice"], F["cloud_ice"], F["density_dry"], F["water_vapor"], rho0[None])
    c = np.zeros(rho0.shape)
    for k in range(dz.shape[0]):
        for vx in v:
            x = (vx[k] * dt) / dz[k]
            c = np.where((x > c) | np.isnan(x), x, c)
    big = c > CFL
    n = np.where(big, np.minimum(np.ceil(np.where(big, c, 1.0) / f8(CFL)), float(MAX_SUB)), 1.0).astype(np.int64)
    if census is not None:
        count(census, "nsub_1", n == 1)
        count(census, "nsub_2_8", (n >= 2) & (n <= 8))
        count(census, "nsub_64", n == MAX_SUB)
        flat = n.reshape(-1)
        waves = [flat[i:i + 64] for i in range(0, flat.size, 64)]
        count(census, "wavefront_unequal_nsub", np.array([w.min() != w.max() for w in waves]))
    return n


def saturation(T, R_v):
    tc = T - f8(273.15)
    rvt = R_v * T
    esw = f8(610.94) * exp_c((f8(17.625) * tc) / (f8(243.04) + tc))
    esi = f8(611.21) * exp_c((f8(22.587) * tc) / (f8(273.86) + tc))
    return tc, esw / rvt, esi / rvt


def local(c, rd, dt, cp_d, R_v, mutant=None, census=None):
    """the local processes on a dict of arrays rv, rc, ri, rr, rs, T; -> the new dict"""
    rv, rc, ri, rr, rs, T = (c[n] for n in ("rv", "rc", "ri", "rr", "rs", "T"))
    cprd = cp_d * rd
    LVc, LSc, LFc = f8(LV), f8(LS), f8(LF)

    # melt
    on = T > T0
    H = (cprd * (T - f8(T0))) / LFc
    if mutant == "melt_order_swapped":
        ms = least(rs, H)
        mi = least(ri, H - ms)
    else:
        mi = least(ri, H)
        ms = least(rs, H - mi)
    count(census, "melt_by_ice", on & ((ri > 0) | (rs > 0)) & (mi == ri) & (ms == rs) & (ri + rs < H))
    count(census, "melt_by_heat", on & (ri + rs > H))
    ri, rc = np.where(on, ri - mi, ri), np.where(on, rc + mi, rc)
    rs, rr = np.where(on, rs - ms, rs), np.where(on, rr + ms, rr)
    T = np.where(on, T - (LFc * (mi + ms)) / cprd, T)

    # freeze
    on = T < TH
    H = (cprd * (f8(TH) - T)) / LFc
    fc = least(rc, H)
    fr = least(rr, H - fc)
    count(census, "freeze_by_liquid", on & ((rc > 0) | (rr > 0)) & (rc + rr < H))
    count(census, "freeze_by_heat", on & (rc + rr > H))
    rc, ri = np.where(on, rc - fc, rc), np.where(on, ri + fc, ri)
    rr, rs = np.where(on, rr - fr, rr), np.where(on, rs + fr, rs)
    T = np.where(on, T + (LFc * (fc + fr)) / cprd, T)

    # adjust
    tc, rsw, rsi = saturation(T, R_v)
    w0 = (T - f8(TW)) / f8(20.0)
    w = np.where(w0 < 0.0, 0.0, np.where(w0 > 1.0, 1.0, w0))
    count(census, "w_zero", w == 0.0)
    count(census, "w_one", w == 1.0)
    count(census, "w_between", (w > 0.0) & (w < 1.0))
    omw = f8(1.0) - w
    rsat = rsi + w * (rsw - rsi)
    L = w * LVc + omw * LSc
    rT = f8(1.0) / T
    bw, bi = f8(243.04) + tc, f8(273.86) + tc
    sw = (f8(17.625) * f8(243.04)) / (bw * bw) - rT
    si = (f8(22.587) * f8(273.86)) / (bi * bi) - rT
    slope = (w * rsw) * sw + (omw * rsi) * si
    x = (rv - rsat) / (f8(1.0) + (L / cprd) * slope)
    up, down = x > 0.0, x < 0.0
    count(census, "condensation", up)
    dc = w * x
    di = x - dc
    tot = rc + ri
    e = least(-x, tot)
    if mutant == "evaporate_ice_first":
        ei = least(e, ri)
        el = least(e - ei, rc)
    else:
        el = least(e, rc)
        ei = least(e - el, ri)
    count(census, "cloud_evaporation_limited", down & (tot > 0) & (-x >= tot))
    count(census, "cloud_evaporation_unlimited", down & (tot > 0) & (-x < tot))
    T = np.where(up, T + (LVc * dc + LSc * di) / cprd, np.where(down, T - (LVc * el + LSc * ei) / cprd, T))
    rv = np.where(up, rv - x, np.where(down, rv + (el + ei), rv))
    rc = np.where(up, rc + dc, np.where(down, rc - el, rc))
    ri = np.where(up, ri + di, np.where(down, ri - ei, ri))

    # collect
    pr = p875(rr / rd)
    ps = p8125(rs / rd)
    dtk = dt * f8(1.0e-3)
    a = pos(rc - f8(1.0e-3) * rd)
    count(census, "auto_liquid_above", a > 0)
    count(census, "auto_liquid_below", (rc > 0) & (a == 0))
    rc1 = pos(rc - dtk * a) / (f8(1.0) + (dt * f8(2.2)) * pr)
    rr = rr + (rc - rc1)
    rc = rc1
    g = exp_c(f8(0.025) * (T - f8(T0)))
    b = pos(ri - f8(1.0e-4) * rd)
    count(census, "auto_ice_above", b > 0)
    count(census, "auto_ice_below", (ri > 0) & (b == 0))
    ri1 = pos(ri - (dtk * g) * b) / (f8(1.0) + (dt * g) * ps)
    rs = rs + (ri - ri1)
    ri = ri1
    on = T < T0
    rc2 = rc / (f8(1.0) + (dt * f8(2.0)) * ps)
    dr = rc - rc2
    count(census, "riming", on & (dr > 0))
    rs = np.where(on, rs + dr, rs)
    T = np.where(on, T + (LFc * dr) / cprd, T)
    rc = np.where(on, rc2, rc)

    # evaporate and sublimate
    tc, rsw, rsi = saturation(T, R_v)

    def loss(r, rsat, coef):
        half = f8(0.5) * (rsat - rv)
        rate = ((dt * f8(coef)) * (f8(1.0) - rv / rsat)) * np.sqrt(r)
        first = least(r, half)
        return least(first, rate), (half < r), (rate < first)

    on = (rv < rsw) & (rr > 0.0)
    l, by_half, by_rate = loss(rr, rsw, 1.0e-4)
    count(census, "rain_limit_all", on & ~by_half & ~by_rate)
    count(census, "rain_limit_half", on & by_half & ~by_rate)
    count(census, "rain_limit_rate", on & by_rate)
    rr, T = np.where(on, rr - l, rr), np.where(on, T - (LVc * l) / cprd, T)
    rv = np.where(on, rv + l, rv)
    on = (rv < rsi) & (rs > 0.0)
    l, by_half, by_rate = loss(rs, rsi, 5.0e-5)
    count(census, "snow_limit_all", on & ~by_half & ~by_rate)
    count(census, "snow_limit_half", on & by_half & ~by_rate)
    count(census, "snow_limit_rate", on & by_rate)
    rs, T = np.where(on, rs - l, rs), np.where(on, T - (LSc * l) / cprd, T)
    rv = np.where(on, rv + l, rv)
    return dict(rv=rv, rc=rc, ri=ri, rr=rr, rs=rs, T=T)


def time_step(case, mutant=None, census=None, trace=None):
    """-> {name: array} of OUTPUTS.  trace: a dict that receives "settled" (the state after the sedimentation, before the local processes)
    and "nsub" """
    F = {n: np.array(case["fields"][n], dtype=f8) for n in WRITTEN + ("density_dry",)}
    dt, R_v, cp_d = f8(case["dt"]), f8(case["R_v"]), f8(case["cp_d"])
    shape = F["temp"].shape
    out = {n: F[n] for n in WRITTEN}
    out["precl"], out["preci"] = np.zeros(shape[1:]), np.zeros(shape[1:])
    if dt == 0.0:
        return out
    with np.errstate(all="ignore"):
        zint = np.asarray(case["zint"], dtype=f8)
        dz = (zint[1:] - zint[:-1])[:, None, None, :]
        rd = F["density_dry"]
        rho0 = (rd[0] + F["water_vapor"][0])[None]
        N = sub_cycles(case, census)
        if mutant == "global_nsub":
            N = np.full_like(N, N.max())
        if trace is not None:
            trace["nsub"] = N
        nsub = N.astype(f8)
        dts = dt / nsub
        vmax = ((f8(CFL) * dz) * nsub[None]) / dt
        q = dts[None] / dz
        pl, pi = out["precl"], out["preci"]
        rv = F["water_vapor"]
        for s in range(int(N.max())):
            active = s < N
            rr, rs, ri = F["precip_liquid"], F["precip_ice"], F["cloud_ice"]
            v = speeds(rr, rs, ri, rd, rv, rho0)
            if mutant != "unclipped_fall_speed":
                count(census, "clipped_fall_speed", active[None] & ((v[0] > vmax) | (v[1] > vmax) | (v[2] > vmax)))
                v = [np.where(vx > vmax, vmax, vx) for vx in v]
            flux = [vx * r for vx, r in zip(v, (rr, rs, ri))]
            pl = np.where(active, pl + (flux[0][0] * dts) / (f8(1000.0) * dt), pl)
            pi = np.where(active, pi + ((flux[1][0] + flux[2][0]) * dts) / (f8(1000.0) * dt), pi)
            for name, fx, r in zip(FALLING, flux, (rr, rs, ri)):
                above = np.concatenate([fx[1:], np.zeros((1,) + shape[1:])], axis=0)
                F[name] = np.where(active[None], r + q * (above - fx), r)
        count(census, "both_surface_rates", (pl > 0) & (pi > 0))
        if trace is not None:
            trace["settled"] = {n: F[n].copy() for n in WRITTEN}
        c = local(dict(rv=F["water_vapor"], rc=F["cloud_liquid"], ri=F["cloud_ice"], rr=F["precip_liquid"], rs=F["precip_ice"], T=F["temp"]),
                  rd, dt, cp_d, R_v, mutant, census)
    out.update(water_vapor=c["rv"], cloud_liquid=c["rc"], cloud_ice=c["ri"], precip_liquid=c["rr"], precip_ice=c["rs"], temp=c["T"],
               precl=pl, preci=pi)
    return out


class RefBackend:
    def run(self, case):
        return time_step(case)


# ---- the budgets and their bounds (the module docstring)

def column_water(fields, zint):
    """M (ny,nx,nens): math.fsum of the rounded products dz r over the levels and the five species"""
    dz = (zint[1:] - zint[:-1])[:, None, None, :]
    prod = np.stack([dz * fields[n] for n in SPECIES])
    flat = prod.reshape(prod.shape[0] * prod.shape[1], -1)
    return np.array([math.fsum(flat[:, i]) for i in range(flat.shape[1])]).reshape(prod.shape[2:])


def water_bound(W, nsub):
    return (33.0 * nsub + 46.0) * W * U


def heat_bound(cp_d, rd, tmax, w):
    return U * (8.0 * cp_d * rd * tmax + 40.0 * LS * w)
