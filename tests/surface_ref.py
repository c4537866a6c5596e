"""Bulk surface fluxes over a slab ocean: the numpy restatement of the contract (include/pam_amd_modules.h at pam_amd_surface_fluxes,
DESIGN.md section 8), operation for operation.  TEST INFRASTRUCTURE ONLY.

numpy's element-wise float64 arithmetic is IEEE and never contracted, np.sqrt is the IEEE square root, no numpy reduction takes part, and
the exponential is the contract's own (sgs_moist_ref.exp_c through sgs_moist_ref.saturation_ratio), so no libm takes part either: the
device body is held to this file bit for bit.  Both branches of the stability function are evaluated for every element and chosen
afterwards, which gives an element the same bits whatever its neighbours are."""
import numpy as np

from sgs_moist_ref import saturation_ratio
from sgs_ref import same_bits, results_differ, shape_id      # noqa: F401

OUTPUTS = ("sfc_shf", "sfc_lhf", "sfc_temp")
FIELDS = ("temp", "density_dry", "water_vapor", "uvel", "vvel")
RADIATION = ("lw_down", "lw_up", "sw_down", "sw_up")
SCALARS = ("gust", "wetness", "grav", "cp_d", "R_v", "latvap", "slab_heat_capacity", "dt")
RHO_W, C_W = 1000.0, 4186.0          # slab_heat_capacity = RHO_W C_W depth
KARMAN, B_LOUIS, C_LOUIS = 0.4, 9.4, 5.3


def transfer_parameters(zmid0, z0):
    """cn and cstar of every member, as surface_fluxes_init forms them on the host: lnz = log(zmid0 / z0); cn = (0.4 / lnz)^2;
    cstar = ((5.3 * 9.4) cn) sqrt(zmid0 / z0)"""
    zmid0, z0 = np.asarray(zmid0, dtype=np.float64), np.asarray(z0, dtype=np.float64)
    r = zmid0 / z0
    lnz = np.log(r)
    k = KARMAN / lnz
    cn = k * k
    cstar = ((C_LOUIS * B_LOUIS) * cn) * np.sqrt(r)
    return cn, cstar


def slab_stepped(case):
    return case["slab_heat_capacity"] > 0 and case["dt"] != 0


def surface(case, internals=False):
    """-> dict of OUTPUTS; internals: also rib, f, ch, w, sa, qs, qv, rho and net (None where the slab is not stepped)"""
    F = case["fields"]
    T, rd, rv, u, v = (np.asarray(F[n][0], dtype=np.float64) for n in FIELDS)
    Ts = np.asarray(case["sfc_temp"], dtype=np.float64)
    z, cn, cstar = np.asarray(case["zmid"][0]), np.asarray(case["cn"]), np.asarray(case["cstar"])
    gust, wet, grav, cp_d, R_v, latvap, cap, dt = (np.float64(case[n]) for n in SCALARS)
    gc = grav / cp_d
    with np.errstate(all="ignore"):
        rho = rd + rv
        qv = rv / rho
        w = np.sqrt((u * u + v * v) + gust * gust)
        sa = T + gc * z
        qs = wet * saturation_ratio(Ts, rho, R_v)
        tva = sa * (1.0 + 0.608 * qv)
        tvs = Ts * (1.0 + 0.608 * qs)
        rib = ((grav * z) * (tva - tvs)) / (tvs * (w * w))
        unstable = 1.0 - (B_LOUIS * rib) / (1.0 + cstar * np.sqrt(-rib))
        d = 1.0 + 4.7 * rib
        stable = 1.0 / (d * d)
        f = np.where(rib < 0.0, unstable, stable)
        ch = cn * f
        shf = ((rho * cp_d) * (ch * w)) * (Ts - sa)
        lhf = ((rho * latvap) * (ch * w)) * (qs - qv)
        net, new = None, Ts.copy()
        if slab_stepped(case):
            pair = lambda a, b: np.float64(0.0) if case.get(a) is None else np.asarray(case[a]) - np.asarray(case[b])
            net = (pair("sw_down", "sw_up") + pair("lw_down", "lw_up")) - (shf + lhf)
            new = Ts + (dt * net) / cap
    out = dict(sfc_shf=shf, sfc_lhf=lhf, sfc_temp=new)
    if internals:
        out.update(rib=rib, f=f, ch=ch, w=w, sa=sa, qs=qs, qv=qv, rho=rho, net=net, tva=tva, tvs=tvs)
    return out


def members(case, idx):
    """the case on a selection of members (members are independent)"""
    sub = dict(case, fields={n: np.ascontiguousarray(a[..., idx]) for n, a in case["fields"].items()},
               zmid=np.ascontiguousarray(case["zmid"][:, idx]), cn=np.ascontiguousarray(case["cn"][idx]),
               cstar=np.ascontiguousarray(case["cstar"][idx]), sfc_temp=np.ascontiguousarray(case["sfc_temp"][..., idx]))
    for n in RADIATION:
        if case.get(n) is not None:
            sub[n] = np.ascontiguousarray(case[n][..., idx])
    return sub


class RefBackend:
    def run(self, case):
        return surface(case)
