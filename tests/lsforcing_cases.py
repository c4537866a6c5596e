"""The shapes and the named cases of the large-scale forcing tests, built once per shape and shared by the CPU and the GPU tests (nobody
writes to them: every backend copies what it changes), and the reference of each, computed once.  TEST INFRASTRUCTURE ONLY.

The shapes (nz, ny, nx, nens) are the smallest at which a kernel can go wrong: nz 1, 2, 4, 5, 9 (both ends in one level, and below, at
and above AHEAD = 4); nens 1, 3, 64, 65, 130 (one lane, a ragged wavefront, two wavefronts); ny nx 1, 15, 16, 17, 33 (empty, full and
wrapped slots of the level means); ny == 1 and ny > 1.  zmid is per member.  The tracer table has 0, 1 or 7 entries, by the case.

wsub is built from Courant numbers within (-0.9, 0.9) of every member's thinnest layer, so every case lies inside the limit the layers
above the C ABI enforce; dt rate <= 0.5."""
import numpy as np

import lsforcing_ref as ref

SHAPES = ((1, 1, 1, 1), (2, 1, 15, 3), (4, 4, 4, 64), (5, 1, 17, 65), (9, 3, 11, 130))
SEVEN = ("cloud_liquid", "precip_liquid", "tracer_a", ref.VAPOUR, "tracer_b", "tracer_c", "tracer_d")
UNFLAGGED = "tracer_c"            # holds both signs and is not flagged positive
ABSENT = ("no_wsub", "no_temp_tend", "no_qv_tend", "no_coriolis", "no_target_t", "no_target_q", "no_target_u", "no_target_v")
CASE_NAMES = ("all_on", "vapour_first", "vapour_last", "one_tracer", "no_tracers", "subsidence_only", "no_nudging", "clamp", "zero_forcing",
              "nan_w", "nan_cell") + ABSENT
CONSTANTS = dict(dt=10.0, grav=9.80616, cp_d=1004.64)
_CACHE, _REF, _CENSUS = {}, {}, {}


def nan_places(shape):
    """(k, e) of the NaN wsub, and (k, j, i, e) of the NaN temp and of the NaN vapour"""
    nz, ny, nx, nens = shape
    return (nz // 2, nens - 1), (nz // 2, ny - 1, nx - 1, nens // 2), (nz - 1, 0, nx // 2, 0)


def grid(nz, nens):
    """stretched midpoints up to 12 km, every member's column scaled a little differently; -> zmid, the thinnest layer of every member"""
    zint = ((np.arange(nz + 1) / nz) ** 1.5 * 12000.0 + 40.0 * np.arange(nz + 1))[:, None] * (1.0 + 0.03 * (np.arange(nens) % 7))[None, :]
    zmid = 0.5 * (zint[:-1] + zint[1:])
    dzmin = (zmid[1:] - zmid[:-1]).min(axis=0) if nz > 1 else np.full(nens, 100.0)
    return zmid, dzmin


def courant(nz, nens):
    """the Courant numbers behind wsub (nz,nens): a sign change inside the column, the opposite sign in every odd member, members at rest,
    members that blow into the ground all the way and members that blow into the lid all the way, and single levels at rest"""
    k, e = np.arange(nz)[:, None], np.arange(nens)[None, :]
    c = 0.9 * np.cos(np.pi * (k + 0.5) / max(nz, 1) + 0.3 * (e % 4)) * np.where(e % 2 == 0, 1.0, -1.0)
    c = np.where(e % 5 == 4, 0.0, c)
    c = np.where(e % 11 == 6, -0.5 - 0.04 * k, c)       # subsiding all the way: w < 0 at the lid
    c = np.where(e % 11 == 8, 0.5 + 0.04 * k, c)        # rising all the way: w > 0 at the ground
    c = np.where((k + e) % 6 == 5, 0.0, c)
    return c


def profiles(rng, dzmin, dt, temp, qv):
    """every profile of a call for fields of the shape of temp: wsub from courant(), tendencies, a geostrophic wind, fcor of either sign,
    targets about the level means of temp and qv, and rates with dt rate <= 0.5 (one profile for both winds)"""
    nz, nens = temp.shape[0], temp.shape[3]
    prof = lambda lo, hi: lo + (hi - lo) * rng.random((nz, nens))
    mean = lambda a: a.mean(axis=(1, 2))
    target = dict(t=mean(temp) + prof(-1.0, 1.0), q=mean(qv) * prof(0.8, 1.2), u=prof(-6.0, 6.0), v=prof(-6.0, 6.0))
    rate_uv = prof(0.0, 0.5 / dt)
    rate = dict(t=prof(0.0, 0.5 / dt), q=prof(0.0, 0.5 / dt), u=rate_uv, v=rate_uv)
    return dict(wsub=courant(nz, nens) * dzmin[None, :] / dt, temp_tend=prof(-2.0e-4, 2.0e-4), qv_tend=prof(-2.0e-8, 2.0e-8), ug=prof(-8.0, 8.0),
                vg=prof(-8.0, 8.0), fcor=1.0e-4 * (1.0 + 0.5 * np.sin(np.arange(nens))) * np.where(np.arange(nens) % 3 == 2, -1.0, 1.0),
                target=target, rate=rate)


def cases(shape):
    if shape in _CACHE:
        return _CACHE[shape]
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(20261023 + 7 * nz + 100 * ny + 1000 * nx + 10000 * nens)
    C = CONSTANTS
    zmid, dzmin = grid(nz, nens)
    Z = zmid[:, None, None, :]
    temp = 299.0 + 4.0 * rng.random(shape) - 0.0065 * Z
    rho = (1.10 + 0.1 * rng.random(shape)) * np.exp(-Z / 8000.0)
    qv = (0.004 + 0.012 * rng.random(shape)) * np.exp(-Z / 2500.0)
    rho_v = qv * rho
    fields = dict(uvel=16.0 * rng.random(shape) - 8.0, vvel=16.0 * rng.random(shape) - 8.0, temp=temp, density_dry=rho - rho_v)
    fields[ref.VAPOUR] = rho_v
    cloud = rng.random(shape)
    fields["cloud_liquid"] = np.where(cloud > 0.6, 1.0e-3 * (cloud - 0.6), 0.0) * rho
    fields["precip_liquid"] = np.where(cloud > 0.85, 5.0e-4 * rng.random(shape), 0.0) * rho
    fields["tracer_a"] = rng.random(shape) * rho
    fields["tracer_b"] = np.exp(-Z / 1500.0) * rho * (1.0 + 0.1 * rng.random(shape))
    fields["tracer_c"] = (rng.random(shape) - 0.5) * rho
    fields["tracer_d"] = 1.0e-6 * rng.random(shape)
    positive = {n: n != UNFLAGGED for n in SEVEN}

    common = dict(C, zmid=zmid, **profiles(rng, dzmin, C["dt"], temp, qv))
    wsub, target = common["wsub"], common["target"]

    def case(tracers=SEVEN, f=None, **kw):
        return dict(common, fields=dict(fields, **(f or {})), tracers=tuple(tracers), positive=tuple(positive[n] for n in tracers), **kw)

    without = lambda x: dict(target=dict(target, **{x: None}))
    order = lambda i: [n for n in SEVEN if n != ref.VAPOUR][:i] + [ref.VAPOUR] + [n for n in SEVEN if n != ref.VAPOUR][i:]
    off = dict(temp_tend=None, qv_tend=None, ug=None, vg=None, fcor=None, target=None)
    (kw_, ew), (kt, jt, it, et), (kq, jq, iq, eq) = nan_places(shape)
    w_nan = wsub.copy()
    w_nan[kw_, ew] = np.nan
    t_nan, q_nan = temp.copy(), rho_v.copy()
    t_nan[kt, jt, it, et] = np.nan
    q_nan[kq, jq, iq, eq] = np.nan
    zero = np.zeros((nz, nens))
    out = dict(
        all_on=case(),
        vapour_first=case(order(0)),
        vapour_last=case(order(6)),
        one_tracer=case((ref.VAPOUR,)),
        no_tracers=case((), qv_tend=None, **without("q")),
        subsidence_only=case(**off),
        no_nudging=case(target=None),
        # a drying that takes more than some cells hold: the clamp acts in those and in no others
        clamp=case(qv_tend=-np.broadcast_to(np.median(qv, axis=(1, 2)), (nz, nens)) / C["dt"] + zero),
        zero_forcing=case(wsub=zero, temp_tend=zero, qv_tend=zero, ug=zero, vg=zero, fcor=np.zeros(nens),
                          target={x: zero for x in ref.QUANTITIES}, rate={x: zero for x in ref.QUANTITIES}),
        nan_w=case(wsub=w_nan),
        nan_cell=case(f={"temp": t_nan, ref.VAPOUR: q_nan}, target=None),
        no_wsub=case(wsub=None),
        no_temp_tend=case(temp_tend=None),
        no_qv_tend=case(qv_tend=None),
        no_coriolis=case(fcor=None, ug=None, vg=None),
        no_target_t=case(**without("t")),
        no_target_q=case(**without("q")),
        no_target_u=case(**without("u")),
        no_target_v=case(**without("v")),
    )
    assert tuple(out) == CASE_NAMES
    _CACHE[shape] = out
    return out


def reference(shape, name):
    key = (shape, name)
    if key not in _REF:
        _CENSUS[key] = {}
        _REF[key] = ref.ls_forcing(cases(shape)[name], census=_CENSUS[key])
    return _REF[key]


def clamped(shape, name):
    """how many elements the positive clamp changed in the reference of a case"""
    reference(shape, name)
    return _CENSUS[shape, name].get("clamped", 0)
