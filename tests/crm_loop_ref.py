"""The whole native CRM loop as a chain of the repository's restatements, in the order of examples/driver.cpp: radiation (grey longwave over
sfc_temp, then shortwave) -> dycore (the oracle) -> sponge layer -> large-scale forcing with Coriolis -> ESMT (2-D) -> surface fluxes over a
slab -> hyperdiffusion -> the SGS closure (TKE or Smagorinsky, moist, with surface fluxes and horizontal mixing) -> ice1m.  TEST
INFRASTRUCTURE ONLY: no torch, no device, no new physics.  Every call is the numpy restatement its own module is held to bit for bit
(tests/*_ref.py), the dycore and the sponge layer are oracle/awfl_oracle.

What is written down HERE, and read back from no coupler, is what the plug-ins hand one another: the tracer table (order, positive flag,
mass flag, the index of the vapour), the constants, the condensate species of option micro = "ice1m", the defaults of every scheme, and
per call the set of entries its contract lets it write (include/pam_amd_modules.h, the class comments of pam_amd/physics.py,
pam_amd/micro.py and pam_amd/modules.py).  tests/test_crm_loop_gpu.py holds the coupler, as the plug-ins' init leave it, to these tables.

A state is a State: `S`, name -> array under the names of the DataManager (the five state fields, every tracer, and whatever a module
keeps between calls: sfc_temp, the radiation outputs, tk, tkh, precl, preci, the ESMT means, the static tables and profiles), the
oracle whose hydrostatic profile was declared on the initial fields, and the count of radiation calls.

The shapes.  The issue's full3d_flat (10,4,6,3) and full3d_members (8,3,5,65) have 1 < ny < 5, which pam_amd_hyperdiffusion refuses (its
five-point periodic stencil needs ny == 1 or ny >= 5, and nx >= 5): both moved to the nearest ny it takes, 5.  Horizontal SGS mixing
(nx >= 3, ny != 2) and every other module take all three."""
import copy

import numpy as np

import esmt_ref
import grayrad_ref as lwref
import grayrad_sw_ref as swref
import hd_ref
import ice1m_ref
import lsforcing_ref
import plugins_ref
import sgs_horizontal_ref as href
import sgs_moist_ref as mref
import sgs_tke_ref as tref
import surface_ref
from oracle import awfl_oracle as ao
from parity_cases import build_inputs

STATE = ("density_dry", "uvel", "vvel", "wvel", "temp")
# ---- the contract tables
# MicrophysicsIce.init writes Kessler's constants to the options; the dycore reads them from there
CONSTS = dict(R_d=287.0, cp_d=1003.0, R_v=461.0, cp_v=1859.0, p0=1.0e5, grav=9.81)
# (name, positive, adds mass), in the order of registration: micro.init, sgs.init, esmt_init, then the dycore takes the table
TRACERS_ICE1M = (("water_vapor", True, True), ("cloud_liquid", True, True), ("cloud_ice", True, True), ("precip_liquid", True, True),
                 ("precip_ice", True, True))
TRACER_TKE = (("tke", True, False),)
TRACERS_ESMT = (("esmt_u", False, False), ("esmt_v", False, False))
CLOUD, PRECIP = ("cloud_liquid", "cloud_ice"), ("precip_liquid", "precip_ice")       # micro = "ice1m": the moist SGS branch
LIQUID, ICE = ("cloud_liquid",), ("cloud_ice",)                                       # and the radiation
LATVAP = 2501000.0                                                                     # option "latvap" is absent
RAD_LW = dict(k_d=1e-4, k_v=0.1, k_l=85.0, k_i=40.0, lw_down_top=0.0, sigma=lwref.SIGMA)
RAD_SW = dict(solar_constant=1361.0, albedo=0.07, a_d=1e-6, a_v=2e-3, a_l=0.1, a_i=0.1, s_l=11.0, s_i=5.0)
SURFACE = dict(gust=1.0, wetness=0.98, z0=1.0e-4)
SPONGE = dict(num_layers=5, time_scale=60.0)
CRM_DT, RAD_EVERY, COSZEN, SLAB_DEPTH, HD_TAU, FCOR = 2.0, 2, 0.8, 1.0, 600.0, 1.0e-4
SGS_CS, SGS_CK, SGS_SEED, SGS_PRANDTL, CLOUD_THRESHOLD = 0.2, 0.1, 1.0e-3, 1.0 / 3.0, 0.0

RAD_LW_OUT = ("rad_heating", "rad_olr", "rad_lw_down_sfc", "rad_lw_up_sfc")
RAD_SW_OUT = ("rad_sw_heating", "rad_sw_down_sfc", "rad_sw_up_sfc", "rad_sw_up_top")
CALLS = ("radiation", "dycore", "sponge_layer", "ls_forcing", "esmt_pgf", "surface_fluxes", "hyperdiffusion", "sgs", "micro")

STACKS = {
    # name: (shape (nz,ny,nx,nens), closure, esmt, CRM steps)
    "full3d_flat": ((10, 5, 6, 3), "tke", False, 3),          # flat lanes
    "full3d_members": ((8, 5, 5, 65), "tke", False, 2),       # the dycore's member lanes, the modules' ragged member block
    "full2d_esmt": ((10, 1, 9, 66), "smagorinsky", True, 3),  # 2-D: ESMT, and the Smagorinsky closure in place of TKE
}


class Stack:
    """one named loop: shape, grid, tracer table, options and the seeded initial state (fields, in the oracle's layout, and S0)"""


def _ls(case):
    inc = lsforcing_ref.nudging(case)
    return lsforcing_ref.forcing(case, inc), inc


def _esmt(case):
    D = esmt_ref.diagnose(case)
    return D, esmt_ref.pgf(case, means=D)


# what computes each module: the numpy restatements.  tests/test_crm_loop.py puts the emulated device bodies in their place
KERNELS = dict(lw=lwref.radiation, sw=swref.radiation, forced=plugins_ref.radiation_forced, ls=_ls, esmt=_esmt, surface=surface_ref.surface,
               hd=hd_ref.hyperdiffusion, tke_coefficients=tref.coefficients, smag_coefficients=mref.coefficients,
               horizontal=href.diffuse_horizontal, diffuse=mref.diffuse, ice=ice1m_ref.time_step)


class State:
    def __init__(self, stack, S, oracle, kernels=None):
        self.stack, self.S, self.oracle, self.rad_calls = stack, S, oracle, 0
        self.kernels = dict(KERNELS, **(kernels or {}))


_STACKS = {}


def stack(name):
    """the named stack, built once and shared: nobody writes to what it holds"""
    if name in _STACKS:
        return _STACKS[name]
    shape, closure, esmt, steps = STACKS[name]
    nz, ny, nx, nens = shape
    k = Stack()
    k.name, k.shape, k.closure, k.esmt, k.steps = name, shape, closure, esmt, steps
    k.tracers = TRACERS_ICE1M + (TRACER_TKE if closure == "tke" else ()) + (TRACERS_ESMT if esmt else ())
    k.names = tuple(t[0] for t in k.tracers)
    k.positive, k.adds_mass = tuple(t[1] for t in k.tracers), tuple(t[2] for t in k.tracers)
    k.idwv = k.names.index("water_vapor")
    k.dt, k.rad_every = CRM_DT, RAD_EVERY
    zint = np.concatenate([[0.0], np.cumsum(1.04 ** np.arange(nz))])
    zint = zint * (12000.0 / zint[-1])
    # shear on both axes in 3-D, dx != dy; 2-D: the supercell state as it is
    f, k.xlen, k.ylen, k.zint, k.dz = build_inputs(nens, nx, ny, nz, list(k.tracers), zint, CONSTS, dxy=500.0,
                                                   dy=800.0 if ny > 1 else None, flow="diag" if ny > 1 else "x")
    if ny == 1:     # a wind along y on the 2-D grid too (the dycore carries it, Coriolis turns it, ESMT's second scalar rides on it)
        f["vvel"] = 0.3 * f["uvel"] - 2.0
    k.dx, k.dy = k.xlen / nx, k.ylen / ny
    k.zmid = 0.5 * (k.zint[:-1] + k.zint[1:])
    _add_condensate(k, f)
    k.fields = f
    k.S0 = _initial_entries(k, f)
    _STACKS[name] = k
    return k


def _add_condensate(k, f):
    """by hand, as the Kessler loop test of tests/test_cpp_driver.py does for rain: supersaturated columns, cloud liquid below the melting
    level and a little far above it, cloud ice above it, rain that reaches the ground, snow through the whole column in some columns (it
    melts in the warm levels, rimes and sublimates aloft, and reaches the ground), and a seeded tke.  Every amount is a smooth function of the column
    and the member times a round factor: no cell sits on a threshold of the ice scheme"""
    nz, ny, nx, nens = k.shape
    rd, T, tr = f["density_dry"], f["temp"], f["tracers"]
    t = {n: i for i, n in enumerate(k.names)}
    col = (np.arange(ny)[:, None, None] * nx + np.arange(nx)[None, :, None]) + 0.37 * np.arange(nens)[None, None, :]
    wave = np.cos(col)[None] ** 2                                        # (1,ny,nx,nens) in [0, 1]
    # a cold layer under the sounding, the same in every column (so nothing starts to move): the two lowest levels 30 K colder, the
    # vapour capped below saturation there before the columns are moistened.  Under the sounding's 296 K every flake melts above the ground
    # and preci is what the implicit mixing leaks downward (1e-21 m/s, a relative floor of 3e-12, beyond a tenth of its cap); over the cold
    # layer snow reaches the ground in every step, and the warm levels above it still melt what falls into them
    T[:2] -= 30.0
    rv = tr[t["water_vapor"]]
    rv[:2] = np.minimum(rv[:2], 0.9 * ice1m_ref.saturation(T[:2], CONSTS["R_v"])[2])
    rv *= 1.0 + 0.3 * wave                                               # supersaturates some columns
    snowing = np.sin(1.7 * col)[None] > 0.3
    warm, cold, very_cold = T > ice1m_ref.T0 + 2.0, T < ice1m_ref.T0 - 8.0, T < ice1m_ref.TH - 4.0
    tr[t["cloud_liquid"]] = np.where(warm | very_cold, 1.6e-3 * wave, np.where(cold, 2.0e-4 * wave, 0.0)) * rd
    tr[t["cloud_ice"]] = np.where(cold, 3.0e-4 * (1.0 - wave), 0.0) * rd
    tr[t["precip_liquid"]] = 0.0
    tr[t["precip_liquid"]][:max(nz // 3, 2)] = (2.0e-3 * wave * rd)[:max(nz // 3, 2)]
    tr[t["precip_ice"]] = np.where(snowing, 1.0e-3 * (0.25 + wave), 0.0) * rd
    if "tke" in t:
        # exact zeros beside turbulent columns, the wind across the edges: the dycore's limiter acts on tke itself in the first step
        tr[t["tke"]] = np.where(np.sin(2.3 * col)[None] > -0.2, (rd + tr[t["water_vapor"]]) * (0.05 + 0.5 * wave), 0.0)
        tr[t["tke"]] *= np.exp(-k.zmid / 3000.0)[:, None, None, :]
    if k.esmt:      # the scalars as esmt_set("crm") leaves them: rho times the level means of the CRM's own wind
        rho = rd + tr[t["water_vapor"]]
        um, vm = esmt_ref.level_mean(f["uvel"]), esmt_ref.level_mean(f["vvel"])
        tr[t["esmt_u"]], tr[t["esmt_v"]] = esmt_ref.set_scalars(rd, tr[t["water_vapor"]], um, vm)
        assert rho.min() > 0


def _initial_entries(k, f):
    """everything beside the fields that the DataManager holds before the first step, under its names"""
    nz, ny, nx, nens = k.shape
    col = (ny, nx, nens)
    S = {}
    # sfc_temp a few K either side of the air above it
    air = f["temp"][0] + (CONSTS["grav"] / CONSTS["cp_d"]) * k.zmid[0]
    idx = np.arange(ny * nx * nens).reshape(col)
    S["sfc_temp"] = air + np.where(idx % 2 == 0, 1.0, -1.0) * (1.0 + 3.0 * np.cos(0.61 * idx) ** 2)
    for n in ("sfc_shf", "sfc_lhf", "sfc_mom_flx_u", "sfc_mom_flx_v", "precl", "preci") + RAD_LW_OUT[1:] + RAD_SW_OUT[1:]:
        S[n] = np.zeros(col)
    for n in ("tk", "tkh", "rad_heating", "rad_sw_heating"):
        S[n] = np.zeros(k.shape)
    S["rad_coszen"] = np.full(nens, COSZEN)
    S["sfc_cn"], S["sfc_cstar"] = surface_ref.transfer_parameters(k.zmid[0], np.full(nens, SURFACE["z0"]))
    # the large-scale profiles: subsidence, cooling and moistening, a geostrophic wind, the winds nudged towards it
    z = k.zmid / k.zint[-1]
    S["ls_wsub"] = -0.02 * np.sin(np.pi * z)
    S["ls_temp_tend"] = -2.0e-5 * (1.0 - z)
    S["ls_qv_tend"] = 2.0e-8 * (1.0 - z)
    S["ls_ug"], S["ls_vg"] = 4.0 + 12.0 * z, -3.0 + 2.0 * z
    S["ls_nudge_u"], S["ls_nudge_v"] = S["ls_ug"].copy(), S["ls_vg"].copy()
    S["ls_nudge_rate_uv"] = np.full((nz, nens), 1.0 / 1800.0)
    S["ls_inc_u"], S["ls_inc_v"] = np.zeros((nz, nens)), np.zeros((nz, nens))
    S["ls_fcor"] = np.full(nens, FCOR)
    if k.esmt:
        S["esmt_cos"], S["esmt_sin"] = esmt_ref.tables(nx)
        for n in ("esmt_rho_mean", "esmt_u_mean", "esmt_v_mean"):
            S[n] = np.zeros((nz, nens))
    return S


def ls_profiles(k):
    """the keyword arguments of modules.ls_forcing_init that give the stack's profiles"""
    S = k.S0
    return dict(wsub=S["ls_wsub"], temp_tend=S["ls_temp_tend"], qv_tend=S["ls_qv_tend"], ug=S["ls_ug"], vg=S["ls_vg"], nudge_u=S["ls_nudge_u"],
                nudge_v=S["ls_nudge_v"], nudge_rate_uv=S["ls_nudge_rate_uv"], fcor=FCOR)


# ---- between the oracle's layout and the entries

def entries(k, fields, held=None):
    """name -> array (copies) of the oracle's field dict, with `held` (default the stack's initial entries) beside them"""
    S = {n: np.array(fields[n], dtype=np.float64, order="C") for n in STATE}
    for t, n in enumerate(k.names):
        S[n] = np.array(fields["tracers"][t], dtype=np.float64, order="C")
    S.update({n: a.copy() for n, a in (k.S0 if held is None else held).items()})
    return S


def to_fields(k, S):
    f = {n: np.ascontiguousarray(S[n], dtype=np.float64).copy() for n in STATE}
    f["tracers"] = np.ascontiguousarray(np.stack([S[n] for n in k.names]), dtype=np.float64)
    return f


def from_fields(k, f):
    out = {n: f[n] for n in STATE}
    out.update({n: np.ascontiguousarray(f["tracers"][t]) for t, n in enumerate(k.names)})
    return out


def make_oracle(k, fields, positive=None):
    """the stack's oracle with the hydrostatic profile declared on `fields` (the oracle's layout, untouched)"""
    nz, ny, nx, nens = k.shape
    o = ao.OracleDycore(nens, nx, ny, nz, k.xlen, k.ylen, k.dz, k.positive if positive is None else positive, k.adds_mass, k.idwv, consts=CONSTS)
    o.declare_current_profile_as_hydrostatic(copy.deepcopy(fields))
    return o


def start(k, fields=None, held=None, positive=None, kernels=None):
    """the State of a run from `fields` (default the stack's own)"""
    fields = k.fields if fields is None else fields
    return State(k, entries(k, fields, held), make_oracle(k, fields, positive), kernels)


# ---- the calls: each -> the entries it writes, name -> new array, from the entries S it reads

def _table(k, S):
    return {n: S[n] for n in STATE + k.names}


def radiation(state, S):
    """RadiationGray with the sun: every rad_every-th call computes the longwave (over sfc_temp) and then the shortwave on the temp the
    longwave left; the calls between apply the two stored heatings, temp + (heating / 1.0) dt twice"""
    k = state.stack
    recompute = state.rad_calls % k.rad_every == 0
    state.rad_calls += 1
    if not recompute:
        temp = state.kernels["forced"](S["temp"], S["rad_heating"], 1.0, k.dt)
        return dict(temp=state.kernels["forced"](temp, S["rad_sw_heating"], 1.0, k.dt))
    case = dict(RAD_LW, fields=_table(k, S), liquid=LIQUID, ice=ICE, zint=k.zint, cp_d=CONSTS["cp_d"], dt=k.dt, sfc_temp=S["sfc_temp"])
    lw = state.kernels["lw"](case)
    sw = state.kernels["sw"](dict(case, fields=dict(case["fields"], temp=lw["temp"]), coszen=S["rad_coszen"], sfc_albedo=None, **RAD_SW))
    out = {n: lw[n] for n in RAD_LW_OUT}
    out.update({n: sw[n] for n in RAD_SW_OUT})
    out["temp"] = sw["temp"]
    return out


def radiation_writes(state):
    """what the NEXT radiation call may write"""
    return ("temp",) + ((RAD_LW_OUT + RAD_SW_OUT) if state.rad_calls % state.stack.rad_every == 0 else ())


def dycore(state, S, info=None):
    k = state.stack
    f = to_fields(k, S)
    n, dt_dyn = state.oracle.time_step(f, k.dt)
    if info is not None:
        info.update(nsub=n, dt_dyn=dt_dyn)
    return from_fields(k, f)


def sponge_layer(state, S):
    k = state.stack
    f = to_fields(k, S)
    ao.sponge_layer(f, k.zint, k.zmid, k.dt, SPONGE["num_layers"], SPONGE["time_scale"])
    return from_fields(k, f)


def ls_case(k, S, coriolis=True):
    return dict(fields=_table(k, S), tracers=k.names, positive=k.positive, zmid=k.zmid, wsub=S["ls_wsub"], temp_tend=S["ls_temp_tend"],
                qv_tend=S["ls_qv_tend"], ug=S["ls_ug"], vg=S["ls_vg"], fcor=S["ls_fcor"] if coriolis else None,
                target=dict(t=None, q=None, u=S["ls_nudge_u"], v=S["ls_nudge_v"]),
                rate=dict(t=None, q=None, u=S["ls_nudge_rate_uv"], v=S["ls_nudge_rate_uv"]), dt=k.dt, grav=CONSTS["grav"], cp_d=CONSTS["cp_d"])


def ls_forcing(state, S):
    case = ls_case(state.stack, S)
    out, inc = state.kernels["ls"](case)
    out = dict(out)
    out.update(ls_inc_u=inc["u"], ls_inc_v=inc["v"])
    return out


def esmt_pgf(state, S):
    """modules.esmt_pgf(coupler, forcing=False): the diagnosis of the three level means, then the pressure force on both scalars"""
    k = state.stack
    case = dict(fields={n: S[n] for n in ("wvel", "density_dry", "water_vapor", "esmt_u", "esmt_v")}, zmid=k.zmid, dz=k.dz, force_u=None,
                force_v=None, cos=S["esmt_cos"], sin=S["esmt_sin"], dx=k.dx, dt=k.dt, kmax=k.shape[2] // 2, skip_v=False, gcm_u=None, gcm_v=None, gcm_dt=1.0)
    D, out = state.kernels["esmt"](case)
    out = dict(out)
    out.update(esmt_rho_mean=D["rho_mean"], esmt_u_mean=D["u_mean"], esmt_v_mean=D["v_mean"])
    return out


def surface_fluxes(state, S):
    k = state.stack
    case = dict(fields=_table(k, S), zmid=k.zmid, cn=S["sfc_cn"], cstar=S["sfc_cstar"], sfc_temp=S["sfc_temp"], lw_down=S["rad_lw_down_sfc"],
                lw_up=S["rad_lw_up_sfc"], sw_down=S["rad_sw_down_sfc"], sw_up=S["rad_sw_up_sfc"], gust=SURFACE["gust"], wetness=SURFACE["wetness"],
                grav=CONSTS["grav"], cp_d=CONSTS["cp_d"], R_v=CONSTS["R_v"], latvap=LATVAP,
                slab_heat_capacity=surface_ref.RHO_W * surface_ref.C_W * SLAB_DEPTH, dt=k.dt)
    return state.kernels["surface"](case)


def hyperdiffusion(state, S):
    k = state.stack
    names = ("temp", "uvel", "vvel", "wvel") + k.names
    positive = (0, 0, 0, 0) + tuple(int(p) for p in k.positive)
    return dict(zip(names, state.kernels["hd"]([S[n] for n in names], positive, k.dt, HD_TAU)))


def sgs_case(k, S):
    ce, ce1, ce2 = tref.constants(SGS_CS, SGS_CK)
    return dict(fields=_table(k, S), tracers=k.names, cloud=CLOUD, precip=PRECIP, moist=True, zint=k.zint, zmid=k.zmid, dx=k.dx, dy=k.dy, dt=k.dt,
                grav=CONSTS["grav"], cp_d=CONSTS["cp_d"], R_d=CONSTS["R_d"], R_v=CONSTS["R_v"], cloud_threshold=CLOUD_THRESHOLD, latvap=LATVAP,
                cs=SGS_CS, prandtl=SGS_PRANDTL, ck=SGS_CK, ce1=ce1, ce2=ce2, seed=SGS_SEED, sfc_flx_u=S["sfc_mom_flx_u"],
                sfc_flx_v=S["sfc_mom_flx_v"], sfc_shf=S["sfc_shf"], sfc_lhf=S["sfc_lhf"])


def sgs(state, S):
    """the closure with moist = surface_fluxes = horizontal = True: the coefficients (the TKE closure steps tke in place), the horizontal
    mixing with the same tk and tkh, the column solve with the surface fluxes in row 0 of temp and of the vapour"""
    k = state.stack
    case = sgs_case(k, S)
    if k.closure == "tke":
        tke, tk, tkh = state.kernels["tke_coefficients"](case)
        case = tref.after_coefficients(case, tke)
    else:
        tk, tkh = state.kernels["smag_coefficients"](case)
    case = dict(case, fields=dict(case["fields"], **state.kernels["horizontal"](case, tk, tkh)))
    out = dict(state.kernels["diffuse"](case, tk, tkh))
    out.update(tk=tk, tkh=tkh)
    return out


def micro(state, S, census=None):
    k = state.stack
    case = dict(fields={n: S[n] for n in ice1m_ref.WRITTEN + ("density_dry",)}, zint=k.zint, dt=k.dt, R_v=CONSTS["R_v"], cp_d=CONSTS["cp_d"])
    return state.kernels["ice"](case, census=census) if census is not None else state.kernels["ice"](case)


RESTATEMENTS = dict(radiation=radiation, dycore=dycore, sponge_layer=sponge_layer, ls_forcing=ls_forcing, esmt_pgf=esmt_pgf,
                    surface_fluxes=surface_fluxes, hyperdiffusion=hyperdiffusion, sgs=sgs, micro=micro)


def writes(state, call):
    """the entries the contract of `call` lets it write, before the call is made"""
    k = state.stack
    table = STATE + k.names
    return {"radiation": radiation_writes(state), "dycore": table, "sponge_layer": table,
            "ls_forcing": ("uvel", "vvel", "temp") + k.names + ("ls_inc_u", "ls_inc_v"),
            "esmt_pgf": ("esmt_u", "esmt_v", "esmt_rho_mean", "esmt_u_mean", "esmt_v_mean", "esmt_workspace"),
            "surface_fluxes": surface_ref.OUTPUTS, "hyperdiffusion": ("temp", "uvel", "vvel", "wvel") + k.names,
            "sgs": ("tk", "tkh", "uvel", "vvel", "wvel", "temp") + k.names, "micro": ice1m_ref.OUTPUTS}[call]


def order(k):
    """the calls of one CRM step of the stack, in the driver's order"""
    return tuple(c for c in CALLS if c != "esmt_pgf" or k.esmt)


def step(state, k, until=None, trace=None, calls=None, backends=None, census=None):
    """one CRM step, in place on state.S.  until: stop after that call.  trace: a list that takes (call, the entries the call may write, a
    copy of S after it) for every call.  calls: another order (the mutants).  backends: call -> function in place of the restatement"""
    S = state.S
    for call in (order(k) if calls is None else calls):
        allowed = writes(state, call)
        fn = (backends or {}).get(call, RESTATEMENTS[call])
        out = fn(state, S, census) if (call == "micro" and census is not None and fn is micro) else fn(state, S)
        assert set(out) <= set(allowed), (call, sorted(set(out) - set(allowed)))
        S.update(out)
        if trace is not None:
            trace.append((call, allowed, dict(S)))
        if call == until:
            break
    return state


def run_state(k, fields=None, steps=None, **kw):
    """`steps` CRM steps from `fields`: -> the State.  The keywords are start's (positive) and step's (calls, backends, census, trace)"""
    state = start(k, fields, positive=kw.pop("positive", None), kernels=kw.pop("kernels", None))
    for _ in range(k.steps if steps is None else steps):
        step(state, k, **kw)
    return state


def runner(k, steps=None, kept=None, **kw):
    """run(fields) with the signature parity_gate.noise_floor wants: advances the oracle-layout dict in place.  kept: a list that takes
    every run's final entries (the column outputs a floor is formed of)"""
    def run(fields):
        state = run_state(k, fields, steps, **kw)
        f = to_fields(k, state.S)
        for n in STATE:
            fields[n][...] = f[n]
        fields["tracers"][...] = f["tracers"]
        if kept is not None:
            kept.append(state.S)
    return run


def run(fields, name="full3d_flat"):
    runner(stack(name))(fields)


# ---- the gate of the free-running comparison (tests/parity_gate.py), shared by the CPU and the GPU tests

COLUMN_OUTPUTS = ("precl", "preci", "sfc_temp", "rad_olr", "rad_lw_down_sfc", "rad_lw_up_sfc", "rad_sw_down_sfc", "rad_sw_up_sfc", "rad_sw_up_top")
CAP_NOISE, CAP_COLUMN = 1.0e-8, 1.0e-10       # the caps of test_cpp_driver_crm_loop_dycore_sponge_kessler: winds and tracers, column outputs
FLOOR_SEED = 0
_FLOORS = {}


def column_errors(got, exp):
    """the worst error of every column output, relative to the largest magnitude of the expected one"""
    return {n: float(np.abs(got[n] - exp[n]).max() / max(np.abs(exp[n]).max(), 1e-300)) for n in COLUMN_OUTPUTS}


def floors(k):
    """-> base (the chain's final fields in the oracle's layout), held (its final entries), floor: parity_gate.noise_floor through the whole
    chain, the column outputs' floors formed the same way from the same three twins.  Computed once per stack and shared"""
    from parity_gate import noise_floor
    if k.name not in _FLOORS:
        kept = []
        run = runner(k, kept=kept)
        base = copy.deepcopy(k.fields)
        run(base)
        held = kept.pop()
        floor = noise_floor(run, k.fields, list(k.names), FLOOR_SEED, base=base)
        for twin in kept:
            for n, e in column_errors(twin, held).items():
                floor[n] = max(floor.get(n, 0.0), e)
        _FLOORS[k.name] = (base, held, floor)
    return _FLOORS[k.name]


def gates(k, base, floor):
    """per quantity: TOL_TIGHT for rho_d, T and the vapour; min(cap, max(1e-12, FLOOR_K floor)) for the rest, the cap 1e-8 for the winds and
    the other tracers and 1e-10 for the column outputs; 0 for a field that is identically zero in the chain"""
    import parity_gate
    gate = parity_gate.gates(base, list(k.names), 0, floor=floor, cap={n: CAP_NOISE for n in floor})
    for n in COLUMN_OUTPUTS:
        gate[n] = parity_gate.floor_gate(floor[n], CAP_COLUMN)
    return gate


def errors(k, got_fields, got_held, base, held):
    """worst_errors of the fields and column_errors of the outputs, in one dict"""
    from parity_gate import worst_errors
    worst = worst_errors(got_fields, base, list(k.names))
    worst.update(column_errors(got_held, held))
    return worst
