"""States for the P3 coupling tests, the binding of the host emulation (tests/emu/p3_emu.cpp) and the restated chain pack -> stand-in ->
unpack, shared by tests/test_p3_coupling.py and tests/test_p3_coupling_gpu.py.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os

import numpy as np

import emu_harness
import moist_surface_cases as mc
import p3_coupling_ref as ref
from pam_amd import capi
from pam_amd.physics import p3_shapes
from tools.native_build import emu_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DP = C.POINTER(C.c_double)
_PP = C.POINTER(C.c_void_p)
# (nz, ny, nx, nens): the SHOC list -- a partial tile on the column and on the level axis, one and several wavefronts, nens around 64,
# ny == 1, nz < 3
SHAPES = [(2, 1, 1, 1), (5, 1, 7, 3), (17, 3, 5, 13), (60, 2, 3, 65), (72, 1, 129, 1), (33, 2, 2, 130)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
EMU_STATE = ("rho_d", "rho_v", "rho_c", "temp", "nccn_prescribed", "nc_nuceat_tend", "ni_activated", "q_prev", "t_prev")
ADJUSTED = ("rho_v", "rho_c", "temp")
# the S_* order of p3_device.h as names of the state after unpack; q0 ... q6 are ref.TRACERS
S_ORDER = ("rho_c", "q0", "q1", "q2", "q3", "q4", "q5", "q6", "rho_v", "temp", "q_prev", "t_prev", "liq_ice_exchange_out",
           "vap_liq_exchange_out", "vap_ice_exchange_out")
STATE_AFTER = S_ORDER + ("precip_liq_surf_out", "precip_ice_surf_out")
# the gate of test_gpu_saturation_adjustment_matches_restatement (tests/moist_surface_cases.py: assert_adjusted_bits): bit for bit; cells
# whose bisection decision margin is below MARGIN are exempt (they get 2 tol in density and the matching dT).  On make_state no cell is
# (the smallest margin is 9.1e-10: test_the_seeds_keep_the_exempt_cells_of_the_device_gate_rare); EXEMPT_MAX, at most 0.5 % of the cells,
# is for the multi-step test, whose second state comes from the GPU.
MARGIN, MIN_MARGIN, EXEMPT_MAX = mc.MARGIN, mc.MIN_MARGIN, 0.005
same_bits = mc.same_bits


@functools.lru_cache(maxsize=None)
def make_state(shape, seed=0):
    """a coupler state that reaches every branch of the adjustment and of pack and, through the stand-in's switches, of unpack.  Returns a
    dict: the EMU_STATE arrays, "q" (list of the seven tracers), "zint" (nz+1,nens)"""
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(1000 * seed + 7 * nz + 3 * nx + nens)
    pick = lambda frac: rng.random(shape) < frac
    s = {"rho_d": rng.uniform(0.05, 1.3, shape), "temp": rng.uniform(230.0, 310.0, shape)}
    tc = s["temp"] - 273.15
    sat = 610.94 * np.exp(17.625 * tc / (243.04 + tc)) / (ref.CONSTS["R_v"] * s["temp"])                  # the saturation vapour density
    s["rho_v"] = np.where(pick(0.1), -rng.uniform(0.0, 1e-4, shape), sat * rng.uniform(0.3, 1.5, shape))    # sub- and super-saturated
    s["rho_c"] = np.where(pick(0.15), -rng.uniform(0.0, 1e-5, shape), rng.uniform(0.0, 2e-3, shape))        # negative cloud in
    s["rho_c"][pick(0.2)] = 0.0                                                                             # no cloud: nothing to evaporate
    s["rho_c"][pick(0.02)] = -0.0
    s["nccn_prescribed"] = rng.uniform(0.0, 1e8, shape)
    s["nc_nuceat_tend"] = rng.standard_normal(shape) * 10.0                                                 # < 0: the stand-in negates
    s["ni_activated"] = rng.standard_normal(shape) * 100.0                                                  # < 0: likewise
    s["q_prev"] = np.where(pick(0.1), -rng.uniform(0.0, 1e-4, shape), rng.uniform(0.0, 0.02, shape))
    s["t_prev"] = rng.uniform(190.0, 310.0, shape)
    s["q"] = [np.where(pick(0.15), -rng.uniform(0.0, 1e-5, shape), rng.uniform(0.0, 1e-3, shape)) * (1.0 + t) for t in range(7)]
    dz = np.linspace(80.0, 600.0, nz)[:, None] * (1.0 + 0.01 * np.arange(nens))[None, :]
    zint = np.concatenate([np.zeros((1, nens)), np.cumsum(dz, axis=0)]) + 25.0 * np.arange(nens)[None, :]   # members differ, zint(0) != 0
    s["zint"] = np.ascontiguousarray(zint)
    for v in list(s.values()) + s["q"]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def restated(state, adjust, first_step, pow=ref.libm_pow, consts=ref.CONSTS, num_tend_out=0):
    """(packed set, set after the stand-in, state after unpack as a dict of STATE_AFTER, the adjusted (rho_v, rho_c, temp), info) of the
    restatement, layout 0"""
    st = {k: state[k] for k in ref.STATE_4D}
    packed, adjusted, info = ref.pack(st, state["q"], state["zint"], adjust, first_step, consts, pow)
    after = ref.standin(packed, num_tend_out)
    out, q = ref.unpack(after, state["rho_d"], adjusted[2], None, consts)
    for t in range(7):
        out["q%d" % t] = q[t]
    return packed, after, out, dict(zip(ADJUSTED, adjusted)), info


@functools.lru_cache(maxsize=None)
def restated_case(shape, adjust, first_step):
    """the restated chain with the device's x^y, computed once per case and shared"""
    return restated(make_state(shape), adjust, first_step, pow=emu_harness.emu_pow)


# ------------------------------------------------------------------------------------------------------------------------------
# the host emulation

def emu():
    lib = C.CDLL(emu_library("p3_emu"))
    lib.emu_p3_offset.restype = C.c_longlong
    lib.emu_p3_offset.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.emu_p3_pack.restype = None
    lib.emu_p3_pack.argtypes = [C.POINTER(capi.P3Args), C.c_int, _PP, _PP, C.c_int, C.c_int, _DP, C.c_int, C.POINTER(C.c_int)]
    lib.emu_p3_standin.restype = None
    lib.emu_p3_standin.argtypes = [C.POINTER(capi.P3Args), C.c_int]
    lib.emu_p3_unpack.restype = None
    lib.emu_p3_unpack.argtypes = [C.POINTER(capi.P3Args), _DP, _PP, _PP, _DP, C.c_int]
    return lib


def _ptrs(arrays):
    for a in arrays:
        assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def host_args(ncol, nz, layout, num_tend_out=0):
    """(P3Args with host pointers, name -> array) with every element NaN"""
    arrays = {n: np.full(shp, np.nan) for n, shp in p3_shapes(ncol, nz, layout, num_tend_out).items()}
    a = capi.P3Args()
    a.ncol, a.nlev, a.dt, a.layout, a.num_tend_out = ncol, nz, 0.0, layout, num_tend_out
    for n, v in arrays.items():
        setattr(a, n, v.ctypes.data if v.size else None)
    return a, arrays


def emulated(state, layout, adjust, first_step, wide=False, consts=ref.CONSTS, num_tend_out=0):
    """(packed set, set after the stand-in, state after unpack, the adjusted (rho_v, rho_c, temp), iterations per cell) of the host
    emulation in `layout`"""
    lib = emu()
    shape = state["rho_d"].shape
    nz, ny, nx, nens = shape
    ncol = ny * nx * nens
    a, arrays = host_args(ncol, nz, layout, num_tend_out)
    st = [np.array(state[k], order="C") for k in EMU_STATE] + [np.array(state["zint"], order="C")]
    q = [np.array(x, order="C") for x in state["q"]]
    c = np.array([consts[k] for k in ("R_d", "R_v", "cp_d", "cp_v", "cp_l", "p0", "grav")])
    iters = np.zeros(shape, dtype=np.int32)
    lib.emu_p3_pack(C.byref(a), nens, _ptrs(st), _ptrs(q), int(adjust), int(first_step), c.ctypes.data_as(_DP), int(wide),
                    iters.ctypes.data_as(C.POINTER(C.c_int)))
    packed = {k: v.copy() for k, v in arrays.items()}
    adjusted = {k: st[EMU_STATE.index(k)].copy() for k in ADJUSTED}
    lib.emu_p3_standin(C.byref(a), int(wide))
    after = {k: v.copy() for k, v in arrays.items()}
    out = {"rho_c": st[2], "rho_v": st[1], "temp": st[3], "q_prev": st[7], "t_prev": st[8]}
    for t in range(7):
        out["q%d" % t] = q[t]
    for k in S_ORDER[-3:]:
        out[k] = np.full(shape, np.nan)
    surf = [np.full((ny, nx, nens), np.nan), np.full((ny, nx, nens), np.nan)]
    c2 = np.array([consts["cp_d"], consts["cv_d"]])
    lib.emu_p3_unpack(C.byref(a), np.ascontiguousarray(state["rho_d"]).ctypes.data_as(_DP), _ptrs([out[k] for k in S_ORDER]), _ptrs(surf),
                      c2.ctypes.data_as(_DP), int(wide))
    out["precip_liq_surf_out"], out["precip_ice_surf_out"] = surf
    return packed, after, out, adjusted, iters


def with_adjusted(state, adjusted):
    """the state with (rho_v, rho_c, temp) replaced"""
    s = dict(state)
    for k in ADJUSTED:
        s[k] = np.ascontiguousarray(adjusted[k])
    return s


def assert_set_equal(got, want, names=None, what=""):
    for n in names or sorted(want):
        assert same_bits(got[n], want[n]), (what, n)


def adjusted_within_gate(got, want, info, before):
    """the gate of test_gpu_saturation_adjustment_matches_restatement on the (rho_v, rho_c, temp) a pack left: an adjusted cell with a
    decision margin >= MARGIN equals the restatement bit for bit; cells below it are exempt and get 2 tol in density and the matching dT
    (rho >= 0.05 in make_state); cells in neither branch are unchanged bit for bit.  Returns the fraction of exempt cells."""
    return mc.assert_adjusted_bits(got, want, info, before, rho_min=0.05) / info["branch"].size
