"""States for the SHOC coupling tests, the binding of the host emulation (tests/emu/shoc_emu.cpp) and the restated chain pack -> stand-in ->
unpack, shared by tests/test_shoc_coupling.py and tests/test_shoc_coupling_gpu.py.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools
import os

import numpy as np

import emu_harness
import shoc_coupling_ref as ref
from pam_amd import capi
from pam_amd.physics import shoc_shapes
from tools.native_build import emu_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DP = C.POINTER(C.c_double)
_PP = C.POINTER(C.c_void_p)
XLEN, YLEN = 16000.0, 12000.0
# (nz, ny, nx, nens): a partial tile on the column and on the level axis, one and several wavefronts, nens around 64, ny == 1
SHAPES = [(2, 1, 1, 1), (5, 1, 7, 3), (17, 3, 5, 13), (60, 2, 3, 65), (72, 1, 129, 1), (33, 2, 2, 130)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
TRACER_SETS = {"kessler": ref.KESSLER_TRACERS, "p3": ref.P3_TRACERS}
EMU_STATE = ("rho_d", "rho_v", "rho_c", "uvel", "vvel", "wvel", "temp", "tke", "wthv_sec", "tk", "tkh", "cldfrac")
UNPACKED = ("temp", "rho_v", "rho_c", "uvel", "vvel", "tke", "wthv_sec", "tk", "tkh", "cldfrac", "inv_qc_relvar")


def same_bits(a, b):
    """NaN in the same places, every other element equal bit for bit (the signs of zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(np.where(np.isnan(a), 0.0, a).view(np.uint64), np.where(np.isnan(b), 0.0, b).view(np.uint64))


@functools.lru_cache(maxsize=None)
def make_state(shape, ntr, seed=0):
    """a coupler state that reaches every branch of pack and, through the stand-in's switches, of unpack.  Returns a dict: the STATE_4D
    arrays, "q" (list of ntr tracers), "flx_u", "flx_v" (ny,nx,nens), "zint" (nz+1,nens), "zmid" (nz,nens)"""
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(1000 * seed + 7 * nz + 3 * nx + nens + ntr)
    n = nz * ny * nx * nens
    pick = lambda frac: rng.random(shape) < frac
    s = {"rho_d": rng.uniform(0.05, 1.3, shape), "temp": rng.uniform(190.0, 310.0, shape)}
    s["rho_v"] = np.where(pick(0.15), -rng.uniform(0.0, 1e-4, shape), rng.uniform(0.0, 0.02, shape))        # negative vapour in
    s["rho_c"] = np.where(pick(0.15), -rng.uniform(0.0, 1e-5, shape), rng.uniform(0.0, 1e-3, shape))        # negative cloud in
    s["rho_c"][pick(0.1)] = 0.0
    for k in ("uvel", "vvel", "wvel"):
        s[k] = rng.standard_normal(shape) * 5.0
    s["tke"] = np.where(pick(0.3), rng.uniform(0.0, 1e-3, shape), rng.uniform(0.01, 2.0, shape))            # tke / rho below the 0.004 floor
    s["wthv_sec"] = rng.standard_normal(shape) * 0.1                                                        # < 0: the stand-in zeroes ql
    s["tk"] = np.where(pick(0.25), -rng.uniform(0.1, 5.0, shape), rng.uniform(0.0, 50.0, shape))            # < 0: it negates qw and the tracers
    s["tkh"] = rng.uniform(0.0, 50.0, shape)
    s["cldfrac"] = rng.uniform(0.0, 1.0, shape)                                                             # picks ql2 and leaves as 3 x - 1
    s["q"] = [np.where(pick(0.15), -rng.uniform(0.0, 1e-5, shape), rng.uniform(0.0, 1e-3, shape)) * (1.0 + t) for t in range(ntr)]
    s["flx_u"], s["flx_v"] = rng.standard_normal((ny, nx, nens)) * 0.05, rng.standard_normal((ny, nx, nens)) * 0.05
    dz = np.linspace(80.0, 600.0, nz)[:, None] * (1.0 + 0.01 * np.arange(nens))[None, :]
    zint = np.concatenate([np.zeros((1, nens)), np.cumsum(dz, axis=0)]) + 25.0 * np.arange(nens)[None, :]   # members differ, zint(0) != 0
    s["zint"] = np.ascontiguousarray(zint)
    s["zmid"] = np.ascontiguousarray(0.5 * (zint[1:] + zint[:-1]))
    assert n == s["rho_d"].size
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def restated(state, pow=ref.libm_pow, consts=ref.CONSTS):
    """(packed set, set after the stand-in, state after unpack, tracers after unpack) of the restatement, layout 0"""
    st = {k: state[k] for k in ref.STATE_4D}
    packed = ref.pack(st, state["q"], state["flx_u"], state["flx_v"], state["zint"], state["zmid"], XLEN, YLEN, consts, pow)
    after = ref.standin(packed)
    out, q = ref.unpack(after, st, state["q"], consts)
    return packed, after, out, q


@functools.lru_cache(maxsize=None)
def restated_case(shape, ntr):
    """the restated chain with the device's x^y, computed once per case and shared"""
    return restated(make_state(shape, ntr), pow=emu_harness.emu_pow)


# ------------------------------------------------------------------------------------------------------------------------------
# the host emulation

def emu():
    lib = C.CDLL(emu_library("shoc_emu"))
    lib.emu_shoc_offset.restype = C.c_longlong
    lib.emu_shoc_offset.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.emu_shoc_pack.restype = None
    lib.emu_shoc_pack.argtypes = [C.POINTER(capi.ShocArgs), C.c_int, _PP, _PP, C.c_double, C.c_double, _DP]
    lib.emu_shoc_standin.restype = None
    lib.emu_shoc_standin.argtypes = [C.POINTER(capi.ShocArgs), C.c_int]
    lib.emu_shoc_unpack.restype = None
    lib.emu_shoc_unpack.argtypes = [C.POINTER(capi.ShocArgs), _DP, _PP, _PP, _DP]
    return lib


def _ptrs(arrays):
    for a in arrays:
        assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def host_args(ncol, nz, ntr, layout):
    """(ShocArgs with host pointers, name -> array) with every element NaN"""
    arrays = {n: np.full(shp, np.nan) for n, shp in shoc_shapes(ncol, nz, ntr, layout).items()}
    a = capi.ShocArgs()
    a.ncol, a.nlev, a.nlevi, a.dt, a.nadv, a.num_qtracers, a.layout = ncol, nz, nz + 1, 0.0, 1, ntr, layout
    for n, v in arrays.items():
        setattr(a, n, v.ctypes.data)
    return a, arrays


def emulated(state, layout, wide=False, consts=ref.CONSTS):
    """(packed set, set after the stand-in, state after unpack, tracers after unpack) of the host emulation in `layout`"""
    lib = emu()
    nz, ny, nx, nens = state["rho_d"].shape
    ncol, ntr = ny * nx * nens, len(state["q"])
    a, arrays = host_args(ncol, nz, ntr, layout)
    st = [np.ascontiguousarray(state[k]) for k in EMU_STATE] + [np.ascontiguousarray(state[k]) for k in ("flx_u", "flx_v", "zint", "zmid")]
    q = [np.ascontiguousarray(x) for x in state["q"]]
    dx = XLEN / nx
    dy = dx if ny == 1 else YLEN / ny
    c = np.array([consts[k] for k in ("p0", "grav", "R_d", "cp_d", "latvap", "pres_R_d", "pres_R_v")])
    lib.emu_shoc_pack(C.byref(a), nens, _ptrs(st), _ptrs(q), dx, dy, c.ctypes.data_as(_DP))
    packed = {k: v.copy() for k, v in arrays.items()}
    lib.emu_shoc_standin(C.byref(a), int(wide))
    after = {k: v.copy() for k, v in arrays.items()}
    out = {k: np.array(state[k], copy=True) if k in state else np.full(state["rho_d"].shape, np.nan) for k in UNPACKED}
    q_out = [x.copy() for x in q]
    c2 = np.array([consts[k] for k in ("cp_d", "cv_d", "latvap")])
    lib.emu_shoc_unpack(C.byref(a), np.ascontiguousarray(state["rho_d"]).ctypes.data_as(_DP), _ptrs([out[k] for k in UNPACKED]), _ptrs(q_out),
                        c2.ctypes.data_as(_DP))
    return packed, after, out, q_out


def assert_set_equal(got, want, names=None, what=""):
    for n in names or sorted(want):
        assert same_bits(got[n], want[n]), (what, n)
