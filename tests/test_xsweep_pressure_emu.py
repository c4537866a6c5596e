"""CPU: the stash parameter of flux_x_update_body leaves the host emulation as it was, and the in-sweep pressure computes the
separate pass's bits.  tests/emu/xsweep_pressure_emu.cpp holds all of tests/emu/awfl_emu.cpp plus the fused stage with the pressure
pass inside the x-sweep (LineStash + xsweep_pressure_epilogue); three runs per shape, all array_equal:
  the harness's own library (flux_x_update_body without a stash argument, pressure_tail_body as a pass of its own),
  the same entry point of the library that has the stash compiled in,
  that library's in-sweep form."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import emu_harness as eh
from pam_amd import idealized as idz
from parity_cases import build_inputs
from tools.native_build import emu_library

_HERE = os.path.dirname(os.path.abspath(__file__))
_DP = C.POINTER(C.c_double)
NZ = 4
FIELDS = ("density_dry", "uvel", "vvel", "wvel", "temp", "tracers")
# (nens, nx, ny, span, mode_a, per-member grid, limited vapour): two of tests/test_xsweep_pressure_gpu.py's shapes, fewer members
SHAPES = {
    "nx32_3d_span4_limited": (3, 32, 5, 4, True, False, True),
    "nx3_2d_whole_perens_B": (2, 3, 1, 0, False, True, False),
    # dx != dy with the sounding's shear along y (an eighth element: options of parity_cases.build_inputs)
    "aniso_800x500_nx9_3d_span4_limited_flowy": (3, 9, 5, 4, True, False, True, dict(dxy=800.0, dy=500.0, flow="y")),
    "aniso_500x800_nx6_3d_whole_perens_B_flowy": (2, 6, 5, 0, False, True, False, dict(dxy=500.0, dy=800.0, flow="y")),
}


@pytest.fixture(scope="module")
def lib():
    so = C.CDLL(emu_library("xsweep_pressure_emu"))
    ref = eh.load()
    for name in ("emu_init", "emu_destroy", "emu_set_grav_balance", "emu_set_span", "emu_set_fused", "emu_buffer", "emu_declare_hydrostatic",
                 "emu_time_step"):
        getattr(so, name).restype = getattr(ref, name).restype
        getattr(so, name).argtypes = getattr(ref, name).argtypes
    so.emu_time_step_xsweep_pressure.restype = C.c_int
    so.emu_time_step_xsweep_pressure.argtypes = ref.emu_time_step.argtypes
    return so


class _Emu(eh.EmuDycore):
    """EmuDycore on another build of the emulation"""

    def __init__(self, so, *args, **kw):
        load, eh.load = eh.load, lambda: so
        try:
            super().__init__(*args, **kw)
        finally:
            eh.load = load

    def time_step_xsweep_pressure(self, f, crm_dt):
        out = C.c_double(0)
        return self.lib.emu_time_step_xsweep_pressure(self.h, *self._f(f), float(crm_dt), 0.0, C.byref(out))


def _inputs(shape):
    nens, nx, ny, span, mode_a, per_ens, limited = SHAPES[shape][:7]
    tr = idz.TRACERS_NONE
    zint = idz.stretched_interfaces(NZ, 6000.0)
    f, xlen, ylen, _, _ = build_inputs(nens, nx, ny, NZ, tr, zint, mag=0.5, dry_air=limited,
                                       **(SHAPES[shape][7] if len(SHAPES[shape]) > 7 else {}))
    dz = np.diff(zint)[:, None] * np.ones((1, nens))
    if per_ens:
        dz = dz * (1 + 0.01 * np.arange(nens))[None, :]
    _, pos, mass, idwv = idz.tracer_flags(tr)
    return (nens, nx, ny, NZ, xlen, ylen, dz, pos, mass, idwv), f


def _run(make, args, f, shape, in_sweep):
    nens, nx, ny, span, mode_a = SHAPES[shape][:5]
    ff = copy.deepcopy(f)
    d = make(*args)
    d.set_grav_balance(mode_a)
    d.set_fused(True)
    d.set_span(span)
    d.declare_current_profile_as_hydrostatic(ff)
    ncyc = []
    for crm_dt in (2.0, 0.7):           # odd and even sub-step counts
        ncyc.append(d.time_step_xsweep_pressure(ff, crm_dt) if in_sweep else d.time_step(ff, crm_dt)[0])
    # the resident state with its ghost levels and the next stage's pressure (field 5 of prim0), bytes and all
    prim = np.array(d.buffer("prim0", (6 + 1, NZ + 6, ny, nx, nens)))
    return ncyc, ff, prim


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_stash_parameter_leaves_the_emulation_unchanged_and_in_sweep_pressure_has_the_same_bits(lib, shape):
    args, f = _inputs(shape)
    n0, a, pa = _run(eh.EmuDycore, args, f, shape, False)
    n1, b, pb = _run(lambda *x: _Emu(lib, *x), args, f, shape, False)
    n2, c, pc = _run(lambda *x: _Emu(lib, *x), args, f, shape, True)
    assert n0 == n1 == n2 and min(n0) > 0
    for k in FIELDS:
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], c[k]), (k, np.abs(a[k] - c[k]).max())
    assert np.isfinite(pa[5, 3:-3]).all()
    assert np.array_equal(pa, pb, equal_nan=True)
    assert np.array_equal(pa, pc, equal_nan=True)


@pytest.mark.parametrize("shape", sorted(k for k in SHAPES if len(SHAPES[k]) > 7))
def test_in_sweep_pressure_matches_the_oracle_on_an_anisotropic_grid(lib, shape):
    """the bit-equality above holds a y difference divided by dx too (every build has it); here the in-sweep form is held to the
    oracle through the parity gate (tests/parity_gate.py) at dx != dy with the shear along y"""
    from oracle import awfl_oracle as ao
    from parity_gate import compare, noise_floor
    args, f = _inputs(shape)
    mode_a = SHAPES[shape][4]
    assert args[5] / args[2] != args[4] / args[1] and np.abs(f["vvel"]).max() >= 0.5 * np.abs(f["uvel"]).max()
    ncyc, got, _ = _run(lambda *x: _Emu(lib, *x), args, f, shape, True)

    def run_oracle(ff):
        o = ao.OracleDycore(*args)
        o.set_grav_balance(mode_a)
        o.declare_current_profile_as_hydrostatic(ff)
        return [o.time_step(ff, crm_dt)[0] for crm_dt in (2.0, 0.7)]
    exp = copy.deepcopy(f)
    assert run_oracle(exp) == ncyc
    names = idz.tracer_flags(idz.TRACERS_NONE)[0]
    compare(got, exp, names, sum(ncyc), floor=noise_floor(run_oracle, f, names, 0, base=exp))


def test_in_sweep_pressure_is_refused_where_the_device_keeps_the_separate_pass(lib):
    """a span longer than the stash"""
    nens, nx, ny = 1, 33, 1
    zint = idz.stretched_interfaces(NZ, 6000.0)
    f = idz.supercell_fields(nens, nx, ny, NZ, zint, tracers=idz.TRACERS_NONE, magnitude=0.5)
    _, pos, mass, idwv = idz.tracer_flags(idz.TRACERS_NONE)
    d = _Emu(lib, nens, nx, ny, NZ, nx * 500.0, nx * 500.0, np.diff(zint), pos, mass, idwv)
    d.set_fused(True)
    d.declare_current_profile_as_hydrostatic(f)
    assert d.time_step_xsweep_pressure(f, 2.0) == -1
