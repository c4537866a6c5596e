"""The Kessler device bodies (pam_amd/csrc/kessler_device.h) without a GPU: the host emulation tests/emu/kessler_emu.cpp (g++ -O2
-ffp-contract=off) against the oracle, cell by cell (tests/kessler_cases.py), on states that reach every branch of the scheme.

  * the oracle's branch census of every named case: every counter reached, the rain-free shortcut divergent in at least half of the
    wavefronts, and the oracle's own noise floor small enough for the gate to come out at 1e-12;
  * the emulated column body against the oracle through the per-cell gate -- not bit for bit: the bodies use pow_pos_fast, the
    pressure in place of pk^(cp/Rd) in a first sub-cycle and reciprocal forms, the oracle glibc's pow and divisions;
  * the four template instances against each other bit for bit (the C ABI never runs <false, IDX> at one sub-cycle);
  * the emulated time-step limit against the oracle's sub-cycle count, and a state whose every fall speed is below 1e-10;
  * the gate itself: 1e-10 relative in one trace-rain cell turns it red where 1e-12 x max|field| stays green."""
import ctypes as C
import functools

import numpy as np
import pytest

import kessler_cases as kc
import test_micro_kessler as tk
from pam_amd.micro import Microphysics
from tools.native_build import emu_library

_DP = C.POINTER(C.c_double)
INSTANCES = {"single_u32": (1, 0), "single_i64": (1, 1), "multi_u32": (0, 0), "multi_i64": (0, 1)}   # (single, wide)


@functools.lru_cache(maxsize=None)
def emu():
    lib = C.CDLL(emu_library("kessler_emu"))
    lib.emu_kessler_max_stable_dt.argtypes = [C.c_int] * 4 + [_DP] * 3 + [C.c_double, C.c_int, _DP]
    lib.emu_kessler_columns.argtypes = [C.c_int] * 4 + [_DP] * 8 + [C.c_double, C.c_int] + [C.c_double] * 4 + [C.c_int] * 2
    return lib


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def emu_dt_max(s, zm, dt, level_step=1):
    """(status, dt_max) of the emulated pam_amd_kessler_max_stable_dt"""
    nz, ny, nx, nens = s["temp"].shape
    out = C.c_double()
    zm = np.ascontiguousarray(zm, dtype=np.float64)
    rc = emu().emu_kessler_max_stable_dt(nens, nx, ny, nz, _p(s["rho_r"]), _p(s["rho_dry"]), _p(zm), dt, level_step, C.byref(out))
    return rc, out.value


def emu_columns(s, zm, dt, n, instance):
    """a copy of `s` advanced by the emulated column kernel of that template instance at n sub-cycles, precl included"""
    nz, ny, nx, nens = s["temp"].shape
    o = {k: v.copy() for k, v in s.items()}
    o["precl"] = np.full((ny, nx, nens), np.nan)
    exner = np.full(s["temp"].shape, np.nan)
    zm = np.ascontiguousarray(zm, dtype=np.float64)
    single, wide = INSTANCES[instance]
    rc = emu().emu_kessler_columns(nens, nx, ny, nz, _p(o["rho_v"]), _p(o["rho_c"]), _p(o["rho_r"]), _p(o["rho_dry"]), _p(o["temp"]),
                                   _p(o["precl"]), _p(zm), _p(exner), dt, n, kc.C0["R_d"], kc.C0["R_v"], kc.C0["cp_d"], kc.C0["p0"],
                                   single, wide)
    assert rc == 0
    assert np.array_equal(o["rho_dry"], s["rho_dry"])
    return o


def emu_time_step(s, zm, dt, forced=0):
    """pam_amd_kessler_time_step as the C ABI runs it: the limit unless a count is forced, then the instance the count selects"""
    n = forced
    if n <= 0:
        rc, dt_max = emu_dt_max(s, zm, dt)
        assert rc == 0
        n = Microphysics.rainsplit_for(dt, dt_max)
    return emu_columns(s, zm, dt, n, "single_u32" if n == 1 else "multi_u32"), n


@functools.lru_cache(maxsize=None)
def _named(i):
    """inputs, the oracle's run with its census, and the oracle's floor of named case i (shared by the tests below)"""
    zi, zm, s, dt, forced = kc.named_state(kc.NAMED[i])
    exp, n, census = kc.run_oracle(s, zm, dt, rainsplit=forced, census=True)
    floor = kc.oracle_floor(s, zm, dt, exp, n)
    return zm, s, dt, forced, exp, n, census, floor


NAMED_IDX = pytest.mark.parametrize("i", range(len(kc.NAMED)), ids=kc.NAMED_IDS)


# ------------------------------------------------------------------------------------------------------------------------------
# the states: branch census, divergence, floor

def test_census_entry_point_shares_the_body():
    """the census run returns what the plain entry point returns, bit for bit"""
    zm, s, dt, forced, exp, n, census, _ = _named(1)
    plain, n2 = kc.run_oracle(s, zm, dt, rainsplit=forced)
    assert n2 == n
    for k in kc.FIELDS:
        assert np.array_equal(plain[k], exp[k]), k
    assert sum(census.values()) > 0


@NAMED_IDX
def test_named_case_reaches_every_branch(i):
    zm, s, dt, forced, exp, n, census, floor = _named(i)
    variant = kc.NAMED[i][2][0]
    assert (n == 1) if variant != "dt60" else (n >= 2), n
    for k in kc.FIELDS:
        assert np.isfinite(exp[k]).all(), k
    for k in kc.WATER:
        assert exp[k].min() >= 0, k
    # the sedimentation of one stable sub-cycle cannot take more than the cell holds: the clamp of qr at zero needs the forced count
    reachable = {name: True for name in census}
    reachable["qr_clamped"] = variant == "dt60_forced1"
    for name, count in census.items():
        if reachable[name]:
            assert count >= 1, (name, census)
        else:
            assert count == 0, (name, census)
    assert kc.mixed_wavefront_fraction(s["rho_r"]) >= 0.5
    # a case whose own physics amplifies one ulp of T beyond this is no input for a 1e-12 gate
    for k in kc.FIELDS:
        assert floor[k] <= kc.FLOOR_MAX, (k, floor)
    assert set(kc.tolerances(floor).values()) == {1e-12}, floor


def test_saturation_limited_evaporation_is_reached_often_enough():
    """tmp2 (rain evaporation ends where the cell saturates) is the rarest bound of the three"""
    total = sum(_named(i)[6]["ern_limited_by_tmp2"] for i in range(len(kc.NAMED)))
    assert total >= 20, total


def test_smooth_case_misses_branches():
    """the census of the suite's older, smooth case (test_micro_kessler._case): the reason for kessler_cases.state()"""
    for heavy, dt in ((False, 5.0), (True, 60.0)):
        zint, zi, zm, s = tk._case(nens=70, nx=6, ny=2, nz=30, heavy_rain=heavy)
        _, _, census = kc.run_oracle(s, zm, dt, census=True)
        for name in ("ern_limited_by_qr", "qr_clamped", "rain_free_cell_receives_sediment", "slow_fall_speed"):
            assert census[name] == 0, (name, census)
        assert kc.mixed_wavefront_fraction(s["rho_r"]) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the device bodies on the host against the oracle

@NAMED_IDX
def test_emulation_matches_oracle_named(i):
    zm, s, dt, forced, exp, n, census, floor = _named(i)
    got, n_emu = emu_time_step(s, zm, dt, forced)
    assert n_emu == n
    kc.gate(got, exp, s, kc.tolerances(floor), kc.NAMED_IDS[i], case="kessler_emu_" + kc.NAMED_IDS[i], floor=floor)


def _sweep_case(seed):
    rng = np.random.default_rng(4001 * seed + 17)
    nens = int(rng.choice([1, 2, 3, 7, 16, 33, 64, 65, 70, 128]))
    nx, ny, nz = int(rng.integers(1, 12)), int(rng.choice([1, 1, 2, 3])), int(rng.integers(4, 61))
    while nens * nx * ny * nz > 60000:
        nx = max(1, nx // 2)
    dt = float(rng.choice([1.0, 5.0, 30.0, 60.0]))
    forced = int(rng.choice([0, 0, 1, 4]))
    return nens, nx, ny, nz, dt, forced


@pytest.mark.parametrize("seed", range(16))
def test_emulation_matches_oracle_sweep(seed):
    """seeded shapes x state seeds x steps (free and forced sub-cycle counts)"""
    nens, nx, ny, nz, dt, forced = _sweep_case(seed)
    zi, zm, s = kc.state(nens, nx, ny, nz, 100 + seed)
    what = "seed %d: nens %d, %dx%dx%d, dt %g, forced %d" % (seed, nens, nx, ny, nz, dt, forced)
    got, n = emu_time_step(s, zm, dt, forced)
    exp, n_ref = kc.run_oracle(s, zm, dt, rainsplit=forced)
    assert n == n_ref, what
    kc.gate_against_oracle(got, s, zm, dt, n, what)


@pytest.mark.parametrize("heavy,dt", [(False, 5.0), (True, 60.0)])
def test_emulation_matches_oracle_smooth_case(heavy, dt):
    zint, zi, zm, s = tk._case(nens=70, nx=6, ny=2, nz=30, heavy_rain=heavy)
    got, n = emu_time_step(s, zm, dt)
    exp, _ = kc.gate_against_oracle(got, s, zm, dt, n, "smooth")
    for k in kc.FIELDS:      # and the max-norm gate of the GPU test
        assert np.abs(got[k] - exp[k]).max() <= 1e-12 * np.abs(exp[k]).max(), k


# ------------------------------------------------------------------------------------------------------------------------------
# the template instances

@NAMED_IDX
def test_instances_agree_bit_for_bit(i):
    zm, s, dt, forced, exp, n, census, floor = _named(i)
    names = list(INSTANCES) if n == 1 else ["multi_u32", "multi_i64"]
    runs = [emu_columns(s, zm, dt, n, inst) for inst in names]
    for inst, r in zip(names[1:], runs[1:]):
        for k in kc.FIELDS:
            assert np.array_equal(r[k], runs[0][k]), (inst, k)


def test_single_instance_refuses_a_sub_cycled_run():
    zm, s, dt, forced, exp, n, census, floor = _named(0)
    nz, ny, nx, nens = s["temp"].shape
    o = {k: v.copy() for k, v in s.items()}
    precl = np.zeros((ny, nx, nens))
    ex = np.zeros(s["temp"].shape)
    zmc = np.ascontiguousarray(zm)
    assert emu().emu_kessler_columns(nens, nx, ny, nz, _p(o["rho_v"]), _p(o["rho_c"]), _p(o["rho_r"]), _p(o["rho_dry"]), _p(o["temp"]),
                                     _p(precl), _p(zmc), _p(ex), dt, 2, 287.0, 461.0, 1003.0, 1e5, 1, 0) == -1
    for k in s:
        assert np.array_equal(o[k], s[k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# the time-step limit

@NAMED_IDX
def test_emulated_limit_gives_the_oracles_rainsplit(i):
    zi, zm, s, dt, _ = kc.named_state(kc.NAMED[i])
    _, n_ref = kc.run_oracle(s, zm, dt)
    before = {k: v.copy() for k, v in s.items()}
    for level_step in (1, 3, s["temp"].shape[0] - 1):        # however the levels are dealt to workgroups
        rc, dt_max = emu_dt_max(s, zm, dt, level_step)
        assert rc == 0 and 0 < dt_max <= dt
        assert Microphysics.rainsplit_for(dt, dt_max) == n_ref, (level_step, dt_max)
    for k in s:
        assert np.array_equal(s[k], before[k]), k


@pytest.mark.parametrize("dt", [5.0, 60.0])
def test_limit_of_a_state_without_fall_speed_is_dt(dt):
    zi, zm, s = kc.state(65, 5, 2, 24, 9, rain="slow")
    assert np.count_nonzero(s["rho_r"]) > 0
    _, n, census = kc.run_oracle(s, zm, dt, census=True)
    assert n == 1 and census["slow_fall_speed"] == np.count_nonzero(s["rho_r"][:-1])
    rc, dt_max = emu_dt_max(s, zm, dt)
    assert rc == 0 and dt_max == dt
    got, n_emu = emu_time_step(s, zm, dt)
    assert n_emu == 1
    kc.gate_against_oracle(got, s, zm, dt, 1, "slow")


@pytest.mark.parametrize("bad", ["nan_rain", "negative_rain", "nan_density"])
def test_emulated_limit_refuses_an_unusable_state(bad):
    """the value the C ABI turns into PAM_AMD_ESTATE: the limit is not positive"""
    zi, zm, s = kc.state(7, 3, 2, 12, 3)
    cell = (5, 1, 2, 4)
    if bad == "nan_rain":
        s["rho_r"][cell] = np.nan
    elif bad == "negative_rain":
        s["rho_r"][cell] = -1e-6
    else:
        s["rho_dry"][cell] = np.nan
    for level_step in (1, 4):
        rc, dt_max = emu_dt_max(s, zm, 5.0, level_step)
        assert rc == -1 and dt_max == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the gate

def test_per_cell_gate_sees_what_the_max_norm_gate_misses():
    zm, s, dt, forced, exp, n, census, floor = _named(kc.NAMED_IDS.index("n70_6x3x30_dt5"))
    tol = kc.tolerances(floor)
    kc.gate(exp, exp, s, tol)
    S = kc.cell_scale(s)
    # a trace of rain by the field's measure (below 1e-3 of its maximum) that is no trace by the cell's own (2% of all the water that
    # can reach it): the upper levels, where the vapour is four decades below the ground's
    trace = (exp["rho_r"] > 2e-2 * S) & (exp["rho_r"] < 1e-3 * exp["rho_r"].max())
    assert trace.any()
    cell = tuple(np.argwhere(trace)[0])
    bad = {k: v.copy() for k, v in exp.items()}
    bad["rho_r"][cell] *= 1 + 1e-10
    assert np.abs(bad["rho_r"] - exp["rho_r"]).max() <= 1e-12 * np.abs(exp["rho_r"]).max()      # today's gate passes
    with pytest.raises(AssertionError):
        kc.gate(bad, exp, s, tol)
