"""Kessler microphysics ("next row" N4; physics/micro/kessler/Microphysics.h): oracle properties
on CPU, HIP-vs-oracle parity on the GPU.  The scheme is floating point with pow/exp; the device's libm differs from
glibc in the last place, so the parity tolerance is 1e-12 relative (written in the test), not bit-exact: of the field's maximum
on the smooth case below, and cell by cell -- 1e-12 of the water that is in a cell or can fall into it -- on every case, the smooth
one and the states of tests/kessler_cases.py that reach every branch (the host emulation of the same bodies: tests/test_kessler_emu.py)."""
import numpy as np
import pytest

import kessler_cases as kc
from oracle import awfl_oracle as ao
from pam_amd import idealized as idz

C0 = kc.C0   # the scheme's own constants (Microphysics.h:66-71)


def _case(nens=3, nx=6, ny=2, nz=30, heavy_rain=False):
    zint = idz.stretched_interfaces(nz, 15000.0)
    zi = zint[:, None] * (1 + 0.01 * np.arange(nens))[None, :]
    zm = 0.5 * (zi[:-1] + zi[1:])
    f = idz.supercell_fields(nens, nx, ny, nz, zint, magnitude=1.0)
    rho_d, T = f["density_dry"], f["temp"]
    rv = np.ascontiguousarray(f["tracers"][0]) * (1.0 + 0.6 * np.cos(np.arange(nx))[None, None, :, None] ** 2)
    rc = np.zeros_like(rv); rr = np.zeros_like(rv)
    rc[3:9] = 1.5e-3 * rho_d[3:9] * (1 + np.sin(np.arange(nens)))[None, None, None, :] ** 2
    rr[0:12] = (8e-3 if heavy_rain else 1e-3) * rho_d[0:12] * (0.5 + np.cos(np.arange(nx))[None, None, :, None] ** 2)
    return zint, zi, zm, dict(rho_v=rv, rho_c=rc, rho_r=rr, rho_dry=np.ascontiguousarray(rho_d), temp=np.ascontiguousarray(T))


def _water(s, zi):
    dz = np.diff(zi, axis=0)[:, None, None, :]
    return ((s["rho_v"] + s["rho_c"] + s["rho_r"]) * dz).sum(axis=0)


def test_oracle_kessler_properties():
    zint, zi, zm, s = _case()
    w0 = _water(s, zi); T0 = s["temp"].copy()
    dt = 5.0
    precl, n = ao.kessler(s["rho_v"], s["rho_c"], s["rho_r"], s["rho_dry"], s["temp"], zm, dt, C0)
    assert n >= 1 and precl.shape == w0.shape
    for k in ("rho_v", "rho_c", "rho_r"):
        assert np.all(s[k] >= 0) and np.all(np.isfinite(s[k]))
    assert precl.min() >= 0 and precl.max() > 0
    # column water budget: what left the column fell out of the bottom (precl is m/s of water at 1000 kg/m3).  The top
    # level's one-sided sedimentation (:400) is not in flux form, so the budget closes only to that term's size.
    w1 = _water(s, zi)
    assert np.all(w1 <= w0 * (1 + 1e-12))
    # sedimentation is not in flux form over non-uniform dz (it divides by the midpoint spacing, :403), so the
    # budget closes to the grid-stretching error, not to round-off
    assert np.abs((w0 - w1) - precl * 1000.0 * dt).max() < 0.15 * (precl * 1000.0 * dt).max()
    # latent heating where cloud condensed, cooling where rain evaporated: bounded temperature change
    assert 0 < np.abs(s["temp"] - T0).max() < 10.0


def test_oracle_kessler_subcycles_when_rain_is_fast():
    zint, zi, zm, s = _case(heavy_rain=True)
    import copy
    s2 = copy.deepcopy(s)
    dt = 60.0
    precl, n = ao.kessler(s["rho_v"], s["rho_c"], s["rho_r"], s["rho_dry"], s["temp"], zm, dt, C0)
    assert n >= 2
    # forcing the same count reproduces the run bit for bit; a different count does not
    precl2, n2 = ao.kessler(s2["rho_v"], s2["rho_c"], s2["rho_r"], s2["rho_dry"], s2["temp"], zm, dt, C0, rainsplit=n)
    assert n2 == n and np.array_equal(precl, precl2) and np.array_equal(s["temp"], s2["temp"])


COUPLER_NAMES = (("water_vapor", "rho_v"), ("cloud_liquid", "rho_c"), ("precip_liquid", "rho_r"), ("density_dry", "rho_dry"),
                 ("temp", "temp"))


def _gpu_setup(s, zi, nens, nx, ny, nz, dt):
    """a coupler on the GPU that holds the state `s`, and the plug-in initialised on it"""
    import torch
    from pam_amd import PamCoupler, Microphysics
    coupler = PamCoupler("cuda:0")
    coupler.set_option("crm_dt", dt)
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(nx * 500.0, ny * 500.0, zi)
    micro = Microphysics()
    micro.init(coupler)
    assert coupler.get_tracer_names() == ["water_vapor", "cloud_liquid", "precip_liquid"]
    assert coupler.get_option("micro") == "kessler" and coupler.get_option("cp_d") == 1003.0
    dm = coupler.get_data_manager_device_readwrite()
    assert float(dm.get("water_vapor").abs().max()) == 0.0
    for name, key in COUPLER_NAMES:
        dm.get(name).copy_(torch.from_numpy(s[key]))
    return coupler, micro, dm


def _gpu_run(s, zi, nens, nx, ny, nz, dt, rainsplit=0):
    import torch
    coupler, micro, dm = _gpu_setup(s, zi, nens, nx, ny, nz, dt)
    dt_max = micro.max_stable_dt(coupler)
    out = {}
    dirty = coupler.run_module("micro", lambda c: out.setdefault("n", micro.timeStep(c, rainsplit)))
    torch.cuda.synchronize()
    assert "temp" in dirty and "precl" in dirty
    got = {key: dm.get(name).cpu().numpy() for name, key in (("water_vapor", "rho_v"), ("cloud_liquid", "rho_c"),
                                                              ("precip_liquid", "rho_r"), ("temp", "temp"), ("precl", "precl"))}
    return got, out["n"], dt_max, micro


@pytest.mark.gpu
@pytest.mark.parametrize("heavy,dt,ny", [(False, 5.0, 2), (True, 60.0, 1), (True, 60.0, 3)])
def test_gpu_kessler_matches_oracle(heavy, dt, ny):
    nens, nx, nz = 70, 6, 30
    zint, zi, zm, s = _case(nens=nens, nx=nx, ny=ny, nz=nz, heavy_rain=heavy)
    s_in = {k: v.copy() for k, v in s.items()}
    got, n, dt_max, micro = _gpu_run(s, zi, nens, nx, ny, nz, dt)
    precl, n_ref = ao.kessler(s["rho_v"], s["rho_c"], s["rho_r"], s["rho_dry"], s["temp"], zm, dt, C0)
    assert n == n_ref and n == micro.rainsplit_for(dt, dt_max)
    if heavy:
        assert n >= 2
    s["precl"] = precl
    tol = 1e-12   # relative to the field's maximum: device pow/exp differ from glibc in the last place
    for k in got:
        assert np.abs(got[k] - s[k]).max() <= tol * np.abs(s[k]).max(), k
    # and cell by cell (tests/kessler_cases.py)
    kc.gate_against_oracle(got, s_in, zm, dt, n, "smooth", case="kessler_gpu_smooth_heavy%d_dt%g_ny%d" % (heavy, dt, ny))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(kc.NAMED)), ids=kc.NAMED_IDS)
def test_gpu_kessler_named_cases_match_oracle_cell_by_cell(i):
    """the states that reach every branch of the scheme and mix rainy and rain-free lanes in every wavefront (kessler_cases.NAMED:
    1 .. 200 members, 2-D / 3-D, one sub-cycle, sub-cycled, and one forced sub-cycle of an unstable step) through the per-cell gate"""
    name, (nens, nx, ny, nz, _), _ = kc.NAMED[i]
    zi, zm, s, dt, forced = kc.named_state(kc.NAMED[i])
    assert s["temp"].size <= 150000
    got, n, dt_max, micro = _gpu_run(s, zi, nens, nx, ny, nz, dt, rainsplit=forced)
    _, n_ref = kc.run_oracle(s, zm, dt, rainsplit=forced)
    assert n == n_ref, (n, n_ref)
    _, n_free = kc.run_oracle(s, zm, dt)
    assert n_free == micro.rainsplit_for(dt, dt_max)
    if not forced:
        assert n == n_free
    kc.gate_against_oracle(got, s, zm, dt, n, name, case="kessler_gpu_" + name)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["nan_rain", "negative_rain", "nan_density"])
def test_gpu_kessler_refuses_an_unusable_state_and_touches_nothing(bad):
    """a NaN or negative rain cell, or a NaN dry density, below the top level: the time-step limit is not positive, timeStep returns
    PAM_AMD_ESTATE before the column kernel runs, and every coupler array is bit for bit what it was"""
    import torch
    from pam_amd.capi import PamAmdError
    nens, nx, ny, nz = 70, 5, 2, 20
    zi, zm, s = kc.state(nens, nx, ny, nz, 21)
    cell = (nz - 2, 1, 3, 66) if bad != "nan_density" else (7, 0, 2, 5)
    if bad == "nan_rain":
        s["rho_r"][cell] = np.nan
    elif bad == "negative_rain":
        s["rho_r"][cell] = -1e-6
    else:
        s["rho_dry"][cell] = np.nan
    coupler, micro, dm = _gpu_setup(s, zi, nens, nx, ny, nz, 5.0)
    names = [n for n, _ in COUPLER_NAMES] + ["precl"]
    before = {n: dm.get(n).cpu().numpy().copy() for n in names}
    for n, key in COUPLER_NAMES:
        assert np.array_equal(_bits(before[n]), _bits(s[key])), n
    for call in (lambda: micro.timeStep(coupler), lambda: micro.max_stable_dt(coupler)):
        with pytest.raises(PamAmdError, match="sedimentation time-step limit is not positive") as err:
            call()
        assert "[code -4]" in str(err.value)      # PAM_AMD_ESTATE
        torch.cuda.synchronize()
        for n in names:
            assert np.array_equal(_bits(dm.get(n).cpu().numpy()), _bits(before[n])), n


@pytest.mark.gpu
def test_gpu_kessler_rainsplit_hint_and_errors():
    import ctypes as C
    from pam_amd import capi
    nens, nx, ny, nz = 8, 4, 1, 12
    zint, zi, zm, s = _case(nens=nens, nx=nx, ny=ny, nz=nz, heavy_rain=True)
    import copy
    s2 = copy.deepcopy(s)
    got, n, dt_max, _ = _gpu_run(s, zi, nens, nx, ny, nz, 30.0, rainsplit=7)
    assert n == 7
    precl, n_ref = ao.kessler(s2["rho_v"], s2["rho_c"], s2["rho_r"], s2["rho_dry"], s2["temp"], zm, 30.0, C0, rainsplit=7)
    assert np.abs(got["temp"] - s2["temp"]).max() <= 1e-12 * s2["temp"].max()
    assert np.abs(got["precl"] - precl).max() <= 1e-12 * precl.max()
    lib = capi.load()
    assert lib.pam_amd_kessler_time_step(nens, nx, ny, 1, None, None, None, None, None, None, None, 1.0, 287., 461., 1003.,
                                         1e5, None, None, 0, None) == -1
    assert b"kessler" in lib.pam_amd_awfl_last_error()


FUZZ_SEEDS = int(__import__("os").environ.get("PAM_AMD_FUZZ_SEEDS", "12"))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_gpu_kessler_random_shapes_match_oracle(seed):
    """seeded random shapes (1 .. 200 members, 2-D / 3-D, 4 .. 60 levels, light / heavy rain, short / long steps): the column kernel's
    staging of the pow tables, its member / column indexing and the sub-cycle count against the oracle (PAM_AMD_FUZZ_SEEDS=N: N seeds).
    Odd seeds draw their state from kessler_cases.state() (every cell its own categories) instead of the smooth case; every seed
    passes the per-cell gate as well."""
    rng = np.random.default_rng(90001 * seed + 3)
    while True:
        nens = int(rng.choice([1, 2, 3, 7, 16, 33, 64, 65, 70, 128, 200]))
        nx, ny, nz = int(rng.integers(1, 20)), int(rng.choice([1, 1, 2, 3, 5])), int(rng.integers(4, 61))
        if nens * nx * ny * nz <= 150000:
            break
    heavy = bool(rng.random() < 0.5)
    dt = float(rng.choice([1.0, 5.0, 30.0, 60.0]))
    if seed % 2:
        zi, zm, s = kc.state(nens, nx, ny, nz, 1000 + seed)
    else:
        zint, zi, zm, s = _case(nens=nens, nx=nx, ny=ny, nz=nz, heavy_rain=heavy)
    s_in = {k: v.copy() for k, v in s.items()}
    got, n, dt_max, micro = _gpu_run(s, zi, nens, nx, ny, nz, dt)
    precl, n_ref = ao.kessler(s["rho_v"], s["rho_c"], s["rho_r"], s["rho_dry"], s["temp"], zm, dt, C0)
    what = "seed %d: nens %d, %dx%dx%d, heavy %d, dt %g, rainsplit %d" % (seed, nens, nx, ny, nz, heavy, dt, n_ref)
    assert n == n_ref and n == micro.rainsplit_for(dt, dt_max), what
    s["precl"] = precl
    for k in got:
        assert np.isfinite(s[k]).all(), (what, k)
        assert np.abs(got[k] - s[k]).max() <= 1e-12 * max(np.abs(s[k]).max(), 1e-300), (what, k)
    kc.gate_against_oracle(got, s_in, zm, dt, n, what)
