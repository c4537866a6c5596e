"""GPU parity tests: the HIP path (through the C ABI, via pam_amd.Dycore) against the CPU oracle on the same seeded
inputs, at sizes the oracle finishes in seconds.

Tolerances (fp64).  north_star: prognostic fields within rtol 1e-12 of the reference.  The HIP kernels are not
bit-identical to the oracle by construction (FMA contraction, v_rcp_f64+Newton reciprocals, algebraically fused
bridge matrices and weight normalisation, device pow), each a ~1e-16 relative perturbation per operation; the
oracle's own response to 1-ulp input noise over the same steps is ~2e-15 (rho, T), ~3e-14 (u), ~1e-12 (w) and up to
~2e-11 (v, which is ~1e-1 m/s noise in these cases) -- see DESIGN.md "Parity budget".  So:
   density_dry, temp, water_vapor:  max|a-b| <= 1e-12 * max|b|          (the north_star gate); density_dry and temp also
                                    ELEMENT-WISE: |a-b| <= 1e-12 |b| in every cell
   uvel, wvel, vvel, other tracers: max|a-b| <= min(1e-11 (1 + nsub/3), max(1e-12, 4 floor)) * max|b|, where `floor` is the
                                    case's own noise floor: the oracle's response to one ulp of noise in T (three twin runs);
                                    exactly zero where the oracle's field is (tests/parity_gate.py -- shared by every HIP-vs-oracle
                                    comparison of the repository)
The named cases (CASES) and their oracle runs live in tests/parity_cases.py, where the CPU tests of the gate build them too.
"""
import copy
import json
import os

import numpy as np
import pytest

from pam_amd import idealized as idz

pytestmark = pytest.mark.gpu

from oracle import awfl_oracle as ao   # noqa: E402
from parity_gate import compare as _compare_gate   # noqa: E402  (tests/parity_gate.py: the gate, documented there)
from parity_cases import CASES, OracleCase, build_inputs, named_case   # noqa: E402  (the named cases, without a device)


def _setup(nens, nx, ny, nz, tr, zint, consts=idz.CONSTS_DEFAULT, supercell=True, per_ens=False, mag=0.5, crm_dt=2.0,
           dxy=500.0, dry_air=False, dy=None, flow="x"):
    from pam_amd import Dycore, PamCoupler
    names, pos, mass, idwv = idz.tracer_flags(tr)
    f, xlen, ylen, zi, dz = build_inputs(nens, nx, ny, nz, tr, zint, consts, supercell, per_ens, mag, dxy, dry_air, dy=dy, flow=flow)
    coupler = PamCoupler("cuda:0")
    coupler.set_option("crm_dt", crm_dt)
    for k, v in consts.items():
        coupler.set_option(k, v)
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(xlen, ylen, zi)
    for n, p, m in tr:
        coupler.add_tracer(n, "", p, m)
    dycore = Dycore()
    dycore.init(coupler)
    coupler.load_fields(f)
    oracle = ao.OracleDycore(nens, nx, ny, nz, xlen, ylen, dz, pos, mass, idwv, consts=consts)
    return coupler, dycore, oracle, copy.deepcopy(f), names


def _compare(got, exp, names, nsub, case=None, factor=1.0, floor=None):
    return _compare_gate(got, exp, names, nsub, case, factor, floor)


@pytest.mark.parametrize("case", sorted(CASES))
def test_time_step_matches_oracle(case):
    import torch
    nens, nx, ny, nz, tr, zint, kw, mode_a, nsteps = CASES[case]
    kw = dict(kw)
    gate_factor = kw.pop("gate_factor", 1.0)
    coupler, dycore, oracle, fo, names = _setup(nens, nx, ny, nz, tr, zint, **kw)
    if not mode_a:
        coupler.set_option("balance_hydrostasis_with_gravity", False)   # after init(), SURVEY 8c
        oracle.set_grav_balance(False)
    dycore.declare_current_profile_as_hydrostatic(coupler)
    oracle.declare_current_profile_as_hydrostatic(fo)
    gv = coupler.dm.get("variable_gravity" if mode_a else "hy_dens_cells", readonly=True).cpu().numpy()
    ov = oracle.variable_gravity if mode_a else oracle.hy_dens_cells
    assert np.abs(gv - ov).max() <= 1e-12 * np.abs(ov).max()
    assert abs(dycore.compute_time_step(coupler) - oracle.compute_time_step(fo)) <= 1e-14 * oracle.compute_time_step(fo)
    nsub = 0
    for _ in range(nsteps):
        n_gpu = dycore.timeStep(coupler)
        n_cpu, dt_cpu = oracle.time_step(fo, coupler.get_option("crm_dt"))
        assert n_gpu == n_cpu
        nsub += n_gpu
        assert abs(dycore.last_dt_dyn - dt_cpu) <= 1e-15 * dt_cpu
        if kw.get("dry_air"):
            flagged, total, any_word = dycore.debug_fct_rows()      # the last stage of this timeStep limited vapour somewhere
            assert 0 < flagged < total and any_word, (flagged, total)
    torch.cuda.synchronize()
    got = coupler.dump_fields()
    # the case's own noise floor: the oracle's response to one ulp of T, three twins (tests/parity_gate.py)
    floor = named_case(case).floor(base=fo)
    _compare(got, fo, names, nsub, case, gate_factor, floor)
    if case == "3d_nt4_stretched_B":
        # the gate itself: a relative perturbation of 1e-10 in ONE field must turn the case red
        for k in ("uvel", "wvel", "temp"):
            bad = copy.deepcopy(got)
            bad[k] = bad[k] * (1.0 + 1.0e-10)
            with pytest.raises(AssertionError):
                _compare(bad, fo, names, nsub)
        bad = copy.deepcopy(got)
        bad["tracers"][1] = bad["tracers"][1] * (1.0 + 1.0e-10)
        with pytest.raises(AssertionError):
            _compare(bad, fo, names, nsub)
    dycore.finalize(coupler)


@pytest.mark.parametrize("seg,span", [(1, 1), (3, 0), (3, 6), (8, 8), (16, 0), (8, 16)])
def test_flux_sweep_geometry_does_not_change_results(seg, span):
    """Chunk length (LDS face slots) and span (faces per thread) of the flux kernel are pure scheduling knobs: every
    cell polynomial and every face flux is the same arithmetic whatever the decomposition -> bit-identical results."""
    import torch
    nens, nx, ny, nz = 4, 9, 4, 9
    tr = idz.TRACERS_KESSLER_SHOC
    res = []
    for s, sp in ((8, 0), (seg, span)):
        coupler, dycore, oracle, fo, names = _setup(nens, nx, ny, nz, tr, idz.stretched_interfaces(nz, 12000.0))
        dycore.set_flux_segment(s)
        dycore.set_flux_span(sp)
        dycore.declare_current_profile_as_hydrostatic(coupler)
        dycore.timeStep(coupler)
        torch.cuda.synchronize()
        res.append(coupler.dump_fields())
        dycore.finalize(coupler)
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


@pytest.mark.parametrize("chunks", [1, 2, 3])
def test_ensemble_chunking_does_not_change_results(chunks):
    """Internal ensemble chunks (member ranges on separate HIP streams) are a scheduling device: members are
    independent, so any chunking gives bit-identical results, including ragged last chunks (nens=150 -> 128+22)."""
    import torch
    nens, nx, ny, nz = 150, 6, 3, 7
    tr = idz.TRACERS_KESSLER_SHOC
    res = []
    for n in (1, chunks):
        coupler, dycore, oracle, fo, names = _setup(nens, nx, ny, nz, tr, idz.stretched_interfaces(nz, 9000.0))
        dycore.set_ensemble_chunks(n)
        dycore.declare_current_profile_as_hydrostatic(coupler)
        dycore.timeStep(coupler)
        dycore.timeStep(coupler)
        torch.cuda.synchronize()
        res.append(coupler.dump_fields())
        dycore.finalize(coupler)
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


# the kernel-level checks below on today's isotropic state and on dx != dy with the sounding's shear along y (build_inputs)
GRIDS = {"isotropic": {}, "anisotropic_y_flow": dict(dxy=500.0, dy=800.0, flow="y")}


@pytest.mark.parametrize("grid", sorted(GRIDS, reverse=True))
def test_raw_fluxes_match_oracle(grid):
    """Kernel-level check of the reconstruction/flux kernel (Dycore.h:334-519) on its own."""
    import torch
    nens, nx, ny, nz = 2, 7, 5, 9
    tr = idz.TRACERS_NONE
    coupler, dycore, oracle, fo, names = _setup(nens, nx, ny, nz, tr, idz.stretched_interfaces(nz, 12000.0), mag=1.0, **GRIDS[grid])
    dycore.declare_current_profile_as_hydrostatic(coupler)
    oracle.declare_current_profile_as_hydrostatic(fo)
    st, trc = oracle.convert_coupler_to_dynamics(fo)
    seed = trc[:, 3:-3, 3:-3, 3:-3, :].copy()
    _, _, fl = oracle.compute_tendencies(st, trc, seed, 1.0, want_fluxes=True)
    dycore.convert_coupler_to_dynamics(coupler)
    dycore.debug_flux_stage(1.0)
    torch.cuda.synchronize()
    nt = 1
    gx = dycore.debug_buffer("flux_x").cpu().numpy().reshape(5 + nt, nz, ny, nx, nens)
    gy = dycore.debug_buffer("flux_y").cpu().numpy().reshape(5 + nt, nz, ny, nx, nens)
    gz = dycore.debug_buffer("flux_z").cpu().numpy().reshape(5 + nt, nz + 1, ny, nx, nens)
    for l in range(5):   # state fluxes are not touched by FCT
        for g, o in ((gx[l], fl[0][l][:, :, :nx]), (gy[l], fl[1][l][:, :ny]), (gz[l], fl[2][l])):
            # the mass flux is (p_L - p_R)/(2 cs) + ...: absolute round-off of a 1e5 Pa reconstruction / 350
            assert np.abs(g - o).max() <= 1e-12 * max(np.abs(o).max(), 1.0)
    dycore.finalize(coupler)


@pytest.mark.parametrize("grid", sorted(GRIDS, reverse=True))
def test_converts_with_halo_arrays_match_oracle(grid):
    """Dycore::convert_coupler_to_dynamics(coupler, state, tracers) and convert_dynamics_to_coupler(coupler, state, tracers) with
    the reference's halo'd arrays (Dycore.h:1336-1388, :1281-1331) against the oracle's restatement of the same two kernels."""
    import torch
    nens, nx, ny, nz = 3, 6, 4, 8
    tr = idz.TRACERS_KESSLER_SHOC
    coupler, dycore, oracle, fo, names = _setup(nens, nx, ny, nz, tr, idz.stretched_interfaces(nz, 12000.0), **GRIDS[grid])
    nt = len(tr)
    st_o, tr_o = oracle.convert_coupler_to_dynamics(fo)
    st = torch.full((5, nz + 6, ny + 6, nx + 6, nens), float("nan"), dtype=torch.float64, device="cuda:0")
    trc = torch.full((nt, nz + 6, ny + 6, nx + 6, nens), float("nan"), dtype=torch.float64, device="cuda:0")
    dycore.convert_coupler_to_dynamics(coupler, st, trc)
    torch.cuda.synchronize()
    gs, gt = st.cpu().numpy(), trc.cpu().numpy()
    inner = (slice(None), slice(3, -3), slice(3, -3), slice(3, -3), slice(None))
    for l in range(5):
        assert np.abs(gs[inner][l] - st_o[inner][l]).max() <= 1e-14 * np.abs(st_o[inner][l]).max(), l
    assert np.array_equal(gt[inner], tr_o[inner])
    halo = np.ones(gs.shape, dtype=bool)
    halo[inner] = False
    assert np.isnan(gs[halo]).all() and np.isnan(gt[np.broadcast_to(halo[:1], gt.shape)]).all(), "halos must stay untouched"
    # back: a modified state (as if the caller had advanced it) -> coupler
    st_o[inner] *= 1.01
    tr_o[inner] *= 0.5
    fexp = copy.deepcopy(fo)
    oracle.convert_dynamics_to_coupler(st_o, tr_o, fexp)
    dycore.convert_dynamics_to_coupler(coupler, torch.from_numpy(st_o).to("cuda:0"), torch.from_numpy(tr_o).to("cuda:0"))
    torch.cuda.synchronize()
    got = coupler.dump_fields()
    for k in ("density_dry", "uvel", "vvel", "wvel", "temp"):
        assert np.abs(got[k] - fexp[k]).max() <= 1e-14 * np.abs(fexp[k]).max(), k
    assert np.array_equal(got["tracers"], fexp["tracers"])
    dycore.finalize(coupler)


def test_gcm_column_hydrostatic_branch():
    """declare_current_profile_as_hydrostatic(use_gcm_data=true), Dycore.h:1415-1434."""
    nens, nx, ny, nz = 3, 6, 1, 12
    tr = idz.TRACERS_NONE
    zint = idz.stretched_interfaces(nz, 12000.0)
    coupler, dycore, oracle, fo, names = _setup(nens, nx, ny, nz, tr, zint)
    rho_d, u, v, w, T, rho_v = idz.supercell_column(zint)
    import torch
    cols = {"gcm_density_dry": rho_d, "gcm_temp": T, "gcm_water_vapor": rho_v, "gcm_cloud_water": 1e-4 * rho_d,
            "gcm_cloud_ice": 0 * rho_d}
    gcm = {}
    for k, c in cols.items():
        a = np.ascontiguousarray(c[:, None] * (1 + 0.001 * np.arange(nens))[None, :])
        gcm[k] = a
        coupler.dm.get(k).copy_(torch.from_numpy(a))
    dycore.declare_current_profile_as_hydrostatic(coupler, use_gcm_data=True)
    oracle.declare_current_profile_as_hydrostatic(fo, gcm=gcm)
    gv = coupler.dm.get("variable_gravity", readonly=True).cpu().numpy()
    assert np.abs(gv - oracle.variable_gravity).max() <= 1e-12 * np.abs(oracle.variable_gravity).max()
    dycore.finalize(coupler)


def test_time_step_requires_hydrostatic_declaration():
    from pam_amd import PamAmdError
    coupler, dycore, oracle, fo, names = _setup(2, 6, 1, 8, idz.TRACERS_NONE, idz.uniform_interfaces(8, 8000.0))
    with pytest.raises(PamAmdError):
        dycore.timeStep(coupler)
    dycore.finalize(coupler)


def test_conservation_and_positivity_at_full_size_slice():
    """Size-independent properties at a BASELINE-shaped grid (32x1x60, L60 grid), nens too large for the oracle:
    total mass / rho*theta / vapour conserved to 1e-10 per timeStep (the reference's own PAM_DEBUG invariant,
    Dycore.h:224-251), positive tracers stay non-negative, everything finite."""
    import torch
    nens, nx, ny, nz = 256, 32, 1, 60
    tr = idz.TRACERS_KESSLER_SHOC
    zint = idz.l60_interfaces()
    from pam_amd import Dycore, PamCoupler
    names, pos, mass, idwv = idz.tracer_flags(tr)
    f = idz.supercell_fields(nens, nx, ny, nz, zint, tracers=tr, magnitude=0.5)
    idz.add_tracer_blobs(f, tr, 32000.0, 32000.0, zint)
    coupler = PamCoupler("cuda:0")
    coupler.set_option("crm_dt", 1.0)
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(32000.0, 32000.0, zint)
    for n, p, m in tr:
        coupler.add_tracer(n, "", p, m)
    dycore = Dycore()
    dycore.init(coupler)
    coupler.load_fields(f)
    dycore.declare_current_profile_as_hydrostatic(coupler)
    dz = torch.from_numpy(np.diff(zint)).to("cuda:0")[:, None, None, None]

    def totals():
        rho = coupler.dm.get("density_dry", readonly=True).clone()
        for n, p, m in tr:
            if m:
                rho = rho + coupler.dm.get(n, readonly=True)
        return (rho * dz).sum(dim=(0, 1, 2)), (coupler.dm.get("water_vapor", readonly=True) * dz).sum(dim=(0, 1, 2))
    m0, v0 = totals()
    n = dycore.timeStep(coupler)
    torch.cuda.synchronize()
    m1, v1 = totals()
    assert n >= 3
    assert torch.all((m1 - m0).abs() <= 1e-10 * m0.abs())
    assert torch.all((v1 - v0).abs() <= 1e-10 * v0.abs())
    for name, p, m in tr:
        t = coupler.dm.get(name, readonly=True)
        assert torch.isfinite(t).all() and (t >= 0).all()
    assert torch.isfinite(coupler.dm.get("temp", readonly=True)).all()
    dycore.finalize(coupler)


def test_full_baseline_size_c2_properties():
    """BASELINE.json configs[1] at full size (nens=1024, 32x32x60 L60, NT=1; 63M cells, too large for the oracle):
    size-independent properties.  (i) dry mass and vapour mass of every member conserved to 1e-10 per timeStep (the
    reference's PAM_DEBUG invariant, Dycore.h:224-251); (ii) all fields finite, vapour non-negative; (iii) members that
    start identical stay bit-identical (the inputs are 16 distinct members tiled 64 times: any cross-member leakage or
    chunk-boundary error would break this); (iv) the automatic overlapped schedule (8 member ranges of 128 on prioritised
    streams) equals the single-range one bit for bit (tools/soak_c2.py repeats this over hundreds of sub-steps)."""
    import torch
    from pam_amd import Dycore, PamCoupler
    nens, nx, ny, nz, ngen = 1024, 32, 32, 60, 16
    zint = idz.l60_interfaces()
    f = idz.supercell_fields(ngen, nx, ny, nz, zint, magnitude=0.1)
    results = []
    for chunks in (0, 1):
        coupler = PamCoupler("cuda:0")
        coupler.set_option("crm_dt", 1.0)
        coupler.allocate_coupler_state(nz, ny, nx, nens)
        coupler.set_grid(nx * 1000.0, ny * 1000.0, zint)
        coupler.add_tracer("water_vapor", "", True, True)
        dycore = Dycore()
        dycore.init(coupler)
        dycore.set_ensemble_chunks(chunks)
        for k in ("density_dry", "uvel", "vvel", "wvel", "temp"):
            coupler.dm.get(k).copy_(torch.from_numpy(f[k]).to("cuda:0").repeat(1, 1, 1, nens // ngen))
        coupler.dm.get("water_vapor").copy_(torch.from_numpy(f["tracers"][0]).to("cuda:0").repeat(1, 1, 1, nens // ngen))
        dycore.declare_current_profile_as_hydrostatic(coupler)
        dz = torch.from_numpy(np.diff(zint)).to("cuda:0")[:, None, None, None]
        rho0 = ((coupler.dm.get("density_dry", readonly=True) + coupler.dm.get("water_vapor", readonly=True)) * dz).sum(dim=(0, 1, 2))
        wv0 = (coupler.dm.get("water_vapor", readonly=True) * dz).sum(dim=(0, 1, 2))
        n = dycore.timeStep(coupler)
        torch.cuda.synchronize()
        assert n >= 3
        rho1 = ((coupler.dm.get("density_dry", readonly=True) + coupler.dm.get("water_vapor", readonly=True)) * dz).sum(dim=(0, 1, 2))
        wv1 = (coupler.dm.get("water_vapor", readonly=True) * dz).sum(dim=(0, 1, 2))
        assert torch.all((rho1 - rho0).abs() <= 1e-10 * rho0)
        assert torch.all((wv1 - wv0).abs() <= 1e-10 * wv0)
        for k in ("density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor"):
            t = coupler.dm.get(k, readonly=True)
            assert torch.isfinite(t).all(), k
            assert torch.equal(t[..., :ngen], t[..., nens - ngen:]), k           # tile 0 == tile 63
            assert torch.equal(t[..., :ngen], t[..., 384:384 + ngen]), k          # across the range boundary at 384 = 3*128
        assert (coupler.dm.get("water_vapor", readonly=True) >= 0).all()
        results.append({k: coupler.dm.get(k, readonly=True)[..., ::37].clone() for k in ("density_dry", "wvel", "temp")})
        dycore.finalize(coupler)
        del coupler, dycore
        torch.cuda.empty_cache()
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k


def test_full_size_c2_vapour_limited_member_ranges_do_not_interfere():
    """C2 at full size with the limiter active on water vapour in nearly every row (dry slabs at member-dependent places), one
    member range against two.  Member ranges of one handle advance on their own streams, so one can be a tendency stage ahead of
    the other: anything they share must not depend on the stage.  (Round 3: the "some row was flagged" word WAS shared -- the range
    that was ahead overwrote it, the other one's fix-up pass left early, and its vapour came out wrong in ~1e6 cells; only this
    size opens the window.  tools/soak_configs.py repeats it over 54 sub-steps for C2, C3 and C4.)"""
    import torch
    from pam_amd import Dycore, PamCoupler
    nens, nx, ny, nz, ngen = 1024, 32, 32, 60, 16
    zint = idz.l60_interfaces()
    f = idz.supercell_fields(ngen, nx, ny, nz, zint, magnitude=0.5)
    idz.carve_dry_air(f, idz.TRACERS_NONE)
    coupler = PamCoupler("cuda:0")
    coupler.set_option("crm_dt", 2.0)
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(nx * 1000.0, ny * 1000.0, zint)
    coupler.add_tracer("water_vapor", "", True, True)
    dycore = Dycore()
    dycore.init(coupler)
    names = ["density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor"]
    init = {k: torch.from_numpy(f[k]).to("cuda:0").repeat(1, 1, 1, nens // ngen).contiguous() for k in names[:5]}
    init["water_vapor"] = torch.from_numpy(f["tracers"][0]).to("cuda:0").repeat(1, 1, 1, nens // ngen).contiguous()
    res = []
    for chunks in (1, 2, 4):
        for k in names:
            coupler.dm.get(k).copy_(init[k])
        dycore.set_ensemble_chunks(chunks)
        dycore.declare_current_profile_as_hydrostatic(coupler)
        n = dycore.timeStep(coupler)
        torch.cuda.synchronize()
        flagged, total, _ = dycore.debug_fct_rows()
        assert n >= 3 and flagged > total // 2
        res.append({k: coupler.dm.get(k, readonly=True).clone() for k in names})
    for k in names:
        assert torch.isfinite(res[0][k]).all(), k
        assert torch.equal(res[0][k], res[1][k]) and torch.equal(res[0][k], res[2][k]), k
    dycore.finalize(coupler)


@pytest.mark.parametrize("cfg", ["c3_nens4096_kessler_shoc", "c4_shard512_p3_shoc", "c4_total_nens4096_p3_shoc"])
def test_full_baseline_size_c3_c4_properties(cfg):
    """BASELINE.json configs[2] (nens=4096, 2-D 32x1x60, 4 tracers) and one GPU's shard of configs[3] (512 of 4096 members, 10
    tracers, P3 constants) at full size: too large for the oracle, so size-independent properties.  Tracers carry blobs with exact
    zeros around them, so the FCT limiter is active and its row flags are set (the fused stage's sparse path).  (i) total mass
    (dry + every mass-adding tracer) and vapour mass of every member conserved to 1e-10 per timeStep (Dycore.h:224-251);
    (ii) positive-definite tracers stay non-negative, everything finite; (iii) members that start identical stay bit-identical
    (16 distinct members tiled); (iv) the fused stage equals the three-kernel stage bit for bit at this size too."""
    import torch
    from pam_amd import Dycore, PamCoupler
    # (c4_total: BASELINE.json configs[3] WHOLE -- nens = 4096 with the 10 P3 + SHOC tracers -- on one GPU: the N = 1 end of its
    # strong-scaling row; ~7 GB of resident arrays)
    nens, tr, consts = (4096, idz.TRACERS_KESSLER_SHOC, idz.CONSTS_DEFAULT) if cfg.startswith("c3") else (
        (512 if "shard" in cfg else 4096), idz.TRACERS_P3_SHOC, idz.CONSTS_P3)
    nx, ny, nz, ngen = 32, 1, 60, 16
    zint = idz.l60_interfaces()
    xlen = nx * 1000.0
    f = idz.supercell_fields(ngen, nx, ny, nz, zint, consts=consts, tracers=tr, magnitude=0.1)
    idz.add_tracer_blobs(f, tr, xlen, xlen, zint)
    dz = torch.from_numpy(np.diff(zint)).to("cuda:0")[:, None, None, None]
    results = []
    for fused in (True, False):
        coupler = PamCoupler("cuda:0")
        coupler.set_option("crm_dt", 2.0)
        for k, v in consts.items():
            coupler.set_option(k, v)
        coupler.allocate_coupler_state(nz, ny, nx, nens)
        coupler.set_grid(xlen, xlen, zint)
        for n, p, m in tr:
            coupler.add_tracer(n, "", p, m)
        dycore = Dycore()
        dycore.init(coupler)
        dycore.set_fused_stage(fused)
        for k in ("density_dry", "uvel", "vvel", "wvel", "temp"):
            coupler.dm.get(k).copy_(torch.from_numpy(f[k]).to("cuda:0").repeat(1, 1, 1, nens // ngen))
        for t, (n, p, m) in enumerate(tr):
            coupler.dm.get(n).copy_(torch.from_numpy(f["tracers"][t]).to("cuda:0").repeat(1, 1, 1, nens // ngen))
        dycore.declare_current_profile_as_hydrostatic(coupler)

        def totals():
            rho = coupler.dm.get("density_dry", readonly=True).clone()
            for n, p, m in tr:
                if m:
                    rho = rho + coupler.dm.get(n, readonly=True)
            return (rho * dz).sum(dim=(0, 1, 2)), (coupler.dm.get("water_vapor", readonly=True) * dz).sum(dim=(0, 1, 2))
        m0, v0 = totals()
        nsub = dycore.timeStep(coupler)
        torch.cuda.synchronize()
        m1, v1 = totals()
        assert nsub >= 3
        assert torch.all((m1 - m0).abs() <= 1e-10 * m0.abs())
        assert torch.all((v1 - v0).abs() <= 1e-10 * v0.abs())
        out = {}
        for k in ["density_dry", "uvel", "wvel", "temp"] + [n for n, p, m in tr]:
            t = coupler.dm.get(k, readonly=True)
            assert torch.isfinite(t).all(), k
            assert torch.equal(t[..., :ngen], t[..., nens - ngen:]), k
            out[k] = t[..., ::29].clone()
        for n, p, m in tr:
            if p:
                assert (coupler.dm.get(n, readonly=True) >= 0).all(), n
        results.append(out)
        dycore.finalize(coupler)
        del coupler, dycore
        torch.cuda.empty_cache()
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k


def test_long_run_parity_120_substeps():
    """north_star: "prognostic state after N steps matches the reference ... rtol 1e-12".  20 timeSteps = 120 SSPRK3
    sub-steps of a 3-D moist-tracer supercell case; measured drift HIP vs oracle: 1e-14 (rho, T), 1e-13 (u), 1e-12 (w)."""
    import torch
    nens, nx, ny, nz = 4, 16, 8, 20
    tr = idz.TRACERS_KESSLER_SHOC
    coupler, dycore, oracle, fo, names = _setup(nens, nx, ny, nz, tr, idz.stretched_interfaces(nz, 15000.0, ratio=1.08),
                                                 crm_dt=4.0, dxy=1000.0)
    dycore.declare_current_profile_as_hydrostatic(coupler)
    oracle.declare_current_profile_as_hydrostatic(fo)
    sub = 0
    for _ in range(20):
        n = dycore.timeStep(coupler)
        n2, _ = oracle.time_step(fo, 4.0)
        assert n == n2
        sub += n
    torch.cuda.synchronize()
    assert sub >= 100
    got = coupler.dump_fields()
    # the floor gate (min(tol_noise_fields(120) = 4.1e-10, max(1e-12, 4 x the oracle's own response to one ulp of T)) for u, v, w
    # and the non-vapour tracers; rho_d, T, vapour 1e-12), recorded like the other oracle cases; u and w additionally keep round 3's
    # flat bounds
    oc = OracleCase(nens, nx, ny, nz, tr, idz.stretched_interfaces(nz, 15000.0, ratio=1.08), crm_dt=4.0, dxy=1000.0, nsteps=20)
    _compare(got, fo, names, sub, "long_run_120_substeps", floor=oc.floor(base=fo))
    for k, tol in (("uvel", 1e-12), ("wvel", 1e-10)):
        assert np.abs(got[k] - fo[k]).max() <= tol * np.abs(fo[k]).max(), k
    dycore.finalize(coupler)


def test_a_single_nan_cell_fails_the_step():
    """The CFL reduction must not swallow a NaN (fmin() drops NaN operands): one bad cell anywhere in the ensemble makes
    timeStep refuse to run instead of sub-cycling on a time step derived from the healthy cells."""
    import torch
    from pam_amd import PamAmdError
    coupler, dycore, oracle, fo, names = _setup(70, 6, 3, 8, idz.TRACERS_NONE, idz.uniform_interfaces(8, 8000.0))
    dycore.declare_current_profile_as_hydrostatic(coupler)
    assert dycore.compute_time_step(coupler) > 0
    coupler.dm.get("temp")[5, 1, 3, 67] = float("nan")
    assert dycore.compute_time_step(coupler) == 0.0
    with pytest.raises(PamAmdError):
        dycore.timeStep(coupler)
    dycore.finalize(coupler)
