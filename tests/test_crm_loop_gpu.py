"""The composed CRM loop on the GPU, through the Python classes, against the chain of the restatements (tests/crm_loop_ref.py): what the
plug-ins' init hand the dycore against the chain's own tables; every call of the loop against its restatement applied to the GPU's own
state from before the call, every other entry of the DataManager keeping its bits; and the free-running loop against the chain through
the noise-floor gate, with and without a host synchronisation after every call."""
import copy
import time

import numpy as np
import pytest

import crm_loop_ref as loop
import esmt_ref
import grayrad_ref
import hd_ref
import ice1m_ref
import lsforcing_ref
import n2_modules_ref as nr
import sgs_tke_ref
import surface_ref
from parity_gate import compare, noise_floor, record

pytestmark = pytest.mark.gpu

# the module's own reference, whose results_differ the call is held with
REFERENCE = dict(radiation=grayrad_ref, ls_forcing=lsforcing_ref, esmt_pgf=esmt_ref, surface_fluxes=surface_ref, hyperdiffusion=hd_ref,
                 sgs=sgs_tke_ref, micro=ice1m_ref)


class Loop:
    """the stack on a coupler, initialised in the driver's order: micro.init, sgs.init, esmt_init, dycore.init, then the radiation's and the
    modules' init; the stack's state loaded; declare_current_profile_as_hydrostatic"""

    def __init__(self, k, chunks=None):
        import torch
        from pam_amd import Dycore, MicrophysicsIce, PamCoupler, RadiationGray, SGSSmagorinsky, SGSTke, modules
        self.torch, self.k = torch, k
        nz, ny, nx, nens = k.shape
        c = self.c = PamCoupler("cuda:0")
        c.set_option("crm_dt", k.dt)
        c.allocate_coupler_state(nz, ny, nx, nens)
        c.set_grid(k.xlen, k.ylen, k.zint)
        self.micro = MicrophysicsIce()
        self.micro.init(c)
        if k.closure == "tke":
            self.sgs = SGSTke(cs=loop.SGS_CS, ck=loop.SGS_CK, seed=loop.SGS_SEED, moist=True, surface_fluxes=True, horizontal=True)
        else:
            self.sgs = SGSSmagorinsky(cs=loop.SGS_CS, prandtl=loop.SGS_PRANDTL, moist=True, surface_fluxes=True)
            self.sgs.horizontal = True
        self.sgs.init(c)
        if k.esmt:
            modules.esmt_init(c)
        self.dycore = Dycore()
        self.dycore.init(c)
        if chunks is not None:
            self.dycore.set_ensemble_chunks(chunks)
        c.set_option("rad_gray_every", k.rad_every)
        self.rad = RadiationGray().shortwave(coszen=loop.COSZEN)
        self.rad.init(c)
        modules.hyperdiffusion_init(c, loop.HD_TAU)
        modules.surface_fluxes_init(c, sst=300.0, slab_depth=loop.SLAB_DEPTH)
        modules.ls_forcing_init(c, **loop.ls_profiles(k))
        self.dm = c.get_data_manager_device_readwrite()
        c.load_fields(k.fields)
        self.dm.get("sfc_temp").copy_(torch.from_numpy(k.S0["sfc_temp"]))
        self.dycore.declare_current_profile_as_hydrostatic(c)
        self.calls = dict(radiation=lambda: self.rad.timeStep(c), dycore=lambda: self.dycore.timeStep(c),
                          sponge_layer=lambda: modules.sponge_layer(c), ls_forcing=lambda: modules.ls_forcing(c),
                          esmt_pgf=lambda: modules.esmt_pgf(c, forcing=False), surface_fluxes=lambda: modules.surface_fluxes(c),
                          hyperdiffusion=lambda: modules.hyperdiffusion(c), sgs=lambda: self.sgs.timeStep(c), micro=lambda: self.micro.timeStep(c))

    def entries(self):
        """every entry of the DataManager, on the host, once the device is idle"""
        self.torch.cuda.synchronize()
        return {n: e["data"].cpu().numpy() for n, e in self.dm._e.items()}

    def run(self, steps, sync):
        for _ in range(steps):
            for call in loop.order(self.k):
                self.calls[call]()
                if sync:
                    self.torch.cuda.synchronize()
        return self.entries()

    def finalize(self):
        self.dycore.finalize(self.c)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _as_fields(k, E):
    return loop.to_fields(k, E)


@pytest.mark.parametrize("name", tuple(loop.STACKS))
def test_plugins_hand_the_dycore_the_chains_table_and_constants(name):
    """after the inits in the driver's order: the tracer names, their order and their flags as the coupler holds them, the flag arrays and
    idWV the dycore registered, the constants in the options and in the dycore, the options the flags of the stack stand for, and every
    static entry (transfer parameters, profiles, tables) equal what tests/crm_loop_ref.py writes down; compute_time_step equals the oracle's"""
    k = loop.stack(name)
    L = Loop(k)
    c, dm = L.c, L.dm
    assert tuple(c.get_tracer_names()) == k.names
    assert tuple((n,) + tuple(c.get_tracer_info(n)[2:]) for n in k.names) == k.tracers
    E = L.entries()
    assert E["tracer_positive"].tolist() == list(k.positive) and E["tracer_adds_mass"].tolist() == list(k.adds_mass)
    assert c.get_option("idWV") == k.idwv
    for n, v in loop.CONSTS.items():
        assert c.get_option(n) == v and L.dycore.get_option(n) == v, n
    assert c.get_option("micro") == "ice1m" and not c.option_exists("latvap") and not c.option_exists("sigma")
    pre = "sgs_tke_" if k.closure == "tke" else "sgs_smag_"
    assert c.get_option("sgs") == k.closure
    assert all(c.get_option(pre + o) is True for o in ("moist", "surface_fluxes", "horizontal"))
    assert c.get_option(pre + "cs") == loop.SGS_CS and c.get_option(pre + "cloud_threshold") == loop.CLOUD_THRESHOLD
    assert (c.get_option("sgs_tke_ck"), c.get_option("sgs_tke_seed")) == (loop.SGS_CK, loop.SGS_SEED) if k.closure == "tke" else \
        c.get_option("sgs_smag_prandtl") == loop.SGS_PRANDTL
    assert c.get_option("rad_gray_every") == k.rad_every and c.get_option("rad_gray_shortwave") is True
    assert [c.get_option("rad_gray_" + o) for o in ("k_d", "k_v", "k_l", "k_i", "lw_down_top")] == [loop.RAD_LW[o] for o in ("k_d", "k_v", "k_l", "k_i", "lw_down_top")]
    assert all(c.get_option("rad_gray_sw_" + o) == v for o, v in loop.RAD_SW.items())
    assert [c.get_option("sfc_" + o) for o in ("slab_depth", "gust", "wetness")] == [loop.SLAB_DEPTH, loop.SURFACE["gust"], loop.SURFACE["wetness"]]
    assert c.get_option("crm_hyperdiff_timescale") == loop.HD_TAU
    assert c.option_exists("esmt_kmax") == k.esmt and (not k.esmt or c.get_option("esmt_kmax") == k.shape[2] // 2)
    assert (c.get_xlen() / k.shape[2], c.get_ylen() / k.shape[1]) == (k.dx, k.dy)
    for n, a in (("vertical_interface_height", k.zint), ("vertical_midpoint_height", k.zmid), ("vertical_cell_dz", k.dz)):
        assert _same(E[n], a), n
    for n, a in k.S0.items():
        assert n in E, n
        if n in ("esmt_cos", "esmt_sin"):       # formed on the host by two libraries' cosines: an ulp of 1 apart at the most
            assert np.abs(E[n] - a).max() <= 2.0 ** -52, n
        else:
            assert _same(E[n], a), n
    fields = _as_fields(k, E)
    for n in loop.STATE:
        assert _same(fields[n], k.fields[n]), n
    assert _same(fields["tracers"], k.fields["tracers"])
    o = loop.make_oracle(k, k.fields)
    want = o.compute_time_step(copy.deepcopy(k.fields))
    assert abs(L.dycore.compute_time_step(c) - want) <= 1e-14 * want
    gv = E["variable_gravity"]
    assert np.abs(gv - o.variable_gravity).max() <= 1e-12 * np.abs(o.variable_gravity).max()
    L.finalize()


@pytest.mark.parametrize("name,steps", [("full3d_flat", 3), ("full2d_esmt", 2)])
def test_every_call_of_the_loop_is_its_restatement_on_the_gpus_own_state(name, steps):
    """call by call: every DataManager entry is read before and after the call.  A call other than the dycore and the sponge layer: what
    its contract lists as written equals the restatement applied to the state from before the call, bit for bit.  The dycore: the oracle
    advanced one time_step from that state, through parity_gate.compare with that step's own noise floor; equal sub-step counts and
    last_dt_dyn within 1e-15.  The sponge layer: bits below the sponge and the per-cell gate of tests/n2_modules_ref.py inside it (its
    level means are sums in another order than any host's).  And after every call every entry outside the call's contract keeps its bits:
    density_dry under all physics, the precipitation and radiation outputs under the dycore, sfc_temp under everything but the surface
    fluxes, the hydrostatic arrays, the grid, the profiles and the flag arrays under everything"""
    k = loop.stack(name)
    L = Loop(k)
    chain = loop.start(k)
    names = list(k.names)
    t_cpu = 0.0
    before = L.entries()
    for step in range(steps):
        for call in loop.order(k):
            allowed = set(loop.writes(chain, call))
            L.calls[call]()
            after = L.entries()
            t0 = time.time()
            where = (name, step, call)
            if call == "dycore":
                info = {}
                f0 = _as_fields(k, before)
                exp = loop.dycore(chain, before, info)
                assert L.dycore.last_ncycles == info["nsub"], where
                assert abs(L.dycore.last_dt_dyn - info["dt_dyn"]) <= 1e-15 * info["dt_dyn"], where
                floor = noise_floor(lambda f: chain.oracle.time_step(f, k.dt), f0, names, loop.FLOOR_SEED, base=_as_fields(k, exp))
                compare(_as_fields(k, after), _as_fields(k, exp), names, info["nsub"], floor=floor)
            elif call == "sponge_layer":
                X = nr.stack(_as_fields(k, before))
                ref = nr.sponge(X, k.zint, k.zmid, k.dt, loop.SPONGE["num_layers"], loop.SPONGE["time_scale"])
                got = nr.stack(_as_fields(k, after))
                bottom = k.shape[0] - loop.SPONGE["num_layers"]
                assert np.array_equal(nr.bits(got[:, :bottom]), nr.bits(X[:, :bottom])), where
                worst, at = nr.worst_ratio(got, ref)
                assert worst < 1.0, where + (worst, at)
            else:
                want = loop.RESTATEMENTS[call](chain, before)
                assert set(want) <= allowed, where
                if call == "hyperdiffusion":      # hd_ref's takes lists and gives indices
                    bad = [list(want)[i] for i in hd_ref.results_differ([after[n] for n in want], list(want.values()))]
                else:
                    bad = REFERENCE[call].results_differ({n: after[n] for n in want}, want)
                assert bad == [], where + (bad,)
            kept = [n for n in before if n not in allowed and not _same(before[n], after[n])]
            assert kept == [], where + (kept,)
            t_cpu += time.time() - t0
            before = after
    assert not _same(before["sfc_temp"], k.S0["sfc_temp"]) and before["preci"].max() > 0 and before["precl"].max() > 0
    print("%s: %d calls held; the restatements took %.1f s on the host" % (name, steps * len(loop.order(k)), t_cpu))
    L.finalize()


# Measured on MI355X, worst / floor of the free-running loop against the chain (the record's crm_loop_<stack> entries; every gate is the
# minimum, 1e-12, but that of the shortwave surface fluxes of full2d_esmt, 1.05e-12):
#   full3d_flat (10,5,6,3), 3 steps: rho_d 1.8e-15 / 1.8e-15, T 1.8e-15 / 1.6e-15, vapour 1.7e-14 / 1.5e-14, u 5.5e-14 / 6.1e-14, v 2.5e-14 /
#     2.2e-14, w 9.8e-14 / 4.7e-14, cloud_liquid 6.3e-14 / 5.5e-14, cloud_ice 6.6e-14 / 8.3e-14, rain 2.6e-15 / 2.1e-15, snow 2.4e-15 /
#     2.6e-15, tke 9.6e-15 / 7.0e-15, precl 1.5e-15 / 2.1e-15, preci 5.3e-15 / 1.1e-14, sfc_temp 0 / 0, rad_olr 4.6e-15 / 5.5e-15,
#     rad_lw_down_sfc 4.2e-14 / 8.6e-14, rad_sw_down_sfc 1.0e-13 / 1.3e-13, rad_sw_up_top 1.3e-14 / 1.2e-14
#   full3d_members (8,5,5,65), 2 steps, three member chunks: rho_d 3.4e-15 / 2.5e-15, T 1.9e-15 / 1.9e-15, vapour 1.7e-14 / 2.0e-14, u 4.5e-14
#     / 5.0e-14, v 2.8e-14 / 2.2e-14, w 1.2e-13 / 1.1e-13, cloud_liquid 5.4e-14 / 6.4e-14, cloud_ice 1.2e-13 / 1.2e-13, rain 1.8e-15 /
#     1.8e-15, snow 6.3e-14 / 6.8e-14, tke 1.9e-14 / 2.2e-14, precl 1.6e-15 / 1.6e-15, preci 1.3e-14 / 1.3e-14, sfc_temp and every
#     radiation flux 0 (computed once, from the loaded state: the same bits as the restatements')
#   full2d_esmt (10,1,9,66), 3 steps: rho_d 2.7e-15 / 2.5e-15, T 2.2e-15 / 2.0e-15, vapour 1.8e-14 / 1.9e-14, u 4.9e-14 / 4.1e-14, v 2.8e-15 /
#     2.2e-15, w 1.1e-13 / 7.3e-14, cloud_liquid 7.5e-14 / 7.3e-14, cloud_ice 1.2e-13 / 1.8e-13, rain 5.8e-15 / 2.0e-14, snow 1.1e-14 /
#     3.8e-14, esmt_u 2.5e-15 / 4.5e-15, esmt_v 2.3e-15 / 3.4e-15, precl 9.7e-15 / 3.3e-14, preci 1.5e-14 / 4.5e-14, sfc_temp 0 / 0,
#     rad_olr 7.2e-15 / 6.1e-15, rad_lw_down_sfc 1.5e-13 / 1.6e-13, rad_sw_down_sfc 2.2e-13 / 2.6e-13, rad_sw_up_top 1.6e-14 / 2.1e-14
@pytest.mark.parametrize("name", tuple(loop.STACKS))
def test_free_running_loop_matches_the_chain_and_does_not_depend_on_host_synchronisation(name):
    """the same loop with no host synchronisation between the calls (the dycore in three member chunks on full3d_members), against
    crm_loop_ref's run through parity_gate: the five state fields, every tracer, precl, preci, sfc_temp and the radiation's surface and top
    fluxes, each at min(cap, max(1e-12, 4 floor)) with the floors of the chain's twins and the caps 1e-8 (winds, tracers) and 1e-10
    (column outputs), rho_d, temp and the vapour at 1e-12.  Then the same loop with a synchronisation after every call: every entry of
    the DataManager has the bits of the unsynchronised run"""
    k = loop.stack(name)
    chunks = 3 if name == "full3d_members" else None
    t0 = time.time()
    base, held, floor = loop.floors(k)
    gate = loop.gates(k, base, floor)
    t_cpu = time.time() - t0
    t0 = time.time()
    L = Loop(k, chunks)
    free = L.run(k.steps, sync=False)
    L.finalize()
    t_gpu = time.time() - t0
    worst = loop.errors(k, _as_fields(k, free), free, base, held)
    keys = [n for n in worst]
    record("crm_loop_" + name, {n: dict(worst=worst[n], floor=floor.get(n), gate=gate[n]) for n in keys})
    print("%s %s: chain and twins %.1f s, GPU loop %.1f s" % (name, k.shape, t_cpu, t_gpu))
    for n in keys:
        print("   %-24s worst %.2e floor %.2e gate %.2e" % (n, worst[n], floor.get(n, float("nan")), gate[n]))
    for n in keys:
        assert worst[n] <= gate[n], (n, worst[n], gate[n], floor.get(n))
    L = Loop(k, chunks)
    synced = L.run(k.steps, sync=True)
    L.finalize()
    differ = [n for n in free if not _same(free[n], synced[n])]
    assert differ == [], differ
