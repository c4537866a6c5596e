"""The GCM-coupled CRM loop on the GPU, through the Python classes on one coupler, against the chain of the restatements
(tests/mmf_loop_ref.py): what the inits leave against the chain's own tables; every call of both GCM steps against its restatement
applied to the GPU's own state from before the call, every other entry of the DataManager keeping its bits; the free-running loop
against the chain through the noise-floor gate, with and without a host synchronisation after every call; and the members of
mmf3d_members run as two ranges on two couplers against the whole run, bit for bit.  Both sides run the one schedule,
mmf_loop_ref.drive."""
import contextlib
import copy
import ctypes as C
import time

import numpy as np
import pytest

import gcm_forcing_cases as gc
import mmf_loop_ref as mmf
import n2_modules_ref as nr
from oracle import awfl_oracle as ao
from parity_gate import compare, noise_floor, record

pytestmark = pytest.mark.gpu

# calls whose own tests hold them to their restatement bit for bit.  The P3 and SHOC coupling layers are among them where P3's pack runs
# no adjustment (SHOC is the SGS), with the device's x^y on the host as tests/test_p3_coupling_gpu.py and tests/test_shoc_coupling_gpu.py
# restate them
BITWISE = ("time_average_init", "msa_init", "vt_init", "rad_aggregate_init", "column_diagnostics_init", "flux_profiles_init", "msa_diagnose",
           "radiation", "sgs", "msa_accelerate", "vt_apply_forcing", "time_average_accumulate", "rad_aggregate", "column_diagnostics",
           "flux_profiles", "vt_compute_feedback", "compute_crm_feedback", "horizontal_average")

class Loop:
    """the stack on a coupler, initialised in the driver's order -- micro.init, sgs.init, dycore.init, the radiation's and the modules'
    init -- with the stack's state and entries loaded; the backend of mmf_loop_ref.drive on the Python classes"""

    def __init__(self, k, chunks=None, sync=False, load=True):
        import torch
        from pam_amd import Dycore, Microphysics, MicrophysicsP3, PamCoupler, Radiation, SGSNone, SGSShoc, SGSSmagorinsky, modules
        self.torch, self.k, self.modules, self.sync, self.vt_loaded = torch, k, modules, sync, False
        nz, ny, nx, nens = k.shape
        c = self.c = PamCoupler("cuda:0")
        c.set_option("crm_dt", k.dt)
        c.set_option("gcm_physics_dt", k.gcm_dt)
        c.allocate_coupler_state(nz, ny, nx, nens)
        c.set_grid(k.xlen, k.ylen, k.zint)
        if k.micro == "p3":
            self.micro = MicrophysicsP3(p3_main=MicrophysicsP3.standin(), layout=k.layout)
        else:
            self.micro = Microphysics()
        self.micro.init(c)
        if k.shoc:
            self.sgs = SGSShoc(shoc_main=SGSShoc.standin(), layout=k.layout)
        elif k.sgs == "smagorinsky":
            self.sgs = SGSSmagorinsky(cs=mmf.SGS_CS, prandtl=mmf.SGS_PRANDTL)
        else:
            self.sgs = SGSNone()
        self.sgs.init(c)
        self.dycore = Dycore()
        self.dycore.init(c)
        if chunks is not None:
            self.dycore.set_ensemble_chunks(chunks)
        c.set_option("rad_ny", k.rad[0])
        c.set_option("rad_nx", k.rad[1])
        self.rad = Radiation()
        self.rad.init(c)
        for o, v in (("sponge_num_layers", mmf.SPONGE["num_layers"]), ("sponge_time_scale", mmf.SPONGE["time_scale"]),
                     ("crm_accel_factor", k.accel), ("crm_accel_uv", k.accel_uv), ("crm_vt_u", k.vt_u), ("crm_vt_scale_limit", mmf.VT_LIMIT),
                     ("crm_diag_p_low", mmf.DIAG_PARAMS["p_low"]), ("crm_diag_p_high", mmf.DIAG_PARAMS["p_high"]),
                     ("crm_diag_cwp_threshold", mmf.DIAG_PARAMS["cwp_threshold"]), ("crm_prof_qc_threshold", mmf.PROF_QC)):
            c.set_option(o, v)
        modules.crm_feedback_init(c)
        self.dm = c.get_data_manager_device_readwrite()
        if load:
            self.load()

    def put(self, name, a):
        t = self.dm.get(name)
        t.copy_(self.torch.from_numpy(np.ascontiguousarray(a)).to(t.dtype))

    def load(self):
        """the stack's seeded fields and every entry the chain starts from that the inits registered; then surface_friction_init, whose
        z0 is held to the chain's and replaced by it, so that both loops start from the same bits"""
        k, c = self.k, self.c
        c.load_fields(k.fields)
        for n, a in k.S0.items():
            if self.dm.entry_exists(n):
                self.put(n, a)
        if k.friction:
            self.modules.surface_friction_init(c, np.full(k.shape[3], mmf.FRICTION_TAU), np.full(k.shape[3], mmf.FRICTION_BFLX))
            E = self.entries()
            assert np.abs(E["z0"] - k.S0["z0"]).max() <= 1e-12 * np.abs(k.S0["z0"]).max()
            assert mmf.same_bits(E["sfc_bflx"], k.S0["sfc_bflx"]) and not E["sfc_mom_flx_u"].any() and not E["sfc_mom_flx_v"].any()
            self.put("z0", k.S0["z0"])

    # ---- the backend of mmf_loop_ref.drive
    def set_option(self, name, value):
        self.c.set_option(name, value)

    def get_option(self, name):
        return self.c.get_option(name)

    def begin_gcm_step(self, g):
        pass

    def clock(self):
        return self.modules.MsaClock(self.k.nstop, self.k.accel)

    def call(self, name, **kw):
        ret = getattr(self, "_" + name)(**kw)
        if self.sync:
            self.torch.cuda.synchronize()
        return ret

    def _time_average_init(self):
        self.modules.time_average_init(self.c, [n for n, _ in mmf.time_average_names(self.k)])

    def _declare_hydrostatic(self):
        self.dycore.declare_current_profile_as_hydrostatic(self.c)

    def _compute_gcm_forcing(self):
        self.modules.compute_gcm_forcing_tendencies(self.c)

    def _msa_init(self):
        self.modules.msa_init(self.c)

    def _vt_init(self):
        self.modules.vt_init(self.c)
        if not self.vt_loaded:              # the GCM's input: registered zero-filled by the first vt_init
            for n in mmf.vt_names(self.k, "tend"):
                self.put(n, self.k.S0[n])
            self.vt_loaded = True

    def _rad_aggregate_init(self):
        self.modules.rad_aggregate_init(self.c)

    def _column_diagnostics_init(self):
        self.modules.column_diagnostics_init(self.c)

    def _flux_profiles_init(self):
        self.modules.flux_profiles_init(self.c)

    def _msa_diagnose(self):
        self.modules.msa_diagnose(self.c)

    def _apply_gcm_forcing(self):
        return self.modules.apply_gcm_forcing_tendencies(self.c)

    def _radiation(self):
        self.rad.timeStep(self.c)

    def _dycore(self):
        self.dycore.timeStep(self.c)

    def _sponge_layer(self):
        self.modules.sponge_layer(self.c)

    def _surface_friction(self):
        self.modules.compute_surface_friction(self.c)

    def _sgs(self):
        self.sgs.timeStep(self.c)

    def _micro(self):
        self.last_rainsplit = self.micro.timeStep(self.c)      # Kessler: the sub-cycles of its sedimentation

    def _saturation_adjustment(self):
        self.modules.saturation_adjustment(self.c)

    def _msa_accelerate(self):
        return self.modules.msa_accelerate(self.c)

    def _vt_apply_forcing(self, dt):
        self.modules.vt_apply_forcing(self.c, dt)

    def _time_average_accumulate(self, weight):
        self.modules.time_average_accumulate(self.c, [n for n, _ in mmf.time_average_names(self.k)], weight)

    def _rad_aggregate(self, weight):
        self.modules.rad_aggregate(self.c, weight)

    def _column_diagnostics(self, weight):
        self.modules.column_diagnostics(self.c, weight)

    def _flux_profiles(self, weight):
        self.modules.flux_profiles(self.c, weight)

    def _vt_compute_feedback(self):
        self.modules.vt_compute_feedback(self.c)

    def _compute_crm_feedback(self):
        self.modules.compute_crm_feedback(self.c)

    def _horizontal_average(self):
        self.modules.horizontal_average(self.c, [(n + "_time_average", v) for n, v in mmf.time_average_names(self.k)])

    def entries(self):
        """every entry of the DataManager, on the host, once the device is idle"""
        self.torch.cuda.synchronize()
        return {n: e["data"].cpu().numpy() for n, e in self.dm._e.items()}

    def finalize(self):
        self.micro.finalize(self.c)
        self.sgs.finalize(self.c)
        self.dycore.finalize(self.c)


def _same(a, b):
    return mmf.same_bits(a, b)


def _as_fields(k, E):
    return mmf.to_fields(k, E)


@pytest.mark.parametrize("name", tuple(mmf.STACKS))
def test_inits_leave_what_the_chains_tables_say(name):
    """after the inits in the driver's order: the tracer names, their order and flags, tracer_positive, tracer_adds_mass and idWV as the
    dycore registered them, the microphysics' constants in the options and in the dycore, the entries P3 and SHOC register (all zero
    before the stack is loaded), and after the per-GCM-step inits the gcm_forcing_tend_*, accel_*, vt_*, rad_*, crm_feedback_*, diag_*,
    prof_* and *_time_average entries present exactly where the stack's microphysics has the species; compute_time_step within 1e-14 of
    the oracle's.  Before that, as in the reference's driver: the gcm_* columns filled, broadcast_initial_gcm_column leaves the column in
    every cell bit for bit, and perturb_temperature with one seed per member stays inside the per-cell gate of tests/n2_modules_ref.py"""
    k = mmf.stack(name)
    L = Loop(k, load=False)
    c = L.c
    assert tuple(c.get_tracer_names()) == k.names
    assert tuple((n,) + tuple(c.get_tracer_info(n)[2:]) for n in k.names) == k.tracers
    E = L.entries()
    assert E["tracer_positive"].tolist() == list(k.positive) and E["tracer_adds_mass"].tolist() == list(k.adds_mass)
    assert c.get_option("idWV") == k.idwv and (k.micro != "p3" or k.idwv == mmf.IDWV_P3)
    for n, v in k.consts.items():
        assert c.get_option(n) == v and L.dycore.get_option(n) == v, n
    assert c.get_option("micro") == k.micro and c.get_option("sgs") == {"shoc": "shoc", "smagorinsky": "smagorinsky", "none": "none"}[k.sgs]
    if k.micro == "p3":
        assert (c.get_option("latvap"), c.get_option("latice")) == (mmf.LATVAP, mmf.LATICE)
        registered = mmf.P3_ENTRIES_4D + mmf.P3_ENTRIES_3D + ((mmf.SHOC_ENTRIES_4D + mmf.SHOC_ENTRIES_3D) if k.shoc else ())
        for n in registered + k.names:
            assert n in E and not E[n].any(), n
        assert ("cldfrac" in E) == k.shoc
    else:
        assert "precl" in E and not E["precl"].any() and "cldfrac" not in E and not c.option_exists("latvap")
    # the CRM starts from the GCM column
    for n, a in k.gcm0.items():
        L.put(n, a)
    L.modules.broadcast_initial_gcm_column(c)
    E = L.entries()
    for n in k.broadcast:
        assert _same(E[n], k.broadcast[n]), n
    keep = L.modules.perturb_temperature(c, k.ids, mmf.PERTURB_MAGNITUDE)
    got = L.entries()["temp"]
    del keep
    ref = nr.perturb(k.broadcast["temp"], k.ids, mmf.PERTURB_MAGNITUDE)
    worst, at = nr.worst_ratio(got, ref)
    assert worst < 1.0, (worst, at)
    assert np.abs(got - k.perturbed).max() <= 1e-12 * np.abs(k.perturbed).max()
    # the seeded state, then the per-GCM-step inits
    L.load()
    E = L.entries()
    fields = _as_fields(k, E)
    for n in mmf.STATE:
        assert _same(fields[n], k.fields[n]), n
    assert _same(fields["tracers"], k.fields["tracers"])
    for n, a in k.S0.items():
        assert n.startswith("vt_tend_") or _same(E[n], a), n
    chain = mmf.Chain(k)
    chain.call("declare_hydrostatic")
    want = chain.oracle.compute_time_step(copy.deepcopy(k.fields))
    L.call("declare_hydrostatic")
    assert abs(L.dycore.compute_time_step(c) - want) <= 1e-14 * want
    c.set_option("crm_accel_max_ttend", k.max_ttend[0])
    for call in ("time_average_init",) + (("compute_gcm_forcing",) if k.forcing else ()) + \
            ("msa_init", "vt_init", "rad_aggregate_init", "column_diagnostics_init", "flux_profiles_init"):
        L.call(call)
    E = L.entries()
    groups = {"gcm_forcing_tend_": mmf.GCM_FORCING_TEND if k.forcing else (),
              "accel_": ("accel_ceaseflag",) + tuple("accel_%s_%s" % (w, q) for w in ("save", "tend") for q in mmf.MSA_Q),
              "vt_": tuple(n for t in mmf.VT_TABLES for n in mmf.vt_names(k, t)), "rad_": mmf.rad_names(k) + ("rad_enthalpy_tend",),
              "crm_feedback_": mmf.feedback_names(k), "diag_": mmf.diag_names(k), "prof_": mmf.prof_names(k)}
    for prefix, names in groups.items():
        assert sorted(n for n in E if n.startswith(prefix)) == sorted(names), prefix
    assert sorted(n for n in E if n.endswith("_time_average")) == sorted(mmf.time_average_entries(k))
    assert c.get_option("crm_accel_ceaseflag") is False and not E["accel_ceaseflag"].any()
    L.finalize()


@contextlib.contextmanager
def _gcm_dt(dt):
    """tests/gcm_forcing_cases.py scales every tendency by its module constant DT_GCM, the gcm_physics_dt of its own cases: for the
    duration of one comparison it is the stack's"""
    keep = gc.DT_GCM
    gc.DT_GCM = dt
    try:
        yield
    finally:
        gc.DT_GCM = keep


def _forcing_gate(k, call, before, after, want, ret, ret_want, where):
    """one GCM-forcing call through the gate of tests/test_gcm_forcing_cells.py (gcm_forcing_cases.gate): per (field, level, member)
    scale, temp element-wise, the mask and the zero set of the application exactly the oracle's, tol = floor_gate(floor, 1e-11) with
    the floor of gcm_forcing_cases' own twins (all ten CRM fields carry the noise) through the oracle on the call's own input -- the
    twins of oracle_floor, with the tendencies the call was handed in place of ones computed anew.  The noise must move no decision:
    neither a mask nor a zero set"""
    crm = {n: np.ascontiguousarray(before[n]) for n in gc.CRM}
    gcm = {n: np.ascontiguousarray(before[n]) for n in gc.GCM}

    def run_of(E, computed, mask):
        steps = [] if call == "compute_gcm_forcing" else [dict(crm={n: E[n] for n in gc.CRM}, tend={n: E[n] for n in gc.DIAGNOSED}, mask=mask)]
        return dict(computed={n: computed[n] for n in gc.COMPUTED}, steps=steps)
    computed = want if call == "compute_gcm_forcing" else before
    exp = run_of(want, computed, ret_want)
    got = run_of(after, after if call == "compute_gcm_forcing" else before, ret)
    floor, problems = {}, []
    with _gcm_dt(k.gcm_dt):
        for i, twin in enumerate(gc.perturbed_twins(crm, mmf.FLOOR_SEED)):
            twin = {n: np.ascontiguousarray(a) for n, a in twin.items()}
            if call == "compute_gcm_forcing":
                run = run_of(None, ao.compute_gcm_forcing_tendencies(twin, gcm, k.gcm_dt), None)
            else:
                tend = {n: np.array(before[n], order="C") for n in gc.TEND}
                mask = ao.apply_gcm_forcing_tendencies(twin, gcm, tend, k.dz, k.dt, k.gcm_dt)
                run = run_of(dict(twin, **tend), before, mask)
                if gc.masks(run) != gc.masks(exp):
                    problems.append("twin %d: masks %s, not %s" % (i, gc.masks(run), gc.masks(exp)))
                if not np.array_equal(gc.zero_sets(run)[0], gc.zero_sets(exp)[0]):
                    problems.append("twin %d: water cells change between zero and non-zero" % i)
            for n, e in gc.run_errors(run, exp, crm, gcm).items():
                floor[n] = max(floor.get(n, 0.0), e)
        assert problems == [], where + (problems,)
        gc.gate(got, exp, crm, gcm, gc.tolerances(floor), what=str(where), floor=floor)


def _friction_gate(k, before, after):
    """compute_surface_friction through the gate of tests/test_moist_surface_cells.py: every cell of both fluxes within G_FLUX units of
    the binary128 reference at the slot-order means (moist_surface_cases.friction_reference, assert_fluxes_within)"""
    import moist_surface_cases as mc
    d = dict(rho_d=before["density_dry"], rho_v=before["water_vapor"], uvel=before["uvel"], vvel=before["vvel"], z0=before["z0"],
             bflx=before["sfc_bflx"], zint=k.zint, zmid=k.zmid)
    return mc.assert_fluxes_within(after["sfc_mom_flx_u"], after["sfc_mom_flx_v"], mc.friction_reference(d))


def _kessler_gate(k, L, before, after, where):
    """Kessler through the gate of tests/test_micro_kessler.py (kessler_cases.gate_against_oracle): the oracle at the device's sub-cycle
    count, which must be the oracle's own, its floor, the per-cell scale"""
    import kessler_cases as kc
    assert all(kc.C0[n] == k.consts[n] for n in ("R_d", "R_v", "cp_d", "p0"))
    pick = lambda E: dict(rho_v=E["water_vapor"], rho_c=E["cloud_liquid"], rho_r=E["precip_liquid"], rho_dry=E["density_dry"], temp=E["temp"])
    s_in = {n: np.array(a, order="C") for n, a in pick(before).items()}
    _, n_ref = kc.run_oracle(s_in, k.zmid, k.dt)
    assert L.last_rainsplit == n_ref, where + (L.last_rainsplit, n_ref)
    kc.gate_against_oracle(dict(pick(after), precl=after["precl"]), s_in, k.zmid, k.dt, n_ref, what=str(where))


class Held:
    """a Loop whose every call is held: every DataManager entry is read before and after it"""

    def __init__(self, L, R):
        self.L, self.R, self.k = L, R, L.k
        self.before = L.entries()
        self.g, self.t_cpu, self.calls = 0, 0.0, 0

    def set_option(self, name, value):
        self.L.set_option(name, value)
        self.R.set_option(name, value)

    def get_option(self, name):
        assert self.L.get_option(name) == self.R.get_option(name), name
        return self.L.get_option(name)

    def begin_gcm_step(self, g):
        self.g = g

    def clock(self):
        return self.L.clock()

    def call(self, name, **kw):
        import moist_surface_cases as mc
        k, R, before = self.k, self.R, self.before
        allowed = set(mmf.writes(k, name))
        ret = self.L.call(name, **kw)
        after = self.L.entries()
        t0 = time.time()
        where = (k.name, self.g, name)
        S = {n: before[n] for n in before}
        want, ret_want = getattr(R, "_" + name)(S, **kw)
        assert set(want) <= allowed, where
        assert ret == ret_want, where + (ret, ret_want)
        assert set(want) <= set(after), where + (sorted(set(want) - set(after)),)
        names = list(k.names)
        if name == "dycore":
            assert self.L.dycore.last_ncycles == R.info["nsub"], where
            assert abs(self.L.dycore.last_dt_dyn - R.info["dt_dyn"]) <= 1e-15 * R.info["dt_dyn"], where
            floor = noise_floor(lambda f: R.oracle.time_step(f, k.dt), _as_fields(k, before), names, mmf.FLOOR_SEED, base=_as_fields(k, want))
            compare(_as_fields(k, after), _as_fields(k, want), names, R.info["nsub"], floor=floor)
        elif name == "sponge_layer":
            X = nr.stack(_as_fields(k, before))
            ref = nr.sponge(X, k.zint, k.zmid, k.dt, mmf.SPONGE["num_layers"], mmf.SPONGE["time_scale"])
            got = nr.stack(_as_fields(k, after))
            bottom = k.shape[0] - mmf.SPONGE["num_layers"]
            assert np.array_equal(nr.bits(got[:, :bottom]), nr.bits(X[:, :bottom])), where
            worst, at = nr.worst_ratio(got, ref)
            assert worst < 1.0, where + (worst, at)
        elif name == "saturation_adjustment":
            cond = mmf.msref_condensate(k)
            pick = lambda E: dict(rho_v=E["water_vapor"], rho_c=E[cond], temp=E["temp"])
            exempt = mc.assert_adjusted_bits(pick(after), pick(want), R.info["saturation"], pick(before), rho_min=0.05)
            assert exempt <= 0.005 * after["temp"].size, where + (exempt,)
        elif name == "micro" and k.micro == "kessler":
            _kessler_gate(k, self.L, before, after, where)
        elif name in ("compute_gcm_forcing", "apply_gcm_forcing"):
            _forcing_gate(k, name, before, after, want, ret, ret_want, where)
        elif name == "surface_friction":
            _friction_gate(k, before, after)
        elif name in BITWISE or name == "micro":
            bad = [n for n in want if not _same(after[n], want[n])]
            assert bad == [], where + (bad,)
        else:                                                   # what the call declares, against the oracle's (the default mode: gravity)
            assert name == "declare_hydrostatic", name
            gv = np.array(R.oracle.variable_gravity)
            assert np.abs(after["variable_gravity"] - gv).max() <= 1e-12 * np.abs(gv).max(), where
        if name == "compute_gcm_forcing" and self.g == 0:      # registered by the call: zero but for what it computed
            assert all(not after[n].any() for n in mmf.GCM_FORCING_DIAGNOSED), where
        kept = [n for n in before if n not in allowed and n in after and not _same(before[n], after[n])]
        if name == "declare_hydrostatic":                       # the dycore's own profile arrays are what the call declares
            kept = [n for n in kept if n not in ("hy_dens_cells", "hy_pressure_cells", "variable_gravity")]
        assert kept == [], where + (kept,)
        self.t_cpu += time.time() - t0
        self.calls += 1
        self.before = after
        return ret


@pytest.mark.parametrize("name", ["mmf3d_p3shoc", "mmf2d_kessler"])
def test_every_call_of_both_gcm_steps_is_its_restatement_on_the_gpus_own_state(name):
    """call by call, the inits and the end-of-step calls included: every DataManager entry is read before and after the call.  A call
    whose own test holds it bit for bit (BITWISE, and the P3 and SHOC coupling layers of mmf3d_p3shoc): what its contract lists as written
    equals the restatement applied to the state from before the call, bit for bit.  The dycore: the oracle advanced one time_step from
    that state, through parity_gate.compare with that step's own noise floor; equal sub-step counts and last_dt_dyn within 1e-15.  The
    sponge layer: bits below the sponge and the per-cell gate of tests/n2_modules_ref.py inside it.  The saturation adjustment: the gate
    of tests/moist_surface_cases.py (bits, but for cells whose bisection margin is below MARGIN, at most 0.5 % of them).  Kessler: the
    gate of tests/test_micro_kessler.py (kessler_cases.gate_against_oracle: per-cell scale, the oracle's floor, equal sub-cycle counts).
    The two GCM-forcing calls: the gate of tests/test_gcm_forcing_cells.py (gcm_forcing_cases.gate: per level and member, the mask and
    the zero set exactly, the floor of its own twins, which must move no decision).  The surface friction: the per-cell gate of
    tests/test_moist_surface_cells.py against the binary128 reference.  declare_current_profile_as_hydrostatic: variable_gravity within
    1e-12 of the oracle's.  The return value of msa_accelerate, the option
    crm_accel_ceaseflag, the weight of MsaClock and the mask of apply_gcm_forcing_tendencies equal the chain's at every step.

    And after every call every entry outside the call's contract keeps its bits: density_dry under all physics (the GCM forcing is the
    one module that writes it); the gcm_* columns under everything; gcm_forcing_tend_* under everything but the two forcing calls, of
    which apply writes rho_v, rho_l and rho_i alone; the aggregates, diagnostics and profiles under everything between their init and
    their accumulate; vt_var_start_* under everything but vt_init; the cease word under everything but msa_init and msa_accelerate; the
    hydrostatic arrays under everything but declare_current_profile_as_hydrostatic; the grid and the flag arrays under everything"""
    k = mmf.stack(name)
    L = Loop(k)
    R = mmf.Chain(k)
    H = Held(L, R)
    log = mmf.drive(H, k)
    _, _, _, logs, _ = mmf.floors(k)
    for what in ("weights", "cease", "flag", "masks"):
        assert log[what] == logs[0][what], (what, log[what], logs[0][what])
    assert tuple(tuple(w) for w in log["weights"]) == mmf.WEIGHTS[name]
    if k.micro == "p3":
        steps = sum(len(w) for w in log["weights"])
        assert L.micro.etime == steps * k.dt and not L.micro.first_step and L.micro.sgs_shoc == k.shoc
    print("%s: %d calls held; the restatements took %.1f s on the host" % (name, H.calls, H.t_cpu))
    L.finalize()


def _run(k, chunks=None, sync=False):
    L = Loop(k, chunks, sync)
    log = mmf.drive(L, k)
    E = L.entries()
    etime = getattr(L.micro, "etime", None)
    L.finalize()
    return E, log, etime


# Measured on MI355X, worst / floor / gate of the free-running loop against the chain (the record's mmf_loop_<stack> entries;
# no quantity beyond 2.1 times its floor, none beyond 0.45 of its gate; rad_cld, the four diag_cld* and prof_cld 0 / 0 in every stack):
#   mmf3d_p3shoc (10,4,6,3), 2 GCM steps of 2 accelerated CRM steps: rho_d 3.8e-15, T 8.3e-15, vapour 8.5e-15 (gate 1e-12); the largest,
#     prof_flux_t 6.5e-13 / 6.4e-13 / 2.6e-12, vt_var_t 6.0e-13 / 4.8e-13 / 1.9e-12, prof_flux_u 4.7e-13 / 6.3e-13 / 2.5e-12, vt_feedback_t
#     3.3e-13 / 2.9e-13 / 1.2e-12, prof_flux_qt 3.2e-13 / 3.1e-13 / 1.2e-12; 6 of 64 gates above the minimum of 1e-12
#   mmf3d_members (8,3,4,65), 4 CRM steps of weight 1 and 2 accelerated ones, three member chunks: rho_d 4.8e-15, T 4.0e-15, vapour
#     3.2e-15; prof_flux_u 3.2e-12 / 2.3e-12 / 9.0e-12, prof_mcup 2.6e-12 / 1.9e-12 / 7.6e-12, wvel 1.3e-12 / 1.3e-12 / 5.2e-12,
#     prof_mcuup 7.2e-13 / 5.7e-13 / 2.3e-12, prof_mcdn 5.0e-13 / 2.9e-13 / 1.2e-12; 11 of 61 gates above 1e-12
#   mmf2d_kessler (10,1,8,66), 2 GCM steps of 2 accelerated CRM steps: rho_d 4.4e-15, T 5.3e-15, vapour 2.2e-14; prof_flux_t 1.7e-12 /
#     1.8e-12 / 7.3e-12, prof_mcudn 1.2e-12 / 7.0e-13 / 2.8e-12, prof_mcuup 1.1e-12 / 9.8e-13 / 3.9e-12, wvel 9.6e-13 / 5.7e-13 / 2.3e-12,
#     vt_var_t 9.1e-13 / 1.4e-12 / 5.5e-12; 11 of 49 gates above 1e-12
@pytest.mark.parametrize("name", tuple(mmf.STACKS))
def test_free_running_loop_matches_the_chain_and_does_not_depend_on_host_synchronisation(name):
    """both GCM steps with no host synchronisation beyond what the calls themselves do (the dycore in three member chunks on
    mmf3d_members), against the chain through parity_gate: the five state fields and every tracer as crm_loop_ref.gates sets them (rho_d,
    temp and the vapour at 1e-12, the rest at min(1e-8, max(1e-12, 4 floor))); every GCM-step output -- aggregates, feedback means and
    tendencies, vt_var_* and vt_feedback_*, diagnostics, profiles, the averaged time averages, the surface precipitation -- at min(1e-10,
    max(1e-12, 4 floor)), with the floors of the chain's twins; a tendency relative to the largest mean divided by gcm_physics_dt.  The
    weights, the cease decisions, the option crm_accel_ceaseflag after every CRM step and the hole-filling masks equal the chain's
    exactly, and P3's etime counts the CRM steps of both GCM steps.  Then the same loop with a synchronisation after every call: every
    entry of the DataManager has the bits of the unsynchronised run"""
    k = mmf.stack(name)
    chunks = 3 if name == "mmf3d_members" else None
    t0 = time.time()
    base, held, floor, logs, _ = mmf.floors(k)
    gate = mmf.gates(k, base, floor)
    t_cpu = time.time() - t0
    t0 = time.time()
    free, log, etime = _run(k, chunks)
    t_gpu = time.time() - t0
    for what in ("weights", "cease", "flag", "masks"):
        assert log[what] == logs[0][what], (what, log[what], logs[0][what])
    assert tuple(tuple(w) for w in log["weights"]) == mmf.WEIGHTS[name]
    if k.micro == "p3":
        assert etime == sum(len(w) for w in log["weights"]) * k.dt
    worst = mmf.errors(k, _as_fields(k, free), free, base, held)
    record("mmf_loop_" + name, {n: dict(worst=worst[n], floor=floor.get(n), gate=gate[n]) for n in worst})
    print("%s %s: chain and twins %.1f s, GPU loop %.1f s" % (name, k.shape, t_cpu, t_gpu))
    for n in worst:
        print("   %-52s worst %.2e floor %.2e gate %.2e" % (n, worst[n], floor.get(n, float("nan")), gate[n]))
    for n in worst:
        assert worst[n] <= gate[n], (n, worst[n], gate[n], floor.get(n))
    synced, log_s, _ = _run(k, chunks, sync=True)
    assert log_s == log
    differ = [n for n in free if not _same(free[n], synced[n])]
    assert differ == [], differ


class Pair:
    """two Loops over two member ranges of one stack in lock step, joined by hand where the ensemble decides as one: the dycore's time
    step is the smaller of the two compute_time_step (pam_amd/parallel.py: sharded_time_step), the cease flag the larger of the two
    (the all-reduce(MAX) of msa_accelerate's group), the hole-filling mask the union"""

    def __init__(self, parts):
        self.parts, self.k = parts, parts[0].k

    def set_option(self, name, value):
        for L in self.parts:
            L.set_option(name, value)

    def get_option(self, name):
        values = [L.get_option(name) for L in self.parts]
        assert len(set(values)) == 1, (name, values)
        return values[0]

    def begin_gcm_step(self, g):
        pass

    def clock(self):
        return self.parts[0].clock()

    def call(self, name, **kw):
        if name == "dycore":
            dt = min(L.dycore.compute_time_step(L.c) for L in self.parts)
            for L in self.parts:
                L.dycore.timeStep(L.c, dt_dyn_hint=dt)
            return None
        if name == "msa_accelerate":
            return self._msa_accelerate()
        rets = [L.call(name, **kw) for L in self.parts]
        if name == "apply_gcm_forcing":
            return rets[0] | rets[1]
        return rets[0]

    def _msa_accelerate(self):
        """modules.msa_accelerate with the flag joined between the tendencies and the apply"""
        from pam_amd import capi, modules
        lib, torch = capi.load(), self.parts[0].torch
        args, flags = [], []
        for L in self.parts:
            c = L.c
            fields, save, tend, cease = modules._msa_arrays(c)
            mine = C.c_int(0)
            with torch.cuda.device(c.device):
                stream = torch.cuda.current_stream(c.device).cuda_stream
                capi.check(lib.pam_amd_msa_tendencies(c.get_nens(), c.get_nx(), c.get_ny(), c.get_nz(), modules._msa_table(fields),
                                                      modules._msa_table(save), modules._msa_table(tend),
                                                      float(c.get_option("crm_accel_max_ttend")), cease.data_ptr(), C.byref(mine), stream))
            args.append((c, fields, tend, cease, stream))
            flags.append(mine.value)
        flag = max(flags)
        for (c, fields, tend, cease, stream), mine in zip(args, flags):
            if flag:
                if not mine:
                    cease.fill_(1)
                c.set_option("crm_accel_ceaseflag", True)
                continue
            with torch.cuda.device(c.device):
                capi.check(lib.pam_amd_msa_apply(c.get_nens(), c.get_nx(), c.get_ny(), c.get_nz(), modules._msa_table(fields),
                                                 modules._msa_table(tend), float(c.get_option("crm_accel_factor")),
                                                 1 if c.get_option("crm_accel_uv") else 0, cease.data_ptr(), stream))
        return bool(flag)


def test_members_run_as_two_ranges_equal_the_whole_ensemble_bit_for_bit():
    """mmf3d_members again as the members 0..36 and 37..64 on two couplers, the cease flag, the dycore's time step and the mask joined
    by hand: every entry with a member dimension equals the whole run's, bit for bit, and so do the weights, the cease decisions and the
    masks"""
    k = mmf.stack("mmf3d_members")
    whole, log, _ = _run(k)
    cuts = ((0, 37), (37, 65))
    parts = [Loop(mmf.members(k, lo, hi)) for lo, hi in cuts]
    log_p = mmf.drive(Pair(parts), k)
    assert log_p == log
    nens = k.shape[3]
    for L, (lo, hi) in zip(parts, cuts):
        E = L.entries()
        differ = [n for n, a in E.items() if a.ndim and a.shape[-1] == hi - lo and whole[n].shape[-1] == nens
                  and not _same(a, np.ascontiguousarray(whole[n][..., lo:hi]))]
        assert differ == [], ((lo, hi), differ)
        assert E["accel_ceaseflag"].tolist() == whole["accel_ceaseflag"].tolist()
        L.finalize()
