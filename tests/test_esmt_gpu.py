"""Explicit scalar momentum transport on the GPU: the three entry points against the numpy restatement (tests/esmt_ref.py) bit for bit on
every named case, through the C ABI and through pam_amd.modules; the end-to-end CRM loop with and without the two scalars; the GCM
round trip.  The driver's --esmt has its own file (tests/test_esmt_driver_gpu.py)."""
import numpy as np
import pytest

import esmt_ref as ref
import esmt_cases as ec
from esmt_harness import MEANS, POISON, call_arguments

RD, RV = ref.RD, ref.RV


class GpuBackend:
    """the interface of esmt_ref.RefBackend over the C ABI: diagnose, then the force with the means it gave; the means, the
    tendencies and the workspace are poisoned before the calls"""

    def __init__(self, wide=False):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check, self.wide = torch, capi.load(), capi.check, wide

    def dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")

    def _diagnose(self, case, sizes, dF, dprof, dmeans, dtend, feedback, with_gcm):
        P = lambda t: None if t is None else t.data_ptr()
        nens, nx, nz = sizes
        self.check(self.lib.pam_amd_esmt_diagnose(nens, nx, 1, nz, P(dF[RD]), P(dF[RV]), P(dF["esmt_u"]), P(dF["esmt_v"]),
                                                  *[P(dmeans[n]) for n in MEANS], P(dprof["gcm_u"]) if with_gcm else None,
                                                  P(dprof["gcm_v"]) if with_gcm else None, float(case["gcm_dt"]), 1 if feedback else 0,
                                                  P(dtend["u"]) if with_gcm else None, P(dtend["v"]) if with_gcm else None,
                                                  self.torch.cuda.current_stream().cuda_stream))

    def diagnose(self, case, feedback=False):
        F, sizes, prof, means, tend, _ = call_arguments(case)
        dF, dprof = {n: self.dev(a) for n, a in F.items()}, {n: self.dev(a) for n, a in prof.items()}
        dmeans, dtend = {n: self.dev(a) for n, a in means.items()}, {n: self.dev(a) for n, a in tend.items()}
        self._diagnose(case, sizes, dF, dprof, dmeans, dtend, feedback, True)
        self.torch.cuda.synchronize()
        out = {n: t.cpu().numpy() for n, t in dmeans.items()}
        out.update({"tend_" + x: t.cpu().numpy() for x, t in dtend.items() if t is not None})
        return out

    def run(self, case, with_everything=False):
        F, sizes, prof, means, tend, work = call_arguments(case)
        nens, nx, nz = sizes
        dF, dprof = {n: self.dev(a) for n, a in F.items()}, {n: self.dev(a) for n, a in prof.items()}
        dmeans, dwork = {n: self.dev(a) for n, a in means.items()}, self.dev(work)
        P = lambda t: None if t is None else t.data_ptr()
        kmax = int(case["kmax"])
        need = self.lib.pam_amd_esmt_workspace_doubles(nens, nz, kmax)
        assert need == 6 * kmax * nz * nens and dwork.numel() >= need
        self.check(self.lib.pam_amd_esmt_debug_wide_index(1 if self.wide else 0))
        try:
            self._diagnose(case, sizes, dF, dprof, dmeans, None, False, False)
            self.check(self.lib.pam_amd_esmt_pgf(nens, nx, 1, nz, P(dF["esmt_u"]), P(dF["esmt_v"]), P(dF["wvel"]), P(dF[RD]), P(dF[RV]),
                                                 P(dprof["zmid"]), P(dprof["dz"]), P(dmeans["rho_mean"]), P(dmeans["u_mean"]),
                                                 None if case.get("skip_v") else P(dmeans["v_mean"]), P(dprof["force_u"]), P(dprof["force_v"]),
                                                 P(dprof["cos"]), P(dprof["sin"]), float(case["dx"]), float(case["dt"]), kmax,
                                                 P(dwork) if kmax > 0 else None, need, self.torch.cuda.current_stream().cuda_stream))
            self.torch.cuda.synchronize()
        finally:
            self.lib.pam_amd_esmt_debug_wide_index(0)
        out = {n: dF[n].cpu().numpy() for n in ref.SCALARS}
        if not with_everything:
            return out
        back = lambda t: None if t is None else t.cpu().numpy()
        return out, {n: back(t) for n, t in dmeans.items()}, {n: back(t) for n, t in dprof.items()}, {n: back(dF[n]) for n in dF if n not in out}

    def set(self, rho_d, rho_v, src_u, src_v):
        nz, _, nx, nens = rho_d.shape
        d = [self.dev(a) for a in (rho_d, rho_v, src_u, src_v)]
        eu, ev = self.dev(np.full(rho_d.shape, POISON)), self.dev(np.full(rho_d.shape, POISON))
        self.check(self.lib.pam_amd_esmt_set(nens, nx, 1, nz, *[t.data_ptr() for t in d], eu.data_ptr(), ev.data_ptr(),
                                             self.torch.cuda.current_stream().cuda_stream))
        self.torch.cuda.synchronize()
        return eu.cpu().numpy(), ev.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("wide", (False, True), ids=("narrow", "wide"))
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ref.shape_id)
def test_gpu_pgf_matches_restatement_bit_for_bit(shape, wide):
    """every named case (the only size-dependent path is the index width); one case twice: two runs are identical"""
    be = GpuBackend(wide)
    for name in ec.CASE_NAMES:
        assert ref.results_differ(be.run(ec.cases(shape)[name]), ec.reference(shape, name), nan_by_place=True) == [], name
    a, b = (be.run(ec.cases(shape)["all_on"]) for _ in range(2))
    assert ref.results_differ(a, b) == []


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ref.shape_id)
def test_gpu_set_and_diagnose_match_restatement_bit_for_bit(shape):
    be = GpuBackend()
    case = ec.cases(shape)["all_on"]
    F = case["fields"]
    for feedback in (False, True):
        got, want = be.diagnose(case, feedback), ref.diagnose(case, feedback)
        assert sorted(got) == sorted(want) and ref.results_differ(got, want) == [], feedback
        assert not any((a == POISON).any() for a in got.values())
    eu, ev = be.set(F[RD], F[RV], case["gcm_u"], case["gcm_v"])
    wu, wv = ref.set_scalars(F[RD], F[RV], case["gcm_u"], case["gcm_v"])
    assert ref.same_bits(eu, wu) and ref.same_bits(ev, wv)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in ec.SHAPES if s[2] >= 64], ids=ref.shape_id)
def test_gpu_members_split_over_calls_equal_the_whole(shape):
    """shards of unequal size (70 = 1 + 5 + 64) give the bits of the whole ensemble"""
    nens, be = shape[2], GpuBackend()
    for name in ("all_on", "nan_w"):
        case, want = ec.cases(shape)[name], ec.reference(shape, name)
        parts = [be.run(ref.members(case, slice(lo, hi))) for lo, hi in ((0, 1), (1, 6), (6, nens))]
        got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
        assert ref.results_differ(got, want, nan_by_place=True) == [], name


@pytest.mark.gpu
def test_gpu_bystanders_and_read_only_inputs():
    """the means were poisoned before the call and hold the restatement's bits after it; wvel, the densities, every profile and both
    tables keep their bits; tensors allocated before and after the calls keep theirs; without a mean esmt_v keeps every bit"""
    import torch
    shape = (5, 21, 3)
    before = torch.full((4096,), 3.25, dtype=torch.float64, device="cuda:0")
    for name in ("all_on", "no_v_mean", "kmax0"):
        case = ec.cases(shape)[name]
        out, means, prof, untouched = GpuBackend().run(case, with_everything=True)
        after = torch.full((4096,), 3.25, dtype=torch.float64, device="cuda:0")
        assert ref.results_differ(out, ec.reference(shape, name)) == [], name
        assert ref.results_differ(means, {n: v for n, v in ref.diagnose(case).items() if n in MEANS}) == [], name
        for n, a in prof.items():
            assert a is None or ref.same_bits(a, np.asarray(case[n], dtype=np.float64)), (name, n)
        assert set(untouched) == {"wvel", RD, RV}
        for n, a in untouched.items():
            assert ref.same_bits(a, case["fields"][n]), (name, n)
        if name == "no_v_mean":
            assert ref.same_bits(out["esmt_v"], case["fields"]["esmt_v"])
        assert (before == 3.25).all() and (after == 3.25).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python functions through a coupler

KESSLER = ("water_vapor", "cloud_liquid", "precip_liquid")


def _coupler(shape, zint, dt, dx, kmax=None, gcm_dt=1200.0):
    """a coupler with Kessler's tracers and the two scalars, on per-member interfaces zint (nz+1,nens)"""
    import torch
    from pam_amd import PamCoupler, modules
    nz, nx, nens = shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", dt)
    c.set_option("gcm_physics_dt", gcm_dt)
    c.allocate_coupler_state(nz, 1, nx, nens)
    c.set_grid(nx * dx, dx, zint)
    for n in KESSLER:
        c.add_tracer(n, "", True, True)
    modules.esmt_init(c, kmax)
    return c, c.get_data_manager_device_readwrite()


def _read(dm, names):
    return {n: dm.get(n, readonly=True).cpu().numpy() for n in names}


def _case_from_coupler(dm, case):
    """the case with the grid and the tables the coupler holds: zmid = 0.5 (zint(k) + zint(k+1)) and the library's tables are the
    coupler's own arithmetic, so the restatement takes them from it"""
    got = _read(dm, ("vertical_midpoint_height", "vertical_cell_dz", "esmt_cos", "esmt_sin"))
    return dict(case, zmid=got["vertical_midpoint_height"], dz=got["vertical_cell_dz"], cos=got["esmt_cos"], sin=got["esmt_sin"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((5, 21, 3), (5, 65, 70), (2, 2, 1)), ids=ref.shape_id)
def test_gpu_python_functions_through_a_coupler(shape):
    """esmt_pgf gives the restatement's bits with and without the forcing and with kmax = 1; esmt_compute_forcing and
    esmt_compute_feedback give diagnose's two senses; wvel, the densities and every other tracer keep their bits"""
    import torch
    from pam_amd import modules
    nz, nx, nens = shape
    base = ec.cases(shape)["all_on"]
    zint = np.concatenate([np.zeros((1, nens)), np.cumsum(base["dz"], axis=0)])
    for name, kmax, forcing in (("all_on", None, True), ("no_force", None, False), ("kmax1", 1, True)):
        case = ec.cases(shape)[name]
        c, dm = _coupler(shape, zint, case["dt"], case["dx"], kmax, case["gcm_dt"])
        assert c.get_tracer_names() == list(KESSLER) + ["esmt_u", "esmt_v"]
        case = _case_from_coupler(dm, case)
        for n, a in case["fields"].items():
            dm.get(n).copy_(torch.from_numpy(a))
        dm.get("cloud_liquid").fill_(1.0e-4)
        dm.get("gcm_uvel").copy_(torch.from_numpy(case["gcm_u"]))
        dm.get("gcm_vvel").copy_(torch.from_numpy(case["gcm_v"]))
        modules.esmt_compute_forcing(c)
        want = ref.diagnose(case, False)
        got = _read(dm, ("esmt_u_forcing", "esmt_v_forcing", "esmt_rho_mean", "esmt_u_mean", "esmt_v_mean"))
        assert ref.same_bits(got["esmt_u_forcing"], want["tend_u"]) and ref.same_bits(got["esmt_v_forcing"], want["tend_v"]), name
        assert all(ref.same_bits(got["esmt_" + n], want[n]) for n in ("rho_mean", "u_mean", "v_mean")), name
        forced = dict(case, force_u=want["tend_u"] if forcing else None, force_v=want["tend_v"] if forcing else None)
        held = _read(dm, ("wvel", RD, RV, "cloud_liquid", "precip_liquid", "esmt_u_forcing", "esmt_cos"))
        modules.esmt_pgf(c, forcing=forcing)
        torch.cuda.synchronize()
        after = ref.pgf(forced)
        assert ref.results_differ(_read(dm, ref.SCALARS), after) == [], name
        assert ref.results_differ(_read(dm, list(held)), held) == [], name
        modules.esmt_compute_feedback(c)
        back = ref.diagnose(dict(case, fields=dict(case["fields"], **after)), True)
        got = _read(dm, ("esmt_u_tend", "esmt_v_tend"))
        assert ref.same_bits(got["esmt_u_tend"], back["tend_u"]) and ref.same_bits(got["esmt_v_tend"], back["tend_v"]), name


@pytest.mark.gpu
def test_gpu_set_from_the_gcm_and_from_the_crm():
    import torch
    from pam_amd import modules
    shape = (5, 21, 3)
    nz, nx, nens = shape
    case = ec.cases(shape)["all_on"]
    F = case["fields"]
    c, dm = _coupler(shape, np.concatenate([np.zeros((1, nens)), np.cumsum(case["dz"], axis=0)]), case["dt"], case["dx"])
    for n in ("wvel", RD, RV):
        dm.get(n).copy_(torch.from_numpy(F[n]))
    rng = np.random.default_rng(5)
    u, v = 16.0 * rng.random(F[RD].shape) - 8.0, 16.0 * rng.random(F[RD].shape) - 8.0
    dm.get("uvel").copy_(torch.from_numpy(u))
    dm.get("vvel").copy_(torch.from_numpy(v))
    dm.get("gcm_uvel").copy_(torch.from_numpy(case["gcm_u"]))
    dm.get("gcm_vvel").copy_(torch.from_numpy(case["gcm_v"]))
    modules.esmt_set(c, "gcm")
    wu, wv = ref.set_scalars(F[RD], F[RV], case["gcm_u"], case["gcm_v"])
    got = _read(dm, ref.SCALARS)
    assert ref.same_bits(got["esmt_u"], wu) and ref.same_bits(got["esmt_v"], wv)
    modules.esmt_set(c)                                       # the default source is the GCM
    assert ref.results_differ(_read(dm, ref.SCALARS), got) == []
    modules.esmt_set(c, "crm")
    wu, wv = ref.set_scalars(F[RD], F[RV], ref.level_mean(u), ref.level_mean(v))
    got = _read(dm, ref.SCALARS + ("uvel", "vvel"))
    assert ref.same_bits(got["esmt_u"], wu) and ref.same_bits(got["esmt_v"], wv)
    assert ref.same_bits(got["uvel"], u) and ref.same_bits(got["vvel"], v)


# ------------------------------------------------------------------------------------------------------------------------------
# the GCM round trip on a state at rest (wvel == 0): nothing but the forcing acts

@pytest.mark.gpu
def test_gpu_gcm_round_trip_on_a_state_at_rest():
    """esmt_set("gcm"), esmt_compute_forcing, steps, esmt_compute_feedback: the feedback has the bits of the chain of the restatements,
    and esmt_x_tend + esmt_x_forcing is zero within the bound on the level means of tests/esmt_cases.py (mean_bound with T == 0: each of
    the steps and each of the two diagnoses moves a mean by no more than one such bound, and the sum is that over gcm_physics_dt).  Then
    the GCM moves on by a known profile and gcm_physics_dt / crm_dt forced steps land the level means on it within the same bound."""
    import torch
    from pam_amd import modules
    shape = (5, 21, 3)
    nz, nx, nens = shape
    base = ec.cases(shape)["all_on"]
    dt, steps = 10.0, 4
    gcm_dt = steps * dt
    c, dm = _coupler(shape, np.concatenate([np.zeros((1, nens)), np.cumsum(base["dz"], axis=0)]), dt, base["dx"], None, gcm_dt)
    case = _case_from_coupler(dm, dict(base, dt=dt, gcm_dt=gcm_dt))
    F = dict(case["fields"], wvel=np.zeros_like(case["fields"]["wvel"]))
    for n in ("wvel", RD, RV):
        dm.get(n).copy_(torch.from_numpy(F[n]))
    dm.get("gcm_uvel").copy_(torch.from_numpy(case["gcm_u"]))
    dm.get("gcm_vvel").copy_(torch.from_numpy(case["gcm_v"]))
    for moved in (False, True):
        modules.esmt_set(c, "gcm")
        F["esmt_u"], F["esmt_v"] = ref.set_scalars(F[RD], F[RV], case["gcm_u"], case["gcm_v"])
        gcm = {x: case["gcm_" + x] + (0.5 + 0.01 * np.arange(nz))[:, None] if moved else case["gcm_" + x] for x in "uv"}
        dm.get("gcm_uvel").copy_(torch.from_numpy(gcm["u"]))
        dm.get("gcm_vvel").copy_(torch.from_numpy(gcm["v"]))
        modules.esmt_compute_forcing(c)
        state = dict(case, fields=dict(F), gcm_u=gcm["u"], gcm_v=gcm["v"])
        force = ref.diagnose(state, False)
        for _ in range(steps):
            modules.esmt_pgf(c)
            state = dict(state, fields=dict(state["fields"], **ref.pgf(dict(state, force_u=force["tend_u"], force_v=force["tend_v"]))))
        modules.esmt_compute_feedback(c)
        torch.cuda.synchronize()
        want = ref.diagnose(state, True)
        got = _read(dm, ("esmt_u_tend", "esmt_v_tend", "esmt_u_forcing", "esmt_v_forcing") + ref.SCALARS)
        assert ref.results_differ({n: got[n] for n in ref.SCALARS}, {n: state["fields"][n] for n in ref.SCALARS}) == []
        bound = (steps + 2) * ec.mean_bound(dict(state, force_u=force["tend_u"], force_v=force["tend_v"]), 0.0) / gcm_dt
        for x in "uv":
            assert ref.same_bits(got["esmt_%s_tend" % x], want["tend_" + x]) and ref.same_bits(got["esmt_%s_forcing" % x], force["tend_" + x]), x
            if moved:          # the forcing carried the mean onto the new profile: nothing is left to hand back
                worst = np.abs(got["esmt_%s_tend" % x]).max()
                assert np.abs(got["esmt_%s_forcing" % x]).min() > 0.4 / gcm_dt
            else:
                worst = np.abs(got["esmt_%s_tend" % x] + got["esmt_%s_forcing" % x]).max()
            print("round trip", "moved" if moved else "at rest", x, "%.3e" % worst, "bound %.3e" % bound)
            assert worst <= bound, (moved, x)


# ------------------------------------------------------------------------------------------------------------------------------
# end to end: two CRM steps of dycore -> sponge -> esmt_pgf -> Kessler, with and without the two scalars

def _crm_run(with_esmt):
    import torch
    from pam_amd import Dycore, Microphysics, PamCoupler, idealized as idz, modules
    nens, nx, ny, nz, crm_dt = 3, 16, 1, 12, 2.0
    zint = idz.stretched_interfaces(nz, 12000.0)
    xlen = nx * 500.0
    f = idz.dry_bubble_fields(nens, nx, ny, nz, xlen, xlen, zint, tracers=idz.TRACERS_KESSLER_SHOC[:3])
    zmid = 0.5 * (zint[:-1] + zint[1:])
    f["uvel"] = f["uvel"] + (6.0 * zmid / zmid[-1])[:, None, None, None]          # a sheared wind for the scalars to take
    f["vvel"] = f["vvel"] + (2.0 - 3.0 * np.tanh(zmid / 4000.0))[:, None, None, None]
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", crm_dt)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(xlen, xlen, zint)
    micro, dyc = Microphysics(), Dycore()
    micro.init(c)
    if with_esmt:
        modules.esmt_init(c)
    dyc.init(c)
    dm = c.get_data_manager_device_readwrite()
    for n in ("density_dry", "uvel", "vvel", "wvel", "temp"):
        dm.get(n).copy_(torch.from_numpy(np.ascontiguousarray(f[n])))
    dm.get("water_vapor").copy_(torch.from_numpy(np.ascontiguousarray(0.012 * f["density_dry"] * np.exp(-zmid / 3000.0)[:, None, None, None])))
    dyc.declare_current_profile_as_hydrostatic(c)
    if with_esmt:
        modules.esmt_set(c, source="crm")
    for _ in range(2):
        dyc.timeStep(c)
        modules.sponge_layer(c)
        if with_esmt:
            modules.esmt_pgf(c, forcing=False)
        c.run_module("micro", micro.timeStep)
    torch.cuda.synchronize()
    names = ["uvel", "vvel", "wvel", "temp", "density_dry"] + c.get_tracer_names()
    out = _read(dm, names)
    dyc.finalize(c)
    return out


@pytest.mark.gpu
def test_gpu_two_crm_steps_with_the_scalars_leave_every_other_field_bit_identical():
    """the scalars add no mass and enter no state equation: uvel, vvel, wvel, temp, density_dry and Kessler's tracers have the bits of the
    run without them; every field is finite; the scalars moved, and stay within the range of the wind they were set from"""
    plain, with_scalars = _crm_run(False), _crm_run(True)
    assert sorted(with_scalars) == sorted(list(plain) + list(ref.SCALARS))
    for n, a in with_scalars.items():
        assert np.isfinite(a).all(), n
    assert ref.results_differ(with_scalars, plain) == []
    rho = with_scalars["density_dry"] + with_scalars["water_vapor"]
    us, vs = with_scalars["esmt_u"] / rho, with_scalars["esmt_v"] / rho
    assert 0.0 < us.min() and us.max() < 6.5 and -1.5 < vs.min() and vs.max() < 2.5
    assert np.ptp(us, axis=2).max() > 1.0e-6                 # the bubble's updraught acted on the sheared scalar
