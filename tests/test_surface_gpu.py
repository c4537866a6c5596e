"""Bulk surface fluxes over a slab ocean on the GPU: pam_amd_surface_fluxes against the numpy restatement (tests/surface_ref.py) bit for
bit (a NaN by its place) on every shape and named case, and run to run; members split over calls against the whole; a bystander tensor,
the read-only inputs, poisoned upper levels and a side stream; the Python functions through a coupler with Kessler's tracer names; the
closed loop of radiation, surface and SGS against the chain of the restatements with the energy budget of column plus slab; and
modules/surface_fluxes.h through examples/driver --surface on a shortened CI input."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import grayrad_ref as lwref
import grayrad_cases as lwc
import grayrad_sw_ref as swref
import grayrad_sw_cases as swc
import sgs_ref
import sgs_moist_ref as mref
import surface_ref as ref
import surface_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")
POISON = -7.0e77
U = 2.0 ** -53
LD = np.longdouble


class GpuBackend:
    """the interface of surface_ref.RefBackend over the C ABI.  The 4-D fields go up with the levels above 0 POISONED (the scheme reads
    level 0 alone), and the two flux outputs poisoned"""

    def __init__(self):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check = torch, capi.load(), capi.check

    def _dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")

    def upload(self, case):
        dev = {}
        for n in ref.FIELDS:
            a = np.array(case["fields"][n], dtype=np.float64, order="C")
            a[1:] = POISON
            dev[n] = self._dev(a)
        for n in ("zmid", "cn", "cstar", "sfc_temp") + ref.RADIATION:
            dev[n] = self._dev(case.get(n))
        col = dev["sfc_temp"].shape
        for n in ("sfc_shf", "sfc_lhf"):
            dev[n] = self.torch.full(tuple(col), POISON, dtype=self.torch.float64, device="cuda:0")
        return dev

    def call(self, case, dev, stream=None):
        nz, ny, nx, nens = dev["temp"].shape
        assert tuple(dev["zmid"].shape) == (nz, nens) and tuple(dev["cn"].shape) == (nens,) == tuple(dev["cstar"].shape)
        stream = self.torch.cuda.current_stream().cuda_stream if stream is None else stream
        rad = [None if dev[n] is None else dev[n].data_ptr() for n in ref.RADIATION]
        self.check(self.lib.pam_amd_surface_fluxes(nens, nx, ny, nz, *[dev[n].data_ptr() for n in ref.FIELDS], dev["zmid"].data_ptr(),
                                                   dev["cn"].data_ptr(), dev["cstar"].data_ptr(), dev["sfc_temp"].data_ptr(), *rad,
                                                   *[float(case[n]) for n in ref.SCALARS], dev["sfc_shf"].data_ptr(), dev["sfc_lhf"].data_ptr(),
                                                   stream))

    def run(self, case):
        dev = self.upload(case)
        self.call(case, dev)
        self.torch.cuda.synchronize()
        return {n: dev[n].cpu().numpy() for n in ref.OUTPUTS}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sc.SHAPES, ids=ref.shape_id)
def test_gpu_matches_restatement_bit_for_bit(shape):
    """every named case, with the levels above 0 poisoned; one case twice: two runs are identical; without a slab and with dt = 0 sfc_temp
    keeps its bits"""
    be = GpuBackend()
    for name in sc.CASE_NAMES:
        got = be.run(sc.cases(shape)[name])
        assert ref.results_differ(got, sc.outputs(sc.reference(shape, name)), nan_by_place=True) == [], name
    a, b = (be.run(sc.cases(shape)["mixed"]) for _ in range(2))
    assert ref.results_differ(a, b) == []
    for name in ("slab_off", "dt_zero"):
        assert ref.same_bits(be.run(sc.cases(shape)[name])["sfc_temp"], sc.cases(shape)[name]["sfc_temp"]), name


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in sc.SHAPES if s[3] >= 64], ids=ref.shape_id)
def test_gpu_members_split_over_calls_equal_the_whole(shape):
    nens, be = shape[3], GpuBackend()
    for name in ("mixed", "nan_cell", "lw_only"):
        case, want = sc.cases(shape)[name], sc.outputs(sc.reference(shape, name))
        parts = [be.run(ref.members(case, slice(lo, hi))) for lo, hi in ((0, 1), (1, 37), (37, nens))]
        got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
        assert ref.results_differ(got, want, nan_by_place=True) == [], name


@pytest.mark.gpu
def test_gpu_bystander_tensor_read_only_inputs_and_a_side_stream():
    """tensors allocated before and after the fields keep their bits, and so does every read-only input, the poison of the upper levels
    included; the call on a non-default stream, the fields produced on that stream just before it, gives the restatement's bits"""
    import torch
    shape = (7, 3, 2, 65)
    case, want = sc.cases(shape)["mixed"], sc.outputs(sc.reference(shape, "mixed"))
    be = GpuBackend()
    before = torch.full((4096,), 3.25, dtype=torch.float64, device="cuda:0")
    host = {}
    for n in ref.FIELDS:
        a = np.array(case["fields"][n], dtype=np.float64, order="C")
        a[1:] = POISON
        host[n] = torch.from_numpy(a).pin_memory()
    for n in ("zmid", "cn", "cstar", "sfc_temp") + ref.RADIATION:
        host[n] = torch.from_numpy(np.ascontiguousarray(case[n])).pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = {n: torch.empty(h.shape, dtype=torch.float64, device="cuda:0") for n, h in host.items()}
        for n in ("sfc_shf", "sfc_lhf"):
            dev[n] = torch.empty(shape[1:], dtype=torch.float64, device="cuda:0")
        after = torch.full((4096,), 3.25, dtype=torch.float64, device="cuda:0")
        for n, h in host.items():
            dev[n].copy_(h, non_blocking=True)
        be.call(case, dev, stream=side.cuda_stream)
    side.synchronize()
    got = {n: dev[n].cpu().numpy() for n in ref.OUTPUTS}
    assert ref.results_differ(got, want) == []
    assert (before == 3.25).all() and (after == 3.25).all()
    for n in ref.FIELDS + ("zmid", "cn", "cstar") + ref.RADIATION:
        assert ref.same_bits(dev[n].cpu().numpy(), host[n].numpy()), n


# ------------------------------------------------------------------------------------------------------------------------------
# the Python functions through a coupler

KESSLER = ("water_vapor", "cloud_liquid", "precip_liquid")
CONST = dict(grav=9.80616, cp_d=1004.64, R_d=287.042, R_v=461.505)


def _coupler(shape, zint, dt):
    import torch
    from pam_amd import PamCoupler
    nz, ny, nx, nens = shape
    c = PamCoupler("cuda:0")
    for n, v in CONST.items():
        c.set_option(n, v)
    c.set_option("crm_dt", dt)
    c.set_option("micro", "kessler")
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(nx * 500.0, ny * 500.0, zint[:, 0].copy())
    for n in KESSLER:
        c.add_tracer(n, "", True, True)
    dm = c.get_data_manager_device_readwrite()
    dm.get("vertical_interface_height").copy_(torch.from_numpy(zint))
    dm.get("vertical_midpoint_height").copy_(torch.from_numpy(0.5 * (zint[:-1] + zint[1:])))
    return c, dm


def _read(dm, names):
    return {n: dm.get(n, readonly=True).cpu().numpy() for n in names}


@pytest.mark.gpu
def test_gpu_python_functions_through_a_coupler():
    """surface_fluxes_init registers the five entries and sets the three options only where absent; a second init overwrites neither
    sfc_temp nor the options; z0 is the entry of surface_friction_init when that ran first; surface_fluxes gives the restatement's bits
    without radiation entries, and with the longwave pair alone once those two entries exist"""
    import torch
    from pam_amd import modules
    shape = (7, 3, 2, 65)
    nz, ny, nx, nens = shape
    case = sc.cases(shape)["mixed"]
    zmid = case["zmid"]
    zint = np.concatenate([np.zeros((1, nens)), 2.0 * zmid[:1], 2.0 * zmid[:1] + np.cumsum(np.full((nz - 1, nens), 900.0), axis=0)])
    c, dm = _coupler(shape, zint, 10.0)
    zmid = dm.get("vertical_midpoint_height", readonly=True).cpu().numpy()
    for n in ref.FIELDS:
        dm.get(n).copy_(torch.from_numpy(case["fields"][n]))
    c.set_option("sfc_wetness", 0.9)
    sst = 299.0 + 0.01 * np.arange(nens)
    modules.surface_fluxes_init(c, sst=sst, z0=3.0e-4, slab_depth=1.0)
    for n in ("sfc_temp", "sfc_shf", "sfc_lhf"):
        assert tuple(dm.get(n, readonly=True).shape) == (ny, nx, nens)
    assert [c.get_option(n) for n in ("sfc_slab_depth", "sfc_gust", "sfc_wetness")] == [1.0, 1.0, 0.9]
    cn, cstar = ref.transfer_parameters(zmid[0], np.full(nens, 3.0e-4))
    assert ref.same_bits(_read(dm, ["sfc_cn"])["sfc_cn"], cn) and ref.same_bits(_read(dm, ["sfc_cstar"])["sfc_cstar"], cstar)
    assert ref.same_bits(_read(dm, ["sfc_temp"])["sfc_temp"], np.broadcast_to(sst, (ny, nx, nens)))
    dm.get("sfc_temp").copy_(torch.from_numpy(case["sfc_temp"]))
    modules.surface_fluxes_init(c, sst=310.0, z0=3.0e-4, slab_depth=5.0, gust=4.0)       # a second init overwrites neither
    assert ref.same_bits(_read(dm, ["sfc_temp"])["sfc_temp"], case["sfc_temp"])
    assert [c.get_option(n) for n in ("sfc_slab_depth", "sfc_gust", "sfc_wetness")] == [1.0, 1.0, 0.9]
    want_case = dict(case, zmid=zmid, cn=cn, cstar=cstar, wetness=0.9, **CONST, lw_down=None, lw_up=None, sw_down=None, sw_up=None)
    modules.surface_fluxes(c)
    torch.cuda.synchronize()
    first = ref.surface(want_case)
    assert ref.results_differ(_read(dm, ref.OUTPUTS), first) == []
    for entry, key in (("rad_lw_down_sfc", "lw_down"), ("rad_lw_up_sfc", "lw_up"), ("rad_sw_down_sfc", "sw_down")):   # sw_up is absent: no shortwave pair
        dm.register_and_allocate(entry, "", (ny, nx, nens), ("y", "x", "nens"))
        dm.get(entry).copy_(torch.from_numpy(case[key]))
    modules.surface_fluxes(c, dt=3.0)
    torch.cuda.synchronize()
    second = ref.surface(dict(want_case, sfc_temp=first["sfc_temp"], lw_down=case["lw_down"], lw_up=case["lw_up"], dt=3.0))
    assert ref.results_differ(_read(dm, ref.OUTPUTS), second) == []
    # z0 from surface_friction_init when it ran first
    c2, dm2 = _coupler(shape, zint, 10.0)
    for n in ref.FIELDS:
        dm2.get(n).copy_(torch.from_numpy(case["fields"][n]))
    dm2.get("gcm_uvel").copy_(dm2.get("uvel").mean(dim=(1, 2)))
    dm2.get("gcm_vvel").copy_(dm2.get("vvel").mean(dim=(1, 2)))
    tau = torch.full((nens,), 0.1, dtype=torch.float64, device="cuda:0") * (1.0 + torch.arange(nens, device="cuda:0") % 4)
    keep = modules.surface_friction_init(c2, tau, torch.zeros(nens, dtype=torch.float64, device="cuda:0"))
    torch.cuda.synchronize()
    z0 = dm2.get("z0", readonly=True).cpu().numpy()
    assert (z0 > 0).all() and np.unique(z0).size > 1
    modules.surface_fluxes_init(c2, z0=7.0)
    cn2, cstar2 = ref.transfer_parameters(zmid[0], z0)
    assert ref.same_bits(_read(dm2, ["sfc_cn"])["sfc_cn"], cn2) and ref.same_bits(_read(dm2, ["sfc_cstar"])["sfc_cstar"], cstar2)
    assert float(dm2.get("sfc_temp", readonly=True).min()) == 300.0 == float(dm2.get("sfc_temp", readonly=True).max())
    del keep


# ------------------------------------------------------------------------------------------------------------------------------
# the closed loop: radiation, surface, SGS

def _sums(F, zint, rho, cp_d, latvap, cap, Ts):
    """cp_d S rho dz temp + latvap S dz rho_v + cap Ts of every column, in np.longdouble; rho is the step's own"""
    dz = (zint[1:] - zint[:-1])[:, None, None, :].astype(LD)
    heat = (rho.astype(LD) * dz * F["temp"].astype(LD)).sum(axis=0)
    vap = (dz * F["water_vapor"].astype(LD)).sum(axis=0)
    return LD(cp_d) * heat + LD(latvap) * vap + LD(cap) * Ts.astype(LD)


def _sgs_gate(case, before, after, tkh, flux_heat, flux_vap):
    """the column-sum gate of tests/test_sgs_moist.py (test_the_fluxes_add_what_they_carry_to_the_column_sums), in J/m2"""
    nz = before["temp"].shape[0]
    rho = before["density_dry"] + before["water_vapor"]
    dz = (case["zint"][1:] - case["zint"][:-1])[:, None, None, :]
    gc, dt = case["grav"] / case["cp_d"], LD(case["dt"])
    total = 0
    for n, cls, flux, scale in (("temp", "heat", flux_heat, case["cp_d"]), ("water_vapor", "tracer", flux_vap, case["latvap"])):
        lower, diag, upper, dzf_m, dzf_p, _ = sgs_ref.rows(cls, rho, tkh, case["zint"], case["zmid"], case["dt"])
        w = (dz + 0 * rho if cls == "tracer" else rho * dz).astype(LD)
        x, r = after[n].astype(LD), before[n].astype(LD)
        xm, xp = np.concatenate([x[:1], x[:-1]]), np.concatenate([x[1:], x[-1:]])
        lim = 18 * U * (w * (np.abs(lower * xm) + np.abs(diag * x) + np.abs(upper * xp))).sum(axis=0)
        if cls == "heat":
            lim = lim + U * (w * (4 * gc * (np.abs(upper * dzf_p) + np.abs(lower * dzf_m)) + np.abs(r) + gc * 1.0e4)).sum(axis=0)
        lim = lim + 2 * nz * LD(2.0) ** -64 * (w * (np.abs(x) + np.abs(r))).sum(axis=0) + 4 * U * np.abs(dt * flux.astype(LD))
        total = total + LD(scale) * lim
    return total


def _radiation_gate(down, up, nz):
    """the energy-closure gate of tests/test_grayrad.py and tests/test_grayrad_sw.py: 4 nz u S, S the magnitudes of the flux differences
    of every level and of the four fluxes at the two ends, in W/m2"""
    S = (np.abs(down[1:] - down[:-1]) + np.abs(up[:-1] - up[1:])).astype(LD).sum(axis=0)
    S = S + np.abs(down[0]) + np.abs(up[0]) + np.abs(down[nz]) + np.abs(up[nz])
    return 4 * nz * U * S


def _loop_case(shape):
    nz, ny, nx, nens = shape
    sw = swc.cases(shape)["cloud"]
    rng = np.random.default_rng(77)
    F = {n: sw["fields"][n].copy() for n in ("temp", "density_dry", "water_vapor", "cloud_liquid")}
    F["precip_liquid"] = np.zeros(shape)
    F["uvel"], F["vvel"], F["wvel"] = 12.0 * rng.random(shape) - 6.0, 12.0 * rng.random(shape) - 6.0, rng.random(shape) - 0.5
    zint = sw["zint"]
    zmid = 0.5 * (zint[:-1] + zint[1:])
    dt, depth = 10.0, 0.05
    sa = F["temp"][0] + (CONST["grav"] / CONST["cp_d"]) * zmid[0]
    Ts = sa + np.where(np.arange(ny * nx * nens).reshape(ny, nx, nens) % 2 == 0, 1.0, -1.0) * (1.0 + 4.0 * rng.random((ny, nx, nens)))
    return dict(fields=F, zint=zint, zmid=zmid, dt=dt, depth=depth, sfc_temp=Ts, coszen=sw["coszen"], dx=500.0, dy=500.0, cs=0.2, prandtl=1.0 / 3.0,
                latvap=2501000.0, tracers=KESSLER, **CONST)


def _chain_step(L, F, Ts, cn, cstar):
    """one step of the loop in numpy: the longwave (over sfc_temp), the shortwave, the surface, the dry coefficients and the solve with the
    fluxes.  -> the new fields, the new sfc_temp, everything the coupler holds, and the budget's pieces"""
    from pam_amd import RadiationGray
    sw_opt = dict(zip(("solar_constant", "albedo", "a_d", "a_v", "a_l", "a_i", "s_l", "s_i"), RadiationGray().shortwave().sw_defaults))
    rad = dict(lwc.K, sigma=lwref.SIGMA, lw_down_top=0.0, liquid=("cloud_liquid",), ice=(), zint=L["zint"], cp_d=L["cp_d"], dt=L["dt"],
               coszen=L["coszen"], sfc_albedo=None, **sw_opt)
    lw = lwref.radiation(dict(rad, fields=F, sfc_temp=Ts), internals=True)
    sw = swref.radiation(dict(rad, fields=dict(F, temp=lw["temp"])), internals=True)
    F1 = dict(F, temp=sw["temp"])
    cap = ref.RHO_W * ref.C_W * L["depth"]
    sfc = ref.surface(dict(fields=F1, zmid=L["zmid"], cn=cn, cstar=cstar, sfc_temp=Ts, lw_down=lw["rad_lw_down_sfc"], lw_up=lw["rad_lw_up_sfc"],
                           sw_down=sw["rad_sw_down_sfc"], sw_up=sw["rad_sw_up_sfc"], gust=1.0, wetness=0.98, grav=L["grav"], cp_d=L["cp_d"],
                           R_v=L["R_v"], latvap=L["latvap"], slab_heat_capacity=cap, dt=L["dt"]), internals=True)
    sgs_case = dict(L, fields=F1, sfc_flx_u=np.zeros_like(Ts), sfc_flx_v=np.zeros_like(Ts), sfc_shf=sfc["sfc_shf"], sfc_lhf=sfc["sfc_lhf"])
    tk, tkh = sgs_ref.coefficients(sgs_case)
    F2 = dict(F1, **mref.diffuse(sgs_case, tk, tkh))
    held = dict(F2, tk=tk, tkh=tkh, sfc_temp=sfc["sfc_temp"], sfc_shf=sfc["sfc_shf"], sfc_lhf=sfc["sfc_lhf"],
                **{n: lw[n] for n in lwref.OUTPUTS[1:]}, **{n: sw[n] for n in swref.OUTPUTS[1:]})
    nz = F["temp"].shape[0]
    top = (sw["Fd"][nz].astype(LD) - sw["rad_sw_up_top"].astype(LD)) + (LD(0.0) - lw["rad_olr"].astype(LD))
    assert ref.same_bits(sw["Fd"][nz], np.broadcast_to(rad["solar_constant"] * L["coszen"], Ts.shape))
    slab_gate = 4.0 * np.spacing(np.maximum(np.abs(Ts) * cap / L["dt"], np.abs(sfc["net"]))).astype(LD)
    gate = (LD(L["dt"]) * (_radiation_gate(lw["D"], lw["U"], nz) + _radiation_gate(sw["Fd"], sw["Fu"], nz) + slab_gate)
            + _sgs_gate(sgs_case, F1, F2, tkh, sfc["sfc_shf"] / LD(L["cp_d"]), sfc["sfc_lhf"] / LD(L["latvap"])))
    return F2, sfc["sfc_temp"], held, dict(top=top, gate=gate, cap=cap, rho=F["density_dry"] + F["water_vapor"])


def _budget_error(L, F_before, Ts_before, F_after, Ts_after, pieces):
    """|the change of cp_d S rho dz temp + latvap S dz rho_v + cap sfc_temp over the step - dt (what passes the model top)| of every
    column, with rho the density the step's kernels worked with"""
    a = _sums(F_before, L["zint"], pieces["rho"], L["cp_d"], L["latvap"], pieces["cap"], Ts_before)
    b = _sums(F_after, L["zint"], pieces["rho"], L["cp_d"], L["latvap"], pieces["cap"], Ts_after)
    return np.abs((b - a) - LD(L["dt"]) * pieces["top"])


@pytest.mark.gpu
def test_gpu_closed_loop_matches_the_chain_and_closes_the_energy_budget():
    """RadiationGray().shortwave(...), surface_fluxes, SGSSmagorinsky(surface_fluxes=True) for 3 steps at (7,3,2,65): every field equals
    the chain of the restatements bit for bit, step by step, and per column the energy of column plus slab changes by dt times what passes
    the model top, within the gates of the SGS flux test and of the two radiation closure tests, added together, plus the slab step's own
    bound.  The chain's own budget is held to the same gate first, so a failure on the GPU is the kernel's"""
    import torch
    from pam_amd import RadiationGray, SGSSmagorinsky, modules
    shape = (7, 3, 2, 65)
    L = _loop_case(shape)
    c, dm = _coupler(shape, L["zint"], L["dt"])
    rad = RadiationGray().shortwave(coszen=L["coszen"])
    rad.init(c)
    sgs = SGSSmagorinsky(surface_fluxes=True)
    sgs.init(c)
    for n, v in L["fields"].items():
        dm.get(n).copy_(torch.from_numpy(v))
    modules.surface_fluxes_init(c, sst=300.0, slab_depth=L["depth"])
    dm.get("sfc_temp").copy_(torch.from_numpy(L["sfc_temp"]))
    cn, cstar = ref.transfer_parameters(L["zmid"][0], np.full(shape[3], 1.0e-4))
    assert ref.same_bits(_read(dm, ["sfc_cn"])["sfc_cn"], cn)
    F, Ts = L["fields"], L["sfc_temp"]
    worst = 0.0
    for step in range(3):
        F2, Ts2, held, pieces = _chain_step(L, F, Ts, cn, cstar)
        err = _budget_error(L, F, Ts, F2, Ts2, pieces)
        print("step %d: the chain's worst fraction of the gate %.3f" % (step, float((err / pieces["gate"]).max())))
        assert (err <= pieces["gate"]).all(), step
        assert (np.abs(LD(L["dt"]) * pieces["top"]) > 100 * pieces["gate"]).mean() > 0.9, step      # the budget is far above the gate: the test sees it
        rad.timeStep(c)
        modules.surface_fluxes(c)
        sgs.timeStep(c)
        torch.cuda.synchronize()
        got = _read(dm, list(held))
        assert ref.results_differ(got, held) == [], step
        gerr = _budget_error(L, F, Ts, {n: got[n] for n in F2}, got["sfc_temp"], pieces)
        assert (gerr <= pieces["gate"]).all(), step
        worst = max(worst, float((gerr / pieces["gate"]).max()))
        F, Ts = F2, Ts2
    print("worst fraction of the gate on the GPU %.3f" % worst)
    assert not ref.same_bits(Ts, L["sfc_temp"])


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ module through the driver

SURFACE_LINE = r"surface: etime (\S+) , shf (\S+) , lhf (\S+) , sfc_temp (\S+)"
LOOP = ["--sgs-smag", "0.2", "0.333", "--radiation-gray", "--shortwave", "0.8"]


def _run_driver(*args, timeout=600):
    return subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3"] + list(args), capture_output=True, text=True, timeout=timeout)


def _surface_rows(r):
    lines = r.stdout.strip().split("\n")
    rows = [re.fullmatch(SURFACE_LINE, l) for l in lines if l.startswith("surface:")]
    assert rows and all(rows) and len(rows) == sum(l.startswith("Etime ,") for l in lines)
    return [tuple(float(m.group(i)) for i in (1, 2, 3, 4)) for m in rows]


@pytest.mark.gpu
def test_gpu_driver_runs_the_surface_over_a_slab(tmp_path):
    """the whole loop of the shortened input with --sgs-smag --radiation-gray --shortwave 0.8 --surface 300 1.0: it exits 0, prints one
    "surface:" line per output step with finite values, shf + lhf > 0 over the warm ocean, and sfc_temp moves off 300"""
    r = _run_driver(*LOOP, "--surface", "300", "1.0", str(tmp_path / "out.bin"))
    assert r.returncode == 0, r.stderr[-2000:]
    rows = _surface_rows(r)
    for etime, shf, lhf, ts in rows:
        assert all(math.isfinite(v) for v in (etime, shf, lhf, ts)) and shf + lhf > 0
    assert rows[-1][3] != 300.0 and abs(rows[-1][3] - 300.0) < 1.0


@pytest.mark.gpu
def test_gpu_driver_without_a_slab_keeps_the_surface_temperature(tmp_path):
    r = _run_driver(*LOOP, "--surface", "300", "0", str(tmp_path / "out.bin"))
    assert r.returncode == 0, r.stderr[-2000:]
    rows = _surface_rows(r)
    assert all(ts == 300.0 for _, _, _, ts in rows) and all(math.isfinite(shf) and math.isfinite(lhf) for _, shf, lhf, _ in rows)


@pytest.mark.gpu
def test_gpu_driver_refuses_the_surface_without_the_closure_or_beside_given_fluxes(tmp_path):
    out = tmp_path / "out.bin"
    r = _run_driver("--steps", "1", "--surface", "300", "1.0", str(out))
    assert r.returncode != 0 and "--surface SST [DEPTH] needs --sgs-smag" in r.stderr + r.stdout and not out.exists()
    r = _run_driver("--steps", "1", "--sgs-smag", "0.2", "0.333", "--sfc-fluxes", "50", "200", "--surface", "300", "1.0", str(out))
    assert r.returncode != 0 and "--surface and --sfc-fluxes both fill" in r.stderr + r.stdout and not out.exists()
