"""Large-scale forcing on the GPU: pam_amd_ls_nudging and pam_amd_ls_forcing against the numpy restatement (tests/lsforcing_ref.py) bit for
bit (a NaN by its place) on every shape and named case, with the narrow and with the wide index, and run to run; members split over calls
against the whole; the increments poisoned before the call, bystanders and read-only inputs; the Python functions through a coupler; the
closed loop of radiation, forcing, surface and SGS against the chain of the restatements; modules/large_scale_forcing.h through
tests/cxx/ls_forcing; and examples/driver --ls-forcing on a shortened CI input."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import grayrad_ref as lwref
import grayrad_cases as lwc
import grayrad_sw_ref as swref
import grayrad_sw_cases as swc
import sgs_ref
import sgs_moist_ref as mref
import surface_ref
import lsforcing_ref as ref
import lsforcing_cases as lc
from lsforcing_harness import NUDGE_FIELDS, POISON, call_arguments
from tools.native_build import cxx_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")


class GpuBackend:
    """the interface of lsforcing_ref.RefBackend over the C ABI: the nudging where a target is given, with its increments poisoned, then
    the forcing"""

    def __init__(self, wide=False):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check, self.wide = torch, capi.load(), capi.check, wide

    def dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")

    def run(self, case, with_everything=False):
        F, sizes, prof, tgt, rate, inc = call_arguments(case)
        dF, dprof = {n: self.dev(a) for n, a in F.items()}, {n: self.dev(a) for n, a in prof.items()}
        shared = {}                                     # one profile under two names (the rate of both winds) is one array on the device
        for a in rate:
            if a is not None and id(a) not in shared:
                shared[id(a)] = self.dev(a)
        dtgt, drate, dinc = [self.dev(a) for a in tgt], [None if a is None else shared[id(a)] for a in rate], [self.dev(a) for a in inc]
        P = lambda t: None if t is None else t.data_ptr()
        table = lambda ts: (C.c_void_p * len(ts))(*[P(t) for t in ts])
        stream = self.torch.cuda.current_stream().cuda_stream
        nudge = any(t is not None for t in tgt)
        self.check(self.lib.pam_amd_ls_forcing_debug_wide_index(1 if self.wide else 0))
        try:
            if nudge:
                self.check(self.lib.pam_amd_ls_nudging(*sizes, table([dF[n] for n in NUDGE_FIELDS]), table(dtgt), table(drate), float(case["dt"]),
                                                       table(dinc), stream))
            tr = [dF[n] for n in case["tracers"]]
            flags = (C.c_ubyte * max(len(tr), 1))(*[1 if p else 0 for p in case["positive"]])
            self.check(self.lib.pam_amd_ls_forcing(*sizes, P(dF["uvel"]), P(dF["vvel"]), P(dF["temp"]), len(tr), table(tr) if tr else None,
                                                   flags if tr else None, P(dF["density_dry"]), P(dF[ref.VAPOUR]), P(dprof["zmid"]), P(dprof["wsub"]),
                                                   P(dprof["temp_tend"]), P(dprof["qv_tend"]), table(dinc) if nudge else None, P(dprof["fcor"]),
                                                   P(dprof["ug"]), P(dprof["vg"]), float(case["dt"]), float(case["grav"]), float(case["cp_d"]), stream))
            self.torch.cuda.synchronize()
        finally:
            self.lib.pam_amd_ls_forcing_debug_wide_index(0)
        out = {n: dF[n].cpu().numpy() for n in ref.STATE + tuple(case["tracers"])}
        if not with_everything:
            return out
        back = lambda t: None if t is None else t.cpu().numpy()
        return out, dict(zip(ref.QUANTITIES, [back(t) for t in dinc])), {n: back(t) for n, t in dprof.items()}, \
            {n: back(dF[n]) for n in dF if n not in out}, [back(t) for t in dtgt + drate]


@pytest.mark.gpu
@pytest.mark.parametrize("wide", (False, True), ids=("narrow", "wide"))
@pytest.mark.parametrize("shape", lc.SHAPES, ids=ref.shape_id)
def test_gpu_matches_restatement_bit_for_bit(shape, wide):
    """every named case; one case twice: two runs are identical"""
    be = GpuBackend(wide)
    for name in lc.CASE_NAMES:
        assert ref.results_differ(be.run(lc.cases(shape)[name]), lc.reference(shape, name), nan_by_place=True) == [], name
    a, b = (be.run(lc.cases(shape)["all_on"]) for _ in range(2))
    assert ref.results_differ(a, b) == []


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in lc.SHAPES if s[3] >= 64], ids=ref.shape_id)
def test_gpu_members_split_over_calls_equal_the_whole(shape):
    nens, be = shape[3], GpuBackend()
    for name in ("all_on", "nan_w", "clamp"):
        case, want = lc.cases(shape)[name], lc.reference(shape, name)
        parts = [be.run(ref.members(case, slice(lo, hi))) for lo, hi in ((0, 1), (1, 37), (37, nens))]
        got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
        assert ref.results_differ(got, want, nan_by_place=True) == [], name


@pytest.mark.gpu
def test_gpu_increments_bystanders_and_read_only_inputs():
    """the increments were poisoned before the call and hold the restatement's bits after it; an absent target's increment does not exist;
    tensors allocated before and after keep their bits, and so do density_dry, every profile, target and rate; without the vapour in the
    table water_vapor is read-only too"""
    import torch
    shape = (5, 1, 17, 65)
    before = torch.full((4096,), 3.25, dtype=torch.float64, device="cuda:0")
    for name in ("all_on", "no_target_u", "no_tracers"):
        case = lc.cases(shape)[name]
        out, inc, prof, untouched, tables = GpuBackend().run(case, with_everything=True)
        after = torch.full((4096,), 3.25, dtype=torch.float64, device="cuda:0")
        assert ref.results_differ(out, lc.reference(shape, name)) == [], name
        want = ref.nudging(case)
        for x in ref.QUANTITIES:
            assert (inc[x] is None) == (want[x] is None)
            if want[x] is not None:
                assert ref.same_bits(inc[x], want[x]) and not (inc[x] == POISON).any(), (name, x)
        for n, a in prof.items():
            assert a is None or ref.same_bits(a, np.asarray(case[n], dtype=np.float64)), (name, n)
        assert "density_dry" in untouched and (name != "no_tracers" or ref.VAPOUR in untouched)
        for n, a in untouched.items():
            assert ref.same_bits(a, case["fields"][n]), (name, n)
        _, _, _, tgt, rate, _ = call_arguments(case)
        for got, a in zip(tables, tgt + rate):
            assert (got is None) == (a is None) and (a is None or ref.same_bits(got, a)), name
        assert (before == 3.25).all() and (after == 3.25).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python functions through a coupler

KESSLER = ("water_vapor", "cloud_liquid", "precip_liquid")
CONST = dict(grav=9.80616, cp_d=1004.64, R_d=287.042, R_v=461.505)


def _coupler(shape, zint, dt, tracers=KESSLER, positive=None):
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
    for i, n in enumerate(tracers):
        c.add_tracer(n, "", True if positive is None else positive[i], True)
    dm = c.get_data_manager_device_readwrite()
    dm.get("vertical_interface_height").copy_(torch.from_numpy(zint))
    dm.get("vertical_midpoint_height").copy_(torch.from_numpy(0.5 * (zint[:-1] + zint[1:])))
    return c, dm


def _read(dm, names):
    return {n: dm.get(n, readonly=True).cpu().numpy() for n in names}


def _init_arguments(case):
    target, rate = case.get("target") or {}, case.get("rate") or {}
    return dict(wsub=case.get("wsub"), temp_tend=case.get("temp_tend"), qv_tend=case.get("qv_tend"), ug=case.get("ug"), vg=case.get("vg"),
                fcor=case.get("fcor"), nudge_temp=target.get("t"), nudge_qv=target.get("q"), nudge_u=target.get("u"), nudge_v=target.get("v"),
                nudge_rate_temp=rate.get("t") if target.get("t") is not None else None,
                nudge_rate_qv=rate.get("q") if target.get("q") is not None else None,
                nudge_rate_uv=rate.get("u") if target.get("u") is not None or target.get("v") is not None else None)


@pytest.mark.gpu
def test_gpu_python_functions_through_a_coupler():
    """ls_forcing_init registers what is given and nothing else; ls_forcing gives the restatement's bits with seven tracers of which one is
    not positive, with the Coriolis term absent, and with the subsidence alone; wvel, density_dry and every ls_ entry keep their bits"""
    import torch
    from pam_amd import modules
    shape = (5, 1, 17, 65)
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(3)
    for name in ("all_on", "no_coriolis", "subsidence_only", "no_target_q"):
        case = lc.cases(shape)[name]
        zmid = case["zmid"]
        zint = np.concatenate([np.zeros((1, nens)), 0.5 * (zmid[1:] + zmid[:-1]), 2.0 * zmid[-1:] - 0.5 * (zmid[-1:] + zmid[-2:-1])])
        c, dm = _coupler(shape, zint, case["dt"], case["tracers"], case["positive"])
        dm.get("vertical_midpoint_height").copy_(torch.from_numpy(zmid))
        wvel = rng.random(shape)
        dm.get("wvel").copy_(torch.from_numpy(wvel))
        for n in ("uvel", "vvel", "temp", "density_dry") + case["tracers"]:
            dm.get(n).copy_(torch.from_numpy(case["fields"][n]))
        modules.ls_forcing_init(c, **_init_arguments(case))
        entries = [n for n, _ in modules.LS_PROFILES if dm.entry_exists(n)] + (["ls_fcor"] if dm.entry_exists("ls_fcor") else [])
        given = {k for k, v in _init_arguments(case).items() if v is not None}
        assert set(entries) == {"ls_" + k for k in given}, name
        assert [dm.entry_exists(i) for i in modules.LS_INCREMENTS] == [(case.get("target") or {}).get(x) is not None for x in ref.QUANTITIES]
        held = _read(dm, entries + ["density_dry", "wvel"])
        modules.ls_forcing(c)
        torch.cuda.synchronize()
        want = lc.reference(shape, name)
        assert ref.results_differ(_read(dm, list(want)), want) == [], name
        assert ref.results_differ(_read(dm, list(held)), held) == [], name
        assert ref.same_bits(held["wvel"], wvel)


# ------------------------------------------------------------------------------------------------------------------------------
# the closed loop: radiation, large-scale forcing, surface, SGS

def _loop_case(shape):
    nz, ny, nx, nens = shape
    sw = swc.cases(shape)["cloud"]
    rng = np.random.default_rng(78)
    F = {n: sw["fields"][n].copy() for n in ("temp", "density_dry", "water_vapor", "cloud_liquid")}
    F["precip_liquid"] = np.zeros(shape)
    F["uvel"], F["vvel"], F["wvel"] = 12.0 * rng.random(shape) - 6.0, 12.0 * rng.random(shape) - 6.0, rng.random(shape) - 0.5
    zint = sw["zint"]
    zmid = 0.5 * (zint[:-1] + zint[1:])
    dt, depth = 10.0, 0.05
    sa = F["temp"][0] + (CONST["grav"] / CONST["cp_d"]) * zmid[0]
    Ts = sa + np.where(np.arange(ny * nx * nens).reshape(ny, nx, nens) % 2 == 0, 1.0, -1.0) * (1.0 + 4.0 * rng.random((ny, nx, nens)))
    ls = lc.profiles(rng, (zmid[1:] - zmid[:-1]).min(axis=0), dt, F["temp"], F["water_vapor"] / (F["density_dry"] + F["water_vapor"]))
    return dict(fields=F, zint=zint, zmid=zmid, dt=dt, depth=depth, sfc_temp=Ts, coszen=sw["coszen"], dx=500.0, dy=500.0, cs=0.2, prandtl=1.0 / 3.0,
                latvap=2501000.0, tracers=KESSLER, positive=(True, True, True), ls=ls, **CONST)


def _chain_step(L, F, Ts, cn, cstar):
    """one step of the loop in numpy: the longwave (over sfc_temp), the shortwave, the large-scale forcing, the surface, the dry
    coefficients and the solve with the fluxes.  -> the new fields, the new sfc_temp, everything the coupler holds"""
    from pam_amd import RadiationGray
    sw_opt = dict(zip(("solar_constant", "albedo", "a_d", "a_v", "a_l", "a_i", "s_l", "s_i"), RadiationGray().shortwave().sw_defaults))
    rad = dict(lwc.K, sigma=lwref.SIGMA, lw_down_top=0.0, liquid=("cloud_liquid",), ice=(), zint=L["zint"], cp_d=L["cp_d"], dt=L["dt"],
               coszen=L["coszen"], sfc_albedo=None, **sw_opt)
    lw = lwref.radiation(dict(rad, fields=F, sfc_temp=Ts), internals=True)
    sw = swref.radiation(dict(rad, fields=dict(F, temp=lw["temp"])), internals=True)
    F1 = dict(F, temp=sw["temp"])
    F1 = dict(F1, **ref.ls_forcing(dict(L["ls"], fields=F1, tracers=L["tracers"], positive=L["positive"], zmid=L["zmid"], dt=L["dt"],
                                        grav=L["grav"], cp_d=L["cp_d"])))
    cap = surface_ref.RHO_W * surface_ref.C_W * L["depth"]
    sfc = surface_ref.surface(dict(fields=F1, zmid=L["zmid"], cn=cn, cstar=cstar, sfc_temp=Ts, lw_down=lw["rad_lw_down_sfc"],
                                   lw_up=lw["rad_lw_up_sfc"], sw_down=sw["rad_sw_down_sfc"], sw_up=sw["rad_sw_up_sfc"], gust=1.0, wetness=0.98,
                                   grav=L["grav"], cp_d=L["cp_d"], R_v=L["R_v"], latvap=L["latvap"], slab_heat_capacity=cap, dt=L["dt"]))
    sgs_case = dict(L, fields=F1, sfc_flx_u=np.zeros_like(Ts), sfc_flx_v=np.zeros_like(Ts), sfc_shf=sfc["sfc_shf"], sfc_lhf=sfc["sfc_lhf"])
    tk, tkh = sgs_ref.coefficients(sgs_case)
    F2 = dict(F1, **mref.diffuse(sgs_case, tk, tkh))
    held = dict(F2, tk=tk, tkh=tkh, sfc_temp=sfc["sfc_temp"], sfc_shf=sfc["sfc_shf"], sfc_lhf=sfc["sfc_lhf"],
                **{n: lw[n] for n in lwref.OUTPUTS[1:]}, **{n: sw[n] for n in swref.OUTPUTS[1:]})
    return F2, sfc["sfc_temp"], held


@pytest.mark.gpu
def test_gpu_closed_loop_matches_the_chain_of_the_restatements():
    """RadiationGray().shortwave(...), ls_forcing, surface_fluxes, SGSSmagorinsky(surface_fluxes=True) for 3 CRM steps at an 8 x 1 x 9 grid
    with 65 members: every field the coupler holds equals the chain of the restatements bit for bit, step by step, and the forcing has
    moved the state (the same chain without it gives other bits)"""
    import torch
    from pam_amd import RadiationGray, SGSSmagorinsky, modules
    shape = (9, 1, 8, 65)
    L = _loop_case(shape)
    c, dm = _coupler(shape, L["zint"], L["dt"])
    rad = RadiationGray().shortwave(coszen=L["coszen"])
    rad.init(c)
    sgs = SGSSmagorinsky(surface_fluxes=True)
    sgs.init(c)
    for n, v in L["fields"].items():
        dm.get(n).copy_(torch.from_numpy(v))
    modules.ls_forcing_init(c, **_init_arguments(L["ls"]))
    modules.surface_fluxes_init(c, sst=300.0, slab_depth=L["depth"])
    dm.get("sfc_temp").copy_(torch.from_numpy(L["sfc_temp"]))
    cn, cstar = surface_ref.transfer_parameters(L["zmid"][0], np.full(shape[3], 1.0e-4))
    F, Ts = L["fields"], L["sfc_temp"]
    for step in range(3):
        F2, Ts2, held = _chain_step(L, F, Ts, cn, cstar)
        rad.timeStep(c)
        modules.ls_forcing(c)
        modules.surface_fluxes(c)
        sgs.timeStep(c)
        torch.cuda.synchronize()
        assert ref.results_differ(_read(dm, list(held)), held) == [], step
        F, Ts = F2, Ts2
    assert not ref.same_bits(F["uvel"], L["fields"]["uvel"]) and not ref.same_bits(F["water_vapor"], L["fields"]["water_vapor"])


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ module through tests/cxx/ls_forcing, and through the driver

PROFILE_ORDER = ("wsub", "temp_tend", "qv_tend", "ug", "vg", ("target", "t"), ("target", "q"), ("target", "u"), ("target", "v"), ("rate", "t"),
                 ("rate", "q"), ("rate", "u"))


def _profile(case, key):
    if isinstance(key, str):
        return case.get(key)
    table, x = key
    if not case.get("target"):
        return None
    if table == "rate":
        return case["rate"][x] if any(case["target"].get(y) is not None for y in (("u", "v") if x == "u" else (x,))) else None
    return case["target"].get(x)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("all_on", "no_coriolis", "no_target_u"))
def test_gpu_cxx_module_matches_restatement(tmp_path, name):
    """modules::ls_forcing_init and modules::ls_forcing on a case file: the entries that exist are those that were given, and one call
    gives the restatement's bits"""
    shape = (5, 1, 17, 65)
    nz, ny, nx, nens = shape
    case = lc.cases(shape)[name]
    tr = case["tracers"]
    profs = [_profile(case, k) for k in PROFILE_ORDER]
    given = sum(1 << i for i, p in enumerate(profs) if p is not None) | ((1 << 12) if case.get("fcor") is not None else 0)
    flags = sum(1 << i for i, p in enumerate(case["positive"]) if p)
    path, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("10i", nz, ny, nx, nens, len(tr), tr.index(ref.VAPOUR), flags, given, 1, 0))
        parts = [np.array([case["dt"]]), case["zmid"]] + [p for p in profs if p is not None]
        parts += [case["fcor"]] if case.get("fcor") is not None else []
        parts += [case["fields"][n] for n in ("density_dry", "uvel", "vvel", "temp") + tr]
        for a in parts:
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([cxx_program("ls_forcing"), str(path), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    entries = re.search(r"### entries(.*)", r.stdout).group(1).split()
    names = ["ls_wsub", "ls_temp_tend", "ls_qv_tend", "ls_ug", "ls_vg", "ls_nudge_temp", "ls_nudge_qv", "ls_nudge_u", "ls_nudge_v",
             "ls_nudge_rate_temp", "ls_nudge_rate_qv", "ls_nudge_rate_uv"]
    want_entries = [n for n, p in zip(names, profs) if p is not None] + (["ls_fcor"] if case.get("fcor") is not None else [])
    want_entries += [i for i, x in zip(("ls_inc_temp", "ls_inc_qv", "ls_inc_u", "ls_inc_v"), ref.QUANTITIES) if (case.get("target") or {}).get(x) is not None]
    assert entries == want_entries
    got = np.fromfile(out, dtype=np.float64).reshape((3 + len(tr),) + shape)
    got = dict(zip(("uvel", "vvel", "temp") + tr, got))
    assert ref.results_differ(got, lc.reference(shape, name)) == []


LS_LINE = r"ls forcing: etime (\S+) , uvel (\S+) , vvel (\S+) , temp0 (\S+)"
LOOP = ["--sgs-smag", "0.2", "0.333", "--surface", "300", "1.0"]


def _run_driver(*args, timeout=600):
    return subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3"] + list(args), capture_output=True, text=True, timeout=timeout)


NZ = 50                           # the input's vcoords_equal_50_20km: 50 levels of 400 m; dt_crm_phys is 20 s, and 12 CRM steps make the run


@pytest.mark.gpu
def test_gpu_driver_runs_the_forcing_and_a_zero_file_changes_nothing(tmp_path):
    """--ls-forcing PATH --coriolis F with --surface and --sgs-smag: a file of wsub, a cooling, a drying, a geostrophic wind and nudging
    towards a wind prints one finite "ls forcing:" line per output step and moves the output; a file of zeros (with --coriolis 0) gives
    the very output of the run without the flag"""
    nz = NZ
    k = np.arange(nz)
    rows = np.full((12, nz), np.nan)
    rows[0] = -0.005 * np.sin(np.pi * (k + 0.5) / nz)
    rows[1], rows[2] = -2.0e-5, -1.0e-9
    rows[3], rows[4] = 5.0, -2.0
    rows[7], rows[8], rows[11] = 3.0, 1.0, 1.0e-3
    forced, zeros = tmp_path / "forced.bin", tmp_path / "zeros.bin"
    rows.tofile(forced)
    np.zeros((12, nz)).tofile(zeros)
    outs = {}
    for tag, extra in (("plain", []), ("zero", ["--ls-forcing", str(zeros), "--coriolis", "0"]), ("forced", ["--ls-forcing", str(forced), "--coriolis", "1e-4"])):
        out = tmp_path / (tag + ".bin")
        r = _run_driver(*LOOP, *extra, str(out))
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        lines = r.stdout.strip().split("\n")
        ls_rows = [re.fullmatch(LS_LINE, l) for l in lines if l.startswith("ls forcing:")]
        if tag == "plain":
            assert not ls_rows
        else:
            assert ls_rows and all(ls_rows) and len(ls_rows) == sum(l.startswith("Etime ,") for l in lines), tag
            assert all(np.isfinite(float(m.group(i))) for m in ls_rows for i in (1, 2, 3, 4))
        outs[tag] = open(out, "rb").read()
    assert outs["zero"] == outs["plain"] and outs["forced"] != outs["plain"]
    r = _run_driver(*LOOP, "--coriolis", "1e-4", str(tmp_path / "no.bin"))
    assert r.returncode != 0 and "--coriolis F needs --ls-forcing PATH" in r.stderr + r.stdout
