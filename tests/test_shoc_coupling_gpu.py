"""The SHOC coupling layer on the GPU: pack, the stand-in for shoc_main and unpack through the C ABI against the host emulation bit for bit,
in both layouts and with both tracer sets; the workspace's canary words; what must stay untouched; run-to-run and shard-to-whole
identity; the Python class SGSShoc; three CRM steps with it; and the refusals."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import shoc_cases as sc
import shoc_coupling_ref as ref
from pam_amd import capi
from tools.native_build import cxx_program

pytestmark = pytest.mark.gpu

CANARY = 0x7ff853484f435f5f
GUARD = 8
CASES = [(s, t, l) for s in sc.SHAPES for t in ("kessler", "p3") for l in (0, 1)]
CASE_IDS = ["%s-%s-layout%d" % ("x".join(map(str, s)), t, l) for s, t, l in CASES]
CONSTS = ref.CONSTS


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _view(ptr, shape, typestr="<f8"):
    import torch
    from pam_amd.physics import _DeviceArray
    a = _DeviceArray(ptr, shape)
    a.__cuda_array_interface__["typestr"] = typestr
    return torch.as_tensor(a, device="cuda")


class Workspace:
    def __init__(self, shape, ntr, layout):
        nz, ny, nx, nens = shape
        self.lib = capi.load()
        self.ws = C.c_void_p()
        capi.check(self.lib.pam_amd_shoc_workspace_create(nens, nx, ny, nz, ntr, layout, C.byref(self.ws)))
        self.args = capi.ShocArgs()
        capi.check(self.lib.pam_amd_shoc_workspace_args(self.ws, C.byref(self.args)))
        n = C.c_longlong()
        capi.check(self.lib.pam_amd_shoc_workspace_bytes(self.ws, C.byref(n)))
        self.bytes = n.value
        from pam_amd.physics import shoc_shapes
        self.shapes = shoc_shapes(ny * nx * nens, nz, ntr, layout)

    def arrays(self):
        import torch
        torch.cuda.synchronize()
        return {n: (_view(getattr(self.args, n), shp).cpu().numpy() if min(shp) > 0 else np.zeros(shp)) for n, shp in self.shapes.items()}

    def words(self):
        """the whole allocation as 64-bit words"""
        import torch
        torch.cuda.synchronize()
        return _view(self.args.host_dx - 8 * GUARD, (self.bytes // 8,), "<i8").cpu().numpy().view(np.uint64)

    def outside(self):
        """mask of the words that belong to no array"""
        mask = np.ones(self.bytes // 8, dtype=bool)
        base = self.args.host_dx - 8 * GUARD
        for n, shp in self.shapes.items():
            at = (getattr(self.args, n) - base) // 8
            mask[at:at + int(np.prod(shp))] = False
        return mask

    def close(self):
        capi.check(self.lib.pam_amd_shoc_workspace_destroy(self.ws))


def gpu_chain(state, layout, consts=CONSTS):
    """pack, stand-in, unpack through the C ABI.  Returns (packed set, set after the stand-in, state after, tracers after, canary report,
    untouched report)"""
    import torch
    shape = state["rho_d"].shape
    ntr = len(state["q"])
    lib = capi.load()
    dev = {k: torch.from_numpy(np.array(state[k], order="C")).cuda() for k in sc.EMU_STATE + ("flx_u", "flx_v", "zint", "zmid")}
    dev["inv_qc_relvar"] = torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    q = [torch.from_numpy(np.array(x, order="C")).cuda() for x in state["q"]]
    qp = (C.c_void_p * max(ntr, 1))(*[t.data_ptr() for t in q])
    w = Workspace(shape, ntr, layout)
    try:
        words0 = w.words()
        fresh = bool((words0 == CANARY).all())
        p = lambda k: dev[k].data_ptr()
        capi.check(lib.pam_amd_shoc_pack(w.ws, p("rho_d"), p("rho_v"), p("rho_c"), p("uvel"), p("vvel"), p("wvel"), p("temp"), p("tke"), qp,
                                         p("wthv_sec"), p("tk"), p("tkh"), p("cldfrac"), p("flx_u"), p("flx_v"), p("zint"), p("zmid"), sc.XLEN,
                                         sc.YLEN, consts["pres_R_d"], consts["pres_R_v"], consts["R_d"], consts["cp_d"], consts["p0"], consts["grav"],
                                         consts["latvap"], _stream()))
        packed = w.arrays()
        untouched_by_pack = all(sc.same_bits(dev[k].cpu().numpy(), state[k]) for k in sc.EMU_STATE + ("flx_u", "flx_v", "zint", "zmid"))
        w.args.dt, w.args.stream = 2.0, _stream()
        capi.check(lib.pam_amd_shoc_main_standin(C.byref(w.args), None))
        after = w.arrays()
        capi.check(lib.pam_amd_shoc_unpack(w.ws, p("rho_d"), p("rho_v"), p("rho_c"), p("uvel"), p("vvel"), p("temp"), p("tke"), qp, p("wthv_sec"),
                                           p("tk"), p("tkh"), p("cldfrac"), p("inv_qc_relvar"), consts["cp_d"], consts["cv_d"], consts["latvap"],
                                           _stream()))
        torch.cuda.synchronize()
        words = w.words()
        outside = w.outside()
        report = dict(fresh=fresh, intact=bool((words[outside] == CANARY).all()), guards=int(outside.sum()),
                      written=bool((words[~outside] != CANARY).all()), bytes=w.bytes)
        out = {k: dev[k].cpu().numpy() for k in sc.UNPACKED}
        kept = untouched_by_pack and all(sc.same_bits(dev[k].cpu().numpy(), state[k]) for k in ("rho_d", "wvel", "flx_u", "flx_v", "zint", "zmid"))
        return packed, after, out, [t.cpu().numpy() for t in q], report, kept
    finally:
        w.close()


@pytest.mark.parametrize("shape,tracers,layout", CASES, ids=CASE_IDS)
def test_c_abi_equals_the_emulation_bit_for_bit(shape, tracers, layout):
    ntr = len(sc.TRACER_SETS[tracers])
    state = sc.make_state(shape, ntr)
    want = sc.emulated(state, layout)
    got = gpu_chain(state, layout)
    sc.assert_set_equal(got[0], want[0], ref.PACKED, "pack")
    sc.assert_set_equal(got[1], want[1], capi.SHOC_ARRAYS, "stand-in")
    sc.assert_set_equal(got[2], want[2], sc.UNPACKED, "unpack")
    assert len(got[3]) == ntr and all(sc.same_bits(a, b) for a, b in zip(got[3], want[3]))
    # and the emulation is the restatement (tests/test_shoc_coupling.py): layout 0 directly, layout 1 transposed
    rest = sc.restated_case(shape, ntr)
    sc.assert_set_equal(got[1], rest[1] if layout == 0 else ref.to_layout1(rest[1]), capi.SHOC_ARRAYS, "restatement")
    sc.assert_set_equal(got[2], rest[2], sc.UNPACKED, "restatement")
    # every array between canary words that are unchanged; the size formula of the header
    report = got[4]
    nz, ny, nx, nens = shape
    N, r8 = ny * nx * nens, lambda n: (n + 7) // 8 * 8
    doubles = 10 * r8(N) + r8(ntr * N) + 22 * r8(nz * N) + r8(2 * nz * N) + r8(ntr * nz * N) + 11 * r8((nz + 1) * N) + 47 * 8
    assert report["bytes"] == 8 * doubles
    assert report["fresh"] and report["intact"] and report["written"] and report["guards"] >= 47 * GUARD, report
    # density_dry, wvel, the surface fluxes and the grid arrays are unchanged; pack alone changes no state array
    assert got[5]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("tracers", ["kessler", "p3"])
def test_the_wide_index_kernels_give_the_same_bits(tracers, layout):
    """the long long instances of the pack, stand-in and unpack kernels, which sizes from 2^29 elements on select, forced at a small shape"""
    shape, ntr = (17, 3, 5, 13), len(sc.TRACER_SETS[tracers])
    state = sc.make_state(shape, ntr)
    lib = capi.load()
    capi.check(lib.pam_amd_shoc_debug_wide_index(1))
    try:
        got = gpu_chain(state, layout)
    finally:
        capi.check(lib.pam_amd_shoc_debug_wide_index(0))
    want = sc.emulated(state, layout, wide=True)
    sc.assert_set_equal(got[0], want[0], ref.PACKED, "pack")
    sc.assert_set_equal(got[1], want[1], capi.SHOC_ARRAYS, "stand-in")
    sc.assert_set_equal(got[2], want[2], sc.UNPACKED, "unpack")
    assert all(sc.same_bits(a, b) for a, b in zip(got[3], want[3]))
    assert got[4]["intact"] and got[4]["written"] and got[5]


@pytest.mark.parametrize("layout", [0, 1])
def test_two_runs_are_identical(layout):
    state = sc.make_state((17, 3, 5, 13), 7)
    a, b = gpu_chain(state, layout), gpu_chain(state, layout)
    for stage in (0, 1, 2):
        sc.assert_set_equal(a[stage], b[stage])
    assert all(sc.same_bits(x, y) for x, y in zip(a[3], b[3]))


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("tracers", ["kessler", "p3"])
def test_the_whole_ensemble_equals_its_member_shards(tracers, layout):
    shape, ntr = (33, 2, 2, 130), len(sc.TRACER_SETS[tracers])
    state = sc.make_state(shape, ntr)
    whole = gpu_chain(state, layout)
    parts = []
    for sl in (slice(0, 37), slice(37, 101), slice(101, 130)):
        shard = {k: np.ascontiguousarray(v[..., sl]) for k, v in state.items() if k != "q"}
        shard["q"] = [np.ascontiguousarray(x[..., sl]) for x in state["q"]]
        parts.append(gpu_chain(shard, layout))
    for k in sc.UNPACKED:
        assert sc.same_bits(np.concatenate([p[2][k] for p in parts], axis=-1), whole[2][k]), k
    for t in range(ntr):
        assert sc.same_bits(np.concatenate([p[3][t] for p in parts], axis=-1), whole[3][t]), t


# ------------------------------------------------------------------------------------------------------------------------------
# the Python class

KESSLER = (("water_vapor", True, True), ("cloud_liquid", True, True), ("precip_liquid", True, True))
P3 = (("cloud_water", True, True), ("cloud_water_num", True, False), ("rain", True, True), ("rain_num", True, False), ("ice", True, True),
      ("ice_num", True, False), ("ice_rime", True, False), ("ice_rime_vol", True, False), ("water_vapor", True, True))


def _coupler(state, micro, sgs):
    import torch
    from pam_amd import PamCoupler
    nz, ny, nx, nens = state["rho_d"].shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", 2.0)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(sc.XLEN, sc.YLEN, np.array(state["zint"]))
    for n, p, m in (KESSLER if micro == "kessler" else P3):
        c.add_tracer(n, "", p, m)
    if micro is not None:
        c.set_option("micro", micro)
    c.set_option("R_d", CONSTS["pres_R_d"])             # what a microphysics sets; compute_pressure_array reads them
    c.set_option("R_v", CONSTS["pres_R_v"])
    sgs.init(c)
    dm = c.get_data_manager_device_readwrite()
    cloud, names = ("cloud_liquid", ref.KESSLER_TRACERS) if micro == "kessler" else ("cloud_water", ref.P3_TRACERS)
    put = lambda name, a: dm.get(name).copy_(torch.from_numpy(np.array(a, order="C")))
    for name, key in (("density_dry", "rho_d"), ("water_vapor", "rho_v"), (cloud, "rho_c"), ("uvel", "uvel"), ("vvel", "vvel"), ("wvel", "wvel"),
                      ("temp", "temp"), ("tke", "tke"), ("wthv_sec", "wthv_sec"), ("tk", "tk"), ("tkh", "tkh"), ("cldfrac", "cldfrac"),
                      ("sfc_mom_flx_u", "flx_u"), ("sfc_mom_flx_v", "flx_v"), ("vertical_midpoint_height", "zmid")):
        put(name, state[key])
    for name, a in zip(names, state["q"]):
        put(name, a)
    return c, cloud, names


def _snapshot(c):
    import torch
    torch.cuda.synchronize()
    dm = c.get_data_manager_device_readwrite()
    return {n: e["data"].cpu().numpy().copy() for n, e in dm._e.items()}


STATE_NAMES = dict(temp="temp", rho_v="water_vapor", uvel="uvel", vvel="vvel", tke="tke", wthv_sec="wthv_sec", tk="tk", tkh="tkh", cldfrac="cldfrac",
                   inv_qc_relvar="inv_qc_relvar")


@pytest.mark.parametrize("micro", ["kessler", "p3"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("how", ["c_pointer", "python_callable"])
def test_sgs_shoc_time_step_equals_the_restatement(how, layout, micro):
    import torch
    from pam_amd import SGSShoc
    shape, ntr = (17, 3, 5, 13), 1 if micro == "kessler" else 7
    state = sc.make_state(shape, ntr)
    seen = {}

    def py_main(arrays, args):
        """the stand-in through the named torch views: checks what it receives, then runs the library's kernel on the same memory"""
        seen["shapes"] = {n: tuple(t.shape) for n, t in arrays.items()}
        seen["args"] = (args.ncol, args.nlev, args.nlevi, args.dt, args.nadv, args.num_qtracers, args.layout)
        seen["ptr"] = all(t.data_ptr() == getattr(args, n) for n, t in arrays.items() if t.numel())
        seen["host_dx"] = float(arrays["host_dx"][0])
        return capi.load().pam_amd_shoc_main_standin(C.byref(args), None)

    sgs = SGSShoc(shoc_main=SGSShoc.standin() if how == "c_pointer" else py_main, layout=layout)
    assert sgs.get_num_tracers() == 1 and sgs.sgs_name() == "shoc"
    c, cloud, names = _coupler(state, micro, sgs)
    assert c.get_option("sgs") == "shoc" and c.get_tracer_info("tke") == ("Turbulent Kinetic Energy (m^2/s^2)", True, True, False)
    before = _snapshot(c)
    dirty = c.run_module("sgs", sgs.timeStep)
    after = _snapshot(c)
    want = sc.restated_case(shape, ntr)
    for key, name in dict(STATE_NAMES, rho_c=cloud).items():
        assert sc.same_bits(after[name], want[2][key]), name
    for name, a in zip(names, want[3]):
        assert sc.same_bits(after[name], a), name
    changed = set(STATE_NAMES.values()) | {cloud} | set(names)
    for name in set(after) - changed:
        assert sc.same_bits(after[name], before[name]), name           # density_dry, wvel, the grid, the fluxes ...
    assert "density_dry" not in dirty and "wvel" not in dirty and "temp" in dirty
    if how == "python_callable":
        from pam_amd.physics import shoc_shapes
        nz, ncol = shape[0], shape[1] * shape[2] * shape[3]
        assert seen["shapes"] == shoc_shapes(ncol, nz, ntr, layout) and seen["ptr"]
        assert seen["args"] == (ncol, nz, nz + 1, 2.0, 1, ntr, layout) and seen["host_dx"] == sc.XLEN / shape[2]
    assert sgs.etime == 2.0 and not sgs.first_step
    assert sgs.workspace_bytes() > 0
    sgs.finalize(c)


def test_sgs_shoc_init_registers_what_the_reference_registers():
    from pam_amd import SGSShoc
    state = sc.make_state((5, 1, 7, 3), 1)
    sgs = SGSShoc()
    c, _, _ = _coupler(state, "kessler", sgs)
    dm = c.get_data_manager_device_readwrite()
    nz, ny, nx, nens = 5, 1, 7, 3
    for n in ("wthv_sec", "tk", "tkh", "cldfrac", "inv_qc_relvar", "tke"):
        assert dm.get_shape(n) == [nz, ny, nx, nens]
    for n in ("sfc_shf", "sfc_lhf", "sfc_mom_flx_u", "sfc_mom_flx_v"):
        assert dm.get_shape(n) == [ny, nx, nens]
    assert c.get_tracer_names()[-1] == "tke"
    c2 = __import__("pam_amd").PamCoupler("cuda:0")
    c2.allocate_coupler_state(nz, ny, nx, nens)
    SGSShoc().init(c2)
    import torch
    torch.cuda.synchronize()
    for n in ("tke", "wthv_sec", "tk", "tkh", "cldfrac", "inv_qc_relvar", "sfc_mom_flx_u", "sfc_mom_flx_v"):
        assert not c2.get_data_manager_device_readwrite().get(n, readonly=True).cpu().numpy().any(), n


def test_refused_time_steps_leave_every_field_untouched():
    from pam_amd import SGSShoc
    state = sc.make_state((5, 1, 7, 3), 1)
    # no shoc_main
    sgs = SGSShoc(layout=1)
    c, _, _ = _coupler(state, "kessler", sgs)
    before = _snapshot(c)
    with pytest.raises(capi.PamAmdError, match="no shoc_main is registered"):
        sgs.timeStep(c)
    # micro unset, micro unknown: the reference's messages
    for micro, msg in ((None, r'SHOC requires coupler.set_option<std::string>\("micro",...\) to be set'),
                       ("none", "SHOC only meant to run with kessler or p3 microphysics")):
        sgs = SGSShoc(shoc_main=SGSShoc.standin())
        c2, _, _ = _coupler(state, "kessler", sgs)
        if micro is None:
            c2.options.delete_option("micro")
        else:
            c2.set_option("micro", micro)
        b2 = _snapshot(c2)
        with pytest.raises(capi.PamAmdError, match=msg):
            sgs.timeStep(c2)
        a2 = _snapshot(c2)
        assert all(sc.same_bits(a2[n], b2[n]) for n in b2), micro
        assert sgs.first_step and sgs.etime == 0
    after = _snapshot(c)
    assert all(sc.same_bits(after[n], before[n]) for n in before)
    with pytest.raises(capi.PamAmdError, match="layout"):
        SGSShoc(layout=2)


def test_pack_and_unpack_refuse_a_missing_tracer_pointer():
    """what needs a real workspace to be reached: the tracer list"""
    lib = capi.load()
    w = Workspace((5, 1, 7, 3), 1, 1)
    try:
        import test_shoc_coupling as cpu
        P = cpu.P
        for args in (None, (C.c_void_p * 1)(None)):
            assert lib.pam_amd_shoc_pack(w.ws, *([P] * 8), args, *cpu.PACK_OK[10:]) == -1
            assert b"qtracers" in lib.pam_amd_awfl_last_error()
            assert lib.pam_amd_shoc_unpack(w.ws, *([P] * 7), args, *cpu.UNPACK_OK[9:]) == -1
            assert b"qtracers" in lib.pam_amd_awfl_last_error()
        assert bool((w.words() == CANARY).all())                 # nothing was launched
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ class

def _cxx_run(tmp_path, state, p3, layout, mode):
    shape = state["rho_d"].shape
    order = ["rho_d", "rho_v", "rho_c", "uvel", "vvel", "wvel", "temp", "tke", "wthv_sec", "tk", "tkh", "cldfrac"]
    src, dst = tmp_path / ("in_%s_%d" % (mode, layout)), tmp_path / ("out_%s_%d" % (mode, layout))
    with open(src, "wb") as f:
        f.write(np.array(list(shape) + [int(p3), layout], dtype=np.int32).tobytes())
        for a in [state[k] for k in ("zint", "zmid", "flx_u", "flx_v")] + [state[k] for k in order] + list(state["q"]):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([cxx_program("shoc_sgs"), str(src), str(dst), mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    names = order + ["q%d" % t for t in range(len(state["q"]))] + ["inv_qc_relvar"]
    flat = np.fromfile(dst, dtype=np.float64).reshape(len(names), *shape)
    return r.stdout, dict(zip(names, flat))


@pytest.mark.parametrize("micro", ["kessler", "p3"])
@pytest.mark.parametrize("layout", [0, 1])
def test_cxx_sgs_time_step_equals_the_restatement(tmp_path, layout, micro):
    shape, ntr = (17, 3, 5, 13), 1 if micro == "kessler" else 7
    state = sc.make_state(shape, ntr)
    stdout, got = _cxx_run(tmp_path, state, micro == "p3", layout, "run")
    assert "threw" not in stdout and "### members 1 etime 2 first_step 0" in stdout, stdout
    want = sc.restated_case(shape, ntr)
    for k in sc.UNPACKED:
        assert sc.same_bits(got[k], want[2][k]), k
    for t in range(ntr):
        assert sc.same_bits(got["q%d" % t], want[3][t]), t
    assert sc.same_bits(got["rho_d"], state["rho_d"]) and sc.same_bits(got["wvel"], state["wvel"])


@pytest.mark.parametrize("mode,message", [("no_shoc_main", "ERROR: SHOC: no shoc_main is registered"),
                                          ("no_micro", 'ERROR: SHOC requires coupler.set_option<std::string>("micro",...) to be set'),
                                          ("bad_micro", "ERROR: SHOC only meant to run with kessler or p3 microphysics")])
def test_cxx_sgs_refusals_leave_every_field_untouched(tmp_path, mode, message):
    state = sc.make_state((5, 1, 7, 3), 1)
    stdout, got = _cxx_run(tmp_path, state, False, 1, mode)
    assert "### threw " + message in stdout and "etime 0 first_step 1" in stdout, stdout
    for k in ("rho_d", "rho_v", "rho_c", "uvel", "vvel", "wvel", "temp", "tke", "wthv_sec", "tk", "tkh", "cldfrac"):
        assert sc.same_bits(got[k], state[k]), k
    assert sc.same_bits(got["q0"], state["q"][0]) and not got["inv_qc_relvar"].any()


# ------------------------------------------------------------------------------------------------------------------------------
# three CRM steps

def test_three_crm_steps_dycore_sponge_shoc_kessler_validate_clean(capsys):
    import torch
    from pam_amd import Dycore, Microphysics, PamCoupler, SGSShoc, idealized as idz, modules
    nens, nx, ny, nz, crm_dt = 4, 8, 6, 16, 4.0
    tr = idz.TRACERS_KESSLER_SHOC
    zint = idz.stretched_interfaces(nz, 15000.0)
    f = idz.supercell_fields(nens, nx, ny, nz, zint, tracers=tr, magnitude=0.5)
    f["tracers"][2][0:6] = 2e-3 * f["density_dry"][0:6]
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", crm_dt)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(nx * 500.0, ny * 500.0, zint)
    micro, sgs, dyc = Microphysics(), SGSShoc(shoc_main=SGSShoc.standin(), layout=1), Dycore()
    micro.init(c)
    sgs.init(c)
    dyc.init(c)
    assert c.get_tracer_names() == [t[0] for t in tr]
    c.load_fields(f)
    dyc.declare_current_profile_as_hydrostatic(c)
    dm = c.get_data_manager_device_readwrite()
    start = {n: dm.get(n, readonly=True).clone() for n in ("temp", "uvel", "tke", "water_vapor")}
    for _ in range(3):
        dyc.timeStep(c)
        modules.sponge_layer(c)
        c.run_module("sgs", sgs.timeStep)
        micro.timeStep(c)
    torch.cuda.synchronize()
    dm.validate_all()
    assert capsys.readouterr().err == ""
    tke = dm.get("tke", readonly=True)
    assert bool((tke > 0).all())                                   # the 0.004 floor times the density
    assert bool((dm.get("uvel", readonly=True) != start["uvel"]).any()) and bool((dm.get("temp", readonly=True) != start["temp"]).any())
    assert bool((dm.get("inv_qc_relvar", readonly=True) >= 0.001).all()) and bool((dm.get("cldfrac", readonly=True) == 0).all())
    assert sgs.etime == 3 * crm_dt
    sgs.finalize(c)
    dyc.finalize(c)
