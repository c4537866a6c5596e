"""The P3 coupling layer on the GPU: pack, the stand-in for p3_main and unpack through the C ABI against the host emulation bit for bit in
both layouts (without the adjustment directly; with it, the adjusted fields by the saturation-adjustment gate and everything else bit for
bit on the GPU's adjusted state); the workspace's canary words; what must stay untouched; layout, index-width, run-to-run and
shard-to-whole identity; the Python class MicrophysicsP3 and the C++ class; three CRM steps of the reference's CI plug-in combination;
and the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import p3_cases as pc
import p3_coupling_ref as ref
from pam_amd import capi
from tools.native_build import cxx_program

pytestmark = pytest.mark.gpu

CANARY = 0x7ff850335f57535f
GUARD = 8
CONSTS = ref.CONSTS
IN_4D = pc.EMU_STATE                      # rho_d, rho_v, rho_c, temp, the three nuclei arrays, q_prev, t_prev
OUT_4D = ("liq_ice_exchange_out", "vap_liq_exchange_out", "vap_ice_exchange_out")
OUT_3D = ("precip_liq_surf_out", "precip_ice_surf_out")


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
    def __init__(self, shape, layout, nout=0):
        nz, ny, nx, nens = shape
        self.lib = capi.load()
        self.ws = C.c_void_p()
        capi.check(self.lib.pam_amd_p3_workspace_create(nens, nx, ny, nz, layout, nout, C.byref(self.ws)))
        self.args = capi.P3Args()
        capi.check(self.lib.pam_amd_p3_workspace_args(self.ws, C.byref(self.args)))
        n = C.c_longlong()
        capi.check(self.lib.pam_amd_p3_workspace_bytes(self.ws, C.byref(n)))
        self.bytes = n.value
        from pam_amd.physics import p3_shapes
        self.shapes = p3_shapes(ny * nx * nens, nz, layout, nout)

    def arrays(self):
        import torch
        torch.cuda.synchronize()
        return {n: (_view(getattr(self.args, n), shp).cpu().numpy() if min(shp) > 0 else np.zeros(shp)) for n, shp in self.shapes.items()}

    def words(self):
        """the whole allocation as 64-bit words"""
        import torch
        torch.cuda.synchronize()
        return _view(self.args.qc - 8 * GUARD, (self.bytes // 8,), "<i8").cpu().numpy().view(np.uint64)

    def outside(self):
        """mask of the words that belong to no array"""
        mask = np.ones(self.bytes // 8, dtype=bool)
        base = self.args.qc - 8 * GUARD
        for n, shp in self.shapes.items():
            if min(shp) > 0:
                at = (getattr(self.args, n) - base) // 8
                mask[at:at + int(np.prod(shp))] = False
        return mask

    def close(self):
        capi.check(self.lib.pam_amd_p3_workspace_destroy(self.ws))


def gpu_chain(state, layout, adjust, first_step, nout=0, consts=CONSTS):
    """pack, stand-in, unpack through the C ABI.  Returns (packed set, set after the stand-in, state after as a dict of pc.STATE_AFTER, the
    coupler's (rho_v, rho_c, temp) after pack, canary report, untouched report)"""
    import torch
    shape = state["rho_d"].shape
    nz, ny, nx, nens = shape
    lib = capi.load()
    dev = {k: torch.from_numpy(np.array(state[k], order="C")).cuda() for k in IN_4D + ("zint",)}
    for k in OUT_4D:
        dev[k] = torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    for k in OUT_3D:
        dev[k] = torch.full((ny, nx, nens), float("nan"), dtype=torch.float64, device="cuda")
    q = [torch.from_numpy(np.array(x, order="C")).cuda() for x in state["q"]]
    qp = (C.c_void_p * 7)(*[t.data_ptr() for t in q])
    w = Workspace(shape, layout, nout)
    try:
        fresh = bool((w.words() == CANARY).all())
        p = lambda k: dev[k].data_ptr()
        capi.check(lib.pam_amd_p3_pack(w.ws, p("rho_d"), p("rho_v"), p("rho_c"), p("temp"), qp, p("nccn_prescribed"), p("nc_nuceat_tend"),
                                       p("ni_activated"), p("q_prev"), p("t_prev"), p("zint"), int(adjust), int(first_step), consts["R_d"],
                                       consts["R_v"], consts["cp_d"], consts["cp_v"], consts["cp_l"], consts["p0"], consts["grav"], _stream()))
        packed = w.arrays()
        adjusted = {k: dev[k].cpu().numpy() for k in pc.ADJUSTED}
        read_only = ("rho_d", "nccn_prescribed", "nc_nuceat_tend", "ni_activated", "q_prev", "t_prev", "zint") + (() if adjust else pc.ADJUSTED)
        kept = all(pc.same_bits(dev[k].cpu().numpy(), state[k]) for k in read_only) and \
            all(pc.same_bits(t.cpu().numpy(), x) for t, x in zip(q, state["q"]))
        w.args.dt, w.args.stream = 2.0, _stream()
        capi.check(lib.pam_amd_p3_main_standin(C.byref(w.args), None))
        after = w.arrays()
        capi.check(lib.pam_amd_p3_unpack(w.ws, p("rho_d"), p("rho_v"), p("rho_c"), qp, p("temp"), p("q_prev"), p("t_prev"),
                                         p("liq_ice_exchange_out"), p("vap_liq_exchange_out"), p("vap_ice_exchange_out"),
                                         p("precip_liq_surf_out"), p("precip_ice_surf_out"), consts["cp_d"], consts["cv_d"], _stream()))
        torch.cuda.synchronize()
        words, outside = w.words(), w.outside()
        report = dict(fresh=fresh, intact=bool((words[outside] == CANARY).all()), guards=int(outside.sum()),
                      written=bool((words[~outside] != CANARY).all()), bytes=w.bytes)
        out = {k: dev[k].cpu().numpy() for k in ("rho_c", "rho_v", "temp", "q_prev", "t_prev") + OUT_4D + OUT_3D}
        for t in range(7):
            out["q%d" % t] = q[t].cpu().numpy()
        kept = kept and all(pc.same_bits(dev[k].cpu().numpy(), state[k]) for k in ("rho_d", "nccn_prescribed", "nc_nuceat_tend", "ni_activated", "zint"))
        return packed, after, out, adjusted, report, kept
    finally:
        w.close()


def _doubles(shape, nout=0):
    nz, ny, nx, nens = shape
    N, r8 = ny * nx * nens, lambda n: (n + 7) // 8 * 8
    return 37 * r8(nz * N) + 2 * r8(N) + 2 * r8((nz + 1) * N) + r8(3 * N) + 43 * 8 + ((r8(nout * nz * N) + 8) if nout else 0)


def _no_tend(d):
    return {k: v for k, v in d.items() if k != "p3_tend_out"}


CASES = [(s, l, f) for s in pc.SHAPES for l in (0, 1) for f in (1, 0)]
CASE_IDS = ["%s-layout%d-first%d" % ("x".join(map(str, s)), l, f) for s, l, f in CASES]


@pytest.mark.parametrize("shape,layout,first_step", CASES, ids=CASE_IDS)
def test_c_abi_equals_the_emulation_bit_for_bit_without_the_adjustment(shape, layout, first_step):
    state = pc.make_state(shape)
    want = pc.emulated(state, layout, 0, first_step)
    got = gpu_chain(state, layout, 0, first_step)
    pc.assert_set_equal(got[0], want[0], ref.PACKED, "pack")
    pc.assert_set_equal(_no_tend(got[1]), _no_tend(want[1]), None, "stand-in")
    pc.assert_set_equal(got[2], want[2], pc.STATE_AFTER, "unpack")
    # and the emulation is the restatement (tests/test_p3_coupling.py): layout 0 directly, layout 1 transposed and flipped
    rest = pc.restated_case(shape, 0, first_step)
    r1 = _no_tend(rest[1])
    pc.assert_set_equal(got[1], r1 if layout == 0 else ref.to_layout1(r1), None, "restatement")
    pc.assert_set_equal(got[2], rest[2], pc.STATE_AFTER, "restatement")
    # every array between canary words that are unchanged; the size formula of the header
    report = got[4]
    assert report["bytes"] == 8 * _doubles(shape)
    assert report["fresh"] and report["intact"] and report["written"] and report["guards"] >= 43 * GUARD, report
    # density_dry, the nuclei arrays, the grid, the coupler's q_prev / t_prev and, without the adjustment, rho_v, rho_c, temp: pack reads only
    assert got[5]


@pytest.mark.parametrize("shape,layout,first_step", CASES, ids=CASE_IDS)
def test_c_abi_with_the_adjustment(shape, layout, first_step):
    """(a) the rho_v, rho_c, temp pack leaves in the coupler state against the restatement, by the gate of
    test_gpu_saturation_adjustment_matches_restatement: bit for bit (the device's exp differs from glibc's in the last place, but enters
    only through decisions none of which is near a tie on these states: no cell is exempt); cells in neither branch are unchanged bit
    for bit.  (b) every other packed array, and the chain through stand-in and unpack, against the emulation run without
    the adjustment ON THE GPU'S ADJUSTED STATE, bit for bit."""
    state = pc.make_state(shape)
    got = gpu_chain(state, layout, 1, first_step)
    rest = pc.restated_case(shape, 1, first_step)
    exempt = pc.adjusted_within_gate(got[3], rest[3], rest[4], state)
    print("p3 pack adjust=1 %s layout %d: %d of %d cells adjusted, %.4f %% exempt (decision margin < 1e-12)"
          % (shape, layout, int((rest[4]["branch"] > 0).sum()), rest[4]["branch"].size, 100 * exempt))
    assert exempt == 0
    want = pc.emulated(pc.with_adjusted(state, got[3]), layout, 0, first_step)
    pc.assert_set_equal(got[0], want[0], ref.PACKED, "pack")
    pc.assert_set_equal(_no_tend(got[1]), _no_tend(want[1]), None, "stand-in")
    pc.assert_set_equal(got[2], want[2], pc.STATE_AFTER, "unpack")
    assert got[4]["intact"] and got[4]["written"] and got[5]


def test_p3_tend_out_planes_lie_between_intact_canaries():
    shape = (5, 1, 7, 3)
    state = pc.make_state(shape)
    got = gpu_chain(state, 0, 0, 1, nout=49)
    want = pc.emulated(state, 0, 0, 1, num_tend_out=49)
    assert got[1]["p3_tend_out"].shape == (49, 5, 21) and pc.same_bits(got[1]["p3_tend_out"], want[1]["p3_tend_out"])
    pc.assert_set_equal(got[2], want[2], pc.STATE_AFTER, "unpack")
    assert got[4]["bytes"] == 8 * _doubles(shape, 49) and got[4]["intact"] and got[4]["written"]


@pytest.mark.parametrize("adjust", [0, 1])
def test_the_state_after_unpack_does_not_depend_on_the_layout_the_index_width_or_the_run(adjust):
    shape = (17, 3, 5, 13)
    state = pc.make_state(shape)
    lib = capi.load()
    a0, a1, again = gpu_chain(state, 0, adjust, 1), gpu_chain(state, 1, adjust, 1), gpu_chain(state, 1, adjust, 1)
    capi.check(lib.pam_amd_p3_debug_wide_index(1))
    try:
        w0, w1 = gpu_chain(state, 0, adjust, 1, nout=49), gpu_chain(state, 1, adjust, 1)
    finally:
        capi.check(lib.pam_amd_p3_debug_wide_index(0))
    for other, what in ((a1, "layout"), (again, "run"), (w0, "wide 0"), (w1, "wide 1")):
        pc.assert_set_equal(other[2], a0[2], pc.STATE_AFTER, what)
        pc.assert_set_equal(other[3], a0[3], pc.ADJUSTED, what)
    for stage in (0, 1):
        pc.assert_set_equal(again[stage], a1[stage], None, "run")
        pc.assert_set_equal(w1[stage], a1[stage], None, "wide")
        pc.assert_set_equal(_no_tend(w0[stage]), _no_tend(a0[stage]), None, "wide")
    assert w0[4]["intact"] and w1[4]["intact"]


@pytest.mark.parametrize("layout", [0, 1])
def test_the_whole_ensemble_equals_its_member_shards(layout):
    shape = (33, 2, 2, 130)
    state = pc.make_state(shape)
    whole = gpu_chain(state, layout, 1, 0)
    parts = []
    for sl in (slice(0, 37), slice(37, 101), slice(101, 130)):
        shard = {k: np.ascontiguousarray(v[..., sl]) for k, v in state.items() if k != "q"}
        shard["q"] = [np.ascontiguousarray(x[..., sl]) for x in state["q"]]
        parts.append(gpu_chain(shard, layout, 1, 0))
    for k in pc.STATE_AFTER:
        assert pc.same_bits(np.concatenate([p[2][k] for p in parts], axis=-1), whole[2][k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# the Python class

NAMES = dict(rho_d="density_dry", rho_v="water_vapor", rho_c="cloud_water", temp="temp", nccn_prescribed="nccn_prescribed",
             nc_nuceat_tend="nc_nuceat_tend", ni_activated="ni_activated", q_prev="q_prev", t_prev="t_prev")
AFTER_NAMES = dict(rho_c="cloud_water", rho_v="water_vapor", temp="temp", q_prev="q_prev", t_prev="t_prev",
                   **{k: k for k in OUT_4D + OUT_3D}, **{"q%d" % t: n for t, n in enumerate(ref.TRACERS)})


def _coupler(state, sgs, micro):
    import torch
    from pam_amd import PamCoupler
    nz, ny, nx, nens = state["rho_d"].shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", 2.0)
    if sgs is not None:
        c.set_option("sgs", sgs)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(16000.0, 12000.0, np.array(state["zint"]))
    micro.init(c)
    dm = c.get_data_manager_device_readwrite()
    put = lambda name, a: dm.get(name).copy_(torch.from_numpy(np.array(a, order="C")))
    for key, name in NAMES.items():
        put(name, state[key])
    for name, a in zip(ref.TRACERS, state["q"]):
        put(name, a)
    return c


def _snapshot(c):
    import torch
    torch.cuda.synchronize()
    dm = c.get_data_manager_device_readwrite()
    return {n: e["data"].cpu().numpy().copy() for n, e in dm._e.items()}


def _state_of(snapshot, state):
    s = {k: snapshot[name] for k, name in NAMES.items()}
    s["q"] = [snapshot[n] for n in ref.TRACERS]
    s["zint"] = state["zint"]
    return s


@pytest.mark.parametrize("sgs", ["shoc", "none"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("how", ["c_pointer", "python_callable"])
def test_microphysics_p3_two_time_steps_equal_the_restatement(how, layout, sgs):
    """two consecutive steps.  sgs = "shoc" (no adjustment): bit for bit.  sgs = "none": the python callable records the state pack left,
    which is held to the restatement by the gate; from there on bit for bit, as in test_c_abi_with_the_adjustment."""
    from pam_amd import MicrophysicsP3
    from pam_amd.physics import p3_shapes
    shape = (17, 3, 5, 13)
    state = pc.make_state(shape)
    seen = []

    def py_main(arrays, args):
        """the stand-in through the named torch views: records what it receives, then runs the library's kernel on the same memory"""
        seen.append(dict(shapes={n: tuple(t.shape) for n, t in arrays.items()},
                         args=(args.ncol, args.nlev, args.dt, args.it, args.its, args.ite, args.kts, args.kte, args.do_predict_nc,
                               args.do_prescribed_CCN, args.layout, args.num_tend_out),
                         ptr=all(t.data_ptr() == getattr(args, n) for n, t in arrays.items() if t.numel()),
                         one=float(arrays["col_location"].sum()), snapshot=_snapshot(c)))
        return capi.load().pam_amd_p3_main_standin(C.byref(args), None)

    micro = MicrophysicsP3(p3_main=MicrophysicsP3.standin() if how == "c_pointer" else py_main, layout=layout)
    c = _coupler(state, sgs, micro)
    assert c.get_option("micro") == "p3"
    current = state
    for step in (0, 1):
        before = _snapshot(c)
        dirty = c.run_module("micro", micro.timeStep)
        after = _snapshot(c)
        rest = pc.restated(current, sgs == "none", step == 0, pow=pc.emu_harness.emu_pow)
        if sgs == "shoc":
            want = rest[2]
        elif how == "python_callable":
            mid = _state_of(seen[step]["snapshot"], state)
            exempt = pc.adjusted_within_gate({k: mid[k] for k in pc.ADJUSTED}, rest[3], rest[4], current)
            assert exempt <= pc.EXEMPT_MAX
            assert all(pc.same_bits(seen[step]["snapshot"][n], before[n]) for n in ("q_prev", "t_prev", "density_dry"))   # pack reads them only
            want = pc.emulated(mid, layout, 0, step == 0)[2]
        else:
            want = None                                     # the C pointer with the adjustment: against the other way in, below
        if want is not None:
            for key, name in AFTER_NAMES.items():
                assert pc.same_bits(after[name], want[key]), (step, name)
        for name in set(after) - set(AFTER_NAMES.values()):
            assert pc.same_bits(after[name], before[name]), (step, name)          # density_dry, the winds, the grid, the nuclei arrays ...
        assert "density_dry" not in dirty and "nccn_prescribed" not in dirty and "temp" in dirty and "q_prev" in dirty
        current = _state_of(after, state)
    if how == "python_callable":
        nz, ncol = shape[0], shape[1] * shape[2] * shape[3]
        nout = 49 if layout == 0 else 0
        for s in seen:
            assert s["shapes"] == p3_shapes(ncol, nz, layout, nout) and s["ptr"] and s["one"] == 3.0 * ncol
            assert s["args"] == ((ncol, nz, 2.0, 1, 1, ncol, 1, nz, 1, 1, 0, 49) if layout == 0 else (ncol, nz, 2.0, 0, 0, ncol - 1, 0, nz - 1, 1, 1, 1, 0))
    assert micro.etime == 4.0 and not micro.first_step and micro.sgs_shoc == (sgs == "shoc")
    assert micro.workspace_bytes() == 8 * _doubles(shape, 49 if layout == 0 else 0)
    final = _snapshot(c)
    micro.finalize(c)
    _FINAL[(how, layout, sgs)] = {name: final[name] for name in AFTER_NAMES.values()}
    other = _FINAL.get(("python_callable" if how == "c_pointer" else "c_pointer", layout, sgs))
    if other is not None:                                   # both ways in run the same kernels: the same bits after two steps
        for name, a in other.items():
            assert pc.same_bits(final[name], a), name


_FINAL = {}


def test_microphysics_p3_init_registers_what_the_reference_registers():
    """against the fixture recorded from the reference's init: tracer names and flags, the ten arrays and their shapes, the nine options"""
    import torch
    from pam_amd import MicrophysicsP3, PamCoupler
    g = np.load(os.path.join(pc.ROOT, "tests", "golden", "p3_coupling_ref.npz"))
    label = "5x2x3x3_none_"
    nz, ny, nx, nens = 5, 2, 3, 3
    c = PamCoupler("cuda:0")
    c.allocate_coupler_state(nz, ny, nx, nens)
    micro = MicrophysicsP3()
    micro.init(c)
    info = list(g[label + "info"])
    assert c.get_tracer_names() == [t[0] for t in MicrophysicsP3.TRACERS] and len(c.get_tracer_names()) == info[0] == micro.get_num_tracers()
    flags = []
    for n in c.get_tracer_names():
        ti = c.get_tracer_info(n)
        flags += [int(ti[2]), int(ti[3])]
        assert ti[0] == dict((t[0], t[1]) for t in MicrophysicsP3.TRACERS)[n]
    assert flags == info[2:]
    dm = c.get_data_manager_device_readwrite()
    for n in ("nccn_prescribed", "nc_nuceat_tend", "ni_activated", "q_prev", "t_prev") + OUT_4D:
        assert dm.get_shape(n) == list(g[label + "out_" + n].shape[1:]) == [nz, ny, nx, nens], n
    for n in OUT_3D:
        assert dm.get_shape(n) == list(g[label + "out_" + n].shape[1:]) == [ny, nx, nens], n
    assert [c.get_option(k) for k in ("latvap", "latice", "R_d", "R_v", "cp_d", "cp_v", "grav", "p0")] == list(g[label + "options"])
    assert c.get_option("micro") == bytes(g[label + "micro"]).rstrip(b"\0").decode() == "p3" and micro.etime == 0
    torch.cuda.synchronize()
    for n in c.get_tracer_names() + list(("nccn_prescribed", "nc_nuceat_tend", "ni_activated", "q_prev", "t_prev") + OUT_4D + OUT_3D):
        assert not dm.get(n, readonly=True).cpu().numpy().any(), n


def test_refused_time_steps_leave_every_field_untouched():
    from pam_amd import MicrophysicsP3
    state = pc.make_state((5, 1, 7, 3))
    # no p3_main: nothing is launched, no workspace is made
    micro = MicrophysicsP3(layout=1)
    c = _coupler(state, "none", micro)
    before = _snapshot(c)
    with pytest.raises(capi.PamAmdError, match="no p3_main is registered"):
        micro.timeStep(c)
    after = _snapshot(c)
    assert all(pc.same_bits(after[n], before[n]) for n in before) and micro._ws is None and micro.first_step and micro.etime == 0
    # a p3_main that fails (SHOC as the SGS: pack writes the workspace only; the coupler's q_prev is not the mixing ratio the reference leaves)
    micro = MicrophysicsP3(p3_main=lambda arrays, args: 7, layout=1)
    c = _coupler(state, "shoc", micro)
    before = _snapshot(c)
    with pytest.raises(capi.PamAmdError, match="p3_main returned 7"):
        micro.timeStep(c)
    after = _snapshot(c)
    assert all(pc.same_bits(after[n], before[n]) for n in before) and micro.first_step and micro.etime == 0
    # option sgs missing: the reference's get_option fails too
    micro = MicrophysicsP3(p3_main=MicrophysicsP3.standin())
    c = _coupler(state, None, micro)
    before = _snapshot(c)
    with pytest.raises(capi.PamAmdError):
        micro.timeStep(c)
    after = _snapshot(c)
    assert all(pc.same_bits(after[n], before[n]) for n in before) and micro._ws is None


def test_pack_and_unpack_refusals_leave_the_workspace_and_the_fields_untouched():
    """what needs a real workspace to be reached: the tracer list; a bad constant and a foreign workspace beside it"""
    import torch
    import test_p3_coupling as cpu
    lib = capi.load()
    shape = (5, 1, 7, 3)
    state = pc.make_state(shape)
    w = Workspace(shape, 1)
    dev = {k: torch.from_numpy(np.array(state[k], order="C")).cuda() for k in IN_4D + ("zint",)}
    q = [torch.from_numpy(np.array(x, order="C")).cuda() for x in state["q"]]
    try:
        p = lambda k: dev[k].data_ptr()
        ok = [w.ws, p("rho_d"), p("rho_v"), p("rho_c"), p("temp"), (C.c_void_p * 7)(*[t.data_ptr() for t in q]), p("nccn_prescribed"),
              p("nc_nuceat_tend"), p("ni_activated"), p("q_prev"), p("t_prev"), p("zint")] + cpu.PACK_OK[12:]
        missing = (C.c_void_p * 7)(*[t.data_ptr() for t in q[:6]] + [None])
        fake = (C.c_ulonglong * 64)()
        for index, value, msg in ((5, None, b"tracers"), (5, missing, b"tracers"), (16, float("nan"), b"finite"), (0, fake, b"not a workspace")):
            args = list(ok)
            args[index] = value
            assert lib.pam_amd_p3_pack(*args) == -1 and msg in lib.pam_amd_awfl_last_error(), (index, lib.pam_amd_awfl_last_error())
        for args in (None, missing):
            assert lib.pam_amd_p3_unpack(w.ws, *([cpu.P] * 3), args, *cpu.UNPACK_OK[5:]) == -1
            assert b"tracers" in lib.pam_amd_awfl_last_error()
        assert bool((w.words() == CANARY).all())                 # nothing was launched
        assert all(pc.same_bits(dev[k].cpu().numpy(), state[k]) for k in IN_4D) and all(pc.same_bits(t.cpu().numpy(), x) for t, x in zip(q, state["q"]))
    finally:
        w.close()
    # num_tend_out in layout 1
    ws = C.c_void_p(1)
    assert lib.pam_amd_p3_workspace_create(3, 7, 1, 5, 1, 49, C.byref(ws)) == -1 and not ws.value
    assert b"num_tend_out" in lib.pam_amd_awfl_last_error()


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ class

CXX_ORDER = ("rho_d", "rho_v", "rho_c", "temp", "nccn_prescribed", "nc_nuceat_tend", "ni_activated", "q_prev", "t_prev")


def _cxx_run(tmp_path, state, shoc, layout, steps, mode):
    shape = state["rho_d"].shape
    nz, ny, nx, nens = shape
    src, dst = tmp_path / ("in_%s_%d" % (mode, layout)), tmp_path / ("out_%s_%d" % (mode, layout))
    with open(src, "wb") as f:
        f.write(np.array(list(shape) + [int(shoc), layout, steps], dtype=np.int32).tobytes())
        for a in [state["zint"]] + [state[k] for k in CXX_ORDER] + list(state["q"]):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([cxx_program("p3_micro"), str(src), str(dst), mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    names = list(CXX_ORDER) + ["q%d" % t for t in range(7)] + list(OUT_4D)
    flat = np.fromfile(dst, dtype=np.float64)
    n4 = int(np.prod(shape))
    got = {n: flat[i * n4:(i + 1) * n4].reshape(shape) for i, n in enumerate(names)}
    for i, n in enumerate(OUT_3D):
        got[n] = flat[len(names) * n4 + i * ny * nx * nens:len(names) * n4 + (i + 1) * ny * nx * nens].reshape(ny, nx, nens)
    return r.stdout, got


@pytest.mark.parametrize("sgs", ["shoc", "none"])
@pytest.mark.parametrize("layout", [0, 1])
def test_cxx_microphysics_two_time_steps_equal_the_restatement(tmp_path, layout, sgs):
    """sgs = "shoc": the restatement bit for bit.  sgs = "none": the Python class, which the test above holds to the restatement by the
    gate, bit for bit (the same kernels on the same device)."""
    from pam_amd import MicrophysicsP3
    shape = (17, 3, 5, 13)
    state = pc.make_state(shape)
    stdout, got = _cxx_run(tmp_path, state, sgs == "shoc", layout, 2, "run")
    assert "threw" not in stdout and "### members 1 etime 4 first_step 0 sgs_shoc %d" % (sgs == "shoc") in stdout, stdout
    if sgs == "shoc":
        current = state
        for step in (0, 1):
            want = pc.restated(current, False, step == 0, pow=pc.emu_harness.emu_pow)[2]
            current = dict(current, **{k: want[k] for k in ("rho_v", "rho_c", "temp", "q_prev", "t_prev")})
            current["q"] = [want["q%d" % t] for t in range(7)]
    else:
        micro = MicrophysicsP3(p3_main=MicrophysicsP3.standin(), layout=layout)
        c = _coupler(state, sgs, micro)
        micro.timeStep(c)
        micro.timeStep(c)
        snap = _snapshot(c)
        micro.finalize(c)
        want = {k: snap[name] for k, name in AFTER_NAMES.items()}
    for k in pc.STATE_AFTER:
        assert pc.same_bits(got[k], want[k]), k
    for k in ("rho_d", "nccn_prescribed", "nc_nuceat_tend", "ni_activated"):
        assert pc.same_bits(got[k], state[k]), k


@pytest.mark.parametrize("mode,message", [("no_p3_main", "ERROR: P3: no p3_main is registered"),
                                          ("failing_p3_main", "ERROR: P3: p3_main returned 7"),
                                          ("tend_out_layout1", "num_tend_out must be 0 in layout 1")])
def test_cxx_microphysics_refusals_leave_every_field_untouched(tmp_path, mode, message):
    state = pc.make_state((5, 1, 7, 3))
    stdout, got = _cxx_run(tmp_path, state, True, 1, 1, mode)
    assert "### threw " in stdout and message in stdout and "etime 0 first_step 1" in stdout, stdout
    for k in CXX_ORDER:
        assert pc.same_bits(got[k], state[k]), k
    assert all(pc.same_bits(got["q%d" % t], state["q"][t]) for t in range(7)) and not any(got[k].any() for k in OUT_4D + OUT_3D)


# ------------------------------------------------------------------------------------------------------------------------------
# three CRM steps

@pytest.mark.parametrize("sgs_name", ["shoc", "none"])
def test_three_crm_steps_dycore_sponge_sgs_p3_validate_clean(capsys, sgs_name):
    """the reference's CI plug-in combination -- dycore -> sponge -> SHOC -> P3, each around its stand-in -- and the same with no SGS, where
    P3's pack runs the saturation adjustment"""
    import torch
    from pam_amd import Dycore, MicrophysicsP3, PamCoupler, SGSNone, SGSShoc, idealized as idz, modules
    nens, nx, ny, nz, crm_dt = 4, 8, 6, 16, 4.0
    tr = idz.TRACERS_P3_SHOC if sgs_name == "shoc" else idz.TRACERS_P3_SHOC[:-1]
    zint = idz.stretched_interfaces(nz, 15000.0)
    f = idz.supercell_fields(nens, nx, ny, nz, zint, tracers=tr, magnitude=0.5)
    f["tracers"][2][0:6] = 2e-3 * f["density_dry"][0:6]                 # rain
    f["tracers"][0][2:5] = 1e-3 * f["density_dry"][2:5]                 # cloud water: something to evaporate
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", crm_dt)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(nx * 500.0, ny * 500.0, zint)
    micro = MicrophysicsP3(p3_main=MicrophysicsP3.standin(), layout=1)
    sgs = SGSShoc(shoc_main=SGSShoc.standin(), layout=1) if sgs_name == "shoc" else SGSNone()
    dyc = Dycore()
    micro.init(c)
    sgs.init(c)
    dyc.init(c)
    assert c.get_tracer_names() == [t[0] for t in tr]
    c.load_fields(f)
    dyc.declare_current_profile_as_hydrostatic(c)
    dm = c.get_data_manager_device_readwrite()
    start = {n: dm.get(n, readonly=True).clone() for n in ("temp", "water_vapor", "cloud_water", "rain")}
    for _ in range(3):
        dyc.timeStep(c)
        modules.sponge_layer(c)
        c.run_module("sgs", sgs.timeStep)
        c.run_module("micro", micro.timeStep)
    torch.cuda.synchronize()
    dm.validate_all()
    assert capsys.readouterr().err == ""
    assert micro.sgs_shoc == (sgs_name == "shoc") and micro.etime == 3 * crm_dt and not micro.first_step
    for n in start:
        assert bool((dm.get(n, readonly=True) != start[n]).any()), n
    assert bool((dm.get("t_prev", readonly=True) == dm.get("temp", readonly=True)).all())
    assert bool((dm.get("q_prev", readonly=True) == dm.get("water_vapor", readonly=True)).all())
    assert bool((dm.get("precip_liq_surf_out", readonly=True) != 0).all())
    if sgs_name == "none":                                              # the adjustment ran: the super-saturated supercell core condensed
        assert bool((dm.get("cloud_water", readonly=True) > 0).any())
    micro.finalize(c)
    sgs.finalize(c)
    dyc.finalize(c)
