"""The CRM-to-GCM handoff on the GPU: the HIP kernels against the numpy restatement (tests/rad_ref.py) bit for bit on every shape, rad
grid and named case under both mappings of slots to threads, with the inputs and the guard elements around every output unchanged, run to
run, and members split over calls against the whole ensemble; the Python layer through a coupler on MsaClock's weights and its refusals;
the C++ driver's --gcm-handoff on a shortened CI input (tests/golden/msa_input.yaml) against the Python layer."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import rad_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
MSA_YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")
GUARD = 8                       # elements on either side of every output
SENTINEL = -1.2345678e300
AUTO, BLOCK_SLOTS, THREAD_SLOTS = 0, 1, 2


class GpuBackend:
    """the interface of rad_ref.RefBackend over the C ABI.  Every output lies between guard elements, and every call checks that they and
    the inputs come back with the bits they had"""

    def __init__(self, mapping=AUTO):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check, self.mapping = torch, capi.load(), capi.check, mapping

    def _dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def _guarded(self, a):
        """-> (the whole buffer, the view the kernel gets)"""
        buf = self.torch.full((a.size + 2 * GUARD,), SENTINEL, dtype=self.torch.float64, device="cuda:0")
        view = buf[GUARD:GUARD + a.size].view(a.shape)
        view.copy_(self.torch.from_numpy(np.ascontiguousarray(a)))
        return buf, view

    @staticmethod
    def _table(ts):
        return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])

    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def _finish(self, ins, host_ins, outs):
        self.torch.cuda.synchronize()
        for t, h in zip(ins, host_ins):
            assert t is None or ref.same_bits(t.cpu().numpy(), np.ascontiguousarray(h)), "an input changed"
        res = []
        for pair in outs:
            if pair is None:
                res.append(None)
                continue
            buf, view = pair
            b = buf.cpu().numpy()
            assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all(), "a guard element changed"
            res.append(view.cpu().numpy())
        return res

    def aggregate(self, f, rad_grid, rad, factor):
        nz, ny, nx, nens = f["temp"].shape
        host = [f.get(n) for n in ref.FIELDS]
        fields = [self._dev(a) for a in host]
        outs = [None if rad[x] is None else self._guarded(rad[x]) for x in ref.RAD]
        self.check(self.lib.pam_amd_radiation_aggregate_debug_mapping(self.mapping))
        try:
            self.check(self.lib.pam_amd_radiation_aggregate(nens, nx, ny, nz, rad_grid[1], rad_grid[0], self._table(fields),
                                                            self._table([None if o is None else o[1] for o in outs]), float(factor), self._stream()))
        finally:
            self.check(self.lib.pam_amd_radiation_aggregate_debug_mapping(AUTO))
        return dict(zip(ref.RAD, self._finish(fields, host, outs)))

    def feedback(self, f, gcm, gcm_dt):
        nz, ny, nx, nens = f["temp"].shape
        absent = {x for x, n in ref.SPECIES.items() if f.get(n) is None}
        gone = {"gcm_cloud_water": "qc", "gcm_cloud_ice": "qi"}
        host = [f.get(n) for n in ref.FB_FIELDS] + [None if gone.get(n) in absent else gcm[n] for n in ref.GCM]
        ins = [self._dev(a) for a in host]
        nan = np.full((nz, nens), np.nan)
        mean = [None if q in absent else self._guarded(nan) for q in ref.QUANTITIES]
        tend = [None if q in absent else self._guarded(nan) for q in ref.QUANTITIES]
        self.check(self.lib.pam_amd_crm_feedback(nens, nx, ny, nz, self._table(ins[:7]), self._table(ins[7:]), float(gcm_dt),
                                                 self._table([None if o is None else o[1] for o in mean]),
                                                 self._table([None if o is None else o[1] for o in tend]), self._stream()))
        res = self._finish(ins, host, mean + tend)
        return dict(zip(ref.QUANTITIES, res[:6])), dict(zip(ref.QUANTITIES, res[6:]))


@pytest.mark.gpu
@pytest.mark.parametrize("config", ref.CONFIGS, ids=ref.config_id)
def test_gpu_matches_restatement_bit_for_bit(config):
    """every aggregate, mean and tendency of every named case, with the mapping chosen by the group's size and with each of the two
    forced; the base case twice: two runs are identical"""
    for mapping in (AUTO, BLOCK_SLOTS, THREAD_SLOTS):
        be = GpuBackend(mapping)
        for name in ref.CASE_NAMES:
            got = ref.run_case(be, ref.cases(config)[name])
            assert ref.results_differ(got, ref.reference(config, name)) == [], (name, mapping)
        again = ref.run_case(be, ref.cases(config)["base"])
        assert ref.results_differ(again, ref.reference(config, "base")) == [], mapping


def _members(d, sl):
    return {k: (None if v is None else np.ascontiguousarray(v[..., sl])) for k, v in d.items()}


def _join(parts):
    return {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts], axis=-1)) for k in parts[0]}


@pytest.mark.gpu
@pytest.mark.parametrize("config", [c for c in ref.CONFIGS if c[0][3] >= 65], ids=ref.config_id)
def test_gpu_member_chunks_equal_the_whole_ensemble(config):
    """members in chunks of 1, 64 and the remainder as separate calls: the whole ensemble's bits, in every named case and both mappings"""
    nens = config[0][3]
    cuts = [sl for sl in (slice(0, 1), slice(1, 65), slice(65, nens)) if sl.start < nens]
    for mapping in (BLOCK_SLOTS, THREAD_SLOTS):
        be = GpuBackend(mapping)
        for name in ref.CASE_NAMES:
            case = ref.cases(config)[name]
            parts = []
            for sl in cuts:
                sub = dict(case, rad0=_members(case["rad0"], sl), gcm=_members(case["gcm"], sl),
                           steps=[(_members(f, sl), factor) for f, factor in case["steps"]])
                parts.append(ref.run_case(be, sub))
            got = {g: _join([p[g] for p in parts]) for g in ("rad", "mean", "tend")}
            assert ref.results_differ(got, ref.reference(config, name)) == [], (name, mapping)


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer

TRACERS = {"kessler": ("water_vapor", "cloud_liquid", "precip_liquid"), "p3": ("water_vapor", "cloud_water", "ice"), "none": ("water_vapor",)}
NAMES = {"kessler": dict(rho_c="cloud_liquid"), "p3": dict(rho_c="cloud_water", rho_i="ice"), "none": {}}


def _coupler(config, micro, cldfrac=False):
    from pam_amd import PamCoupler
    (nz, ny, nx, nens), (rad_ny, rad_nx) = config
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", ref.CRM_DT)
    c.set_option("gcm_physics_dt", ref.GCM_DT)
    c.allocate_coupler_state(nz, ny, nx, nens)
    for t in TRACERS[micro]:
        c.add_tracer(t, "", True, True)
    c.set_option("micro", micro)
    c.set_option("rad_nx", rad_nx)
    c.set_option("rad_ny", rad_ny)
    if cldfrac:
        c.get_data_manager_device_readwrite().register_and_allocate("cldfrac", "cloud fraction", (nz, ny, nx, nens), ("z", "y", "x", "nens"))
    return c


def _load(c, f, micro, gcm=None):
    import torch
    dm = c.get_data_manager_device_readwrite()
    names = dict(temp="temp", rho_d="density_dry", rho_v="water_vapor", uvel="uvel", vvel="vvel", **NAMES[micro])
    if dm.entry_exists("cldfrac"):
        names["cldfrac"] = "cldfrac"
    for ours, theirs in names.items():
        dm.get(theirs).copy_(torch.from_numpy(f[ours]))
    for n, a in (gcm or {}).items():
        dm.get(n).copy_(torch.from_numpy(a))


def _without(case, micro, cldfrac):
    """the case as this microphysics sees it: the species it lacks are absent"""
    def strip(f):
        g = dict(f)
        for n in ("rho_c", "rho_i"):
            if n not in NAMES[micro]:
                g[n] = None
        if not cldfrac:
            g["cldfrac"] = None
        return g
    rad0 = dict(case["rad0"], qc=case["rad0"]["qc"] if "rho_c" in NAMES[micro] else None, qi=case["rad0"]["qi"] if "rho_i" in NAMES[micro] else None)
    return dict(case, steps=[(strip(f), fac) for f, fac in case["steps"]], rad0=rad0)


@pytest.mark.gpu
@pytest.mark.parametrize("micro, cldfrac", [("p3", False), ("kessler", False), ("none", False), ("p3", True)])
def test_gpu_python_layer_three_steps_on_the_clock(micro, cldfrac):
    """rad_aggregate_init, then three CRM steps whose states are the three_steps case's and whose weights are MsaClock's (3 while it
    accelerates, 1 after the cease), then compute_crm_feedback: the restatement's bits in the coupler's entries, and exactly the entries
    this microphysics has"""
    import torch
    from pam_amd import modules
    from pam_amd.modules import MsaClock
    config = ((3, 8, 8, 70), (2, 4))
    case = ref.cases(config)["cldfrac" if cldfrac else "three_steps"]
    states = [f for f, _ in ref.cases(config)["three_steps"]["steps"]]
    if cldfrac:
        states = [dict(f, cldfrac=case["steps"][0][0]["cldfrac"]) for f in states]
    c = _coupler(config, micro, cldfrac)
    modules.rad_aggregate_init(c)
    modules.crm_feedback_init(c)
    dm = c.get_data_manager_device_readwrite()
    have = [x for x in ref.RAD if dm.entry_exists("rad_" + x)]
    assert have == [x for x in ref.RAD if not (x == "qc" and "rho_c" not in NAMES[micro]) and not (x == "qi" and "rho_i" not in NAMES[micro])]
    for x in have:
        assert dm.get_shape("rad_" + x) == [3, 2, 4, 70]
        dm.get("rad_" + x).fill_(7.0)
    modules.rad_aggregate_init(c)                                   # the start of a GCM step: zeroes what is there
    clock, weights = MsaClock(12, 2), []
    for step, f in enumerate(states):
        _load(c, f, micro, case["gcm"])
        weights.append(clock.advance(step == 1))                    # the second step's acceleration ceases
        modules.rad_aggregate(c, weights[-1])
    assert weights == [3, 1, 1]
    modules.compute_crm_feedback(c)
    torch.cuda.synchronize()
    zeros = {x: (np.zeros((3, 2, 4, 70)) if x in have else None) for x in ref.RAD}
    want_case = _without(dict(case, rad0=zeros, steps=[(f, ref.CRM_DT / ref.GCM_DT * float(w)) for f, w in zip(states, weights)]), micro, cldfrac)
    want = ref.run_case(ref.RefBackend(), want_case)
    for x in ref.RAD:
        assert dm.entry_exists("rad_" + x) == (want["rad"][x] is not None), x
        if want["rad"][x] is not None:
            assert ref.same_bits(dm.get("rad_" + x, readonly=True).cpu().numpy(), want["rad"][x]), x
    for q in ref.QUANTITIES:
        for what in ("mean", "tend"):
            n = "crm_feedback_%s_%s" % (what, q)
            assert dm.entry_exists(n) == (want[what][q] is not None), n
            if want[what][q] is not None:
                assert dm.get_shape(n) == [3, 70] and ref.same_bits(dm.get(n, readonly=True).cpu().numpy(), want[what][q]), n


@pytest.mark.gpu
def test_gpu_python_layer_refuses_every_misuse_before_a_launch():
    from pam_amd import modules
    from pam_amd.capi import PamAmdError
    config = ((2, 4, 4, 3), (2, 2))
    c = _coupler(config, "p3")
    for fn in (modules.rad_aggregate, modules.compute_crm_feedback):              # no init
        with pytest.raises(PamAmdError, match="init first"):
            fn(c)
    for opt, bad in (("rad_nx", 3), ("rad_ny", 0), ("rad_nx", 8)):                # bad options
        good = c.get_option(opt)
        c.set_option(opt, bad)
        for fn in (modules.rad_aggregate_init, modules.rad_aggregate):
            with pytest.raises(PamAmdError, match="rad_nx"):
                fn(c)
        c.set_option(opt, good)
    modules.rad_aggregate_init(c)
    modules.crm_feedback_init(c)
    dm = c.get_data_manager_device_readwrite()
    before = {n: dm.get(n, readonly=True).clone() for n in ("rad_temperature", "crm_feedback_tend_t")}
    c.set_option("rad_nx", 4)                                                     # the aggregates have another shape now
    for fn in (modules.rad_aggregate_init, modules.rad_aggregate):
        with pytest.raises(PamAmdError, match="shape|not \\(nz"):
            fn(c)
    c.set_option("rad_nx", 2)
    for weight in (float("nan"), float("inf")):
        with pytest.raises(PamAmdError, match="not finite"):
            modules.rad_aggregate(c, weight)
    for dt in (0.0, -1.0, float("inf")):
        c.set_option("gcm_physics_dt", dt)
        with pytest.raises(PamAmdError, match="gcm_physics_dt"):
            modules.compute_crm_feedback(c)
        if not dt > 0:
            with pytest.raises(PamAmdError, match="gcm_physics_dt"):
                modules.rad_aggregate(c)
    c.set_option("gcm_physics_dt", ref.GCM_DT)
    c.set_option("micro", "morrison")
    for fn in (modules.rad_aggregate, modules.compute_crm_feedback):
        with pytest.raises(PamAmdError, match="kessler, p3 and none"):
            fn(c)
    c.set_option("micro", "p3")
    dm.register_and_allocate("cldfrac", "", (2, 4, 4))
    with pytest.raises(PamAmdError, match="cldfrac"):
        modules.rad_aggregate(c)
    import torch
    torch.cuda.synchronize()
    for n, t in before.items():
        assert torch.equal(dm.get(n, readonly=True), t), n


# ------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ driver

def _run_driver(*args):
    r = subprocess.run([DRIVER, "--yaml", MSA_YAML, "--nens", "3"] + list(args), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().split("\n")


def _python_handoff(states, weights, rad_nx, rad_ny):
    """the Python layer on the states the driver wrote: a Kessler coupler whose gcm_* columns are the driver's (the supercell column)"""
    import torch
    from pam_amd import Microphysics, PamCoupler, modules
    nz, ny, nx, nens = states[0]["temp"].shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", 20.0)
    c.set_option("gcm_physics_dt", 240.0)
    c.allocate_coupler_state(nz, ny, nx, nens)
    zint = np.linspace(0.0, 20000.0, nz + 1)
    c.set_grid(128000.0, 64000.0, zint)
    Microphysics().init(c)
    dm = c.get_data_manager_device_readwrite()
    cols = modules.supercell_init(torch.from_numpy(zint).to("cuda:0"), c.get_option("R_d"), c.get_option("R_v"), c.get_option("grav"))
    for name, col in zip(("gcm_density_dry", "gcm_uvel", "gcm_vvel", "gcm_wvel", "gcm_temp", "gcm_water_vapor"), cols):
        dm.get(name).copy_(col[:, None].expand(nz, nens))
    c.set_option("rad_nx", rad_nx)
    c.set_option("rad_ny", rad_ny)
    modules.rad_aggregate_init(c)
    modules.crm_feedback_init(c)
    for st, w in zip(states, weights):
        for n, a in st.items():
            dm.get(n).copy_(torch.from_numpy(a))
        modules.rad_aggregate(c, w)
    modules.compute_crm_feedback(c)
    torch.cuda.synchronize()
    agg = {n: dm.get(n, readonly=True).cpu().numpy() for n in modules.RAD_AGGREGATES if dm.entry_exists(n)}
    fb = {"%s_%s" % (what, q): dm.get("crm_feedback_%s_%s" % (what, q), readonly=True).cpu().numpy()
          for what in ("mean", "tend") for q in modules.CRM_FEEDBACK_QUANTITIES if dm.entry_exists("crm_feedback_%s_%s" % (what, q))}
    return agg, fb


def _state(path, nz=50, ny=1, nx=65, nens=3):
    raw = np.fromfile(path, dtype=np.float64)
    names = ("density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor", "cloud_liquid", "precip_liquid")
    n = nz * ny * nx * nens
    assert raw.size == len(names) * n + ny * nx * nens
    return {name: raw[i * n:(i + 1) * n].reshape(nz, ny, nx, nens) for i, name in enumerate(names)}


@pytest.mark.gpu
@pytest.mark.parametrize("extra, weight", [((), 1), (("--accelerate", "2", "--accel-uv", "--hyperdiff", "600"), 3)], ids=["plain", "accelerated"])
def test_gpu_driver_handoff_is_the_python_layer(tmp_path, extra, weight):
    """--gcm-handoff 5 1 on two CRM steps: the state after step 1 is the output of a run of one step, the state after step 2 the run's
    own output; the Python layer, fed these two states with the clock's weights, gives the bits the driver wrote.  Kessler has no ice:
    no rad_qi, no mean_qi.  The run's fields are those of a run without the flag"""
    outs, files = [], []
    for steps in (1, 2):
        out, js = tmp_path / ("out%d.bin" % steps), tmp_path / ("handoff%d.json" % steps)
        lines = _run_driver("--steps", str(steps), "--gcm-handoff", "5", "1", str(js), *extra, str(out))
        assert json.loads(lines[-1])["crm_steps"] == steps
        outs.append(out)
        files.append(json.loads(js.read_text()))
    plain = tmp_path / "plain.bin"
    _run_driver("--steps", "2", *extra, str(plain))
    assert plain.read_bytes() == outs[1].read_bytes()
    got = files[1]
    assert (got["nens"], got["nz"], got["rad_nx"], got["rad_ny"], got["crm_dt"], got["gcm_physics_dt"]) == (3, 50, 5, 1, 20.0, 240.0)
    assert len(got["gcm_steps"]) == 1 and got["gcm_steps"][0]["crm_steps"] == 2
    step = got["gcm_steps"][0]
    assert sorted(step["aggregates"]) == ["rad_cld", "rad_qc", "rad_qv", "rad_temperature"]
    assert sorted(step["feedback"]) == sorted("%s_%s" % (w, q) for w in ("mean", "tend") for q in ("t", "qv", "qc", "u", "v"))
    agg, fb = _python_handoff([_state(o) for o in outs], [weight, weight], 5, 1)
    for n, a in agg.items():
        assert a.shape == (50, 1, 5, 3) and ref.same_bits(np.array(step["aggregates"][n], dtype=np.float64), a), n
    for n, a in fb.items():
        assert a.shape == (50, 3) and ref.same_bits(np.array(step["feedback"][n], dtype=np.float64), a), n
    assert np.isfinite(agg["rad_temperature"]).all() and (agg["rad_temperature"] > 0).all()


@pytest.mark.gpu
def test_gpu_driver_refuses_two_rad_grids_and_prints_the_flag_in_its_usage(tmp_path):
    rad = tmp_path / "rad.bin"
    np.zeros((50, 1, 13, 3)).tofile(rad)
    r = subprocess.run([DRIVER, "--yaml", MSA_YAML, "--nens", "3", "--steps", "1", "--radiation", "13", "1", str(rad), "--gcm-handoff", "5", "1",
                        str(tmp_path / "h.json"), "-"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "same rad grid" in r.stderr
    r = subprocess.run([DRIVER, "--yaml", MSA_YAML, "--gcm-handoff", "5", "-"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--gcm-handoff RAD_NX RAD_NY PATH]" in r.stderr
