"""The CRM column diagnostics on the GPU: the HIP kernels against the numpy restatement (tests/coldiag_ref.py) bit for bit on every shape
and named case under the automatic and under each forced mapping of the column mean, with the inputs and the guard elements around every
output unchanged, run to run, members split over calls against the whole ensemble, and a larger shape after a smaller one (the workspace
grows); the Python layer through a coupler with Kessler's and with P3's field set on MsaClock's weights, and its refusals; the C++ module
through tests/cxx/column_diag; the C++ driver's --column-diag on a shortened CI input (tests/golden/msa_input.yaml) against the Python
layer."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import coldiag_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
MSA_YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")
GUARD = 8                       # elements on either side of every output
SENTINEL = -1.2345678e300
AUTO, BLOCK_SLOTS, THREAD_SLOTS = 0, 1, 2


class GpuBackend:
    """the interface of coldiag_ref.RefBackend over the C ABI.  Every output lies between guard elements, checked after every call; an
    input goes to the device once per backend, and inputs_unchanged() checks that all of them still hold the bits they had"""

    def __init__(self, mapping=AUTO):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check, self.mapping = torch, capi.load(), capi.check, mapping
        self.inputs = {}

    def _dev(self, a):
        if a is None:
            return None
        if id(a) not in self.inputs:
            self.inputs[id(a)] = (a, self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"))
        return self.inputs[id(a)][1]

    def inputs_unchanged(self):
        self.torch.cuda.synchronize()
        return all(ref.same_bits(t.cpu().numpy(), np.ascontiguousarray(a)) for a, t in self.inputs.values())

    @staticmethod
    def _table(ts):
        return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])

    def diagnose(self, f, zint, precip, params, out, factor):
        torch = self.torch
        nz, ny, nx, nens = f["rho_v"].shape
        fields = [self._dev(f.get(n)) for n in ref.FIELDS]
        pr = None if precip is None else [self._dev(precip.get(n)) for n in ref.PRECIP]
        # the nine outputs in ONE buffer, each between its own guard elements
        row = nens + 2 * GUARD
        host = np.full((len(ref.OUT), row), SENTINEL)
        for q, x in enumerate(ref.OUT):
            if out[x] is not None:
                host[q, GUARD:GUARD + nens] = out[x]
        buf = torch.from_numpy(host).to("cuda:0")
        outs = [None if out[x] is None else buf[q, GUARD:GUARD + nens] for q, x in enumerate(ref.OUT)]
        self.check(self.lib.pam_amd_column_diagnostics_debug_mapping(self.mapping))
        try:
            self.check(self.lib.pam_amd_column_diagnostics(nens, nx, ny, nz, self._table(fields), self._dev(zint).data_ptr(),
                                                           None if pr is None else self._table(pr), params["R_d"], params["R_v"], params["p_low"],
                                                           params["p_high"], params["cwp_threshold"], self._table(outs), float(factor),
                                                           torch.cuda.current_stream().cuda_stream))
        finally:
            self.check(self.lib.pam_amd_column_diagnostics_debug_mapping(AUTO))
        got = buf.cpu().numpy()
        new = {}
        for q, x in enumerate(ref.OUT):
            if out[x] is None:
                assert (got[q] == SENTINEL).all(), "an absent output's place changed"
                new[x] = None
            else:
                assert (got[q, :GUARD] == SENTINEL).all() and (got[q, -GUARD:] == SENTINEL).all(), "a guard element changed"
                new[x] = got[q, GUARD:GUARD + nens].copy()
        return new


@pytest.mark.gpu
@pytest.mark.parametrize("config", ref.CONFIGS, ids=ref.config_id)
def test_gpu_matches_restatement_bit_for_bit(config):
    """every output of every named case, with the mean's mapping chosen by the number of columns and with each of the two forced; the base
    case twice: two runs are identical"""
    for mapping in (AUTO, BLOCK_SLOTS, THREAD_SLOTS):
        be = GpuBackend(mapping)
        for name in ref.CASE_NAMES:
            got = ref.run_case(be, ref.cases(config)[name])
            assert ref.results_differ(got, ref.reference(config, name)) == [], (name, mapping)
        again = ref.run_case(be, ref.cases(config)["base"])
        assert ref.results_differ(again, ref.reference(config, "base")) == [], mapping
        assert be.inputs_unchanged(), mapping


@pytest.mark.gpu
def test_gpu_every_number_of_occupied_slots():
    """lines of 2 .. 15 columns: the base case under both mean mappings"""
    for config in ref.SLOT_CONFIGS:
        for mapping in (BLOCK_SLOTS, THREAD_SLOTS):
            got = ref.run_case(GpuBackend(mapping), ref.cases(config)["base"])
            assert ref.results_differ(got, ref.reference(config, "base")) == [], (config, mapping)


@pytest.mark.gpu
@pytest.mark.parametrize("config", [c for c in ref.CONFIGS if c[3] == 65], ids=ref.config_id)
def test_gpu_member_chunks_equal_the_whole_ensemble(config):
    """members in chunks of 1, 63 and 1 as separate calls: the whole ensemble's bits, in every named case and both mean mappings"""
    cuts = (slice(0, 1), slice(1, 64), slice(64, 65))
    for mapping in (BLOCK_SLOTS, THREAD_SLOTS):
        for name in ref.CASE_NAMES:
            case = ref.cases(config)[name]
            got = ref.join([ref.run_case(GpuBackend(mapping), ref.members(case, sl)) for sl in cuts])
            assert ref.results_differ(got, ref.reference(config, name)) == [], (name, mapping)


@pytest.mark.gpu
def test_gpu_workspace_grows_with_the_shape():
    """from no workspace at all: the smallest shape, then the largest, then a shape between them on the workspace the largest left, then
    again from nothing after pam_amd_modules_finalize"""
    from pam_amd import capi
    lib = capi.load()
    capi.check(lib.pam_amd_modules_finalize())
    be = GpuBackend()
    for config in ((1, 1, 1, 1), (4, 8, 8, 65), (5, 3, 7, 3), (7, 1, 16, 65)):
        got = ref.run_case(be, ref.cases(config)["base"])
        assert ref.results_differ(got, ref.reference(config, "base")) == [], config
    capi.check(lib.pam_amd_modules_finalize())
    got = ref.run_case(be, ref.cases((4, 8, 8, 65))["two_steps"])
    assert ref.results_differ(got, ref.reference((4, 8, 8, 65), "two_steps")) == []
    assert be.inputs_unchanged()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer

TRACERS = {"kessler": ("water_vapor", "cloud_liquid", "precip_liquid"), "p3": ("water_vapor", "cloud_water", "ice"), "none": ("water_vapor",)}
NAMES = {"kessler": dict(rho_c="cloud_liquid"), "p3": dict(rho_c="cloud_water", rho_i="ice"), "none": {}}
PRECIP_NAMES = {"kessler": dict(precip_liq="precl"), "p3": dict(precip_liq="precip_liq_surf_out", precip_ice="precip_ice_surf_out"), "none": {}}
CRM_DT, GCM_DT = 20.0, 240.0


def _coupler(config, micro, zint, cldfrac=False):
    import torch
    from pam_amd import PamCoupler
    nz, ny, nx, nens = config
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", CRM_DT)
    c.set_option("gcm_physics_dt", GCM_DT)
    c.set_option("R_d", ref.PARAMS["R_d"])                  # what a microphysics sets
    c.set_option("R_v", ref.PARAMS["R_v"])
    c.allocate_coupler_state(nz, ny, nx, nens)
    for t in TRACERS[micro]:
        c.add_tracer(t, "", True, True)
    c.set_option("micro", micro)
    dm = c.get_data_manager_device_readwrite()
    for n in PRECIP_NAMES[micro].values():
        dm.register_and_allocate(n, "surface precipitation rate", (ny, nx, nens), ("y", "x", "nens"))
    if cldfrac:
        dm.register_and_allocate("cldfrac", "cloud fraction", (nz, ny, nx, nens), ("z", "y", "x", "nens"))
    dm.get("vertical_interface_height").copy_(torch.from_numpy(zint))
    return c


def _load(c, f, precip, micro):
    import torch
    dm = c.get_data_manager_device_readwrite()
    names = dict(temp="temp", rho_d="density_dry", rho_v="water_vapor", **NAMES[micro])
    if dm.entry_exists("cldfrac"):
        names["cldfrac"] = "cldfrac"
    for ours, theirs in names.items():
        dm.get(theirs).copy_(torch.from_numpy(f[ours]))
    for ours, theirs in PRECIP_NAMES[micro].items():
        dm.get(theirs).copy_(torch.from_numpy(precip[ours]))


def _as_seen_by(micro, f, precip, cldfrac):
    """the fields and the precipitation as this microphysics has them: what it lacks is absent"""
    g = {n: (f[n] if n in ("temp", "rho_d", "rho_v") or n in NAMES[micro] or (n == "cldfrac" and cldfrac) else None) for n in ref.FIELDS}
    return g, {n: (precip[n] if n in PRECIP_NAMES[micro] else None) for n in ref.PRECIP}


@pytest.mark.gpu
@pytest.mark.parametrize("micro, cldfrac", [("p3", False), ("kessler", False), ("none", False), ("p3", True)])
def test_gpu_python_layer_on_the_clock(micro, cldfrac):
    """column_diagnostics_init, then three CRM steps whose states are the two_steps case's two and the base again and whose weights are
    MsaClock's (3 while it accelerates, 1 after the cease): the restatement's bits in the coupler's entries, and exactly the entries this
    field set has"""
    import torch
    from pam_amd import modules
    from pam_amd.modules import MsaClock
    config = (4, 8, 8, 65)
    cs = ref.cases(config)
    steps = [(f, p) for f, p, _ in cs["two_steps"]["steps"]] + [cs["base"]["steps"][0][:2]]
    frac = cs["cldfrac"]["steps"][0][0]["cldfrac"]
    steps = [_as_seen_by(micro, dict(f, cldfrac=frac), p, cldfrac) for f, p in steps]
    c = _coupler(config, micro, cs["base"]["zint"], cldfrac)
    modules.column_diagnostics_init(c)
    dm = c.get_data_manager_device_readwrite()
    f0, p0 = steps[0]
    there = {"cldtot": micro != "none", "cldlow": micro != "none", "cldmed": micro != "none", "cldhgh": micro != "none",
             "lwp": f0["rho_c"] is not None, "iwp": f0["rho_i"] is not None, "pw": True, "precip_liq": p0["precip_liq"] is not None,
             "precip_ice": p0["precip_ice"] is not None}
    for x in ref.OUT:
        assert dm.entry_exists("diag_" + x) == there[x], x
        if there[x]:
            assert dm.get_shape("diag_" + x) == [65]
            dm.get("diag_" + x).fill_(7.0)
    assert [c.get_option(o) for o in ("crm_diag_p_low", "crm_diag_p_high", "crm_diag_cwp_threshold")] == [70000.0, 40000.0, 1.0e-3]
    modules.column_diagnostics_init(c)                              # the start of a GCM step: zeroes what is there
    clock, weights = MsaClock(12, 2), []
    for step, (f, p) in enumerate(steps):
        _load(c, f, p, micro)
        weights.append(clock.advance(step == 1))                    # the second step's acceleration ceases
        modules.column_diagnostics(c, weights[-1])
    assert weights == [3, 1, 1]
    torch.cuda.synchronize()
    zeros = {x: (np.zeros(65) if there[x] else None) for x in ref.OUT}
    want = ref.run_case(ref.RefBackend(), dict(zint=cs["base"]["zint"], params=ref.PARAMS, out0=zeros,
                                               steps=[(f, p, CRM_DT / GCM_DT * float(w)) for (f, p), w in zip(steps, weights)]))
    for x in ref.OUT:
        if there[x]:
            assert ref.same_bits(dm.get("diag_" + x, readonly=True).cpu().numpy(), want[x]), x
    assert (want["pw"] > 0).all() and (micro == "none" or (want["cldtot"] > 0).all())


@pytest.mark.gpu
def test_gpu_python_layer_refuses_every_misuse_before_a_launch():
    import torch
    from pam_amd import modules
    from pam_amd.capi import PamAmdError
    config = (2, 4, 4, 3)
    cs = ref.cases((2, 1, 5, 3))
    c = _coupler(config, "p3", np.ascontiguousarray(cs["base"]["zint"]))
    with pytest.raises(PamAmdError, match="init first"):            # no init
        modules.column_diagnostics(c)
    modules.column_diagnostics_init(c)
    modules.column_diagnostics(c)
    dm = c.get_data_manager_device_readwrite()
    torch.cuda.synchronize()
    before = {n: dm.get(n, readonly=True).clone() for n in modules.COLUMN_DIAGNOSTICS}
    for weight in (float("nan"), float("inf")):
        with pytest.raises(PamAmdError, match="not finite"):
            modules.column_diagnostics(c, weight)
    for opt, bad, match in (("crm_diag_p_high", 80000.0, "must not exceed"), ("crm_diag_p_low", float("nan"), "finite"),
                            ("crm_diag_cwp_threshold", -1.0, ">= 0"), ("crm_diag_cwp_threshold", float("nan"), ">= 0"),
                            ("R_d", float("inf"), "finite"), ("gcm_physics_dt", 0.0, "gcm_physics_dt"), ("gcm_physics_dt", -1.0, "gcm_physics_dt")):
        good = c.get_option(opt)
        c.set_option(opt, bad)
        with pytest.raises(PamAmdError, match=match):
            modules.column_diagnostics(c)
        c.set_option(opt, good)
    c.set_option("micro", "morrison")
    for fn in (modules.column_diagnostics_init, modules.column_diagnostics):
        with pytest.raises(PamAmdError, match="kessler, p3 and none"):
            fn(c)
    c.set_option("micro", "kessler")                                # another field set than the init saw: cloud_liquid does not exist here
    with pytest.raises(PamAmdError):
        modules.column_diagnostics(c)
    c.set_option("micro", "p3")
    dm.register_and_allocate("cldfrac", "", (2, 4, 4))
    with pytest.raises(PamAmdError, match="cldfrac"):
        modules.column_diagnostics(c)
    c2 = _coupler(config, "none", np.ascontiguousarray(cs["base"]["zint"]))
    c2.get_data_manager_device_readwrite().register_and_allocate("precl", "", (4, 4))
    for fn in (modules.column_diagnostics_init, modules.column_diagnostics):
        with pytest.raises(PamAmdError, match="precl"):
            fn(c2)
    c3 = _coupler(config, "none", np.ascontiguousarray(cs["base"]["zint"]))
    c3.get_data_manager_device_readwrite().register_and_allocate("diag_pw", "", (3, 2))
    with pytest.raises(PamAmdError, match="shape|not \\(nens"):
        modules.column_diagnostics_init(c3)
    torch.cuda.synchronize()
    for n, t in before.items():
        assert torch.equal(dm.get(n, readonly=True), t), n


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ module through tests/cxx/column_diag

@pytest.mark.gpu
@pytest.mark.parametrize("micro", ["none", "kessler", "p3"])
def test_gpu_cxx_module_is_the_restatement(tmp_path, micro):
    from test_coldiag import cxx_program
    config = (5, 3, 7, 3)
    cs = ref.cases(config)
    steps = [_as_seen_by(micro, f, p, False) for f, p, _ in cs["two_steps"]["steps"]]
    weights = (3.0, 1.0)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(struct.pack("6i", *config, ("none", "kessler", "p3").index(micro), len(steps)))
        cs["base"]["zint"].tofile(fh)
        for (f, p), w in zip(steps, weights):
            np.array([w]).tofile(fh)
            for a in [f[n] for n in ("temp", "rho_d", "rho_v", "rho_c", "rho_i")] + [p[n] for n in ref.PRECIP]:
                if a is not None:
                    np.ascontiguousarray(a).tofile(fh)
    r = subprocess.run([cxx_program(), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "### failed" not in r.stdout, (r.stdout[-1000:], r.stderr[-1000:])
    f0, p0 = steps[0]
    there = [x for x in ref.OUT if not ((x in ref.COVERS and micro == "none") or (x == "lwp" and f0["rho_c"] is None) or
                                        (x == "iwp" and f0["rho_i"] is None) or (x in ref.PRECIP and p0[x] is None))]
    lines = r.stdout.strip().split("\n")
    assert lines[0].split() == ["###", "entries"] + ["diag_" + x for x in there] and lines[1] == "### options 70000 40000 0.001"
    zeros = {x: (np.zeros(3) if x in there else None) for x in ref.OUT}
    want = ref.run_case(ref.RefBackend(), dict(zint=cs["base"]["zint"], params=ref.PARAMS, out0=zeros,
                                               steps=[(f, p, CRM_DT / GCM_DT * w) for (f, p), w in zip(steps, weights)]))
    got = np.fromfile(dst).reshape(len(there), 3)
    for row, x in zip(got, there):
        assert ref.same_bits(row, want[x]), x


# ------------------------------------------------------------------------------------------------------------------------------
# end to end through the C++ driver

def _run_driver(*args):
    r = subprocess.run([DRIVER, "--yaml", MSA_YAML, "--nens", "3"] + list(args), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().split("\n")


def _state(path, nz=50, ny=1, nx=65, nens=3):
    raw = np.fromfile(path, dtype=np.float64)
    names = ("density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor", "cloud_liquid", "precip_liquid")
    n = nz * ny * nx * nens
    assert raw.size == len(names) * n + ny * nx * nens
    st = {name: raw[i * n:(i + 1) * n].reshape(nz, ny, nx, nens) for i, name in enumerate(names)}
    st["precl"] = raw[len(names) * n:].reshape(ny, nx, nens)
    return st


def _python_diagnostics(states, weights):
    """the Python layer on the states the driver wrote: a Kessler coupler on the driver's grid"""
    import torch
    from pam_amd import Microphysics, PamCoupler, modules
    nz, ny, nx, nens = states[0]["temp"].shape
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", 20.0)
    c.set_option("gcm_physics_dt", 240.0)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(128000.0, 64000.0, np.linspace(0.0, 20000.0, nz + 1))
    Microphysics().init(c)
    dm = c.get_data_manager_device_readwrite()
    modules.column_diagnostics_init(c)
    for st, w in zip(states, weights):
        for n, a in st.items():
            dm.get(n).copy_(torch.from_numpy(a))
        modules.column_diagnostics(c, w)
    torch.cuda.synchronize()
    return {n: dm.get(n, readonly=True).cpu().numpy() for n in modules.COLUMN_DIAGNOSTICS if dm.entry_exists(n)}


@pytest.mark.gpu
@pytest.mark.parametrize("extra, weight", [((), 1), (("--accelerate", "2", "--accel-uv", "--hyperdiff", "600"), 3)], ids=["plain", "accelerated"])
def test_gpu_driver_column_diag_is_the_python_layer(tmp_path, extra, weight):
    """--column-diag on two CRM steps: the state after step 1 is the output of a run of one step, the state after step 2 the run's own
    output; the Python layer, fed these two states with the clock's weights, gives the bits the driver wrote.  Kessler has no ice: no
    diag_iwp, no diag_precip_ice.  The run's fields are those of a run without the flag"""
    outs, files = [], []
    for steps in (1, 2):
        out, js = tmp_path / ("out%d.bin" % steps), tmp_path / ("coldiag%d.json" % steps)
        lines = _run_driver("--steps", str(steps), "--column-diag", str(js), *extra, str(out))
        assert json.loads(lines[-1])["crm_steps"] == steps
        outs.append(out)
        files.append([json.loads(line) for line in js.read_text().strip().split("\n")])
    plain = tmp_path / "plain.bin"
    _run_driver("--steps", "2", *extra, str(plain))
    assert plain.read_bytes() == outs[1].read_bytes()
    assert len(files[1]) == 1                                       # one record per GCM step
    got = files[1][0]
    assert (got["gcm_step"], got["crm_steps"], got["nens"]) == (0, 2, 3)
    assert sorted(got["diagnostics"]) == sorted(["diag_cldtot", "diag_cldlow", "diag_cldmed", "diag_cldhgh", "diag_lwp", "diag_pw", "diag_precip_liq"])
    want = _python_diagnostics([_state(o) for o in outs], [weight, weight])
    assert sorted(want) == sorted(got["diagnostics"])
    for n, a in want.items():
        assert a.shape == (3,) and ref.same_bits(np.array(got["diagnostics"][n], dtype=np.float64), a), n
    assert np.isfinite(want["diag_pw"]).all() and (want["diag_pw"] > 0).all()


@pytest.mark.gpu
def test_gpu_driver_composes_the_flag_and_prints_it_in_its_usage(tmp_path):
    """with --gcm-handoff and --radiation beside it the records are those of the flag alone; the usage text lists the flag"""
    rad = tmp_path / "rad.bin"
    np.zeros((50, 1, 5, 3)).tofile(rad)
    alone, both = tmp_path / "alone.json", tmp_path / "both.json"
    _run_driver("--steps", "2", "--column-diag", str(alone), "-")
    _run_driver("--steps", "2", "--radiation", "5", "1", str(rad), "--gcm-handoff", "5", "1", str(tmp_path / "h.json"), "--column-diag", str(both), "-")
    assert alone.read_text() == both.read_text() and alone.read_text().count("\n") == 1
    r = subprocess.run([DRIVER, "--yaml", MSA_YAML, "--column-diag", "-"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--column-diag PATH]" in r.stderr
