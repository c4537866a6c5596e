"""The CRM flux profiles on the GPU: the HIP kernel against the numpy restatement (tests/fluxprof_ref.py) bit for bit on every shape and
named case, with the inputs and the guard elements around every output unchanged, run to run, and members split over calls against the
whole ensemble; the Python layer through a coupler with Kessler's and with P3's field set on MsaClock's weights, and its refusals; the C++
module through tests/cxx/flux_profiles; the C++ driver's --flux-profiles on a shortened CI input (tests/golden/msa_input.yaml) against the
Python layer."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import fluxprof_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
MSA_YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")
GUARD = 8                       # elements on either side of every output
SENTINEL = -1.2345678e300


class GpuBackend:
    """the interface of fluxprof_ref.RefBackend over the C ABI.  Every output lies between guard elements, checked after every call; an
    input goes to the device once per backend, and inputs_unchanged() checks that all of them still hold the bits they had"""

    def __init__(self):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check = torch, capi.load(), capi.check
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

    def profiles(self, f, qc, out, factor):
        torch = self.torch
        nz, ny, nx, nens = f["rho_d"].shape
        fields = [self._dev(f.get(n)) for n in ref.FIELDS]
        # the ten outputs in ONE buffer, each between its own guard elements
        n = nz * nens
        row = n + 2 * GUARD
        host = np.full((len(ref.OUT), row), SENTINEL)
        for q, x in enumerate(ref.OUT):
            if out[x] is not None:
                host[q, GUARD:GUARD + n] = out[x].reshape(-1)
        buf = torch.from_numpy(host).to("cuda:0")
        outs = [None if out[x] is None else buf[q, GUARD:GUARD + n] for q, x in enumerate(ref.OUT)]
        self.check(self.lib.pam_amd_flux_profiles(nens, nx, ny, nz, self._table(fields), float(qc), self._table(outs), float(factor),
                                                  torch.cuda.current_stream().cuda_stream))
        got = buf.cpu().numpy()
        new = {}
        for q, x in enumerate(ref.OUT):
            if out[x] is None:
                assert (got[q] == SENTINEL).all(), "an absent output's place changed"
                new[x] = None
            else:
                assert (got[q, :GUARD] == SENTINEL).all() and (got[q, -GUARD:] == SENTINEL).all(), "a guard element changed"
                new[x] = got[q, GUARD:GUARD + n].reshape(nz, nens).copy()
        return new


@pytest.mark.gpu
@pytest.mark.parametrize("config", ref.CONFIGS, ids=ref.config_id)
def test_gpu_matches_restatement_bit_for_bit(config):
    """every output of every named case; the base case twice: two runs are identical"""
    be = GpuBackend()
    for name in ref.CASE_NAMES:
        got = ref.run_case(be, ref.cases(config)[name])
        assert ref.results_differ(got, ref.reference(config, name)) == [], name
    again = ref.run_case(be, ref.cases(config)["base"])
    assert ref.results_differ(again, ref.reference(config, "base")) == []
    assert be.inputs_unchanged()


@pytest.mark.gpu
@pytest.mark.parametrize("config", [c for c in ref.CONFIGS if c[3] == 65], ids=ref.config_id)
def test_gpu_member_chunks_equal_the_whole_ensemble(config):
    """members in chunks of 1, 63 and 1 as separate calls: the whole ensemble's bits, in every named case"""
    cuts = (slice(0, 1), slice(1, 64), slice(64, 65))
    for name in ref.CASE_NAMES:
        case = ref.cases(config)[name]
        got = ref.join([ref.run_case(GpuBackend(), ref.members(case, sl)) for sl in cuts])
        assert ref.results_differ(got, ref.reference(config, name)) == [], name


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer

TRACERS = {"kessler": ("water_vapor", "cloud_liquid", "precip_liquid"), "p3": ("water_vapor", "cloud_water", "ice"), "none": ("water_vapor",)}
NAMES = {"kessler": dict(rho_c="cloud_liquid"), "p3": dict(rho_c="cloud_water", rho_i="ice"), "none": {}}
COMMON = dict(rho_d="density_dry", rho_v="water_vapor", temp="temp", uvel="uvel", vvel="vvel", wvel="wvel")
CRM_DT, GCM_DT = 20.0, 240.0


def _coupler(config, micro):
    from pam_amd import PamCoupler
    nz, ny, nx, nens = config
    c = PamCoupler("cuda:0")
    c.set_option("crm_dt", CRM_DT)
    c.set_option("gcm_physics_dt", GCM_DT)
    c.allocate_coupler_state(nz, ny, nx, nens)
    for t in TRACERS[micro]:
        c.add_tracer(t, "", True, True)
    c.set_option("micro", micro)
    return c


def _load(c, f, micro):
    import torch
    dm = c.get_data_manager_device_readwrite()
    for ours, theirs in dict(COMMON, **NAMES[micro]).items():
        dm.get(theirs).copy_(torch.from_numpy(f[ours]))


def _as_seen_by(micro, f):
    """the fields as this microphysics has them: what it lacks is absent"""
    return {n: (f[n] if n in COMMON or n in NAMES[micro] else None) for n in ref.FIELDS}


def _there(micro):
    return {x: (micro != "none" or x not in ref.SAMPLED) for x in ref.OUT}


@pytest.mark.gpu
@pytest.mark.parametrize("micro", ["p3", "kessler", "none"])
def test_gpu_python_layer_on_the_clock(micro):
    """flux_profiles_init, then three CRM steps whose states are the two_steps case's two and the base again and whose weights are
    MsaClock's (3 while it accelerates, 1 after the cease): the restatement's bits in the coupler's entries, and exactly the entries this
    field set has"""
    import torch
    from pam_amd import modules
    from pam_amd.modules import MsaClock
    config = (4, 8, 8, 65)
    cs = ref.cases(config)
    steps = [_as_seen_by(micro, f) for f in [s[0] for s in cs["two_steps"]["steps"]] + [cs["base"]["steps"][0][0]]]
    c = _coupler(config, micro)
    modules.flux_profiles_init(c)
    dm = c.get_data_manager_device_readwrite()
    there = _there(micro)
    for x in ref.OUT:
        assert dm.entry_exists("prof_" + x) == there[x], x
        if there[x]:
            assert dm.get_shape("prof_" + x) == [4, 65]
            dm.get("prof_" + x).fill_(7.0)
    assert c.get_option("crm_prof_qc_threshold") == 1.0e-5
    modules.flux_profiles_init(c)                                   # the start of a GCM step: zeroes what is there
    clock, weights = MsaClock(12, 2), []
    for step, f in enumerate(steps):
        _load(c, f, micro)
        weights.append(clock.advance(step == 1))                    # the second step's acceleration ceases
        modules.flux_profiles(c, weights[-1])
    assert weights == [3, 1, 1]
    torch.cuda.synchronize()
    zeros = {x: (np.zeros((4, 65)) if there[x] else None) for x in ref.OUT}
    want = ref.run_case(ref.RefBackend(), dict(qc=1.0e-5, out0=zeros, steps=[(f, CRM_DT / GCM_DT * float(w)) for f, w in zip(steps, weights)]))
    for x in ref.OUT:
        if there[x]:
            assert ref.same_bits(dm.get("prof_" + x, readonly=True).cpu().numpy(), want[x]), x
    assert (want["tke"] > 0).all() and (micro == "none" or (want["cld"] > 0).all())


@pytest.mark.gpu
def test_gpu_python_layer_refuses_every_misuse_before_a_launch():
    import torch
    from pam_amd import modules
    from pam_amd.capi import PamAmdError
    config = (2, 4, 4, 3)
    c = _coupler(config, "p3")
    with pytest.raises(PamAmdError, match="init first"):            # no init
        modules.flux_profiles(c)
    modules.flux_profiles_init(c)
    _load(c, ref.base_fields(config, np.random.default_rng(5)), "p3")
    modules.flux_profiles(c)
    dm = c.get_data_manager_device_readwrite()
    torch.cuda.synchronize()
    before = {n: dm.get(n, readonly=True).cpu().numpy() for n in modules.FLUX_PROFILES}
    assert all(np.isfinite(a).all() for a in before.values()) and (before["prof_tke"] > 0).all()
    for weight in (float("nan"), float("inf")):
        with pytest.raises(PamAmdError, match="not finite"):
            modules.flux_profiles(c, weight)
    for opt, bad, match in (("crm_prof_qc_threshold", -1.0, ">= 0"), ("crm_prof_qc_threshold", float("nan"), ">= 0"),
                            ("crm_prof_qc_threshold", float("inf"), "finite"), ("gcm_physics_dt", 0.0, "gcm_physics_dt"),
                            ("gcm_physics_dt", -1.0, "gcm_physics_dt")):
        good = c.get_option(opt)
        c.set_option(opt, bad)
        with pytest.raises(PamAmdError, match=match):
            modules.flux_profiles(c)
        c.set_option(opt, good)
    c.set_option("micro", "morrison")
    for fn in (modules.flux_profiles_init, modules.flux_profiles):
        with pytest.raises(PamAmdError, match="kessler, p3 and none"):
            fn(c)
    c.set_option("micro", "kessler")                                # another field set than the init saw: cloud_liquid does not exist here
    with pytest.raises(PamAmdError):
        modules.flux_profiles(c)
    c.set_option("micro", "none")                                   # the sampled entries exist, but there is no condensate any more
    with pytest.raises(PamAmdError, match="changed since"):
        modules.flux_profiles(c)
    c.set_option("micro", "p3")
    c2 = _coupler(config, "none")
    modules.flux_profiles_init(c2)
    c2.add_tracer("cloud_liquid", "", True, True)
    c2.set_option("micro", "kessler")                               # a condensate the init did not see: prof_mcup does not exist
    with pytest.raises(PamAmdError, match="init first"):
        modules.flux_profiles(c2)
    c3 = _coupler(config, "none")
    c3.get_data_manager_device_readwrite().register_and_allocate("prof_tke", "", (3, 2))
    with pytest.raises(PamAmdError, match="shape"):
        modules.flux_profiles_init(c3)
    c4 = _coupler(config, "none")
    c4.set_option("crm_prof_qc_threshold", 1.0e-5)
    for n in modules.FLUX_PROFILES:                                 # entries somebody else registered, one of them with another shape
        if n not in ("prof_mcup", "prof_mcdn", "prof_cld"):
            c4.get_data_manager_device_readwrite().register_and_allocate(n, "", (3, 2) if n == "prof_flux_u" else (2, 3))
    with pytest.raises(PamAmdError, match="not \\(nz,nens"):
        modules.flux_profiles(c4)
    torch.cuda.synchronize()
    for n, a in before.items():
        assert ref.same_bits(dm.get(n, readonly=True).cpu().numpy(), a), n


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ module through tests/cxx/flux_profiles

@pytest.mark.gpu
@pytest.mark.parametrize("micro", ["none", "kessler", "p3"])
def test_gpu_cxx_module_is_the_restatement(tmp_path, micro):
    from test_fluxprof import cxx_program
    config = (5, 3, 7, 3)
    cs = ref.cases(config)
    steps = [_as_seen_by(micro, f) for f, _ in cs["two_steps"]["steps"]]
    weights = (3.0, 1.0)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(struct.pack("6i", *config, ("none", "kessler", "p3").index(micro), len(steps)))
        for f, w in zip(steps, weights):
            np.array([w]).tofile(fh)
            for n in ref.FIELDS:
                if f[n] is not None:
                    np.ascontiguousarray(f[n]).tofile(fh)
    r = subprocess.run([cxx_program(), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "### failed" not in r.stdout, (r.stdout[-1000:], r.stderr[-1000:])
    there = [x for x in ref.OUT if _there(micro)[x]]
    lines = r.stdout.strip().split("\n")
    assert lines[0].split() == ["###", "entries"] + ["prof_" + x for x in there] and lines[1] == "### options 1e-05"
    zeros = {x: (np.zeros((5, 3)) if x in there else None) for x in ref.OUT}
    want = ref.run_case(ref.RefBackend(), dict(qc=1.0e-5, out0=zeros, steps=[(f, CRM_DT / GCM_DT * w) for f, w in zip(steps, weights)]))
    got = np.fromfile(dst).reshape(len(there), 5, 3)
    for a, x in zip(got, there):
        assert ref.same_bits(a, want[x]), x


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
    return {name: raw[i * n:(i + 1) * n].reshape(nz, ny, nx, nens) for i, name in enumerate(names)}


def _python_profiles(states, weights):
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
    modules.flux_profiles_init(c)
    for st, w in zip(states, weights):
        for n, a in st.items():
            dm.get(n).copy_(torch.from_numpy(a))
        modules.flux_profiles(c, w)
    torch.cuda.synchronize()
    return {n: dm.get(n, readonly=True).cpu().numpy() for n in modules.FLUX_PROFILES if dm.entry_exists(n)}


@pytest.mark.gpu
@pytest.mark.parametrize("extra, weight", [((), 1), (("--accelerate", "2", "--accel-uv", "--hyperdiff", "600"), 3)], ids=["plain", "accelerated"])
def test_gpu_driver_flux_profiles_is_the_python_layer(tmp_path, extra, weight):
    """--flux-profiles on one and on two CRM steps: the state after step 1 is the output of a run of one step, the state after step 2 the
    run's own output; the Python layer, fed these states with the clock's weights, gives the bits the driver wrote.  The run's fields are
    those of a run without the flag"""
    from pam_amd import modules
    outs, files = [], []
    for steps in (1, 2):
        out, js = tmp_path / ("out%d.bin" % steps), tmp_path / ("fluxprof%d.json" % steps)
        lines = _run_driver("--steps", str(steps), "--flux-profiles", str(js), *extra, str(out))
        assert json.loads(lines[-1])["crm_steps"] == steps
        outs.append(out)
        files.append([json.loads(line) for line in js.read_text().strip().split("\n")])
    plain = tmp_path / "plain.bin"
    _run_driver("--steps", "2", *extra, str(plain))
    assert plain.read_bytes() == outs[1].read_bytes()
    states = [_state(o) for o in outs]
    for nsteps, records in zip((1, 2), files):
        assert len(records) == 1                                    # one record per GCM step
        got = records[0]
        assert (got["gcm_step"], got["crm_steps"], got["nens"], got["nz"]) == (0, nsteps, 3, 50)
        assert list(got["profiles"]) == list(modules.FLUX_PROFILES)
        want = _python_profiles(states[:nsteps], [weight] * nsteps)
        assert sorted(want) == sorted(got["profiles"])
        for n, a in want.items():
            assert a.shape == (50, 3) and ref.same_bits(np.array(got["profiles"][n], dtype=np.float64), a), (nsteps, n)
        assert np.isfinite(want["prof_tke"]).all() and (want["prof_tke"] >= 0).all() and (want["prof_tke"] > 0).any()


@pytest.mark.gpu
def test_gpu_driver_composes_the_flag_and_prints_it_in_its_usage(tmp_path):
    """with --column-diag, --gcm-handoff and --radiation beside it the records are those of the flag alone; the usage text lists the flag"""
    rad = tmp_path / "rad.bin"
    np.zeros((50, 1, 5, 3)).tofile(rad)
    alone, both = tmp_path / "alone.json", tmp_path / "both.json"
    _run_driver("--steps", "2", "--flux-profiles", str(alone), "-")
    _run_driver("--steps", "2", "--radiation", "5", "1", str(rad), "--gcm-handoff", "5", "1", str(tmp_path / "h.json"), "--column-diag",
                str(tmp_path / "cd.json"), "--flux-profiles", str(both), "-")
    assert alone.read_text() == both.read_text() and alone.read_text().count("\n") == 1
    r = subprocess.run([DRIVER, "--yaml", MSA_YAML, "--flux-profiles", "-"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--column-diag PATH] [--flux-profiles PATH]" in r.stderr
