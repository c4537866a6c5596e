"""The native grey two-stream longwave radiation scheme on the GPU: pam_amd_radiation_gray against the numpy restatement
(tests/grayrad_ref.py) bit for bit (a NaN by its place) on every shape and named case; the wide-index instance against the narrow one;
members split over calls against the whole; a bystander tensor and a side stream; the Python class through a coupler with Kessler's and
with P3's tracer names, every step and every third step; and the C++ class through examples/driver --radiation-gray on a shortened CI
input."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import grayrad_ref as ref
import grayrad_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
YAML = os.path.join(ROOT, "tests", "golden", "msa_input.yaml")
SCALARS = ("k_d", "k_v", "k_l", "k_i", "sigma", "cp_d", "lw_down_top", "dt")
POISON = -7.0e77


class GpuBackend:
    """the interface of grayrad_ref.RefBackend over the C ABI; wide: pam_amd_radiation_gray_debug_wide_index, set for the call and reset
    after it"""

    def __init__(self, wide=False):
        import torch
        from pam_amd import capi
        self.torch, self.lib, self.check, self.wide = torch, capi.load(), capi.check, wide

    def _dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def upload(self, case):
        dev = {n: self._dev(a) for n, a in case["fields"].items()}
        dev["zint"], dev["sfc_temp"] = self._dev(case["zint"]), self._dev(case.get("sfc_temp"))
        shape = dev["temp"].shape
        dev["rad_heating"] = self.torch.full(shape, POISON, dtype=self.torch.float64, device="cuda:0")
        for n in ref.OUTPUTS[2:]:
            dev[n] = self.torch.full(shape[1:], POISON, dtype=self.torch.float64, device="cuda:0")
        return dev

    def call(self, case, dev, stream=None):
        nz, ny, nx, nens = dev["temp"].shape
        liquid = (C.c_void_p * 2)(*[dev[n].data_ptr() for n in case["liquid"]])
        ice = (C.c_void_p * 2)(*[dev[n].data_ptr() for n in case["ice"]])
        sfc = None if dev["sfc_temp"] is None else dev["sfc_temp"].data_ptr()
        stream = self.torch.cuda.current_stream().cuda_stream if stream is None else stream
        self.check(self.lib.pam_amd_radiation_gray_debug_wide_index(int(self.wide)))
        try:
            self.check(self.lib.pam_amd_radiation_gray(nens, nx, ny, nz, dev["temp"].data_ptr(), dev["density_dry"].data_ptr(),
                                                       dev["water_vapor"].data_ptr(), len(case["liquid"]), liquid, len(case["ice"]), ice,
                                                       dev["zint"].data_ptr(), sfc, *[float(case[n]) for n in SCALARS],
                                                       *[dev[n].data_ptr() for n in ref.OUTPUTS[1:]], stream))
        finally:
            self.check(self.lib.pam_amd_radiation_gray_debug_wide_index(0))

    def run(self, case):
        dev = self.upload(case)
        self.call(case, dev)
        self.torch.cuda.synchronize()
        return {n: dev[n].cpu().numpy() for n in ref.OUTPUTS}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", gc.SHAPES, ids=ref.shape_id)
def test_gpu_matches_restatement_bit_for_bit(shape):
    """every named case, with each member's own grid; one case with identical columns; one case twice: two runs are identical"""
    be = GpuBackend()
    for name in gc.CASE_NAMES:
        got = be.run(gc.cases(shape)[name])
        assert ref.results_differ(got, gc.outputs(gc.reference(shape, name)), nan_by_place=True) == [], name
    got = be.run(gc.cases(shape, False)["two_and_two"])
    assert ref.results_differ(got, gc.outputs(gc.reference(shape, "two_and_two", False))) == []
    a, b = (be.run(gc.cases(shape)["p3_set"]) for _ in range(2))
    assert ref.results_differ(a, b) == []
    case = gc.cases(shape)["dt_zero"]
    assert ref.same_bits(be.run(case)["temp"], case["fields"]["temp"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(7, 3, 2, 65), (60, 1, 2, 130)], ids=ref.shape_id)
def test_gpu_wide_index_instance_equals_the_narrow_one(shape):
    for name in ("two_and_two", "thick_cloud", "nan_cell"):
        case = gc.cases(shape)[name]
        wide, narrow = GpuBackend(wide=True).run(case), GpuBackend().run(case)
        assert ref.results_differ(wide, narrow, nan_by_place=True) == [], name
        assert ref.results_differ(wide, gc.outputs(gc.reference(shape, name)), nan_by_place=True) == [], name


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(7, 3, 2, 65), (60, 1, 2, 130)], ids=ref.shape_id)
def test_gpu_members_split_over_calls_equal_the_whole(shape):
    nens, be = shape[3], GpuBackend()
    for name in ("two_and_two", "nan_cell"):
        case, want = gc.cases(shape)[name], gc.outputs(gc.reference(shape, name))
        parts = [be.run(gc.members(case, slice(lo, hi))) for lo, hi in ((0, 1), (1, 37), (37, nens))]
        got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
        assert ref.results_differ(got, want, nan_by_place=True) == [], name


@pytest.mark.gpu
def test_gpu_bystander_tensor_and_a_side_stream():
    """tensors allocated before and after the fields keep their bits, and so do the read-only inputs; the call on a non-default stream,
    the fields produced on that stream just before it, gives the restatement's bits"""
    import torch
    shape = (12, 2, 5, 70)
    case, want = gc.cases(shape)["two_and_two"], gc.outputs(gc.reference(shape, "two_and_two"))
    be = GpuBackend()
    before = torch.full((4096,), 3.25, dtype=torch.float64, device="cuda:0")
    host = {n: torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for n, a in case["fields"].items()}
    host["zint"], host["sfc_temp"] = (torch.from_numpy(np.ascontiguousarray(case[n])).pin_memory() for n in ("zint", "sfc_temp"))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = {n: torch.empty(h.shape, dtype=torch.float64, device="cuda:0") for n, h in host.items()}
        dev["rad_heating"] = torch.empty(shape, dtype=torch.float64, device="cuda:0")
        for n in ref.OUTPUTS[2:]:
            dev[n] = torch.empty(shape[1:], dtype=torch.float64, device="cuda:0")
        after = torch.full((4096,), 3.25, dtype=torch.float64, device="cuda:0")
        for n, h in host.items():
            dev[n].copy_(h, non_blocking=True)
        be.call(case, dev, stream=side.cuda_stream)
    side.synchronize()
    got = {n: dev[n].cpu().numpy() for n in ref.OUTPUTS}
    assert ref.results_differ(got, want) == []
    assert (before == 3.25).all() and (after == 3.25).all()
    for n in ("density_dry", "water_vapor", "cloud_liquid", "liquid_b", "ice", "ice_b"):
        assert ref.same_bits(dev[n].cpu().numpy(), np.ascontiguousarray(case["fields"][n])), n
    for n in ("zint", "sfc_temp"):
        assert ref.same_bits(dev[n].cpu().numpy(), np.ascontiguousarray(case[n])), n


# ------------------------------------------------------------------------------------------------------------------------------
# the Python class through a coupler

def _coupler(shape, micro, case, rad):
    import torch
    from pam_amd import PamCoupler
    nz, ny, nx, nens = shape
    c = PamCoupler("cuda:0")
    c.set_option("cp_d", case["cp_d"])
    c.set_option("crm_dt", case["dt"])
    c.set_option("micro", micro)
    c.allocate_coupler_state(nz, ny, nx, nens)
    c.set_grid(nx * 500.0, ny * 500.0, case["zint"][:, 0].copy())
    for n in ("water_vapor",) + case["liquid"] + case["ice"]:
        c.add_tracer(n, "", True, True)
    rad.init(c)
    dm = c.get_data_manager_device_readwrite()
    for n in ref.OUTPUTS[1:]:
        assert dm.entry_exists(n) and float(dm.get(n, readonly=True).abs().max()) == 0.0
    for n in ("temp", "density_dry", "water_vapor") + case["liquid"] + case["ice"]:
        dm.get(n).copy_(torch.from_numpy(case["fields"][n]))
    dm.get("vertical_interface_height").copy_(torch.from_numpy(case["zint"]))
    return c, dm


@pytest.mark.gpu
@pytest.mark.parametrize("micro", ["kessler", "p3"])
@pytest.mark.parametrize("shape", [(2, 1, 3, 3), (7, 3, 2, 65)], ids=ref.shape_id)
def test_gpu_python_class_through_a_coupler(shape, micro):
    """RadiationGray().init / timeStep with Kessler's and with P3's tracer names: temp and the four outputs equal the restatement; the
    options are set only where absent; with an "sfc_temp" entry the surface radiates at it"""
    import torch
    from pam_amd import RadiationGray
    species = dict(kessler=dict(liquid=("cloud_liquid",), ice=()), p3=dict(liquid=("cloud_water",), ice=("ice",)))[micro]
    case = dict(gc.cases(shape)["clear_sky"], k_v=0.2, lw_down_top=12.0, **species)
    rad = RadiationGray(k_v=0.2, lw_down_top=12.0)
    assert rad.radiation_name() == "gray"
    c, dm = _coupler(shape, micro, case, rad)
    assert c.get_option("radiation") == "gray" and c.get_option("rad_gray_every") == 1
    assert [c.get_option("rad_gray_" + n) for n in ("k_d", "k_v", "k_l", "k_i", "lw_down_top")] == [1e-4, 0.2, 85.0, 40.0, 12.0]
    rad.timeStep(c)
    torch.cuda.synchronize()
    got = {n: dm.get(n, readonly=True).cpu().numpy() for n in ref.OUTPUTS}
    assert ref.results_differ(got, ref.radiation(case)) == []
    # a second class on the same coupler does not overwrite the options; with "sfc_temp" and option "sigma" the call takes both
    sfc = gc.cases(shape)["two_and_two"]["sfc_temp"]
    dm.register_and_allocate("sfc_temp", "surface temperature [K]", sfc.shape, ("y", "x", "nens"))
    dm.get("sfc_temp").copy_(torch.from_numpy(sfc))
    c.set_option("sigma", 5.67e-8)
    again = RadiationGray(k_v=0.7)
    again.init(c)
    assert c.get_option("rad_gray_k_v") == 0.2
    case2 = dict(case, fields=dict(case["fields"], temp=got["temp"]), sfc_temp=sfc, sigma=5.67e-8)
    again.timeStep(c)
    torch.cuda.synchronize()
    got2 = {n: dm.get(n, readonly=True).cpu().numpy() for n in ref.OUTPUTS}
    assert ref.results_differ(got2, ref.radiation(case2)) == []
    rad.finalize(c)


@pytest.mark.gpu
def test_gpu_python_class_every_third_step():
    """every = 3 over 6 steps: steps 0 and 3 compute the fluxes, steps 1, 2, 4 and 5 are temp += rad_heating * dt of the stored field,
    bit for bit against numpy, and leave the four outputs alone"""
    import torch
    from pam_amd import RadiationGray
    shape = (7, 3, 2, 65)
    case = dict(gc.cases(shape)["clear_sky"], liquid=("cloud_liquid",))
    rad = RadiationGray(every=3)
    c, dm = _coupler(shape, "kessler", case, rad)
    temp, stored = case["fields"]["temp"], None
    for step in range(6):
        rad.timeStep(c)
        torch.cuda.synchronize()
        got = {n: dm.get(n, readonly=True).cpu().numpy() for n in ref.OUTPUTS}
        if step % 3 == 0:
            stored = ref.radiation(dict(case, fields=dict(case["fields"], temp=temp)))
            temp = stored["temp"]
        else:
            temp = temp + stored["rad_heating"] * case["dt"]
        assert ref.results_differ(got, dict(stored, temp=temp)) == [], step


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ class through the driver

def _run_driver(*args, timeout=600):
    return subprocess.run([DRIVER, "--yaml", YAML, "--nens", "3"] + list(args), capture_output=True, text=True, timeout=timeout)


@pytest.mark.gpu
def test_gpu_driver_runs_the_gray_scheme(tmp_path):
    """the whole loop of the shortened input (Kessler, sponge layer) with --radiation-gray: it exits 0, prints finite, positive OLR on
    every output step and ends with a lower ensemble-mean temp than the same run without the flag (a longwave-only scheme cools)"""
    from test_sgs_smag_gpu import _fields
    a, b = tmp_path / "gray.bin", tmp_path / "none.bin"
    ra, rb = _run_driver("--radiation-gray", str(a)), _run_driver(str(b))           # 12 CRM steps, one output step (out_freq = 200 s)
    assert ra.returncode == 0, ra.stderr[-2000:]
    assert rb.returncode == 0, rb.stderr[-2000:]
    la, lb = ra.stdout.strip().split("\n"), rb.stdout.strip().split("\n")
    rows = [re.fullmatch(r"radiation gray: etime (\S+) , olr (\S+) , lw_down_sfc (\S+)", l) for l in la if l.startswith("radiation gray:")]
    assert rows and all(rows) and len(rows) == sum(l.startswith("Etime ,") for l in la)
    for m in rows:
        olr, down = float(m.group(2)), float(m.group(3))
        assert np.isfinite(olr) and olr > 0 and np.isfinite(down) and down > 0
    assert not any(l.startswith("radiation gray:") for l in lb)
    last = json.loads(la[-1])
    assert last["crm_steps"] == 12 and last["finite"] is True and json.loads(lb[-1])["crm_steps"] == 12
    fa, fb = _fields(a, last), _fields(b, last)
    assert np.isfinite(fa[4]).all() and fa[4].mean() < fb[4].mean()
    # EVERY as the optional argument: the same run with the fluxes computed every other step still cools
    rc = _run_driver("--radiation-gray", "2", str(tmp_path / "two.bin"))
    assert rc.returncode == 0, rc.stderr[-2000:]
    assert _fields(tmp_path / "two.bin", last)[4].mean() < fb[4].mean()


@pytest.mark.gpu
def test_gpu_driver_refuses_both_radiation_flags(tmp_path):
    tend = tmp_path / "tend.bin"
    tend.write_bytes(b"")
    r = _run_driver("--steps", "1", "--radiation-gray", "--radiation", "1", "1", str(tend), "-")
    assert r.returncode != 0 and "--radiation-gray and --radiation" in r.stderr + r.stdout
