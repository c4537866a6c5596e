"""GPU: the fused x-sweep that loads water vapour's FCT seed only where a lower bound of it does not settle the multiplier
(set_seed_skip("on"); awfl_xupd_kernel<., ., ., true>, seed_lower_bound) against the sweep that always loads it ("off") and against
the three-kernel stage: bit for bit on every output and on the seed.  Smooth vapour (no wavefront needs its seed) and carved dry air
(rows of both kinds in every stage; tests/test_seed_bound.py counts them in the host emulation)."""
import numpy as np
import pytest

from pam_amd import idealized as idz
from parity_cases import build_inputs

pytestmark = pytest.mark.gpu

# (nens, nx, ny, nz): one member block; a ragged second block; 2-D with a span above 32 cells (the separate pressure pass)
SHAPES = {"64_8x4x5": (64, 8, 4, 5), "96_8x4x5_ragged": (96, 8, 4, 5), "128_33x1x6_2d": (128, 33, 1, 6)}
INPUTS = ("smooth", "dry_air_spread", "dry_air_aligned")
FIELDS = ("density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor", "seed")
_cache = {}


def _fields(shape, inputs):
    nens, nx, ny, nz = SHAPES[shape]
    tr = idz.TRACERS_NONE
    zint = idz.stretched_interfaces(nz, 6000.0)
    f, xlen, ylen, zi, _ = build_inputs(nens, nx, ny, nz, tr, zint, mag=0.5)
    if inputs != "smooth":       # parity_cases' dry_air wind across the carved edges, with the slabs spread over the members or aligned
        f["uvel"] -= 25.0
        f["vvel"] += 7.0
        idz.carve_dry_air(f, tr, spread=(inputs == "dry_air_spread"))
    return f, xlen, ylen, zi


def _run(shape, inputs, fused=True, skip="off", fold="off", tail="auto"):
    key = (shape, inputs, fused, skip, fold, tail)
    if key in _cache:
        return _cache[key]
    import torch
    from pam_amd import Dycore, PamCoupler
    nens, nx, ny, nz = SHAPES[shape]
    f, xlen, ylen, zi = _fields(shape, inputs)
    coupler = PamCoupler("cuda:0")
    coupler.set_option("crm_dt", 2.0)
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(xlen, ylen, zi)
    for n, p, m in idz.TRACERS_NONE:
        coupler.add_tracer(n, "", p, m)
    dycore = Dycore()
    dycore.init(coupler)
    dycore.set_fused_stage(fused)
    dycore.set_lane_mapping("member", "sweep")
    dycore.set_ensemble_chunks(1)
    dycore.set_tail_fusion(tail)
    dycore.set_yz_fold(fold)
    dycore.set_seed_skip(skip)
    coupler.load_fields(f)
    dycore.declare_current_profile_as_hydrostatic(coupler)
    ncyc = dycore.timeStep(coupler)
    torch.cuda.synchronize()
    out = coupler.dump_fields()
    out["water_vapor"] = out["tracers"][0]
    out["seed"] = dycore.debug_buffer("seed").cpu().numpy().copy()
    if not fused:
        out["mult"] = dycore.debug_buffer("mult").cpu().numpy().copy()
    dycore.finalize(coupler)
    _cache[key] = (ncyc, out)
    return _cache[key]


def _same(a, b):
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), (k, np.abs(a[k] - b[k]).max())


@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_seed_skip_on_equals_off_equals_three_kernel_stage(shape, inputs):
    n3, three = _run(shape, inputs, fused=False)
    n0, off = _run(shape, inputs, skip="off")
    n1, on = _run(shape, inputs, skip="on")
    assert n3 == n0 == n1 and n3 >= 2           # two sub-steps: stage 1 reads init_prim's seeds, then stage 3's
    for k in FIELDS:
        assert np.isfinite(three[k]).all(), k
    _same(off, three)
    _same(on, off)
    limited = (three["mult"] < 1.0).any()       # (the last three-kernel stage's multipliers: complete)
    assert limited == (inputs != "smooth") and (three["mult"] == 1.0).any()


@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("option", ({"fold": "on"}, {"tail": "off"}), ids=("yz_fold", "pressure_pass"))
def test_seed_skip_with_the_folded_handoff_and_with_the_separate_pressure_pass(option, inputs):
    shape = "64_8x4x5"
    _, ref = _run(shape, inputs, skip="off")
    _, off = _run(shape, inputs, skip="off", **option)
    _, on = _run(shape, inputs, skip="on", **option)
    _same(on, off)
    _same(on, ref)             # (both options are schedules, not arithmetics)
