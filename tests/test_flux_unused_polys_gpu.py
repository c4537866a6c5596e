"""GPU: the y/z flux sweeps that build only the polynomials a face uses (flux_line_body_zt, pam_amd/csrc/awfl_device.h) on the device,
in every kernel the body is compiled into: member lanes with whole and ragged blocks of 64 members (awfl_flux_kernel; per-member
vertical grids: awfl_fluxz_pe_kernel, whose workgroup barriers the table hooks hold), and small ensembles (flat lanes; their tile
kernels do not go through the body and must be untouched).

Per case: the fused stage equals the three-kernel stage and member lanes equal flat lanes, bit for bit, and the default schedule's
fields pass the oracle gate of tests/parity_gate.py.  Every case runs in a child process of its own under a time limit: a sweep that
waits at a barrier another wavefront never reaches ends there and not with the suite."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIMIT = 120          # seconds per case (a case takes a few)

# (nx, ny, nz, NT): 3-D with a single-field last pair (NT = 4), 2-D (no y sweep; the fused stage skips v)
GRIDS = [(6, 5, 10, 4), (6, 1, 9, 1)]
NENS = [64, 130, 8]
CASES = [(g, nens, perens) for g in GRIDS for nens in NENS for perens in (0, 1)]
# dx = 500 m, dy = 800 m with the sounding's shear along y (a fourth element): member lanes on per-member grids, and flat lanes
ANISO_CASES = [((6, 5, 10, 4), 64, 1, 1), ((6, 7, 8, 1), 8, 0, 1)]


def _id(c):
    (nx, ny, nz, nt), nens, perens = c[:3]
    return "%dx%dx%d_nt%d_nens%d_%s" % (nx, ny, nz, nt, nens, "perens" if perens else "shared") + ("_dx500_dy800_flowy" if len(c) > 3 else "")


def _inputs(nx, ny, nz, nt, nens, perens, aniso=0):
    import numpy as np
    from pam_amd import idealized as idz
    from parity_cases import build_inputs
    tr = idz.TRACERS_NONE if nt == 1 else idz.TRACERS_KESSLER_SHOC
    zint = idz.stretched_interfaces(nz, 12000.0)
    f, xlen, ylen, _, _ = build_inputs(nens, nx, ny, nz, tr, zint, mag=0.5, **(dict(dxy=500.0, dy=800.0, flow="y") if aniso else {}))
    # smooth periodic waves on the wind: both signs of the mass flux at the faces of every line, motion next to both walls
    k, j, i, e = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), np.arange(nens), indexing="ij")
    px, py = 2.0 * np.pi * i / nx, 2.0 * np.pi * j / ny
    f["uvel"] = f["uvel"] - 25.0 + 3.0 * np.sin(px + 0.1 * e)
    if ny > 1:
        f["vvel"] = f["vvel"] - 2.0 + 6.0 * np.cos(py + px + 0.2 * e)
    f["wvel"] = f["wvel"] + 0.5 * np.sin(px + py + 0.6 * k + 0.3 * e)
    idz.carve_dry_air(f, tr)
    zi = np.asarray(zint)[:, None] * np.ones((1, nens))
    if perens:
        zi = zi * (1 + 0.01 * (np.arange(nens) % 16) + 1.0e-4 * (np.arange(nens) // 16))[None, :]
    return f, tr, zi, xlen, ylen


def _run(inp, nx, ny, nz, nens, fused, lanes=None):
    import copy
    import torch
    from pam_amd import Dycore, PamCoupler
    f, tr, zi, xlen, ylen = inp
    coupler = PamCoupler("cuda:0")
    coupler.set_option("crm_dt", 2.0)
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(xlen, ylen, zi)
    for n, p, m in tr:
        coupler.add_tracer(n, "", p, m)
    dycore = Dycore()
    dycore.init(coupler)
    dycore.set_fused_stage(fused)
    if lanes is not None:
        dycore.set_lane_mapping(*lanes)
    coupler.load_fields(copy.deepcopy(f))
    dycore.declare_current_profile_as_hydrostatic(coupler)
    ncyc = dycore.timeStep(coupler)
    torch.cuda.synchronize()
    out = coupler.dump_fields()
    dycore.finalize(coupler)
    return ncyc, out


def _worker(nx, ny, nz, nt, nens, perens, aniso=0):
    import copy
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from pam_amd import idealized as idz
    from oracle import awfl_oracle as ao
    from parity_gate import compare
    inp = _inputs(nx, ny, nz, nt, nens, perens, aniso)
    f, tr, zi, xlen, ylen = inp
    names, pos, mass, idwv = idz.tracer_flags(tr)
    keys = ("density_dry", "uvel", "vvel", "wvel", "temp", "tracers")

    def same(a, b, what):
        assert a[0] == b[0], (what, a[0], b[0])
        for k in keys:
            assert np.isfinite(a[1][k]).all(), (what, k)
            assert np.array_equal(a[1][k], b[1][k]), (what, k, float(np.abs(a[1][k] - b[1][k]).max()))

    default = _run(inp, nx, ny, nz, nens, True)
    same(default, _run(inp, nx, ny, nz, nens, False), "fused stage == three-kernel stage")
    member = _run(inp, nx, ny, nz, nens, True, ("member", "sweep"))
    same(member, _run(inp, nx, ny, nz, nens, True, ("flat", "sweep")), "member lanes == flat lanes")
    same(default, member, "default schedule == member lanes")
    fo = copy.deepcopy(f)
    o = ao.OracleDycore(nens, nx, ny, nz, xlen, ylen, np.diff(zi, axis=0), pos, mass, idwv)
    o.declare_current_profile_as_hydrostatic(fo)
    n2, _ = o.time_step(fo, 2.0)
    assert n2 == default[0], (n2, default[0])
    worst = compare(default[1], fo, names, n2)
    print("worst", {k: "%.2e" % v for k, v in worst.items()})
    print("CASE OK")


@pytest.mark.parametrize("case", CASES + ANISO_CASES, ids=_id)
def test_walls_and_periodic_closing_on_the_device(case):
    (nx, ny, nz, nt), nens, perens = case[:3]
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(v) for v in (nx, ny, nz, nt, nens, perens) + case[3:]],
                       capture_output=True, text=True, timeout=LIMIT, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "CASE OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    _worker(*[int(v) for v in sys.argv[1:8]])
