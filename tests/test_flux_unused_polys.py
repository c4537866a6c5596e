"""CPU: the y/z flux sweeps build only the polynomials a face uses (flux_line_body_zt, pam_amd/csrc/awfl_device.h) -- and compute what
they computed when they built them all.

The host emulation of the kernel bodies runs one sub-step (three stages; the flux arrays are those of the last one) on small grids and
is compared, with numpy.array_equal (-0 equals +0, NaN equals nothing), with arrays recorded from the emulation of the commit before the
skips: tests/golden/flux_unused_polys_parent.npz, written by tests/golden/make_flux_unused_polys_golden.py.  Every schedule of a physics
case -- member or flat lanes, the z sweep whole or cut into two spans (one starts at a wall, the other ends at one), the y differences
folded into the z sweep, the fused or the three-kernel stage -- is held to the same recorded arrays (tests/flux_unused_polys_cases.py).

The recorded cases have dx == dy.  The anisotropic cases with the shear along y (fc.ANISO_PHYSICS) have no recorded arrays: their plain
schedule is held to the oracle through the parity gate (tests/parity_gate.py), every other schedule to the plain one's bits."""
import copy
import os

import numpy as np
import pytest

import emu_harness
import flux_unused_polys_cases as fc
from oracle import awfl_oracle as ao
from pam_amd import idealized as idz
from parity_gate import compare, noise_floor

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flux_unused_polys_parent.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        g = {k: z[k] for k in z.files}
    for k, a in g.items():
        assert np.isfinite(a).all(), k
        a.setflags(write=False)
    return g


def test_the_cases_cover_what_they_claim():
    grids = set(fc.GRIDS)
    assert {(5, 3, 6), (5, 4, 7), (5, 5, 9), (5, 6, 10), (5, 7, 11), (5, 11, 12), (5, 1, 8)} == grids
    assert {ny % 5 for _, ny, _ in grids if ny > 1} == {0, 1, 2, 3, 4}           # trips of a periodic line
    assert {(nz + 1) % 5 for _, _, nz in grids} == {0, 1, 2, 3, 4}               # trips of a column: faces 0 .. nz
    variants = {v for g in fc.GRIDS for v in fc.GRIDS[g]}
    assert variants == {(nt, c, pe) for nt in (1, 4) for c in (0, 1) for pe in (0, 1)}
    assert fc.PLAIN in fc.SCHEDULES and len(fc.SCHEDULES) == 8


@pytest.mark.parametrize("p", fc.PHYSICS, ids=fc.physics_id)
def test_every_schedule_reproduces_the_parent_commit(p, gold):
    for s in fc.SCHEDULES:
        if not fc.applies(p, s):
            continue
        got = fc.run(emu_harness, p, s)
        where = (fc.physics_id(p), fc.schedule_id(s))
        for name, (a, m) in got.items():
            if name in fc.FIELDS:
                assert np.array_equal(a, gold[fc.key(p, True, name)]), where + (name,)
            elif s[3]:            # the fused stage: differences of the state, faces of the mass flux and the tracers
                assert np.array_equal(a[m], gold[fc.key(p, True, name)][m]), where + (name,)
            else:                 # the three-kernel stage: faces everywhere; those of the mass flux and the tracers are the fused stage's
                assert m.all()
                assert np.array_equal(a[1:5], gold[fc.key(p, False, name)]), where + (name,)
                for fld in [0] + list(range(5, a.shape[0])):
                    assert np.array_equal(a[fld], gold[fc.key(p, True, name)][fld]), where + (name, fld)


@pytest.mark.parametrize("p", fc.ANISO_PHYSICS, ids=fc.physics_id)
def test_anisotropic_y_flow_case_matches_the_oracle_in_every_schedule(p):
    (nx, ny, nz), (nt, carve, perens) = p[:2]
    plain = {fused: fc.run(emu_harness, p, ("member", 1, False, fused)) for fused in (True, False)}
    f, tr, zi, xlen, ylen = fc.make_fields(p)
    assert ylen / ny != xlen / nx and np.abs(f["vvel"]).max() >= 0.5 * np.abs(f["uvel"]).max()
    names, pos, mass, idwv = idz.tracer_flags(tr)

    def run_oracle(ff):
        o = ao.OracleDycore(fc.NENS, nx, ny, nz, xlen, ylen, np.diff(zi, axis=0), pos, mass, idwv)
        o.declare_current_profile_as_hydrostatic(ff)
        assert o.time_step(ff, fc.DT, fc.DT) == (1, fc.DT)
    exp = copy.deepcopy(f)
    run_oracle(exp)
    got = {k: plain[True][k][0] for k in fc.FIELDS}
    compare(got, exp, names, 1, floor=noise_floor(run_oracle, f, names, 0, base=exp))
    for s in fc.SCHEDULES:
        got = fc.run(emu_harness, p, s)
        where = (fc.physics_id(p), fc.schedule_id(s))
        for name, (a, m) in got.items():
            if name in fc.FIELDS:
                assert np.array_equal(a, plain[True][name][0]), where + (name,)
            elif s[3]:
                assert np.array_equal(a[m], plain[True][name][0][m]), where + (name,)
            else:
                assert m.all()
                assert np.array_equal(a, plain[False][name][0]), where + (name,)
                for fld in [0] + list(range(5, a.shape[0])):
                    assert np.array_equal(a[fld], plain[True][name][0][fld]), where + (name, fld)
