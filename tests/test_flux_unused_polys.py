"""CPU: the y/z flux sweeps build only the polynomials a face uses (flux_line_body_zt, pam_amd/csrc/awfl_device.h) -- and compute what
they computed when they built them all.

The host emulation of the kernel bodies runs one sub-step (three stages; the flux arrays are those of the last one) on small grids and
is compared, with numpy.array_equal (-0 equals +0, NaN equals nothing), with arrays recorded from the emulation of the commit before the
skips: tests/golden/flux_unused_polys_parent.npz, written by tests/golden/make_flux_unused_polys_golden.py.  Every schedule of a physics
case -- member or flat lanes, the z sweep whole or cut into two spans (one starts at a wall, the other ends at one), the y differences
folded into the z sweep, the fused or the three-kernel stage -- is held to the same recorded arrays (tests/flux_unused_polys_cases.py)."""
import os

import numpy as np
import pytest

import emu_harness
import flux_unused_polys_cases as fc

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
