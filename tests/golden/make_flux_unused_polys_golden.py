"""Records tests/golden/flux_unused_polys_parent.npz from the host emulation of the tree this script stands in.

Run it on the PARENT of the commit that stopped building the polynomials no face uses (check that commit's parent out, copy this script
and tests/flux_unused_polys_cases.py into it, run `python tests/golden/make_flux_unused_polys_golden.py`): the recorded arrays are
what tests/test_flux_unused_polys.py holds every later emulation to, with numpy.array_equal.

Per physics case, from the plain schedule (member lanes, whole lines, no fold): the y and z flux arrays of the sub-step's last fused stage,
the state variables' face fluxes of the same stage run as three kernels (its mass-flux and tracer faces are checked to be the fused
stage's own), and all prognostic fields after the sub-step.  Before anything is written the script checks that every recorded value is
finite and that, on this tree, every other schedule reproduces the plain one -- so a later mismatch is the later tree's.
The x fluxes are not recorded: the x sweep forms no difference, has no wall and closes no line."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import emu_harness  # noqa: E402
import flux_unused_polys_cases as fc  # noqa: E402


def main():
    gold = {}
    for p in fc.PHYSICS:
        ref = fc.run(emu_harness, p, fc.PLAIN)
        three = fc.run(emu_harness, p, ("member", 1, False, False))
        for name, (a, m) in ref.items():
            assert np.isfinite(a[m]).all(), (fc.physics_id(p), name)
            gold[fc.key(p, True, name)] = np.where(m, a, 0.0)
        for name in ("flux_y", "flux_z"):
            if name not in three:
                continue
            a, m = three[name]
            assert m.all() and np.isfinite(a).all(), (fc.physics_id(p), name)
            f, fm = ref[name]
            for fld in [0] + list(range(5, a.shape[0])):          # mass flux and tracers: faces in both stages
                assert fm[fld].all() and np.array_equal(a[fld], f[fld]), (fc.physics_id(p), name, fld)
            gold[fc.key(p, False, name)] = a[1:5].copy()
        for k in fc.FIELDS:
            assert np.array_equal(three[k][0], ref[k][0]), (fc.physics_id(p), k)
        for s in fc.SCHEDULES:
            if not fc.applies(p, s):
                continue
            got = fc.run(emu_harness, p, s)
            for name, (a, m) in got.items():
                if s[3]:
                    assert np.array_equal(a[m], gold[fc.key(p, True, name)][m]), (fc.physics_id(p), fc.schedule_id(s), name)
                elif name in fc.FIELDS:
                    assert np.array_equal(a, gold[fc.key(p, True, name)]), (fc.physics_id(p), fc.schedule_id(s), name)
                else:
                    assert np.array_equal(a[1:5], gold[fc.key(p, False, name)]), (fc.physics_id(p), fc.schedule_id(s), name)
        print(fc.physics_id(p), "ok")
    out = os.path.join(HERE, "flux_unused_polys_parent.npz")
    np.savez_compressed(out, **gold)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
