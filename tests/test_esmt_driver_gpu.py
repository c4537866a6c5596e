"""examples/driver --esmt [KMAX] on the reference's CI input (65 x 1 x 50, one member: an odd nx, no Nyquist wavenumber), run the way
tests/test_reference_ci_run.py runs the driver: a handful of CRM steps with and without the flag."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
YAML = os.path.join(ROOT, "tests", "golden", "ci_input_pama.yaml")
NX, NY, NZ = 65, 1, 50
STEPS = 12                        # dt_crm_phys is 20 s and out_freq 200 s: one output step
ESMT_LINE = r"esmt: etime (\S+) , u_s (\S+) , v_s (\S+) , max_T_dt (\S+)"

pytestmark = pytest.mark.gpu


def _run(tmp_path, tag, *opts):
    assert os.path.exists(DRIVER), "examples/driver missing: run __graft_entry__.build()"
    outp = str(tmp_path / ("out_%s.bin" % tag))
    r = subprocess.run([DRIVER, "--yaml", YAML, "--steps", str(STEPS)] + list(opts) + [outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (tag, r.stderr[-2000:])
    return r.stdout.strip().split("\n"), np.fromfile(outp, dtype="<f8")


def test_driver_esmt_prints_its_line_and_changes_no_other(tmp_path):
    """--esmt and --esmt 0 exit with 0 and print one finite "esmt:" line per output step; every other line of the output is that of
    the run without the flag, and so are the eight fields and precl of the output file; with every wavenumber the force is there, with
    KMAX = 0 it is not, and the scalars' domain means are the CRM's own mean wind at the start and stay near it"""
    ncell = NZ * NY * NX
    plain, raw = _run(tmp_path, "plain")
    assert not any(l.startswith("esmt:") for l in plain)
    assert raw.size == 8 * ncell + NY * NX
    means = {}
    for tag, opts in (("all", ["--esmt"]), ("none", ["--esmt", "0"]), ("three", ["--esmt", "3"])):
        lines, got = _run(tmp_path, tag, *opts)
        rows = [re.fullmatch(ESMT_LINE, l) for l in lines if l.startswith("esmt:")]
        assert rows and all(rows) and len(rows) == sum(l.startswith("Etime ,") for l in lines) == 1, tag
        vals = [float(rows[0].group(i)) for i in (1, 2, 3, 4)]
        assert np.isfinite(vals).all(), (tag, vals)
        assert [l for l in lines if not l.startswith("esmt:")] == plain, tag
        assert got.size == 10 * ncell + NY * NX
        assert np.array_equal(got[:8 * ncell].view(np.uint64), raw[:8 * ncell].view(np.uint64)), tag
        assert np.array_equal(got[10 * ncell:].view(np.uint64), raw[8 * ncell:].view(np.uint64)), tag
        assert np.isfinite(got).all()
        means[tag] = vals
    assert means["none"][3] == 0.0 and means["all"][3] > 0.0 and means["three"][3] > 0.0
    uvel = raw[ncell:2 * ncell]
    assert abs(means["all"][1] - uvel.mean()) < 1.0           # the supercell sounding's wind spans tens of m/s; the scalars began at its level means

