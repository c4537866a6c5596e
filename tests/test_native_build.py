"""tools/native_build.py: the one staleness rule and the one build step of every native artefact, on a temporary tree and on this one.
CPU only; nothing here needs the library."""
import glob
import os
import re
import subprocess
import sys
import time

import pytest

from tools import native_build as nb

ROOT = nb.ROOT
BASE = time.time() - 1000.0           # the age of the temporary trees' files: every time a test sets lies in the past
EMU_FLAGS = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"]
# the test-side files that build through the helper: the harnesses, the two case modules and the tests with a build of their own
ROUTED = sorted(glob.glob(os.path.join(ROOT, "tests", "*_emu_harness.py"))) + [os.path.join(ROOT, "tests", f + ".py") for f in (
    "emu_harness", "shoc_cases", "p3_cases", "test_diagnostics", "test_statistics_modules", "test_vertical_interp", "test_xsweep_pressure_emu",
    "test_validate", "test_kessler_emu", "moist_surface_cases", "test_physics_plugins", "test_coldiag", "test_fluxprof",
    "test_shoc_coupling_gpu", "test_p3_coupling_gpu", "test_p3_coupling", "test_shoc_coupling", "test_grayrad", "test_grayrad_sw", "test_sgs_smag",
    "test_sgs_moist", "test_surface")]


def _tree(tmp_path):
    """one source, one header root with one header, an output path; the files are as old as BASE"""
    inc = tmp_path / "inc"
    inc.mkdir()
    hdr, src, out = inc / "seven.h", tmp_path / "seven.cpp", tmp_path / "libseven.so"
    hdr.write_text("#define SEVEN 7\n")
    src.write_text('#include "seven.h"\nextern "C" int seven() { return SEVEN; }\n')
    for f in (hdr, src):
        os.utime(f, (BASE, BASE))
    return hdr, src, str(out), dict(sources=[str(src)], command=EMU_FLAGS + ["-I" + str(inc), str(src)], header_roots=[str(inc)])


def _stamp(path):
    st = os.stat(path)
    return st.st_ino, st.st_mtime_ns


def _move_past(path, out, step):
    """`path` 50 s past the output, both in the past and later than every earlier step; returns the output's stamp"""
    t = BASE + 100.0 * step
    os.utime(out, (t, t))
    os.utime(path, (t + 50.0, t + 50.0))
    return _stamp(out)


def test_the_rule_on_a_temporary_tree(tmp_path):
    hdr, src, out, kw = _tree(tmp_path)
    assert nb.stale(out, kw["sources"], kw["header_roots"])
    assert nb.build(out, **kw) == out and os.path.exists(out)                  # missing: it compiles
    first = _stamp(out)
    nb.build(out, **kw)
    assert _stamp(out) == first                                                # fresh: it does not
    aged = _move_past(hdr, out, 1)
    nb.build(out, **kw)
    assert _stamp(out) != aged and not nb.stale(out, kw["sources"], kw["header_roots"])    # a header past the output: it compiles again
    aged = _move_past(src, out, 2)
    nb.build(out, **kw)
    assert _stamp(out) != aged and not nb.stale(out, kw["sources"], kw["header_roots"])    # and so after its source
    src.write_text('#include "seven.h"\nextern "C" int seven() { return SEVEN }\n')
    aged = _move_past(src, out, 3)
    with pytest.raises(subprocess.CalledProcessError):
        nb.build(out, **kw)
    assert _stamp(out) == aged and glob.glob(str(tmp_path / "*.tmp")) == []    # a failed compile: the earlier output, no temporary file


def test_a_header_below_a_root_counts(tmp_path):
    """the roots are walked: pam_amd/csrc/host/** is under pam_amd/csrc"""
    hdr, src, out, kw = _tree(tmp_path)
    deep = tmp_path / "inc" / "a" / "b"
    deep.mkdir(parents=True)
    (deep / "deep.h").write_text("\n")
    nb.build(out, **kw)
    aged = _move_past(deep / "deep.h", out, 1)
    nb.build(out, **kw)
    assert _stamp(out) != aged
    assert os.path.join(nb.HOST, "pam_coupler.h") in nb.headers() and os.path.join(nb.INCLUDE, "pam_amd_awfl.h") in nb.headers()


def test_two_builders_at_once_both_load_the_library(tmp_path):
    hdr, src, out, kw = _tree(tmp_path)
    code = ("import ctypes, sys\nsys.path.insert(0, %r)\nfrom tools import native_build as nb\n"
            "sys.stdin.readline()\n"                                           # both wait here, then start together
            "lib = ctypes.CDLL(nb.build(%r, **%r))\nassert lib.seven() == 7\nprint('seven')\n" % (ROOT, out, kw))
    procs = [subprocess.Popen([sys.executable, "-c", code], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for _ in range(2)]
    for p in procs:
        p.stdin.write("\n")
        p.stdin.flush()
    for p in procs:
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0 and so.strip() == "seven", se[-2000:]
    assert glob.glob(str(tmp_path / "*.tmp")) == []


def test_the_rule_covers_what_the_compiler_sees():
    """every file g++ -MM names for an emulation is one the rule compares it with: a header under the roots or an emulation source"""
    sources = nb.emu_sources()
    assert len(sources) >= 22
    covered = {os.path.realpath(d) for d in nb.dependencies(sources)}
    for src in sources:
        r = subprocess.run(["g++", "-std=c++17", "-MM", src], capture_output=True, text=True, cwd=nb.EMU_DIR)
        assert r.returncode == 0, r.stderr[-2000:]
        seen = r.stdout.split(":", 1)[1].replace("\\\n", " ").split()
        missed = [d for d in seen if os.path.realpath(os.path.join(nb.EMU_DIR, d)) not in covered]
        assert len(seen) >= 2 and not missed, (src, missed)


def test_nothing_builds_beside_the_helper():
    assert len(ROUTED) == 33
    for path in ROUTED:
        text = open(path).read()
        assert "getmtime" not in text and '"g++"' not in text and "HIPCC" not in text and "--offload-arch" not in text, path
        assert re.search(r"^from tools(\.native_build)? import ", text, flags=re.M), path


def test_gen_constants_is_idempotent():
    """the committed headers are the generator's own output: a run leaves their bytes and their mtimes as they are"""
    targets = [os.path.join(nb.CSRC, "awfl_constants.h"), os.path.join(ROOT, "oracle", "awfl_constants.h")]
    before = [(open(t, "rb").read(), os.stat(t).st_mtime_ns) for t in targets]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_constants.py")], check=True)
    assert [(open(t, "rb").read(), os.stat(t).st_mtime_ns) for t in targets] == before
