"""The one staleness rule and the one build step of every native artefact: the library and the drivers (__graft_entry__.build()), the
host emulations (tests/emu), the C++ programs (tests/cxx) and the syntax checks of the host headers.

The rule: an artefact is stale when it is missing, older than one of its own sources, or older than ANY header under the header roots
(pam_amd/csrc with host/**, and include/).  That is wider than what any one artefact includes, on purpose: there is no list to keep
and none to forget.  A program that links the library names the library among its sources.

The step: compile to <target>.<pid>.tmp beside the target and move it into place, so that another process never loads half a file and
a failed compile leaves the previous artefact where it was."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pam_amd", "csrc")
HOST = os.path.join(CSRC, "host")
INCLUDE = os.path.join(ROOT, "include")
HEADER_ROOTS = (CSRC, INCLUDE)
LIB = os.path.join(ROOT, "pam_amd", "libpam_amd_awfl.so")
LIB_SOURCES = [os.path.join(CSRC, f) for f in ("awfl_kernels.hip", "modules_kernels.hip")]
DRIVER_SOURCE = os.path.join(ROOT, "examples", "driver.cpp")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CXX_DIR = os.path.join(ROOT, "tests", "cxx")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def headers(header_roots=HEADER_ROOTS):
    """every *.h under the roots, recursively"""
    return [os.path.join(d, f) for root in header_roots for d, _, files in os.walk(root) for f in files if f.endswith(".h")]


def dependencies(sources, header_roots=HEADER_ROOTS):
    """what an artefact built from `sources` is compared with"""
    return list(sources) + headers(header_roots)


def stale(target, sources, header_roots=HEADER_ROOTS):
    if not os.path.exists(target):
        return True
    built = os.path.getmtime(target)
    return any(os.path.getmtime(d) > built for d in dependencies(sources, header_roots))


def build(target, sources, command, header_roots=HEADER_ROOTS, force=False):
    """run `command` + ["-o", <temporary>] if `target` is stale (or `force`), and move the result into place; returns `target`"""
    if force or stale(target, sources, header_roots):
        tmp = "%s.%d.tmp" % (target, os.getpid())
        try:
            subprocess.run(list(command) + ["-o", tmp], check=True)
            os.replace(tmp, target)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return target


def emu_sources():
    """every tests/emu/*_emu.cpp is a source of every emulation: one of them includes another (xsweep_pressure_emu.cpp: awfl_emu.cpp)"""
    return sorted(glob.glob(os.path.join(EMU_DIR, "*_emu.cpp")))


def emu_library(name, libs=()):
    """tests/emu/<name>.cpp -> tests/emu/lib<name>.so, the device bodies under g++ without contraction.  libs: libraries the source needs
    at link time (moist_surface_quad_emu: "quadmath", "pthread"), so that loading the result needs nothing loaded before it"""
    src = os.path.join(EMU_DIR, name + ".cpp")
    return build(os.path.join(EMU_DIR, "lib%s.so" % name), emu_sources(),
                 ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src] + ["-l" + x for x in libs])


def cxx_program(name):
    """tests/cxx/<name>.cpp -> tests/cxx/<name>, a program above the C ABI linked against the library"""
    src = os.path.join(CXX_DIR, name + ".cpp")
    return build(os.path.join(CXX_DIR, name), [src, LIB],
                 [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wno-unused-value", "-I" + INCLUDE, "-I" + HOST, src,
                  "-L" + os.path.join(ROOT, "pam_amd"), "-lpam_amd_awfl", "-Wl,-rpath,$ORIGIN/../../pam_amd"])


def syntax_check(path):
    """the CompletedProcess of hipcc -fsyntax-only on a translation unit that includes host headers"""
    return subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-Wno-unused-value", "-I" + INCLUDE, "-I" + HOST, str(path)],
                          capture_output=True, text=True)
