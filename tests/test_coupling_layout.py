"""CPU-only: where the arrays of the SHOC and the P3 coupling workspaces lie (pam_amd/csrc/coupling_workspace.h).

tests/cxx/coupling_layout.cpp, compiled here with g++ under the address and undefined-behaviour sanitizers, runs the carve function under
both zero-size policies and the two layers' tables at ragged shapes and checks every offset, the guards between the slots and the total
against the closed formulas of include/pam_amd_modules.h -- the layout decides what memory a handed-in shoc_main / p3_main may write."""
import os
import subprocess

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx", "coupling_layout.cpp")


def test_the_layout_arithmetic_holds_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "coupling_layout")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, _SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every check held" in r.stdout
