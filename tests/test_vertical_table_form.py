"""CPU-only: the factored upper polynomial of the stored vertical WENO table (awfl_device.h: VTable, make_vtable).

tests/emu/vtable_check.cpp, compiled here with g++, builds the tables of a grid with build_vertical_tables (awfl_vertical.h) and, on
random stencils of every level (and member), compares the factored blended TV (a sum of four squares from the Cholesky rows), the even
part e3 and the odd part o3 with the same quantities formed from h1..h4 of the level's DTable, and the whole polynomial (weno5_table)
with the unfactored evaluation.  Every pivot of every level must be positive."""
import os
import subprocess

import numpy as np
import pytest

from pam_amd import idealized as idz

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "vtable_check.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vtable") / "vtable_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, _SRC], check=True)
    return exe


def _run(checker, tmp_path, dz, nsamples=1500, seed=7):
    nz, nens = dz.shape
    grid = tmp_path / "grid.txt"
    grid.write_text("%d %d\n" % (nz, nens) + "\n".join("%.17g" % x for x in dz.ravel()))
    out = subprocess.run([checker, str(grid), str(nsamples), str(seed)], capture_output=True, text=True, check=True).stdout
    return {k: float(v) for k, v in (kv.split("=") for kv in out.split())}


def _per_member_grids(nz=40, nens=5, seed=3):
    rng = np.random.default_rng(seed)
    cols = [np.diff(idz.stretched_interfaces(nz, 12000.0, 1.0 + 0.08 * rng.random())) * (1.0 + 0.3 * rng.random(nz))
            for _ in range(nens)]
    return np.stack(cols, axis=1)


GRIDS = {
    "L60": lambda: np.diff(idz.l60_interfaces())[:, None],
    "uniform": lambda: np.diff(idz.uniform_interfaces(60, 20000.0))[:, None],
    "per_member_stretched": _per_member_grids,
}


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_factored_upper_polynomial_reproduces_the_unfactored_one(checker, tmp_path, grid):
    dz = GRIDS[grid]()
    r = _run(checker, tmp_path, dz)
    assert r["per_ens"] == (1.0 if dz.shape[1] > 1 else 0.0)
    assert r["samples"] > 0
    assert r["pivots_ok"] == 1.0 and r["min_pivot"] > 0.0
    assert r["err_tvb"] <= 1e-14, r      # relative to the blended TV (a positive form)
    assert r["err_e3"] <= 1e-14, r       # relative to the sum of the magnitudes of its terms
    assert r["err_o3"] <= 1e-14, r
    assert r["err_lr"] <= 1e-14, r       # edge values, relative to max |u| of the stencil
