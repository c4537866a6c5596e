"""pam::VerticalInterp<ord> on the GPU (pam_amd/csrc/modules_kernels.hip: vertical_interp_member_kernel, vertical_interp_shared_kernel)
against the CPU restatement (tests/vertical_interp_ref.py), bit for bit: only + - * / occur and contraction is off in the shared
bodies (pam_amd/csrc/vertical_interp_device.h), so any difference is a mistake.  The inputs are those of tests/test_vertical_interp.py.
The sizes that select the `long long` instances: tests/test_vertical_interp_wide_index.py."""
import os
import subprocess

import numpy as np
import pytest

import test_vertical_interp as tv
import vertical_interp_ref as ref
from pam_amd import idealized as idz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "driver")
CI_YAML = os.path.join(ROOT, "tests", "golden", "ci_input_pama.yaml")
NENS = [1, 3, 64, 65, 130]

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _interp(ord, zint):
    import pam_amd
    v = pam_amd.VerticalInterp(ord)
    v.init(_dev(zint))
    return v


def _edges(v, data, bl, bu):
    """through a NaN-filled output, so that an element the kernel does not write shows"""
    import torch
    out = torch.full((data.shape[0] + 1,) + tuple(data.shape[1:]), float("nan"), dtype=torch.float64, device="cuda:0")
    return _host(v.cells_to_edges(_dev(data), bl, bu, out=out))


def _check_tables(v, zint, ord, shared):
    lo, hi = ref.tables(zint, ord)
    glo, ghi, gshared = v.tables()
    assert gshared == shared
    if shared:
        lo, hi = lo[..., :1], hi[..., :1]
    assert tv.same_bits(_host(glo), lo) and tv.same_bits(_host(ghi), hi)
    return lo, hi


@pytest.mark.parametrize("nens", NENS)
@pytest.mark.parametrize("kind", tv.GRIDS)
@pytest.mark.parametrize("nz", tv.NZS)
@pytest.mark.parametrize("ord", tv.ORDERS)
def test_gpu_tables_and_edges_match_restatement_bit_for_bit(ord, nz, kind, nens):
    """the tables, then the edges of a 1 x 65 and a 1 x 1 field of mixed sign and magnitude for all four boundary pairs; identical
    columns select the shared table (lanes along the flattened (column, member) index), per-member columns the member kernel"""
    zint = tv.grid(kind, nz, nens)
    v = _interp(ord, zint)
    lo, hi = _check_tables(v, zint, ord, shared=(kind != "stretched" or nens == 1))
    for ny, nx in ((1, 65), (1, 1)):
        data = tv.mixed_field((nz, ny, nx, nens), seed=1000 * ord + 10 * nz + nens + nx)
        for bl, bu in tv.BCS:
            assert tv.same_bits(_edges(v, data, bl, bu), ref.cells_to_edges(data, lo, hi, ord, bl, bu)), (ny, nx, bl, bu)
    v.finalize()


@pytest.mark.parametrize("nens", [3, 65, 130])
@pytest.mark.parametrize("kind", tv.GRIDS)
@pytest.mark.parametrize("ord", tv.ORDERS)
def test_gpu_32x32_columns_match_restatement_bit_for_bit(ord, kind, nens):
    """60 levels, 32 x 32 columns: several column groups per member block, the last member block ragged (nens 3, 65, 130)"""
    nz = 60
    zint = tv.grid(kind, nz, nens, seed=7)
    v = _interp(ord, zint)
    lo, hi = _check_tables(v, zint, ord, shared=(kind != "stretched"))
    data = tv.mixed_field((nz, 32, 32, nens), seed=ord + nens)
    bl, bu = tv.BCS[(ord + nens) % 4]
    assert tv.same_bits(_edges(v, data, bl, bu), ref.cells_to_edges(data, lo, hi, ord, bl, bu))
    v.finalize()


@pytest.mark.parametrize("nens", NENS)
@pytest.mark.parametrize("ord", tv.ORDERS)
def test_gpu_7_levels_of_32x32_columns_match_restatement(ord, nens):
    zint = tv.grid("stretched", 7, nens, seed=3)
    v = _interp(ord, zint)
    lo, hi = ref.tables(zint, ord)
    data = tv.mixed_field((7, 32, 32, nens), seed=5 * ord + nens)
    for bl, bu in tv.BCS:
        assert tv.same_bits(_edges(v, data, bl, bu), ref.cells_to_edges(data, lo, hi, ord, bl, bu)), (bl, bu)
    v.finalize()


def _supercell_temp(nens, nx, ny, zint):
    f = idz.supercell_fields(nens, nx, ny, len(zint) - 1, zint, tracers=idz.TRACERS_KESSLER_SHOC, magnitude=0.5)
    return np.ascontiguousarray(f["temp"])


@pytest.mark.parametrize("ord", tv.ORDERS)
def test_gpu_state_like_field_and_forced_per_member_tables(ord):
    """the supercell's perturbed temperature on the L60 grid: the shared-table run equals the restatement, and a forced per-member run
    on the same (identical) columns equals the shared-table run bit for bit -- both kernels, one answer"""
    nens, ny, nx = 65, 6, 9
    z = idz.l60_interfaces()
    zint = tv.grid("l60", 60, nens)
    temp = _supercell_temp(nens, nx, ny, z)
    mixed = tv.mixed_field(temp.shape, seed=ord)
    v = _interp(ord, zint)
    lo, hi = ref.tables(zint, ord)
    assert v.shared_table
    shared = {(n, bc): _edges(v, d, *bc) for n, d in (("temp", temp), ("mixed", mixed)) for bc in tv.BCS}
    for (n, bc), got in shared.items():
        assert tv.same_bits(got, ref.cells_to_edges({"temp": temp, "mixed": mixed}[n], lo, hi, ord, *bc)), (n, bc)
    assert 150 < shared[("temp", (0, 0))].min() and shared[("temp", (0, 0))].max() < 350
    v.set_table_sharing(False)
    glo, ghi, gshared = v.tables()
    assert not gshared and tv.same_bits(_host(glo), lo) and tv.same_bits(_host(ghi), hi)
    for (n, bc), want in shared.items():
        assert tv.same_bits(_edges(v, {"temp": temp, "mixed": mixed}[n], *bc), want), (n, bc)
    v.set_table_sharing(True)
    assert v.shared_table and tv.same_bits(_edges(v, temp, 0, 1), shared[("temp", (0, 1))])
    v.finalize()


def test_gpu_sharing_is_refused_where_the_columns_differ():
    from pam_amd import capi
    v = _interp(5, tv.grid("stretched", 7, 3))
    assert not v.shared_table
    with pytest.raises(capi.PamAmdError, match="vertical_interp_set_table_sharing"):
        v.set_table_sharing(True)
    v.finalize()


def test_gpu_init_refuses_columns_that_are_not_increasing():
    import pam_amd
    from pam_amd import capi
    z = tv.grid("stretched", 7, 5)
    for bad in (np.where(np.arange(8)[:, None] * np.ones((1, 5)) == 3, np.nan, z), z[::-1].copy()):
        with pytest.raises(capi.PamAmdError, match="vertical_interp_init"):
            pam_amd.VerticalInterp(5).init(_dev(bad))
    z[4, 2] = z[3, 2]
    with pytest.raises(capi.PamAmdError, match="member 2"):
        pam_amd.VerticalInterp(3).init(_dev(z))


@pytest.mark.parametrize("kind", ["l60", "stretched"])
@pytest.mark.parametrize("ord", tv.ORDERS)
def test_gpu_whole_ensemble_equals_member_chunks(ord, kind):
    n1, n2 = 37, 93
    zint = tv.grid(kind, 60, n1 + n2)
    data = tv.mixed_field((60, 5, 13, n1 + n2), seed=11 * ord)

    def run(sl):
        v = _interp(ord, zint[:, sl])
        out = _edges(v, data[..., sl], 0, 1)
        v.finalize()
        return out

    whole = run(slice(None))
    assert tv.same_bits(np.concatenate([run(slice(0, n1)), run(slice(n1, None))], axis=-1), whole)


@pytest.mark.parametrize("kind", ["l60", "stretched"])
def test_gpu_non_default_stream_equals_default_stream(kind):
    import torch
    import pam_amd
    nens = 65
    zint = tv.grid(kind, 60, nens)
    data = tv.mixed_field((60, 4, 8, nens), seed=2)
    v = _interp(5, zint)
    want = _edges(v, data, 1, 0)
    v.finalize()
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        v2 = pam_amd.VerticalInterp(5)
        v2.init(_dev(zint))
        d = _dev(data)
        got = v2.cells_to_edges(d, 1, 0)
    s.synchronize()
    assert tv.same_bits(_host(got), want)
    v2.finalize()


def test_gpu_python_mirror_and_driver_edges_give_the_same_bits(tmp_path):
    """examples/driver --yaml ... --edges writes `temp` on the interfaces (the C++ adaptor pam::VerticalInterp<5>, zero gradient at both
    ends); the same field through pam_amd.VerticalInterp and through the restatement gives the same bits"""
    out, e = tmp_path / "out.bin", tmp_path / "edges.bin"
    nens, nz, ny, nx = 3, 50, 1, 65
    r = subprocess.run([DRIVER, "--yaml", CI_YAML, "--nens", str(nens), "--steps", "1", "--edges", str(e), str(out)], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    ncell = nz * ny * nx * nens
    temp = np.fromfile(out, dtype=np.float64)[4 * ncell:5 * ncell].reshape(nz, ny, nx, nens)
    edges = np.fromfile(e, dtype=np.float64)
    assert edges.size == (nz + 1) * ny * nx * nens
    edges = edges.reshape(nz + 1, ny, nx, nens)
    zint = np.repeat(np.array([20.0 * 1000.0 * k / nz for k in range(nz + 1)]).reshape(-1, 1), nens, axis=1)
    v = _interp(5, zint)
    assert tv.same_bits(_edges(v, temp, 0, 0), edges)
    assert tv.same_bits(ref.interp(temp, zint, 5, 0, 0), edges)
    v.finalize()
    # and without --edges the run's own output is unchanged
    plain = tmp_path / "plain.bin"
    r2 = subprocess.run([DRIVER, "--yaml", CI_YAML, "--nens", str(nens), "--steps", "1", str(plain)], capture_output=True, text=True,
                        timeout=900)
    assert r2.returncode == 0 and plain.read_bytes() == out.read_bytes() and r2.stdout.strip().split("\n")[-1] == r.stdout.strip().split("\n")[-1]
