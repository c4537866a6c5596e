"""pam::VerticalInterp<ord> (pam_core/vertical_interp.h), orders 3 and 5, without a GPU: the CPU restatement
(tests/vertical_interp_ref.py) against mathematics; the host emulation of the device bodies (pam_amd/csrc/vertical_interp_device.h
under g++) against the restatement bit for bit; the uniform-grid matrices against the reference's recorded constants; the C ABI's
argument checks; the C++ adaptor against the work-alike.  The GPU tests are in tests/test_vertical_interp_gpu.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import vertical_interp_ref as ref
from pam_amd import capi
from pam_amd import idealized as idz
from tools.native_build import emu_library, syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
_DP = C.POINTER(C.c_double)

ORDERS = [3, 5]
BCS = [(0, 0), (0, 1), (1, 0), (1, 1)]
BC_IDS = ["grad_grad", "grad_value", "value_grad", "value_value"]
NZS = [1, 2, 3, 7, 60]
GRIDS = ["uniform", "l60", "stretched"]


# ------------------------------------------------------------------------------------------------------------------------------
# inputs, shared with the GPU tests

def grid(kind, nz, nens, seed=0):
    """(nz+1, nens) interfaces.  uniform: 20 km in nz cells, every member alike; l60: the first nz cells of the L60 interfaces, every
    member alike; stretched: every member its own randomly stretched column"""
    if kind == "uniform":
        z = idz.uniform_interfaces(nz, 20000.0)
    elif kind == "l60":
        z = idz.l60_interfaces()[:nz + 1]
    elif kind == "stretched":
        rng = np.random.default_rng(1000 + 10 * nz + seed)
        dz = rng.uniform(40.0, 400.0, (nz, nens)) * np.exp(np.linspace(0.0, 2.5, nz))[:, None] ** rng.uniform(0.0, 1.0, (1, nens))
        return np.ascontiguousarray(np.concatenate([np.zeros((1, nens)), np.cumsum(dz, axis=0)]))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.repeat(np.asarray(z, dtype=np.float64).reshape(nz + 1, 1), nens, axis=1))


def mixed_field(shape, seed):
    """values of mixed sign and magnitude (10^-3 .. 10^3): every candidate polynomial gets weight somewhere"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def cell_averages(coefs, z):
    """exact cell averages of sum_m coefs[m] z^m between consecutive interfaces z"""
    out = 0.0
    for m, c in enumerate(coefs):
        out = out + c * (z[1:] ** (m + 1) - z[:-1] ** (m + 1)) / ((m + 1) * (z[1:] - z[:-1]))
    return out


def column(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1, 1, 1, 1))


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement against mathematics

@pytest.mark.parametrize("ord,coefs,measured", [(3, (280.0, -6.5e-3), "1.2e-15"), (5, (280.0, -6.5e-3, 1.1e-7), "2.9e-15")], ids=["ord3", "ord5"])
def test_restatement_is_exact_for_polynomials_on_the_l60_grid(ord, coefs, measured):
    """cell averages of a polynomial the scheme's smooth-data limit reproduces: interfaces hs+1 .. nz-hs-1 equal the polynomial to
    1e-13 of its maximum (measured: see the parameters); with zero gradient at both ends the end interfaces are the end cells"""
    z = idz.l60_interfaces()
    nz, hs = len(z) - 1, (ord - 1) // 2
    d = column(cell_averages(coefs, z))
    e = ref.interp(d, z.reshape(-1, 1), ord, ref.BC_ZERO_GRADIENT, ref.BC_ZERO_GRADIENT)[:, 0, 0, 0]
    exact = sum(c * z ** m for m, c in enumerate(coefs))
    err = np.abs(e - exact)[hs + 1:nz - hs].max() / np.abs(exact).max()
    print("order %d: interior error %.3g of the maximum (recorded: %s)" % (ord, err, measured))
    assert err <= 1e-13
    assert e[0] == d[0, 0, 0, 0] and e[nz] == d[nz - 1, 0, 0, 0]


def test_restatement_converges_at_fifth_order():
    """cell averages of sin(2 pi z - pi/10) on 16, 32, 64 uniform cells of [0,1]: observed order of the maximum interior-interface
    error >= 5.0 at both refinements (measured 5.91 and 5.96: the two one-sided samples average to a centred estimate)"""
    errs = []
    for n in (16, 32, 64):
        z = np.linspace(0.0, 1.0, n + 1)
        prim = -np.cos(2 * np.pi * z - np.pi / 10) / (2 * np.pi)
        d = column((prim[1:] - prim[:-1]) / (z[1:] - z[:-1]))
        e = ref.interp(d, z.reshape(-1, 1), 5)[:, 0, 0, 0]
        errs.append(np.abs(e - np.sin(2 * np.pi * z - np.pi / 10))[3:n - 2].max())
    orders = [np.log2(errs[0] / errs[1]), np.log2(errs[1] / errs[2])]
    print("errors %s, observed orders %s" % (errs, orders))
    assert orders[0] >= 5.0 and orders[1] >= 5.0


@pytest.mark.parametrize("ord", ORDERS)
def test_restatement_keeps_a_step_within_its_bounds(ord):
    """ten 0s then ten 1s on a uniform grid: every interface within [-1e-12, 1 + 1e-12] (measured minimum -5e-19)"""
    z = np.linspace(0.0, 20.0, 21)
    e = ref.interp(column(np.r_[np.zeros(10), np.ones(10)]), z.reshape(-1, 1), ord)
    print("order %d: min %.3g, max - 1 %.3g" % (ord, e.min(), e.max() - 1))
    assert e.min() >= -1e-12 and e.max() <= 1 + 1e-12


@pytest.mark.parametrize("ord", ORDERS)
def test_restatement_zero_value_ends_are_zero(ord):
    z = idz.l60_interfaces()
    d = column(cell_averages((280.0, -6.5e-3), z)) + 1.0
    e = ref.interp(d, z.reshape(-1, 1), ord, ref.BC_ZERO_VALUE, ref.BC_ZERO_VALUE)[:, 0, 0, 0]
    assert e[0] == 0.0 and e[-1] == 0.0 and np.all(e[1:-1] != 0.0)


def test_restatement_refuses_what_the_c_abi_refuses():
    z = grid("uniform", 4, 2)
    for ord in (1, 7, 9):
        with pytest.raises(ValueError):
            ref.tables(z, ord)
    bad = z.copy()
    bad[2, 1] = bad[1, 1]
    for zz in (bad, np.where(z == z[3, 0], np.nan, z), z[:1]):
        with pytest.raises(ValueError):
            ref.tables(zz, 5)
    lo, hi = ref.tables(z, 5)
    with pytest.raises(ValueError):
        ref.cells_to_edges(np.zeros((4, 1, 1, 2)), lo, hi, 5, 0, 2)


def test_uniform_grid_tables_are_the_reference_constants():
    """an interior level of a uniform grid: recon_hi = sten_to_coefs<5,5>, recon_lo = weno_lower_sten_to_coefs<3,3,3> as recorded from
    the reference's generated constants.  Tolerance: SURVEY.md Appendix B measured this comparison at 1.33e-15 / 8.9e-16 absolute for a
    Gauss-Jordan inverse; a factor 4 over it"""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_extract.json")))["constants"]["matrices"]
    z = (100.0 * np.arange(13)).reshape(-1, 1)
    lo, hi = ref.tables(z, 5)
    dhi = np.abs(hi[6, :, :, 0] - np.array(rec["sten_to_coefs_5x5"])).max()
    dlo = np.abs(lo[6, :, :, :, 0] - np.array(rec["weno_lower_sten_to_coefs_3x3x3"])).max()
    print("recon_hi %.3g, recon_lo %.3g" % (dhi, dlo))
    assert dhi <= 4 * 1.33e-15 and dlo <= 4 * 8.9e-16
    for k in range(12):      # the ghost interfaces continue the uniform grid: every level has the interior level's matrices
        assert np.abs(hi[k] - hi[6]).max() <= 4 * 1.33e-15 and np.abs(lo[k] - lo[6]).max() <= 4 * 8.9e-16


# ------------------------------------------------------------------------------------------------------------------------------
# the host emulation of the device bodies

def emu():
    lib = C.CDLL(emu_library("vertical_interp_emu"))
    lib.emu_vertical_interp_tables.argtypes = [C.c_int] * 3 + [_DP] * 3
    lib.emu_vertical_interp_cells_to_edges.argtypes = [C.c_int] * 5 + [_DP] * 3 + [C.c_int] * 2 + [_DP]
    return lib


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


def emu_tables(lib, zint, ord):
    nz, nens, n = zint.shape[0] - 1, zint.shape[1], (ord - 1) // 2 + 1
    lo, hi = np.empty((nz, n, n, n, nens)), np.empty((nz, ord, ord, nens))
    assert lib.emu_vertical_interp_tables(ord, nz, nens, _p(zint), _p(lo), _p(hi)) == 0
    return lo, hi


def emu_cells_to_edges(lib, data, lo, hi, ord, bc_lower, bc_upper):
    nz, ny, nx, nens = data.shape
    out = np.full((nz + 1, ny, nx, nens), np.nan)
    assert lib.emu_vertical_interp_cells_to_edges(ord, nz, ny * nx, nens, lo.shape[-1], _p(data), _p(np.ascontiguousarray(lo)),
                                                  _p(np.ascontiguousarray(hi)), bc_lower, bc_upper, _p(out)) == 0
    return out


@pytest.mark.parametrize("kind", GRIDS)
@pytest.mark.parametrize("nz", NZS)
@pytest.mark.parametrize("ord", ORDERS)
def test_emulation_matches_restatement_bit_for_bit(ord, nz, kind):
    """tables and edges, all four boundary pairs, nz below hs included, data of mixed sign and magnitude: only + - * / occur and
    contraction is off, so any difference is an operation-order mistake"""
    lib = emu()
    nens = 5
    zint = grid(kind, nz, nens)
    lo, hi = ref.tables(zint, ord)
    elo, ehi = emu_tables(lib, zint, ord)
    assert same_bits(elo, lo) and same_bits(ehi, hi)
    data = mixed_field((nz, 2, 3, nens), seed=100 * ord + nz)
    for bl, bu in BCS:
        want = ref.cells_to_edges(data, lo, hi, ord, bl, bu)
        assert np.all(np.isfinite(want))
        assert same_bits(emu_cells_to_edges(lib, data, elo, ehi, ord, bl, bu), want), (bl, bu)
    # one shared table (the members' columns are identical) == the same table repeated per member
    if kind != "stretched":
        got = emu_cells_to_edges(lib, data, elo[..., :1], ehi[..., :1], ord, 0, 1)
        assert same_bits(got, ref.cells_to_edges(data, lo, hi, ord, 0, 1))
        assert same_bits(got, ref.cells_to_edges(data, lo[..., :1], hi[..., :1], ord, 0, 1))


def test_emulation_refuses_bad_orders_and_columns():
    lib = emu()
    z = grid("uniform", 4, 2)
    lo, hi = np.empty((4, 3, 3, 3, 2)), np.empty((4, 5, 5, 2))
    assert lib.emu_vertical_interp_tables(7, 4, 2, _p(z), _p(lo), _p(hi)) == -1
    bad = z.copy()
    bad[2, 1] = bad[1, 1]
    assert lib.emu_vertical_interp_tables(5, 4, 2, _p(bad), _p(lo), _p(hi)) == -1


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI

NEW_SYMBOLS = ("pam_amd_vertical_interp_init", "pam_amd_vertical_interp_cells_to_edges", "pam_amd_vertical_interp_tables",
               "pam_amd_vertical_interp_set_table_sharing", "pam_amd_vertical_interp_finalize")


def test_new_entry_points_are_exported_and_declared():
    import re
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    assert lib.pam_amd_awfl_abi_version() == 5


def test_new_entry_points_reject_bad_arguments_before_touching_a_device():
    lib = capi.load()
    init, c2e = lib.pam_amd_vertical_interp_init, lib.pam_amd_vertical_interp_cells_to_edges
    tables, share = lib.pam_amd_vertical_interp_tables, lib.pam_amd_vertical_interp_set_table_sharing
    h = C.c_void_p()
    fake = C.create_string_buffer(256)            # not a handle: no magic number; read, never written
    hp = C.cast(fake, C.c_void_p)
    lo, hi, sh = C.c_void_p(), C.c_void_p(), C.c_int()
    Z, D, E = 64, 128, 256                          # "device pointers": never dereferenced, validation fails first
    cases = [
        ("vertical_interp_init", lambda: init(7, 4, 2, Z, None, C.byref(h))),
        ("vertical_interp_init", lambda: init(9, 4, 2, Z, None, C.byref(h))),
        ("vertical_interp_init", lambda: init(1, 4, 2, Z, None, C.byref(h))),
        ("vertical_interp_init", lambda: init(4, 4, 2, Z, None, C.byref(h))),
        ("vertical_interp_init", lambda: init(5, 0, 2, Z, None, C.byref(h))),
        ("vertical_interp_init", lambda: init(5, 4, 0, Z, None, C.byref(h))),
        ("vertical_interp_init", lambda: init(5, 4, 2, None, None, C.byref(h))),
        ("vertical_interp_init", lambda: init(5, 4, 2, Z, None, None)),
        ("vertical_interp_cells_to_edges", lambda: c2e(None, 2, 3, D, 0, 0, E, None)),
        ("vertical_interp_cells_to_edges", lambda: c2e(hp, 0, 3, D, 0, 0, E, None)),
        ("vertical_interp_cells_to_edges", lambda: c2e(hp, 2, 0, D, 0, 0, E, None)),
        ("vertical_interp_cells_to_edges", lambda: c2e(hp, 2, 3, None, 0, 0, E, None)),
        ("vertical_interp_cells_to_edges", lambda: c2e(hp, 2, 3, D, 0, 0, None, None)),
        ("vertical_interp_cells_to_edges", lambda: c2e(hp, 2, 3, D, 0, 0, D, None)),
        ("vertical_interp_cells_to_edges", lambda: c2e(hp, 2, 3, D, 2, 0, E, None)),
        ("vertical_interp_cells_to_edges", lambda: c2e(hp, 2, 3, D, 0, -1, E, None)),
        ("vertical_interp_cells_to_edges", lambda: c2e(hp, 2, 3, D, 0, 0, E, None)),          # not a handle
        ("vertical_interp_tables", lambda: tables(None, C.byref(lo), C.byref(hi), C.byref(sh))),
        ("vertical_interp_tables", lambda: tables(hp, C.byref(lo), C.byref(hi), C.byref(sh))),
        ("vertical_interp_set_table_sharing", lambda: share(None, 0, None)),
        ("vertical_interp_set_table_sharing", lambda: share(hp, 1, None)),
        ("vertical_interp_finalize", lambda: lib.pam_amd_vertical_interp_finalize(hp)),
    ]
    for who, call in cases:
        assert call() == -1, who                                   # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert who.encode() in lib.pam_amd_awfl_last_error(), who
        assert not h.value
    assert lib.pam_amd_vertical_interp_finalize(None) == 0


def test_python_mirror_refuses_orders_7_and_9():
    import pam_amd
    for ord in (1, 7, 9):
        with pytest.raises(capi.PamAmdError):
            pam_amd.VerticalInterp(ord)
    v = pam_amd.VerticalInterp(5)
    assert (v.hs, v.BC_ZERO_GRADIENT, v.BC_ZERO_VALUE) == (2, 0, 1) and pam_amd.VerticalInterp(3).hs == 1
    with pytest.raises(capi.PamAmdError):
        v.tables()


# ------------------------------------------------------------------------------------------------------------------------------
# the C++ adaptor

ADAPTOR = os.path.join(HOST, "vertical_interp.h")


def _compile(tmp_path, body):
    src = tmp_path / "use.cpp"
    src.write_text('#include "vertical_interp.h"\n' + body)
    return syntax_check(src)


def test_adaptor_compiles_against_the_workalike(tmp_path):
    r = _compile(tmp_path, """
template <unsigned int ord> real4d use(realConst2d zint, realConst4d data) {
  static pam::VerticalInterp<ord> v;
  static_assert(pam::VerticalInterp<ord>::hs == (ord - 1) / 2, "hs");
  static_assert(pam::VerticalInterp<ord>::BC_ZERO_GRADIENT == 0 && pam::VerticalInterp<ord>::BC_ZERO_VALUE == 1, "bc");
  v.init(zint);
  pam::VerticalInterp<ord> const &c = v;
  return c.cells_to_edges(data, v.BC_ZERO_GRADIENT, v.BC_ZERO_VALUE);
}
template real4d use<3>(realConst2d, realConst4d);
template real4d use<5>(realConst2d, realConst4d);
real1d a; real2d b; real3d c3; realConst3d d3;
""")
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("ord", [7, 9])
def test_adaptor_refuses_orders_7_and_9_at_compile_time(tmp_path, ord):
    r = _compile(tmp_path, "pam::VerticalInterp<%d> v;\n" % ord)
    assert r.returncode != 0 and "orders 3 and 5 only" in r.stderr


def test_adaptor_has_the_reference_members():
    import test_boundary_surface as tb
    text = tb._norm(tb._strip_comments(open(ADAPTOR).read()))
    for sig in ("template <unsigned int ord> class VerticalInterp {", "int static constexpr hs = (ord-1)/2;",
                "int static constexpr BC_ZERO_GRADIENT = 0;", "int static constexpr BC_ZERO_VALUE = 1;",
                "inline void init( realConst2d zint ) {",
                "inline real4d cells_to_edges( realConst4d data , int bc_lower , int bc_upper ) const {"):
        assert tb._norm(sig) in text, sig
    assert "OWNERSHIP" in open(ADAPTOR).read() and "VerticalInterp" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
