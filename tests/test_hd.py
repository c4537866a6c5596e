"""Horizontal hyperdiffusion, everything that needs no GPU: the numpy restatement of the contract (tests/hd_ref.py) against a scalar loop;
the device bodies under g++ (tests/emu/hd_emu.cpp), every path IN PLACE, against the restatement bit for bit on every shape and named
case; the census of the branches the named cases reach; the mutants; the known answers; what the update and the fill do to a level sum
and to a single Fourier mode within derived bounds; the C ABI's refusals; the adaptor's boundary."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import hd_ref as ref
import test_boundary_surface as tb
from hd_emu_harness import PATHS, EmuBackend, ring_block
from pam_amd import capi
from tools import native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
U = 2.0 ** -53
LD = np.longdouble
EVEN = [s for s in ref.SHAPES if s[2] % 2 == 0 and (s[1] == 1 or s[1] % 2 == 0)]


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement itself

def _scalar(f, positive, dt, tau):
    """the contract's sentences, one Python float at a time"""
    nz, ny, nx, nens = f.shape
    c = dt / (16.0 * tau)
    out = np.empty_like(f)

    def d4(v):
        n = len(v)
        res = []
        for i in range(n):
            e1 = v[(i - 1) % n] - v[(i - 2) % n]
            e2 = v[i] - v[(i - 1) % n]
            e3 = v[(i + 1) % n] - v[i]
            e4 = v[(i + 2) % n] - v[(i + 1) % n]
            a = e4 - e1
            b = e3 - e2
            t = 3.0 * b
            res.append(a - t)
        return res

    for k in range(nz):
        for e in range(nens):
            lvl = [[float(f[k, j, i, e]) for i in range(nx)] for j in range(ny)]
            dx = [d4(row) for row in lvl]
            if ny > 1:
                dy = [d4([lvl[j][i] for j in range(ny)]) for i in range(nx)]
            new = []
            for j in range(ny):
                for i in range(nx):
                    D = dx[j][i] + dy[i][j] if ny > 1 else dx[j][i]
                    p = c * D
                    new.append(lvl[j][i] - p)
            if positive:
                pos, neg = [0.0] * 16, [0.0] * 16
                for cell, v in enumerate(new):
                    pos[cell % 16] = pos[cell % 16] + (v if v > 0 else 0.0)
                    neg[cell % 16] = neg[cell % 16] + (v if v < 0 else 0.0)
                P = N = 0.0
                for s in range(16):
                    P, N = P + pos[s], N + neg[s]
                if N < 0:
                    if P + N > 0:
                        factor = 1.0 + N / P
                        new = [(v if v > 0 else 0.0) * factor for v in new]
                    else:
                        new = [0.0] * len(new)
            out[k, :, :, e] = np.array(new).reshape(ny, nx)
    return out


@pytest.mark.parametrize("shape", [(1, 1, 5, 1), (3, 1, 17, 3), (1, 5, 5, 3), (3, 6, 6, 1), (3, 9, 17, 3)], ids=ref.shape_id)
def test_restatement_is_the_scalar_loop(shape):
    for name in ("base", "spike", "edge", "all_negative", "neg_zero", "dt_equals_tau"):
        case, got = ref.cases(shape)[name], ref.reference(shape, name)
        for f, pos, g in zip(case["fields"], case["positive"], got):
            assert ref.same_bits(g, _scalar(f, pos, case["dt"], case["tau"])), name


# ------------------------------------------------------------------------------------------------------------------------------
# the device bodies under g++, in place, against the restatement

@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape):
    """every named case on every path: the line walker (ny == 1) or the row ring at the entry point's member block, at a quarter of it
    and at one member (ny > 1), and the workspace path; the fill at the kernel's member block and at two other widths"""
    nens = shape[3]
    for name in ref.CASE_NAMES:
        want = ref.reference(shape, name)
        for path in PATHS:
            got = ref.run_case(EmuBackend(path), ref.cases(shape)[name])
            assert ref.results_differ(got, want) == [], (name, path)
        for me in sorted({min(nens, 37), 1}):
            got = ref.run_case(EmuBackend("in_place", fill_me=me), ref.cases(shape)[name])
            assert ref.results_differ(got, want) == [], (name, me)


def _sparse(nbytes):
    """address space without memory behind it: only the pages a test touches are ever committed"""
    import mmap
    noreserve = getattr(mmap, "MAP_NORESERVE", 0x4000)      # Linux's value where this Python does not name it
    m = mmap.mmap(-1, nbytes, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | noreserve)
    return m, C.addressof(C.c_char.from_buffer(m))


def _cell(addr, offset):
    return C.c_double.from_address(addr + 8 * offset)


def test_emulation_at_strides_that_need_64_bit_offsets():
    """the line walker, the cell of the ring and of the workspace path, and the fill walks at synthetic strides beyond 2^30 elements, so
    that single element offsets pass 2^31 and 2^32: a 32-bit product anywhere in hd_device.h reads or writes another cell, or none.  The
    cells are scattered into a sparse mapping, and what comes back is gathered and held to the restatement on the dense field."""
    from hd_emu_harness import load
    lib = load()
    c = lib.emu_hd_coefficient(ref.DT, ref.TAU)
    xs, rs = 2 ** 30 + 7, 2 ** 30 + 1
    # one line of five cells xs apart, in place
    for case in ("base", "spike"):
        for k, f in enumerate(ref.cases((1, 1, 5, 1))[case]["fields"]):
            m, addr = _sparse(8 * (4 * xs + 1))
            for i in range(5):
                _cell(addr, i * xs).value = f[0, 0, i, 0]
            lib.emu_hd_line_at(addr, xs, 5, c)
            got = np.array([_cell(addr, i * xs).value for i in range(5)]).reshape(1, 1, 5, 1)
            assert 4 * xs > 2 ** 32 and ref.same_bits(got, ref.update(f, c)), (case, k)
            if k == 2:          # the fill of the same line: ncol = 5 cells xs apart
                mode = lib.emu_hd_fill_at(addr, xs, 5)
                got = np.array([_cell(addr, i * xs).value for i in range(5)]).reshape(1, 1, 5, 1)
                assert ref.same_bits(got, ref.fill(ref.update(f, c))) and mode == int(ref.fill_levels(ref.update(f, c))[2][0, 0]), case
            del m
    # a level of 5 x 5 cells, x neighbours xs apart and rows rs apart (every (j, i) at its own address), and the same with ny == 1
    for shape in ((1, 5, 5, 3), (1, 1, 5, 1)):
        ny = shape[1]
        f = ref.cases(shape)["base"]["fields"][1][..., :1]
        m, addr = _sparse(8 * (4 * xs + 4 * rs + 1))
        for j in range(ny):
            for i in range(5):
                _cell(addr, j * rs + i * xs).value = f[0, j, i, 0]
        got = np.array([[lib.emu_hd_cell_at(addr, xs, rs, 5, ny, i, j, c) for i in range(5)] for j in range(ny)]).reshape(1, ny, 5, 1)
        assert min(4 * xs, 4 * rs) > 2 ** 32 and ref.same_bits(got, ref.update(f, c)), shape
        del m


def test_emulated_member_blocks_differ_between_the_ring_paths():
    """the three ring widths are three mappings wherever the ensemble allows it, and the block never outgrows 64 KB of LDS"""
    for nz, ny, nx, nens in ref.SHAPES:
        me = ring_block(nens, nx)
        assert 10 * nx * me * 8 <= 65536 and me <= 64 and (me >= nens or 10 * nx * 2 * me * 8 > 65536 or me == 64)
    assert ring_block(130, 8) == 64 and ring_block(130, 33) == 16 and ring_block(3, 17) == 4 and ring_block(8192, 32) == 16


def test_fill_pass_does_not_write_a_clean_level():
    shape = (3, 6, 8, 130)
    for name in ("base", "edge", "neg_zero"):
        be = EmuBackend()
        ref.run_case(be, ref.cases(shape)[name])
        _, _, mode = ref.fill_levels(ref.update(ref.cases(shape)[name]["fields"][2], ref.coefficient(ref.DT, ref.TAU)))
        assert be.written[0] is None and be.written[1] is None
        assert ((be.written[2] != 0) == (mode != 0)).all(), name


# ------------------------------------------------------------------------------------------------------------------------------
# the named cases reach every branch

def test_census_of_the_named_cases():
    """every case reaches the branch it is named after on every shape; a case that reaches none of its branches fails here rather than
    passing empty"""
    total = dict.fromkeys(("clean", "filled", "zeroed"), 0)
    for shape in ref.SHAPES:
        nz, ny, nx, nens = shape
        cs = ref.cases(shape)

        def modes(name):
            case = cs[name]
            fn = ref.update(case["fields"][2], ref.coefficient(case["dt"], case["tau"]))
            return fn, ref.fill_levels(fn)[2]

        fn, mode = modes("base")
        assert (mode == 0).all() and (fn > 0).all()                                   # nothing goes negative
        assert all(not ref.same_bits(a, b) for a, b in zip(ref.reference(shape, "base"), cs["base"]["fields"]))
        fn, mode = modes("spike")
        assert (fn < 0).any(axis=(1, 2)).all() and (mode == 1).all()                  # negatives before the fill, on every level
        assert (ref.reference(shape, "spike")[2] >= 0).all()
        fn, mode = modes("edge")
        # (five cells hold a wet run of three and a dry run of two: no dry cell lies two cells from the wet run on both sides)
        assert ((mode == 1).all() or nx == 5) and (ref.reference(shape, "edge")[2] >= 0).all()
        fn, mode = modes("all_negative")
        assert (mode[0] == 2).all() and (ref.reference(shape, "all_negative")[2][0] == 0).all()
        assert nz == 1 or (mode[1:] == 0).all()
        for m, kind in enumerate(("clean", "filled", "zeroed")):
            total[kind] += sum(int((modes(n)[1] == m).sum()) for n in ("base", "spike", "edge", "all_negative"))
        assert ref.results_differ(ref.reference(shape, "constant"), cs["constant"]["fields"]) == []
        nan = ref.reference(shape, "nan_cell")
        kk, jj, ii, ee = nz // 2, ny // 2, nx // 2, nens // 2
        stencil = np.zeros(shape, dtype=bool)
        for d in range(-2, 3):
            stencil[kk, jj, (ii + d) % nx, ee] = True
            if ny > 1:
                stencil[kk, (jj + d) % ny, ii, ee] = True
        for g in nan[:2]:
            assert (np.isnan(g) == stencil).all()                                     # its stencil and nowhere else
        assert not np.isnan(nan[2]).any() or (np.isnan(nan[2]) <= stencil).all()
        others = np.ones(nens, dtype=bool)
        others[ee] = False
        assert ref.same_bits(nan[2][..., others], ref.reference(shape, "spike")[2][..., others])
        nz0 = ref.reference(shape, "neg_zero")[2]
        assert np.signbit(nz0[0]).all() and (nz0[0] == 0).all()                       # a clean level of -0.0 keeps its signs
        assert (modes("neg_zero")[1][0] == 0).all()
        free = ref.reference(shape, "no_positive_fields")[2]
        assert (free < 0).any() and ref.same_bits(free, modes("spike")[0])            # no flag, no fill
        assert cs["dt_equals_tau"]["dt"] == cs["dt_equals_tau"]["tau"] and ((modes("dt_equals_tau")[1] == 1).all() or nx == 5)
        assert not np.isnan(np.concatenate([g.ravel() for g in ref.reference(shape, "dt_equals_tau")])).any()
    assert all(v >= 1 for v in total.values()), total


# ------------------------------------------------------------------------------------------------------------------------------
# mutants of the restatement: each is caught by a named case

CAUGHT_BY = {"wrap_off_by_one": ("base", 0), "inplace_x": ("base", 0), "inplace_y": ("base", 1), "stencil_form": ("base", 0),
             "update_fma": ("base", 1), "fill_clean_level": ("neg_zero", 2), "slots_descending": ("edge", 2)}


@pytest.mark.parametrize("mutant", sorted(CAUGHT_BY))
def test_every_mutant_is_caught(mutant):
    name, expect = CAUGHT_BY[mutant]
    for shape in ((3, 6, 8, 130),) + (() if mutant == "inplace_y" else ((3, 1, 8, 65),)):
        got = ref.run_case(ref.RefBackend(mutant), ref.cases(shape)[name])
        bad = ref.results_differ(got, ref.reference(shape, name))
        assert expect in bad, (mutant, shape, bad)


def test_y_plus_x_cannot_be_told_from_the_restatement():
    """D4y + D4x for D4x + D4y: IEEE addition of two operands commutes bit for bit (one rounding of the same exact sum), so this variant
    IS the contract on every finite input, and no case can catch it.  It is kept in the list and shown to be equal, not dropped."""
    assert "y_plus_x" in ref.MUTANTS and set(CAUGHT_BY) | {"y_plus_x"} == set(ref.MUTANTS)
    for shape in ((3, 6, 8, 130), (3, 9, 17, 3)):
        for name in ("base", "spike", "edge", "dt_equals_tau"):
            got = ref.run_case(ref.RefBackend("y_plus_x"), ref.cases(shape)[name])
            assert ref.results_differ(got, ref.reference(shape, name)) == []


def test_no_mutant_is_the_restatement():
    shape = (3, 6, 8, 130)
    assert ref.results_differ(ref.run_case(ref.RefBackend(None), ref.cases(shape)["base"]), ref.reference(shape, "base")) == []


# ------------------------------------------------------------------------------------------------------------------------------
# known answers

@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.shape_id)
def test_constant_lines_keep_their_bits(shape):
    case = ref.cases(shape)["constant"]
    for be in (ref.RefBackend(), EmuBackend("in_place"), EmuBackend("workspace")):
        assert ref.results_differ(ref.run_case(be, case), case["fields"]) == []


@pytest.mark.parametrize("shape", EVEN, ids=ref.shape_id)
def test_checkerboards_at_dt_equal_tau(shape):
    """+-a in x: D4 = 16 f exactly, so f - f = 0.0 (with ny > 1 the y term is an exact zero); +-a in x and y: D4 = 32 f, so -f"""
    assert len(EVEN) >= 4 and any(s[1] > 1 for s in EVEN) and any(s[1] == 1 for s in EVEN)
    cx = ref.cases(shape)["checkerboard_x"]
    for g in ref.reference(shape, "checkerboard_x"):
        assert (g == 0.0).all() and not np.signbit(g).any()
    assert (np.abs(cx["fields"][0]) >= 2.0 ** -3).all()
    if shape[1] > 1:
        cxy = ref.cases(shape)["checkerboard_xy"]
        for g, f in zip(ref.reference(shape, "checkerboard_xy"), cxy["fields"]):
            assert ref.same_bits(g, -f)


# ------------------------------------------------------------------------------------------------------------------------------
# what the call does to a level sum, and to one Fourier mode

def _d4_roundings(f, axis):
    """D4 along the axis and the sum of the magnitudes its four roundings act on (the first differences are shared between cells)"""
    m2, m1, p1, p2 = (np.roll(f, s, axis=axis) for s in (2, 1, -1, -2))
    e1, e2, e3, e4 = m1 - m2, f - m1, p1 - f, p2 - p1
    outer, inner = e4 - e1, e3 - e2
    three = 3.0 * inner
    D = outer - three
    mags = np.abs(outer).astype(LD) + 3 * np.abs(inner).astype(LD) + np.abs(three).astype(LD) + np.abs(D).astype(LD)
    return D, mags


@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[3] in (3, 65)], ids=ref.shape_id)
def test_level_sum_of_an_unflagged_field_is_kept_within_the_roundings(shape):
    """The first differences are computed once: e(i) is the same double wherever it is used.  In exact arithmetic on those doubles the sum
    over a periodic line of (e(i+2) - e(i-1)) - 3 (e(i+1) - e(i)) is zero term by term.  So the level sum of the computed D4 is the sum of
    its rounding errors alone, and a rounding of a result r is at most u |r| (u = 2^-53, r the rounded result):
      per direction and cell   u (|outer| + 3 |inner| + |three| + |D4d|): inner's rounding is tripled, the others enter once
      ny > 1                   + u |D4| for the add D4x + D4y
    times c; then u |p| for p = c D4 and u |f_new| for the subtraction.  The sums of the test itself are taken in np.longdouble, whose
    own error is at most 2 ncol 2^-64 times the sum of the magnitudes."""
    nz, ny, nx, nens = shape
    worst = 0.0
    for name in ("base", "spike", "dt_equals_tau"):
        case = ref.cases(shape)[name]
        c = ref.coefficient(case["dt"], case["tau"])
        for f, g in list(zip(case["fields"], ref.reference(shape, name)))[:2]:
            D, mags = _d4_roundings(f, 2)
            if ny > 1:
                Dy, my = _d4_roundings(f, 1)
                D = D + Dy
                mags = mags + my + np.abs(D).astype(LD)
            p = c * D
            assert ref.same_bits(f - p, g)
            lim = U * (LD(c) * mags + np.abs(p).astype(LD) + np.abs(g).astype(LD)).sum(axis=(1, 2))
            lim = lim + 2 * ny * nx * LD(2.0) ** -64 * (np.abs(f).astype(LD) + np.abs(g).astype(LD)).sum(axis=(1, 2))
            err = np.abs(g.astype(LD).sum(axis=(1, 2)) - f.astype(LD).sum(axis=(1, 2)))
            assert (err <= lim).all(), name
            worst = max(worst, float((err / lim).max()))
    print("worst fraction of the bound %.3f" % worst)


@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[3] in (3, 65)], ids=ref.shape_id)
def test_level_sum_of_a_filled_level_is_kept_within_the_division(shape):
    """Pe, Ne: the exact sums of max(f_new, 0) and min(f_new, 0); P, N: the computed ones, each within g = n u / (1 - n u) of its exact
    value in relative terms, n = ceil(ncol / 16) + 15 adds on the longest path.  The exact fill Pe (1 + N / P) misses Pe + Ne by
    N (Pe - P) / P + (N - Ne): at most g |N| Pe / P + g |Ne|.  The computed factor carries the rounding of the division, u Pe |N / P|,
    and of the add, u Pe |factor|; every product max(f_new, 0) factor rounds once: u times the filled sum.  First order; the
    second-order terms are below 1e-9 of the bound at these sizes."""
    nz, ny, nx, nens = shape
    n = math.ceil(ny * nx / 16) + 15
    g = n * U / (1 - n * U)
    worst, seen = 0.0, 0
    for name in ("spike", "edge", "dt_equals_tau"):
        case = ref.cases(shape)[name]
        fn = ref.update(case["fields"][2], ref.coefficient(case["dt"], case["tau"]))
        P, N, mode = ref.fill_levels(fn)
        out = ref.reference(shape, name)[2]
        Pe = np.where(fn > 0, fn, 0.0).astype(LD).sum(axis=(1, 2))
        Ne = np.where(fn < 0, fn, 0.0).astype(LD).sum(axis=(1, 2))
        factor = 1.0 + N / P
        lim = g * np.abs(N) * Pe / P + g * np.abs(Ne) + U * Pe * np.abs(N / P) + U * Pe * np.abs(factor) + U * out.astype(LD).sum(axis=(1, 2))
        lim = lim * (1 + 1e-9) + 2 * ny * nx * LD(2.0) ** -64 * np.abs(fn).astype(LD).sum(axis=(1, 2))
        err = np.abs(out.astype(LD).sum(axis=(1, 2)) - (Pe + Ne))
        filled = mode == 1
        if not filled.any():          # the edge of five cells leaves no negative value (see the census)
            assert nx == 5 and name != "spike", name
            continue
        assert (err[filled] <= lim[filled]).all(), name
        seen += int(filled.sum())
        worst = max(worst, float((err[filled] / lim[filled]).max()))
    assert seen > 0
    print("worst fraction of the bound %.3f" % worst)


@pytest.mark.parametrize("shape", [(1, 1, 16, 3), (1, 1, 33, 3), (1, 6, 16, 3), (1, 9, 17, 3)], ids=ref.shape_id)
@pytest.mark.parametrize("ratio", [1.0, 1.0 / 3.0])
def test_a_single_fourier_mode_is_damped_by_its_factor(shape, ratio):
    """f = A cos(kx i + ky j + phase) is multiplied by 1 - (dt/tau)(sin^4(kx/2) + sin^4(ky/2)).  Bound, with |f| <= A: the samples are
    rounded, u A each, and the operator's norm is at most 1 + 2 dt/tau <= 3: 3 u A.  Per direction the first differences (|e| <= 2A)
    enter with weights 1, 3, 3, 1: 16 u A; outer (<= 4A) 4 u A; inner (<= 4A) tripled 12 u A; three (<= 12A) 12 u A; D4d (<= 16A) 16 u A:
    60 u A, twice, and the add (<= 32A) 32 u A: 152 u A, times c <= 1/16: 9.5 u A.  p = c D4 (<= 2A): 2 u A.  The subtraction (<= 3A):
    3 u A.  In all 17.5 u A; the np.longdouble yardstick adds less than 2^-60 A."""
    nz, ny, nx, nens = shape
    A, worst = 7.3, 0.0
    i = np.arange(nx, dtype=LD)[None, None, :, None]
    j = np.arange(ny, dtype=LD)[None, :, None, None]
    for mx, my in ((1, 0), (nx // 2, 0), (3, 1), (nx // 2, ny // 2)):
        if ny == 1 and my:
            continue
        kx, ky = 2 * LD(np.pi) * mx / nx, 2 * LD(np.pi) * my / ny
        phase = LD(0.3) * np.arange(nens, dtype=LD)[None, None, None, :]
        exact = A * np.cos(kx * i + ky * j + phase) + np.zeros(shape, dtype=LD)
        lam = 1 - LD(ratio) * (np.sin(kx / 2) ** 4 + (np.sin(ky / 2) ** 4 if ny > 1 else 0))
        got = ref.hyperdiffusion([exact.astype(np.float64)], [0], ratio * 60.0, 60.0)[0]
        err = np.abs(got.astype(LD) - lam * exact).max()
        lim = 17.5 * U * A + LD(2.0) ** -60 * A
        assert err <= lim, (mx, my, float(err / lim))
        assert abs(float(lam)) <= 1.0
        worst = max(worst, float(err / lim))
    print("worst fraction of the bound %.3f" % worst)


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI: refusals before any device is asked for; the symbols

NEW_SYMBOLS = ("pam_amd_hyperdiffusion", "pam_amd_hyperdiffusion_debug_path")


def test_entry_points_are_exported_and_declared_and_the_abi_stays_5():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    assert lib.pam_amd_awfl_abi_version() == 5


def test_entry_point_rejects_bad_arguments_and_leaves_the_arrays_untouched():
    """the pointers are host arrays here: a refusal comes before the first HIP call, so nothing dereferences them, and afterwards every
    array still holds the pattern it was filled with"""
    lib = capi.load()
    arrays = [np.full(64, 7.25) for _ in range(3)]
    ptr = [a.ctypes.data for a in arrays]
    F = (C.c_void_p * 3)(*ptr)
    Fhole = (C.c_void_p * 3)(ptr[0], None, ptr[2])
    F65 = (C.c_void_p * 65)(*([ptr[0]] * 65))
    pos = (C.c_ubyte * 65)(*([0, 0, 1] + [0] * 62))
    hd = lib.pam_amd_hyperdiffusion
    big = 65536                                                    # ny nx = 2^32 > 2^31 - 1
    calls = [
        lambda: hd(4, 8, 8, 4, 3, None, pos, 20.0, 60.0, None),
        lambda: hd(4, 8, 8, 4, 3, F, None, 20.0, 60.0, None),
        lambda: hd(4, 8, 8, 4, 3, Fhole, pos, 20.0, 60.0, None),
        lambda: hd(4, 8, 8, 4, 0, F, pos, 20.0, 60.0, None),
        lambda: hd(4, 8, 8, 4, -1, F, pos, 20.0, 60.0, None),
        lambda: hd(4, 8, 8, 4, 65, F65, pos, 20.0, 60.0, None),
        lambda: hd(0, 8, 8, 4, 3, F, pos, 20.0, 60.0, None),
        lambda: hd(4, 0, 8, 4, 3, F, pos, 20.0, 60.0, None),
        lambda: hd(4, 8, 0, 4, 3, F, pos, 20.0, 60.0, None),
        lambda: hd(4, 8, 8, 0, 3, F, pos, 20.0, 60.0, None),
        lambda: hd(4, 4, 8, 4, 3, F, pos, 20.0, 60.0, None),           # nx < 5
        lambda: hd(4, 1, 1, 4, 3, F, pos, 20.0, 60.0, None),
        lambda: hd(4, 8, 2, 4, 3, F, pos, 20.0, 60.0, None),           # 1 < ny < 5
        lambda: hd(4, 8, 4, 4, 3, F, pos, 20.0, 60.0, None),
        lambda: hd(4, big, big, 4, 3, F, pos, 20.0, 60.0, None),
        lambda: hd(4, 8, 8, 4, 3, F, pos, 0.0, 60.0, None),
        lambda: hd(4, 8, 8, 4, 3, F, pos, -20.0, 60.0, None),
        lambda: hd(4, 8, 8, 4, 3, F, pos, math.nan, 60.0, None),
        lambda: hd(4, 8, 8, 4, 3, F, pos, math.inf, math.inf, None),
        lambda: hd(4, 8, 8, 4, 3, F, pos, 20.0, 0.0, None),
        lambda: hd(4, 8, 8, 4, 3, F, pos, 20.0, -60.0, None),
        lambda: hd(4, 8, 8, 4, 3, F, pos, 20.0, math.nan, None),
        lambda: hd(4, 8, 8, 4, 3, F, pos, 20.0, math.inf, None),
        lambda: hd(4, 8, 8, 4, 3, F, pos, 60.0 + 2.0 ** -40, 60.0, None),      # dt > tau
        lambda: hd(4, 8, 1, 4, 3, F, pos, 61.0, 60.0, None),
        lambda: lib.pam_amd_hyperdiffusion_debug_path(-1),
        lambda: lib.pam_amd_hyperdiffusion_debug_path(4),
    ]
    for i, call in enumerate(calls):
        assert call() == -1, i                                     # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert b"hyperdiffusion" in lib.pam_amd_awfl_last_error(), i
        assert all((a == 7.25).all() for a in arrays), i
    for path in (1, 2, 3, 0):
        assert lib.pam_amd_hyperdiffusion_debug_path(path) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# the boundary of the C++ adaptor, the driver, the build

ADAPTOR = os.path.join(HOST, "modules", "hyperdiffusion.h")


def test_adaptor_calls_only_members_the_reference_has():
    coupler, dm = tb._used_members(open(ADAPTOR).read())
    assert {"get_option", "set_option", "option_exists", "get_tracer_names", "get_tracer_info"} <= coupler and {"get"} <= dm, (coupler, dm)
    assert coupler <= tb.REF_COUPLER, sorted(coupler - tb.REF_COUPLER)
    assert dm <= tb.REF_DM, sorted(dm - tb.REF_DM)
    ours = tb._declared(os.path.join(HOST, "pam_coupler.h"))
    assert (coupler | dm) <= ours, sorted((coupler | dm) - ours)
    coupler, dm = tb._used_members(open(os.path.join(ROOT, "examples", "driver.cpp")).read())
    assert coupler <= tb.REF_COUPLER and dm <= tb.REF_DM


def test_adaptor_and_python_mirror_name_the_same_fields_and_options():
    import inspect
    from pam_amd import modules
    text, py = open(ADAPTOR).read(), inspect.getsource(modules)
    for s in ('"crm_hyperdiff_timescale"', '"crm_dt"', '"temp"', '"uvel"', '"vvel"', '"wvel"'):
        assert s in text and s in py, s
    assert '"density_dry"' not in tb._strip_comments(text)
    assert modules.HYPERDIFFUSION_FIELDS == ("temp", "uvel", "vvel", "wvel")
    n = tb._norm(tb._strip_comments(text))
    for f in ("inlinevoidhyperdiffusion_init(PamCoupler&coupler,realtau){", "inlinevoidhyperdiffusion(PamCoupler&coupler,realdt){",
              "inlinevoidhyperdiffusion(PamCoupler&coupler){hyperdiffusion(coupler,coupler.get_option<real>(\"crm_dt\"));}"):
        assert f.replace("PamCoupler", "pam::PamCoupler") in n or f in n, f
    assert callable(modules.hyperdiffusion_init) and inspect.signature(modules.hyperdiffusion).parameters["dt"].default is None


def test_build_depends_on_the_device_header_and_the_driver_has_the_option():
    deps = native_build.dependencies(native_build.LIB_SOURCES)
    assert os.path.join(native_build.CSRC, "hd_device.h") in deps and os.path.join(HOST, "modules", "hyperdiffusion.h") in deps
    assert '#include "hd_device.h"' in open(os.path.join(ROOT, "pam_amd", "csrc", "modules_kernels.hip")).read()
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert drv.count('"--hyperdiff"') == 2 and '#include "modules/hyperdiffusion.h"' in drv
