"""The SHOC coupling layer without a GPU (physics/sgs/shoc/SGS.h:254-411 pack, :718-756 unpack, and the stand-in for shoc_main): the numpy
restatement (tests/shoc_coupling_ref.py) by hand, the host emulation of the device bodies (pam_amd/csrc/shoc_device.h under g++) against the
restatement bit for bit, a census of the branches the test states reach, layout 1 against layout 0, the flat index by value at sizes past
2^31 elements, and the C ABI's argument checks."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import emu_harness
import shoc_cases as sc
import shoc_coupling_ref as ref
from pam_amd import capi
from tools.native_build import syntax_check

# constants whose products and quotients are exact: kappa = 1/2, so exner = sqrt(pmid / p0)
HAND = dict(R_d=2.0, cp_d=4.0, R_v=4.0, p0=80.0, grav=8.0, latvap=16.0, cv_d=2.0, pres_R_d=2.0, pres_R_v=4.0)


def hand_state():
    f = lambda *v: np.array(v, dtype=np.float64).reshape(2, 1, 1, 1)
    st = dict(rho_d=f(0.75, 0.5), rho_v=f(0.25, 0.0), rho_c=f(0.125, 0.0), uvel=f(3.0, -2.0), vvel=f(1.0, 5.0), wvel=f(0.5, 0.25),
              temp=f(128.0, 80.0), tke=f(0.5, 0.001), wthv_sec=f(0.125, -0.5), tk=f(2.0, -4.0), tkh=f(6.0, 7.0), cldfrac=f(0.5, 0.75))
    return st, [f(0.0625, -1.0)], np.array([[[0.25]]]), np.array([[[-0.5]]]), np.array([[8.0], [24.0], [56.0]]), np.array([[16.0], [40.0]])


def test_restatement_pack_by_hand():
    """nz = 2, one column.  Cell 0: rho = 1, pmid = 0.75*2*128 + 0.25*4*128 = 320, exner = sqrt(4) = 2, theta = 64, qv = 0.25, ql = 0.125;
    cell 1: rho = 0.5, pmid = 80, exner = 1.  pdel = 8*1*16 = 8*0.5*32 = 128, so the three interface branches give 320 + 64,
    0.5 * (320 - 64 + 80 + 64) and 80 - 64."""
    st, q, fu, fv, zint, zmid = hand_state()
    A = ref.pack(st, q, fu, fv, zint, zmid, 1000.0, 500.0, HAND)
    col = lambda name: list(A[name][:, 0])                      # SHOC's order: the top cell first
    assert col("pres") == [80.0, 320.0] and col("exner") == [1.0, 2.0] and col("inv_exner") == [1.0, 0.5]
    assert col("pdel") == [128.0, 128.0] and col("zt_grid") == [32.0, 8.0] and col("zi_grid") == [48.0, 16.0, 0.0]
    assert col("presi") == [16.0, 200.0, 384.0]                 # k = nz, the interior branch, k = 0
    assert col("ql") == [0.0, 0.125] and col("qw") == [0.0, 0.375]
    assert col("thetal") == [80.0, 64.0 - 0.5 * 4.0 * 0.125] and col("thv") == [80.0, 64.0 * (1 + 0.61 * 0.25 - 0.125)]
    assert col("host_dse") == [4.0 * 80.0 + 8.0 * 32.0 + 64.0, 4.0 * 128.0 + 8.0 * 8.0 + 64.0]
    assert col("tke") == [0.004, 0.5]                           # 0.001 / 0.5 is below the floor
    assert list(A["qtracers"][0, :, 0]) == [0.0, 0.0625]        # -1 / 0.5 clamped
    assert list(A["hwind"][:, :, 0].reshape(-1)) == [-2.0, 3.0, 5.0, 1.0] and col("w_field") == [0.25, 0.5]
    assert col("wthv_sec") == [-0.5, 0.125] and col("tk") == [-4.0, 2.0] and col("tkh") == [7.0, 6.0] and col("cldfrac") == [0.75, 0.5]
    assert A["host_dx"][0] == 1000.0 and A["host_dy"][0] == 1000.0          # ny == 1: crm_dy = crm_dx
    assert A["phis"][0] == 64.0 and A["uw_sfc"][0] == 0.25 and A["vw_sfc"][0] == -0.5
    assert A["wthl_sfc"][0] == 0 and A["wqw_sfc"][0] == 0 and A["wtracer_sfc"].shape == (1, 1) and A["wtracer_sfc"][0, 0] == 0


def test_restatement_unpack_by_hand():
    """one cell per branch of SGS.h:718-756 with exact arithmetic: cv_d / cp_d = 1/2"""
    st, q, *_ = hand_state()
    one = lambda *v: np.array(v, dtype=np.float64).reshape(2, 1)
    A = dict(qw=one(0.25, 0.5), ql=one(0.5, 0.25), thetal=one(60.0, 70.0), exner=one(1.0, 2.0), tke=one(2.0, 4.0), wthv_sec=one(1.0, 2.0),
             tk=one(3.0, 4.0), tkh=one(5.0, 6.0), cldfrac=one(1.5, -0.5), ql2=one(0.0, 0.125),
             hwind=np.array([[[1.0], [2.0]], [[3.0], [4.0]]]), qtracers=np.array([[[-1.0], [0.5]]]))
    out, qo = ref.unpack(A, st, q, HAND)
    g = lambda name: list(out[name].reshape(-1))               # the coupler's order: SHOC's level 1 is cell 0
    # cell 0 (SHOC level 1): qv = 0.25, temp_new = 70*2 + 4*0.25 = 141, temp = 128 + 13 * 2 / 4
    # cell 1 (SHOC level 0): qv = -0.25: rho_v = -0.25*0.5/1.25 clamped to 0; temp_new = 60 + 4*0.5 = 62, temp = 80 - 18 * 2 / 4
    assert g("temp") == [134.5, 71.0]
    assert g("rho_v") == [0.25 * 0.75 / 0.75, 0.0] and g("rho_c") == [0.25 * 1.0, 0.5 * 0.5]
    assert g("uvel") == [2.0, 1.0] and g("vvel") == [4.0, 3.0] and g("tke") == [4.0 * 1.0, 2.0 * 0.5]
    assert g("wthv_sec") == [2.0, 1.0] and g("tk") == [4.0, 3.0] and g("tkh") == [6.0, 5.0]
    assert g("cldfrac") == [0.0, 1.0]                          # -0.5 and 1.5 clamped
    assert list(qo[0].reshape(-1)) == [0.5, 0.0]               # -1 * 0.5 clamped
    assert g("inv_qc_relvar") == [0.5, 1.0]                    # 0.25^2 / 0.125; rcm2 == 0


def test_restatement_inv_qc_relvar_branches():
    st, q, *_ = hand_state()
    for ql, ql2, want in ((0.0, 1.0, 1.0), (0.5, 0.0, 1.0), (0.5, 1024.0, 0.001), (0.5, 0.5, 0.5), (0.5, 0.0078125, 10.0)):
        A = dict(qw=np.full((2, 1), 0.75), ql=np.full((2, 1), ql), thetal=np.ones((2, 1)), exner=np.ones((2, 1)), tke=np.ones((2, 1)),
                 wthv_sec=np.ones((2, 1)), tk=np.ones((2, 1)), tkh=np.ones((2, 1)), cldfrac=np.ones((2, 1)), ql2=np.full((2, 1), ql2),
                 hwind=np.ones((2, 2, 1)), qtracers=np.ones((1, 2, 1)))
        assert list(ref.unpack(A, st, q, HAND)[0]["inv_qc_relvar"].reshape(-1)) == [want, want], (ql, ql2)


def test_default_pow_is_the_c_librarys_and_the_devices_stays_within_an_ulp_of_it():
    x = np.random.default_rng(3).uniform(0.05, 1.2, 4000)
    y = ref.CONSTS["R_d"] / ref.CONSTS["cp_d"]
    a, b = ref.libm_pow(x, y), emu_harness.emu_pow(x, y)
    assert a[7] == math.pow(x[7], y)
    assert np.max(np.abs(a - b) / np.spacing(a)) <= 1.0


def test_restatement_standin_by_hand():
    """nlev = 2, one column, one tracer, values whose products are exact.  Level 0: tk < 0 (qw and the tracer leave negated), wthv_sec >= 0,
    cldfrac 0.5 (ql2 = 2 ql^2); level 1: tk >= 0, wthv_sec < 0 (ql leaves as 0), cldfrac 0.125 (ql2 = 0).  With two levels and the ends
    repeated the mixed profile is (0.75 a + 0.25 b, 0.25 a + 0.75 b)."""
    c = lambda a, b: np.array([[a], [b]], dtype=np.float64)
    e = lambda a, b, d: np.array([[a], [b], [d]], dtype=np.float64)
    one = lambda v: np.array([v], dtype=np.float64)
    A = dict(host_dx=one(1024.0), host_dy=one(2048.0), wthl_sfc=one(1.0), wqw_sfc=one(2.0), uw_sfc=one(1.0), vw_sfc=one(-1.0), phis=one(256.0),
             wtracer_sfc=np.array([[2.0]]), thv=c(0.0, 0.0), zt_grid=c(0.0, 0.0), pres=c(0.0, 0.0), pdel=c(0.0, 0.0), w_field=c(2.0, 4.0),
             inv_exner=c(0.0, 0.0), zi_grid=e(0.0, 0.0, 0.0), presi=e(0.0, 0.0, 0.0), host_dse=c(8.0, 16.0), tke=c(4.0, 8.0), thetal=c(16.0, 32.0),
             qw=c(4.0, 8.0), hwind=np.array([[[4.0], [12.0]], [[-8.0], [8.0]]]), qtracers=np.array([[[8.0], [16.0]]]), wthv_sec=c(4.0, -4.0),
             tk=c(-4.0, 12.0), ql=c(4.0, 8.0), cldfrac=c(0.5, 0.125), tkh=c(1.0, 1.0), exner=c(1.0, 1.0))
    B = ref.standin(A)
    col = lambda name: list(B[name][:, 0])
    # 1024/1024 + 2048/2048 + 3*1 + 5*2 + 7*1 - 11*1 + 256/256 + 13*2, then w_field: 1 * (2 * 0.5) + 1.0625 * (4 * 0.5)
    assert B["pblh"][0] == 1 + 1 + 3 + 10 + 7 - 11 + 1 + 26 + 1.0 + 2.125 and B["ustar"][0] == B["pblh"][0] * 0.5
    assert B["obklen"][0] == B["pblh"][0] * -0.25
    assert col("host_dse") == [10.0, 14.0] and col("tke") == [5.0, 7.0] and col("thetal") == [20.0, 28.0]
    assert col("qw") == [-5.0, 7.0]                              # tk < 0 at level 0 only
    assert list(B["qtracers"][0, :, 0]) == [-10.0, 14.0]
    assert list(B["hwind"][:, :, 0].reshape(-1)) == [6.0, 10.0, -4.0, 4.0]
    assert col("wthv_sec") == [2.0, -2.0] and col("tk") == [0.0, 8.0] and col("tkh") == [0.0, 16.0]
    assert col("ql") == [5.0, 0.0]                               # wthv_sec < 0 at level 1 only
    assert col("cldfrac") == [3 * 0.40625 - 1, 3 * 0.21875 - 1]
    assert col("ql2") == [50.0, 0.0]                             # cldfrac 0.5: 2 ql^2; 0.125: 0
    assert col("wqls_sec") == [0.5, 1.0] and col("mix") == [0.0, 0.0]
    for lo, hi, factor in ((0.2, 0.25, 2048.0), (0.4, 0.69, 2.0), (0.7, 1.0, 0.0078125), (0.0, 0.19, 0.0)):      # the thresholds
        for cf in (lo, hi):
            A2 = dict(A, cldfrac=c(cf, cf), wthv_sec=c(1.0, 1.0))
            assert list(ref.standin(A2)["ql2"][:, 0]) == [25.0 * factor, 49.0 * factor], cf


def test_restatement_equals_the_reference_outputs_bit_for_bit():
    """tests/golden/shoc_coupling_ref.npz: the reference's own SGS.h (Fortran-call path, the C library's pow) around the stand-in body:
    what shoc_main received and the coupler state after timeStep, for the Kessler and the P3 tracer set"""
    g = np.load(GOLDEN)
    xlen, ylen, crm_dt, R_d, R_v = g["params"]
    consts = dict(ref.CONSTS, pres_R_d=R_d, pres_R_v=R_v)
    for label, ntr in (("kessler", 1), ("p3", 7)):
        st = {k: g["%s_%s" % (label, k)] for k in ref.STATE_4D}
        q = list(g[label + "_q"])
        assert len(q) == ntr and len(set(st["rho_d"].shape)) > 1
        A = ref.pack(st, q, g[label + "_flx_u"], g[label + "_flx_v"], g[label + "_zint"], g[label + "_zmid"], xlen, ylen, consts)
        received = {k[len(label) + 10:]: g[k] for k in g.files if k.startswith(label + "_received_")}
        assert sorted(received) == sorted(set(ref.PACKED) - {"exner", "hwind"} | {"u_wind", "v_wind"})
        for name, want in received.items():
            got = A["hwind"][0] if name == "u_wind" else A["hwind"][1] if name == "v_wind" else A[name]
            assert sc.same_bits(got, want), (label, name)
            assert not np.isnan(want).any(), (label, name)         # the reference wrote every element it handed over
        out, q_out = ref.unpack(ref.standin(A), st, q, consts)
        for k in sc.UNPACKED:
            assert sc.same_bits(out[k], g["%s_out_%s" % (label, k)]), (label, k)
        assert sc.same_bits(np.stack(q_out), g[label + "_out_q"]), label
        for k in ("rho_d", "wvel", "flx_u", "flx_v"):                # what timeStep leaves alone
            assert sc.same_bits(g["%s_out_%s" % (label, k)], g["%s_%s" % (label, k)]), (label, k)
        assert list(g[label + "_info"]) == [1, 1, 0, 1]            # get_num_tracers(), tke positive, not adds_mass, one shoc_main call
        assert bytes(g[label + "_sgs"]).rstrip(b"\0") == b"shoc"
        from pam_amd.physics import SGSShoc as S
        assert list(g[label + "_consts"]) == [S.R_d, S.cp_d, S.cv_d, S.gamma_d, S.kappa_d, S.R_v, S.cp_v, S.cv_v, S.p0, S.grav, S.cp_l, S.latvap,
                                              S.latice, S.karman, S.npbl if hasattr(S, "npbl") else -1.0, crm_dt]
    # the states of the fixture are the ones the other tests use
    assert sc.same_bits(g["p3_temp"], sc.make_state((4, 1, 5, 2), 7)["temp"])


@pytest.mark.skipif(not os.path.isfile(os.path.join(os.environ.get("PAM_REF", os.path.join(os.path.dirname(sc.ROOT), "reference")), "physics",
                                                    "sgs", "shoc", "SGS.h")), reason="no reference tree at hand")
def test_the_fixture_is_reproduced_from_the_reference_tree():
    import sys
    r = subprocess.run([sys.executable, os.path.join(sc.ROOT, "tests", "golden", "make_ref_shoc_golden.py"), REFERENCE, "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------------------------
# the host emulation against the restatement

CASES = [(s, t) for s in sc.SHAPES for t in ("kessler", "p3")]
CASE_IDS = ["%s-%s" % ("x".join(map(str, s)), t) for s, t in CASES]


@pytest.mark.parametrize("shape,tracers", CASES, ids=CASE_IDS)
def test_emulation_matches_restatement_bit_for_bit(shape, tracers):
    ntr = len(sc.TRACER_SETS[tracers])
    state = sc.make_state(shape, ntr)
    want = sc.restated_case(shape, ntr)
    got = sc.emulated(state, layout=0)
    sc.assert_set_equal(got[0], want[0], ref.PACKED, "pack")
    for n in set(got[0]) - set(ref.PACKED):
        assert np.isnan(got[0][n]).all(), n                    # pack writes its own arrays only
    sc.assert_set_equal(got[1], want[1], capi.SHOC_ARRAYS, "stand-in")
    assert not any(np.isnan(v).any() for v in want[1].values())               # the stand-in wrote every array
    sc.assert_set_equal(got[2], want[2], sc.UNPACKED, "unpack")
    assert len(got[3]) == ntr and all(sc.same_bits(a, b) for a, b in zip(got[3], want[3]))


def test_emulation_carries_nans_to_the_same_places():
    shape, ntr = (5, 1, 7, 3), 7
    state = dict(sc.make_state(shape, ntr))
    for k, at in (("temp", 3), ("rho_c", 11), ("tke", 17), ("cldfrac", 23), ("tk", 29), ("wthv_sec", 31)):
        state[k] = state[k].copy()
        state[k].reshape(-1)[at] = np.nan
    state["q"] = [x.copy() for x in state["q"]]
    state["q"][2].reshape(-1)[5] = np.nan
    want = sc.restated(state, pow=emu_harness.emu_pow)
    got = sc.emulated(state, layout=0)
    sc.assert_set_equal(got[1], want[1], capi.SHOC_ARRAYS, "stand-in")
    sc.assert_set_equal(got[2], want[2], sc.UNPACKED, "unpack")
    assert np.isnan(want[2]["temp"]).any() and not np.isnan(want[2]["temp"]).all()


@pytest.mark.parametrize("shape,tracers", CASES, ids=CASE_IDS)
def test_wide_index_instances_give_the_same_bits(shape, tracers):
    ntr = len(sc.TRACER_SETS[tracers])
    state = sc.make_state(shape, ntr)
    a, b = sc.emulated(state, layout=1, wide=False), sc.emulated(state, layout=1, wide=True)
    sc.assert_set_equal(a[1], b[1], capi.SHOC_ARRAYS)


# ------------------------------------------------------------------------------------------------------------------------------
# which branches the states reach

def census(shape, ntr):
    s = sc.make_state(shape, ntr)
    packed, after, out, q = sc.restated_case(shape, ntr)
    up = lambda x: x[::-1].reshape(shape)
    rho = s["rho_d"] + s["rho_v"]
    qv_out = up(after["qw"]) - up(after["ql"])
    rcm, rcm2 = up(after["ql"]), up(after["ql2"])
    with np.errstate(all="ignore"):
        ratio = rcm * rcm / rcm2
    both = (rcm != 0) & (rcm2 != 0)
    cf = up(after["cldfrac"])
    return {
        "negative rho_v in": (s["rho_v"] < 0).sum(), "negative rho_c in": (s["rho_c"] < 0).sum(),
        "tke / rho below 0.004": (s["tke"] / rho < 0.004).sum(), "tke / rho above 0.004": (s["tke"] / rho > 0.004).sum(),
        "negative tracer in": sum((x < 0).sum() for x in s["q"]),
        "negative tracer out": sum((x < 0).sum() for x in after["qtracers"]), "tracer clamped out": sum((x == 0).sum() for x in q),
        "qv < 0 out": (qv_out < 0).sum(), "rho_v clamped": ((qv_out < 0) & (out["rho_v"] == 0)).sum(), "qv > 0 out": (qv_out > 0).sum(),
        "cldfrac above 1": (cf > 1).sum(), "cldfrac below 0": (cf < 0).sum(), "cldfrac inside": ((cf > 0) & (cf < 1)).sum(),
        "rcm == 0": (rcm == 0).sum(), "rcm2 == 0 with rcm != 0": ((rcm != 0) & (rcm2 == 0)).sum(),
        "ratio below 0.001": (both & (ratio < 0.001)).sum(), "ratio inside": (both & (ratio > 0.001) & (ratio < 10)).sum(),
        "ratio above 10": (both & (ratio > 10)).sum(),
        "relvar 0.001": (out["inv_qc_relvar"] == 0.001).sum(), "relvar 10": (out["inv_qc_relvar"] == 10).sum(),
        "relvar 1": (out["inv_qc_relvar"] == 1).sum(),
    }


@pytest.mark.parametrize("shape", sc.SHAPES[1:], ids=sc.SHAPE_IDS[1:])
@pytest.mark.parametrize("tracers", ["kessler", "p3"])
def test_every_branch_is_reached(shape, tracers):
    """every shape but the one-column one (2 cells cannot hold 20 branches; it is there for the smallest grid)"""
    c = census(shape, len(sc.TRACER_SETS[tracers]))
    assert all(v > 0 for v in c.values()), {k: int(v) for k, v in c.items() if v == 0}


# ------------------------------------------------------------------------------------------------------------------------------
# layout 1 is layout 0 transposed

@pytest.mark.parametrize("shape,tracers", CASES, ids=CASE_IDS)
def test_layout_1_is_layout_0_transposed(shape, tracers):
    ntr = len(sc.TRACER_SETS[tracers])
    state = sc.make_state(shape, ntr)
    l0, l1 = sc.emulated(state, layout=0), sc.emulated(state, layout=1)
    for stage in (0, 1):
        want = ref.to_layout1(l0[stage])
        for n in capi.SHOC_ARRAYS:
            assert l1[stage][n].shape == want[n].shape and sc.same_bits(l1[stage][n], want[n]), (stage, n)
    sc.assert_set_equal(l1[2], l0[2], sc.UNPACKED)
    assert all(sc.same_bits(a, b) for a, b in zip(l1[3], l0[3]))
    nz, ncol = shape[0], shape[1] * shape[2] * shape[3]
    assert l1[0]["hwind"].shape == (ncol, 2, nz) and l1[0]["qtracers"].shape == (ncol, ntr, nz) and l1[0]["wtracer_sfc"].shape == (ncol, ntr)


# ------------------------------------------------------------------------------------------------------------------------------
# the flat index by value, nothing allocated

NCOL, NLEV, NTR = 2 ** 26 + 5, 72, 7


@pytest.mark.parametrize("layout", [0, 1])
def test_offset_by_value_past_2_to_the_31(layout):
    lib = sc.emu()
    last = NTR * NLEV * NCOL - 1
    assert last > 2 ** 31
    points = [(0, 0, 0), (NCOL - 1, NLEV - 1, NTR - 1), (NCOL - 1, 0, 0), (0, NLEV - 1, 0), (0, 0, NTR - 1), (2 ** 26 + 1, 35, 6), (12345, 71, 3)]
    for col, s, tr in points:
        want = ref.shoc_index(layout, col, s, NCOL, NLEV, tr, NTR)
        assert lib.emu_shoc_offset(layout, col, s, NCOL, NLEV, tr, NTR, 1) == want, (col, s, tr)
        if want < 2 ** 32:                                      # representable in the unsigned instances
            assert lib.emu_shoc_offset(layout, col, s, NCOL, NLEV, tr, NTR, 0) == want, (col, s, tr)
    assert lib.emu_shoc_offset(layout, 0, 0, NCOL, NLEV, 0, NTR, 1) == 0
    assert lib.emu_shoc_offset(layout, NCOL - 1, NLEV - 1, NCOL, NLEV, NTR - 1, NTR, 1) == last
    # a field ((lev, col), one component) and the interface arrays: first and last element; an element between 2^31 and 2^32 in both widths
    for nlev in (NLEV, NLEV + 1):
        assert lib.emu_shoc_offset(layout, NCOL - 1, nlev - 1, NCOL, nlev, 0, 1, 1) == nlev * NCOL - 1 > 2 ** 32
        col, s = (NCOL - 1, 62) if layout == 0 else (58000000, nlev - 1)
        want = ref.shoc_index(layout, col, s, NCOL, nlev)
        assert 2 ** 31 < want < 2 ** 32
        for wide in (0, 1):
            assert lib.emu_shoc_offset(layout, 0, 0, NCOL, nlev, 0, 1, wide) == 0
            assert lib.emu_shoc_offset(layout, col, s, NCOL, nlev, 0, 1, wide) == want
    # hwind and wtracer_sfc
    assert lib.emu_shoc_offset(layout, NCOL - 1, NLEV - 1, NCOL, NLEV, 1, 2, 1) == 2 * NLEV * NCOL - 1
    assert lib.emu_shoc_offset(layout, NCOL - 1, 0, NCOL, 1, NTR - 1, NTR, 1) == NTR * NCOL - 1
    assert lib.emu_shoc_offset(layout, 3, 0, NCOL, 1, 2, NTR, 1) == (2 * NCOL + 3 if layout == 0 else 3 * NTR + 2)


def test_the_library_picks_the_wide_instances_before_a_byte_offset_passes_32_bits():
    """COUPLING_NARROW in modules_kernels.hip, shared with the P3 layer: arrays of 2^29 doubles (4 GiB) and more take the long long kernels"""
    import os
    import re
    text = open(os.path.join(sc.ROOT, "pam_amd", "csrc", "modules_kernels.hip")).read()
    assert len(re.findall(r"COUPLING_NARROW = 1ll << 29;", text)) == 1 and "SHOC_NARROW" not in text
    # one narrow expression on the one constant; pack, unpack and the stand-in hand it SHOC's largest array
    assert len(re.findall(r"\bcoupling_narrow\(bool force_wide, long long largest\) \{ return !force_wide && largest < COUPLING_NARROW; \}", text)) == 1
    assert len(re.findall(r"coupling_narrow\(g_shoc_force_wide, shoc_largest\(", text)) == 3
    assert (2 ** 29 - 1) * 8 + 7 < 2 ** 32


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI

NEW_SYMBOLS = ("pam_amd_shoc_workspace_create", "pam_amd_shoc_workspace_args", "pam_amd_shoc_workspace_bytes", "pam_amd_shoc_workspace_destroy",
               "pam_amd_shoc_pack", "pam_amd_shoc_unpack", "pam_amd_shoc_main_standin", "pam_amd_shoc_debug_wide_index")


def test_new_entry_points_are_exported_and_declared():
    import os
    import re
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(sc.ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    # the struct: the arguments of pam::shoc_main_cxx in its order, plus exner
    body = re.search(r"typedef struct pam_amd_shoc_args_t \{(.*?)\} pam_amd_shoc_args_t;", text, flags=re.S).group(1)
    assert tuple(re.findall(r"\*(\w+)", body)) == ("stream",) + capi.SHOC_ARRAYS
    assert [f[0] for f in capi.ShocArgs._fields_[:8]] == ["ncol", "nlev", "nlevi", "dt", "nadv", "num_qtracers", "layout", "stream"]
    assert re.search(r"typedef int \(\*pam_amd_shoc_main_fn\)\(const pam_amd_shoc_args_t \*\w+, void \*\w+\);", text)


def _refused(lib, who, call):
    assert call() == -1, who                                    # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
    assert who.encode() in lib.pam_amd_awfl_last_error(), (who, lib.pam_amd_awfl_last_error())


CREATE_BAD = [dict(nens=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(ntr=-1), dict(ntr=8), dict(layout=2), dict(layout=-1),
              dict(nens=2 ** 20, nx=2 ** 10, ny=2)]


@pytest.mark.parametrize("bad", CREATE_BAD, ids=[str(sorted(b.items())) for b in CREATE_BAD])
def test_workspace_create_refuses(bad):
    lib = capi.load()
    a = dict(nens=4, nx=4, ny=6, nz=3, ntr=1, layout=1)
    a.update(bad)
    ws = C.c_void_p(1)
    _refused(lib, "shoc_workspace_create", lambda: lib.pam_amd_shoc_workspace_create(a["nens"], a["nx"], a["ny"], a["nz"], a["ntr"], a["layout"],
                                                                                     C.byref(ws)))
    assert not ws.value


def test_workspace_calls_refuse_what_is_no_workspace():
    lib = capi.load()
    _refused(lib, "shoc_workspace_create", lambda: lib.pam_amd_shoc_workspace_create(4, 4, 6, 3, 1, 1, None))
    n, a = C.c_longlong(), capi.ShocArgs()
    _refused(lib, "shoc_workspace_args", lambda: lib.pam_amd_shoc_workspace_args(None, C.byref(a)))
    _refused(lib, "shoc_workspace_bytes", lambda: lib.pam_amd_shoc_workspace_bytes(None, C.byref(n)))
    assert lib.pam_amd_shoc_workspace_destroy(None) == 0
    fake = (C.c_ulonglong * 64)()                               # readable memory without the workspace's mark
    for who, call in (("shoc_workspace_args", lambda: lib.pam_amd_shoc_workspace_args(fake, C.byref(a))),
                      ("shoc_workspace_bytes", lambda: lib.pam_amd_shoc_workspace_bytes(fake, C.byref(n))),
                      ("shoc_workspace_destroy", lambda: lib.pam_amd_shoc_workspace_destroy(fake))):
        _refused(lib, who, call)


P = 1 << 20                                                     # never dereferenced: validation fails first
PACK_OK = [None] + [P] * 8 + [None] + [P] * 8 + [16000.0, 12000.0, 287.0, 461.0, 287.042, 1004.64, 1.0e5, 9.80616, 2501000.0, None]
UNPACK_OK = [None] + [P] * 7 + [None] + [P] * 5 + [1004.64, 717.598, 2501000.0, None]
PACK_BAD = [(i, None) for i in list(range(1, 9)) + list(range(10, 18))] + \
           [(i, v) for i in range(18, 27) for v in (0.0, -1.0, math.nan, math.inf)]
UNPACK_BAD = [(i, None) for i in list(range(1, 8)) + list(range(9, 14))] + [(i, v) for i in range(14, 17) for v in (0.0, -1.0, math.nan, math.inf)]


@pytest.mark.parametrize("index,value", PACK_BAD, ids=["%d-%s" % b for b in PACK_BAD])
def test_pack_refuses(index, value):
    lib = capi.load()
    args = list(PACK_OK)
    args[index] = value
    _refused(lib, "shoc_pack", lambda: lib.pam_amd_shoc_pack(*args))
    assert b"workspace" not in lib.pam_amd_awfl_last_error()    # refused for the argument, before the workspace is looked at


@pytest.mark.parametrize("index,value", UNPACK_BAD, ids=["%d-%s" % b for b in UNPACK_BAD])
def test_unpack_refuses(index, value):
    lib = capi.load()
    args = list(UNPACK_OK)
    args[index] = value
    _refused(lib, "shoc_unpack", lambda: lib.pam_amd_shoc_unpack(*args))
    assert b"workspace" not in lib.pam_amd_awfl_last_error()


def test_pack_and_unpack_refuse_what_is_no_workspace():
    lib = capi.load()
    fake = (C.c_ulonglong * 64)()
    for ws in (None, fake):
        _refused(lib, "shoc_pack: not a workspace", lambda: lib.pam_amd_shoc_pack(ws, *PACK_OK[1:]))
        _refused(lib, "shoc_unpack: not a workspace", lambda: lib.pam_amd_shoc_unpack(ws, *UNPACK_OK[1:]))


def _standin_args(**kw):
    a = capi.ShocArgs()
    a.ncol, a.nlev, a.nlevi, a.dt, a.nadv, a.num_qtracers, a.layout = 24, 3, 4, 1.0, 1, 1, 1
    for n in capi.SHOC_ARRAYS:
        setattr(a, n, P)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


STANDIN_BAD = [dict(ncol=0), dict(ncol=2 ** 31 - 64), dict(nlev=0), dict(nlevi=3), dict(num_qtracers=-1), dict(num_qtracers=8), dict(layout=2)] + \
              [{n: None} for n in capi.SHOC_ARRAYS]


@pytest.mark.parametrize("bad", STANDIN_BAD, ids=[next(iter(b)) + "=" + str(next(iter(b.values()))) for b in STANDIN_BAD])
def test_standin_refuses(bad):
    lib = capi.load()
    _refused(lib, "shoc_main_standin", lambda: lib.pam_amd_shoc_main_standin(C.byref(_standin_args(**bad)), None))


def test_standin_refuses_null_args():
    lib = capi.load()
    _refused(lib, "shoc_main_standin", lambda: lib.pam_amd_shoc_main_standin(None, None))


# ------------------------------------------------------------------------------------------------------------------------------
# the boundary of the C++ plug-in class

SGS_H = os.path.join(sc.ROOT, "pam_amd", "csrc", "host", "physics", "sgs", "shoc_amd", "SGS.h")
HOST = os.path.join(sc.ROOT, "pam_amd", "csrc", "host")
GOLDEN = os.path.join(sc.ROOT, "tests", "golden", "shoc_coupling_ref.npz")
EXTRACT = os.path.join(sc.ROOT, "tests", "golden", "shoc_extract.json")
REFERENCE = os.environ.get("PAM_REF", os.path.join(os.path.dirname(sc.ROOT), "reference"))
# the member signatures of physics/sgs/shoc/SGS.h, as written there (:85, :92, :150, :782, :786)
SIGNATURES = ("static int constexpr get_num_tracers()", "void init(pam::PamCoupler &coupler)", "void timeStep( pam::PamCoupler &coupler )",
              "void finalize(pam::PamCoupler &coupler)", "std::string sgs_name() const")


def test_plugin_header_calls_only_members_the_reference_has():
    import test_boundary_surface as tb
    coupler, dm = tb._used_members(open(SGS_H).read())
    assert coupler and dm, "scan found no coupler / DataManager calls"
    assert coupler <= tb.REF_COUPLER, sorted(coupler - tb.REF_COUPLER)
    assert dm <= tb.REF_DM, sorted(dm - tb.REF_DM)
    ours = tb._declared(os.path.join(HOST, "pam_coupler.h"))
    assert (coupler | dm) <= ours, sorted((coupler | dm) - ours)


def test_plugin_header_has_the_reference_members():
    import re
    import test_boundary_surface as tb
    text = tb._norm(tb._strip_comments(open(SGS_H).read()))
    for sig in SIGNATURES:
        assert tb._norm(sig) + "{" in text, sig
    assert tb._norm("void set_shoc_main(pam_amd_shoc_main_fn fn, void *user = nullptr)") + "{" in text         # the one addition
    raw = tb._strip_comments(open(SGS_H).read())
    # the constructor's constants (SGS.h:60-80) and the registered entries (:103-120, :145)
    for k, v in dict(R_d=287.042, cp_d=1004.64, R_v=461.505, cp_v=1859, p0=1.e5, grav=9.80616, cp_l=4218., latvap=2501000.0, latice=333700.0,
                     karman=0.4, npbl=-1, etime=0).items():
        m = re.findall(r"\b%s\s*=\s*(-?[0-9.e+]+)\s*;" % k, raw)
        assert [float(x) for x in m] == [float(v)], (k, m)
    registered = re.findall(r'register_and_allocate<real>\(\s*"(\w+)"', raw)
    assert registered == ["wthv_sec", "tk", "tkh", "cldfrac", "inv_qc_relvar", "sfc_shf", "sfc_lhf", "sfc_mom_flx_u", "sfc_mom_flx_v"]
    assert re.search(r'add_tracer\("tke"\s*,\s*"Turbulent Kinetic Energy \(m\^2/s\^2\)"\s*,\s*true\s*,\s*false\s*\)', raw)
    assert 'set_option<std::string>("sgs","shoc")' in raw
    assert re.findall(r'"(cloud_water_num|rain|rain_num|ice|ice_num|ice_rime|ice_rime_vol)"', raw) == list(ref.P3_TRACERS)


def test_the_signatures_and_messages_are_the_reference_lines():
    """against digests recorded from the reference's header (tests/golden/shoc_extract.json): runs without the reference tree"""
    import json
    import test_boundary_surface as tb
    rec = json.load(open(EXTRACT))
    ours = tb._norm(tb._strip_comments(open(SGS_H).read()))
    lines = dict(zip(SIGNATURES, (85, 92, 150, 782, 786)))
    assert sorted(rec["signature_sha256"]) == sorted("physics/sgs/shoc/SGS.h:%d" % ln for ln in lines.values())
    for sig, ln in lines.items():
        assert tb._digest(tb._norm(sig)) == rec["signature_sha256"]["physics/sgs/shoc/SGS.h:%d" % ln], sig
        assert tb._norm(sig) + "{" in ours, sig
    for msg, ln in (('endrun("ERROR: SHOC requires coupler.set_option<std::string>(\\"micro\\",...) to be set");', 190),
                    ('else { endrun("ERROR: SHOC only meant to run with kessler or p3 microphysics"); }', 195)):
        assert tb._digest(tb._norm(msg)) == rec["endrun_line_sha256"]["physics/sgs/shoc/SGS.h:%d" % ln], msg
        assert tb._norm(msg) in ours, msg


def test_plugin_header_compiles_with_a_microphysics_and_the_workalike(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "physics/micro/kessler_amd/Microphysics.h"\n#include "physics/sgs/shoc_amd/SGS.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  Microphysics micro;\n  SGS sgs;\n  micro.init(coupler);\n  sgs.init(coupler);\n"
                   "  sgs.set_shoc_main(pam_amd_shoc_main_standin);\n  sgs.timeStep(coupler);\n  micro.timeStep(coupler);\n"
                   "  static_assert(SGS::get_num_tracers() == 1 && SGS::ID_TKE == 0, \"\");\n  sgs.finalize(coupler);\n"
                   "  return (int)sgs.sgs_name().size() + (int)sgs.etime;\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]
