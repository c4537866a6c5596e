"""The P3 coupling layer without a GPU (physics/micro/p3/Microphysics.h:342-409 pack with the adjustment of :769-852, :680-717 unpack, and
the stand-in for p3_main): the numpy restatement (tests/p3_coupling_ref.py) by hand and against the fixture recorded from the reference's
own header, the host emulation of the device bodies (pam_amd/csrc/p3_device.h under g++) against the restatement bit for bit, a census of
the branches the test states reach, layout 1 against layout 0, the flat index by value at sizes past 2^31 elements, the C ABI's argument
checks and the boundary of the C++ plug-in class."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import emu_harness
import p3_cases as pc
import p3_coupling_ref as ref
from pam_amd import capi
from tools.native_build import syntax_check

GOLDEN = os.path.join(pc.ROOT, "tests", "golden", "p3_coupling_ref.npz")
EXTRACT = os.path.join(pc.ROOT, "tests", "golden", "p3_extract.json")
REFERENCE = os.environ.get("PAM_REF", os.path.join(os.path.dirname(pc.ROOT), "reference"))
MICRO_H = os.path.join(pc.ROOT, "pam_amd", "csrc", "host", "physics", "micro", "p3_amd", "Microphysics.h")
HOST = os.path.join(pc.ROOT, "pam_amd", "csrc", "host")

# constants whose products and quotients are exact: kappa = 1/2, so exner = sqrt(pressure / p0); cv_d / cp_d = 1/2
HAND = dict(R_d=2.0, cp_d=4.0, R_v=4.0, cp_v=8.0, cp_l=16.0, p0=80.0, grav=8.0, cv_d=2.0)


def hand_state():
    f = lambda *v: np.array(v, dtype=np.float64).reshape(2, 1, 1, 1)
    st = dict(rho_d=f(0.5, 0.25), rho_v=f(0.25, 0.0), rho_c=f(0.125, -0.5), temp=f(128.0, 160.0), nccn_prescribed=f(3.0, 4.0),
              nc_nuceat_tend=f(-1.0, 2.0), ni_activated=f(5.0, -6.0), q_prev=f(0.125, 0.5), t_prev=f(100.0, 200.0))
    q = [f(0.25, 1.0), f(0.5, -1.0), f(1.0, 2.0), f(2.0, 0.0), f(4.0, 0.5), f(8.0, 0.25), f(16.0, 0.125)]
    return st, q, np.array([[8.0], [24.0], [56.0]])


@pytest.mark.parametrize("first_step", [True, False])
def test_restatement_pack_by_hand(first_step):
    """nz = 2, one column, no adjustment, p0 = 64.  Cell 0: pressure_dry = 2*0.5*128 = 128, pressure = 128 + 4*0.25*128 = 256, exner =
    sqrt(256 / 64) = 2, theta = 64.  Cell 1: pressure_dry = pressure = 2*0.25*160 = 80, exner = sqrt(1.25).  dz = 16 and 32."""
    st, q, zint = hand_state()
    consts = dict(HAND, p0=64.0)                       # 256 / 64 = 4 -> exner = 2 in cell 0; 80 / 64 = 1.25 in cell 1
    A, adjusted, info = ref.pack(st, q, zint, False, first_step, consts)
    col = lambda name: list(A[name][:, 0])             # P3's layout-0 order is the coupler's: the ground first
    assert info is None and all(pc.same_bits(a, st[k]) for a, k in zip(adjusted, pc.ADJUSTED))
    assert col("qc") == [0.25, -2.0] and col("qv") == [0.5, 0.0]
    assert col("nc") == [0.5, 4.0] and col("qr") == [1.0, -4.0] and col("nr") == [2.0, 8.0] and col("qi") == [4.0, 0.0]
    assert col("ni") == [8.0, 2.0] and col("qm") == [16.0, 1.0] and col("bm") == [32.0, 0.5]
    assert col("pres") == [128.0, 80.0]
    assert col("exner") == [2.0, math.pow(1.25, 0.5)] and col("inv_exner") == [0.5, 1.0 / math.pow(1.25, 0.5)]
    assert col("th_atm") == [64.0, 160.0 * (1.0 / math.pow(1.25, 0.5))]
    assert col("dz") == [16.0, 32.0] and col("dpres") == [0.5 * 8.0 * 16.0, 0.25 * 8.0 * 32.0]
    for k in ("cld_frac_l", "cld_frac_i", "cld_frac_r", "inv_qc_relvar"):
        assert col(k) == [1.0, 1.0]
    assert A["col_location"].shape == (3, 1) and list(A["col_location"][:, 0]) == [1.0, 1.0, 1.0]
    assert col("nccn_prescribed") == [3.0, 4.0] and col("nc_nuceat_tend") == [-1.0, 2.0] and col("ni_activated") == [5.0, -6.0]
    if first_step:
        assert col("q_prev") == [0.5, 0.0] and col("t_prev") == [128.0, 160.0]
    else:
        assert col("q_prev") == [0.25, 2.0] and col("t_prev") == [100.0, 200.0]


def test_restatement_one_cell_rounds_as_the_reference_does():
    """the exact roundings of one cell with the class's own constants, operation by operation in the reference's order (:351-373)"""
    f = lambda v: np.array([v, v], dtype=np.float64).reshape(2, 1, 1, 1)
    rd, rv, rc, t = 1.1, 0.013, 0.0007, 287.3
    st = dict(rho_d=f(rd), rho_v=f(rv), rho_c=f(rc), temp=f(t), nccn_prescribed=f(0.0), nc_nuceat_tend=f(0.0), ni_activated=f(0.0),
              q_prev=f(0.011), t_prev=f(280.0))
    A, _, _ = ref.pack(st, [f(1e-4 * (i + 1)) for i in range(7)], np.array([[0.0], [100.3], [250.9]]), False, False)
    c = ref.CONSTS
    pd = c["R_d"] * rd * t
    pressure = pd + c["R_v"] * rv * t
    exner = math.pow(pressure / c["p0"], c["R_d"] / c["cp_d"])
    assert A["pres"][0, 0] == pd and A["exner"][0, 0] == exner and A["inv_exner"][0, 0] == 1. / exner
    assert A["th_atm"][0, 0] == t * (1. / exner) and A["qv"][0, 0] == rv / rd and A["qc"][0, 0] == rc / rd
    assert A["dz"][1, 0] == 250.9 - 100.3 and A["dpres"][1, 0] == rd * c["grav"] * (250.9 - 100.3)
    assert A["q_prev"][0, 0] == 0.011 / rd and A["t_prev"][0, 0] == 280.0 and A["bm"][0, 0] == 7e-4 / rd


def test_restatement_unpack_by_hand():
    """every clamp of :682-690 and :702 on both sides, the cv_d / cp_d scaling (1/2) and the copies"""
    st, q, zint = hand_state()
    one = lambda *v: np.array(v, dtype=np.float64).reshape(2, 1)
    A = dict(qc=one(0.5, -1.0), nc=one(-2.0, 4.0), qr=one(1.0, -0.0), nr=one(-1.0, 8.0), qi=one(2.0, -2.0), ni=one(-4.0, 1.0),
             qm=one(3.0, -3.0), bm=one(-5.0, 2.0), qv=one(0.25, -0.5), th_atm=one(70.0, 100.0), exner=one(2.0, 1.5),
             liq_ice_exchange=one(1.0, 2.0), vap_liq_exchange=one(3.0, 4.0), vap_ice_exchange=one(5.0, 6.0),
             precip_liq_surf=np.array([7.0]), precip_ice_surf=np.array([-8.0]))
    out, qo = ref.unpack(A, st["rho_d"], st["temp"], None, HAND)
    g = lambda a: list(np.asarray(a).reshape(-1))
    assert g(out["rho_c"]) == [0.25, 0.0] and g(out["rho_v"]) == [0.125, 0.0]
    assert [g(x) for x in qo] == [[0.0, 1.0], [0.5, 0.0], [0.0, 2.0], [1.0, 0.0], [0.0, 0.25], [1.5, 0.0], [0.0, 0.5]]
    assert math.copysign(1.0, qo[1].reshape(-1)[1]) == -1.0          # std::max(-0 * rho, 0) keeps the -0: (a < b) ? b : a
    # temp_new = 140 and 150: 128 + (140 - 128) * 2 / 4, 160 + (150 - 160) * 2 / 4
    assert g(out["temp"]) == [134.0, 155.0] and g(out["t_prev"]) == [134.0, 155.0] and g(out["q_prev"]) == [0.125, 0.0]
    assert g(out["liq_ice_exchange_out"]) == [1.0, 2.0] and g(out["vap_liq_exchange_out"]) == [3.0, 4.0]
    assert g(out["vap_ice_exchange_out"]) == [5.0, 6.0]
    assert out["precip_liq_surf_out"].shape == (1, 1, 1) and g(out["precip_liq_surf_out"]) == [7.0] and g(out["precip_ice_surf_out"]) == [-8.0]
    nan = ref.unpack(dict(A, qc=one(math.nan, 1.0)), st["rho_d"], st["temp"], None, HAND)[0]["rho_c"].reshape(-1)
    assert math.isnan(nan[0])                                         # std::max(NaN, 0) is NaN


def test_restatement_adjustment_by_hand():
    """a cell in each branch of :781-851 and one in neither, with the class's constants.
    Evaporation of all the cloud into very dry air: every midpoint is still unsaturated, so the bracket is [rho_c (1 - 2^-n), rho_c]; with
    rho_c = 2^-10 it closes at 2^-20 <= 1e-6 after 10 iterations, all in exact arithmetic.
    Condensation: the bracket [0, rho_v] halves until it is <= 1e-6: ceil(log2(rho_v / 1e-6)) iterations; the result is saturated to
    within the bracket.  Neither: sub-saturated without cloud, and a NaN temperature."""
    c = ref.CONSTS
    args = (c["R_v"], c["cp_d"], c["cp_v"], c["cp_l"])
    rho_d, rho_c, t = 1.0, 2.0 ** -10, 300.0
    rv, rc, tt, br, it, _ = ref.compute_adjusted_state(rho_d + 0.0, rho_d, 0.0, rho_c, t, *args)
    x = 2.0 ** -10 - 2.0 ** -20
    assert (br, it) == ("evap", 10) and rv == x and rc == 2.0 ** -20
    tcel = t - 273.15
    Lv = (2500.8 - 2.36 * tcel + 0.0016 * tcel * tcel - 0.00006 * tcel * tcel * tcel) * 1000
    rho = rho_d + rv + rc
    cp = rho_d / rho * c["cp_d"] + rv / rho * c["cp_v"] + rc / rho * c["cp_l"]
    assert tt == t - x * Lv / (1.0 * cp) and tt < t
    rho_v = 0.03
    rv, rc, tt, br, it, _ = ref.compute_adjusted_state(rho_d + rho_v, rho_d, rho_v, 0.001, 290.0, *args)
    assert (br, it) == ("cond", math.ceil(math.log2(rho_v / 1e-6))) and tt > 290.0 and 0 < rv < rho_v
    assert abs((rv + rc) - (rho_v + 0.001)) < 1e-15
    sat = lambda v, T: v * c["R_v"] * T / ref.saturation_vapor_pressure(T)
    dT = (tt - 290.0) / (rho_v - rv)                                  # per unit of density moved
    assert sat(rv + 2e-6, tt - 2e-6 * dT) > 1 > sat(rv - 2e-6, tt + 2e-6 * dT)
    for v, cl, T in ((0.001, 0.0, 300.0), (0.001, -1e-5, 300.0), (0.001, 0.5, math.nan)):
        got = ref.compute_adjusted_state(rho_d + v, rho_d, v, cl, T, *args)
        assert got[3] is None and got[4] == 0 and pc.same_bits(np.array(got[:3]), np.array([v, cl, T]))
    # the clamps are std::max(0._fp, x): a NaN candidate becomes 0, where YAKL's max keeps it
    assert ref._smax(0.0, math.nan) == 0.0 and math.copysign(1.0, ref._smax(0.0, -0.0)) == 1.0


def test_restatement_standin_by_hand():
    """the mixing with repeated ends, the two negation switches, the folded sum and the flux arrays, on the hand state"""
    st, q, zint = hand_state()
    A, _, _ = ref.pack(st, q, zint, False, True, dict(HAND, p0=64.0))
    B = ref.standin(A, 2)
    col = lambda name: list(B[name][:, 0])
    # level 0: nc_nuceat_tend = -1 < 0 negates the even-numbered profiles (qc qr qv* qi ni; th_atm never); level 1: ni_activated < 0 the odd
    assert col("qc") == [-(0.25 * 0.25 + 0.5 * 0.25 + 0.25 * -2.0), 0.25 * 0.25 + 0.5 * -2.0 + 0.25 * -2.0]
    assert col("nc") == [0.75 * 0.5 + 0.25 * 4.0, -(0.25 * 0.5 + 0.75 * 4.0)]
    assert col("th_atm") == [(0.25 * A["th_atm"][0, 0] + 0.5 * A["th_atm"][0, 0]) + 0.25 * A["th_atm"][1, 0],
                             (0.25 * A["th_atm"][0, 0] + 0.5 * A["th_atm"][1, 0]) + 0.25 * A["th_atm"][1, 0]]
    assert col("liq_ice_exchange") == [0.5 * (0.25 * 0.25 + 0.5 * 0.25 + 0.25 * -2.0), 0.5 * (0.25 * 0.25 + 0.5 * -2.0 + 0.25 * -2.0)]
    assert col("diag_eff_radius_qc") == [0.016, 0.032] and col("bulk_qi") == [1.0, 0.0] and col("nevapr") == [0.875, 0.875]
    assert col("qr_evap_tend") == [3.0, 3.0] and col("qv2qi_depos_tend") == [1.5, 2.0] and col("mu_c") == [-0.25, 0.5]
    assert col("precip_liq_flux") == [128.0 * 0.00001, 80.0 * 0.00001 + 1, 80.0 * 0.00001 + 2]
    assert col("precip_ice_flux") == [0.16, 0.16 - 1, 0.32 - 2]
    assert B["p3_tend_out"].shape == (2, 2, 1) and list(B["p3_tend_out"][1, :, 0]) == [128.0 * 0.000001 + 1, 80.0 * 0.000001 + 1]
    acc = 1.0 + 2.0 + 3.0
    for k in range(2):
        t = None
        for name, w in (("pres", 0.00001), ("dz", 0.001), ("nc_nuceat_tend", 3.0), ("nccn_prescribed", 5.0), ("ni_activated", 7.0),
                        ("inv_qc_relvar", 0.5), ("dpres", 0.0001), ("inv_exner", 0.25), ("cld_frac_r", 0.125), ("cld_frac_l", 0.0625),
                        ("cld_frac_i", 0.03125), ("q_prev", 11.0), ("t_prev", 0.001)):
            t = A[name][k, 0] * w if t is None else t + A[name][k, 0] * w
        acc = acc + (1.0 + k * 0.0625) * t
    assert B["precip_liq_surf"][0] == acc and B["precip_ice_surf"][0] == acc * -0.25
    for name in ("pres", "dz", "q_prev", "t_prev", "exner", "col_location", "cld_frac_r"):      # pure inputs are left alone
        assert pc.same_bits(B[name], A[name]), name


# ------------------------------------------------------------------------------------------------------------------------------
# the fixture recorded from the reference's own header

G_SHAPES = [(5, 2, 3, 3), (4, 1, 5, 2)]
G_RECEIVED = ("qc", "nc", "qr", "nr", "th_atm", "qv", "qi", "qm", "ni", "bm", "pres", "dz", "nc_nuceat_tend", "nccn_prescribed", "ni_activated",
              "inv_qc_relvar", "dpres", "inv_exner", "cld_frac_r", "cld_frac_l", "cld_frac_i", "q_prev", "t_prev", "col_location")
G_STATE = dict(rho_v="water_vapor", rho_c="cloud_water", temp="temp", q_prev="q_prev", t_prev="t_prev",
               liq_ice_exchange_out="liq_ice_exchange_out", vap_liq_exchange_out="vap_liq_exchange_out",
               vap_ice_exchange_out="vap_ice_exchange_out", precip_liq_surf_out="precip_liq_surf_out", precip_ice_surf_out="precip_ice_surf_out")


@pytest.mark.parametrize("sgs", ["none", "shoc"])
@pytest.mark.parametrize("shape", G_SHAPES, ids=["x".join(map(str, s)) for s in G_SHAPES])
def test_restatement_equals_the_reference_outputs_bit_for_bit(shape, sgs):
    """tests/golden/p3_coupling_ref.npz: the reference's own Microphysics.h (Fortran-call path, the C library's exp and pow) around the
    stand-in body over two consecutive steps: what p3_main_fortran received on each call and the coupler state after each step"""
    g = np.load(GOLDEN)
    label = "%s_%s_" % ("x".join(map(str, shape)), sgs)
    nz, ny, nx, nens = shape
    state = {k: g[label + k] for k in ref.STATE_4D}
    state["q"], state["zint"] = list(g[label + "q"]), g[label + "zint"]
    assert pc.same_bits(state["temp"], pc.make_state(shape)["temp"])          # the states of the fixture are the ones the other tests use
    for step in (0, 1):
        packed, after, out, adjusted, info = pc.restated(state, sgs == "none", step == 0, num_tend_out=49)
        for name in G_RECEIVED:
            want = g[label + "received_" + name][step]
            assert pc.same_bits(packed[name], want), (step, name)
            assert not np.isnan(want).any(), (step, name)                     # the reference wrote every element it handed over
        assert list(g[label + "scalars"][step]) == [2.0, 1, 1, ny * nx * nens, 1, nz, 1, 1]
        for k, name in G_STATE.items():
            assert pc.same_bits(out[k], g[label + "out_" + name][step]), (step, name)
        for t, name in enumerate(ref.TRACERS):
            assert pc.same_bits(out["q%d" % t], g[label + "out_" + name][step]), (step, name)
        for k, name in (("rho_d", "density_dry"), ("nccn_prescribed",) * 2, ("nc_nuceat_tend",) * 2, ("ni_activated",) * 2):
            assert pc.same_bits(g[label + "out_" + name][step], state[k]), (step, name)      # what timeStep leaves alone
        if sgs == "none":
            assert set(np.unique(info["branch"])) == {0, 1, 2}               # the fixture's states reach every branch
        state = dict(state, **{k: out[k] for k in ("rho_v", "rho_c", "temp", "q_prev", "t_prev")})
        state["q"] = [out["q%d" % t] for t in range(7)]
    from pam_amd.physics import MicrophysicsP3 as M
    assert list(g[label + "info"]) == [9, 2] + [int(x) for t in M.TRACERS for x in t[2:]]
    assert list(g[label + "consts"]) == [M.R_d, M.cp_d, M.cv_d, M.gamma_d, M.kappa_d, M.R_v, M.cp_v, M.cv_v, M.p0, M.grav, M.cp_l]
    assert list(g[label + "options"]) == [M.latvap, M.latice, M.R_d, M.R_v, M.cp_d, M.cp_v, M.grav, M.p0]
    assert list(g[label + "etime"]) == [2.0, 4.0] and bytes(g[label + "micro"]).rstrip(b"\0") == b"p3"


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "physics", "micro", "p3", "Microphysics.h")), reason="no reference tree at hand")
def test_the_fixture_is_reproduced_from_the_reference_tree():
    r = subprocess.run([sys.executable, os.path.join(pc.ROOT, "tests", "golden", "make_ref_p3_golden.py"), REFERENCE, "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_default_functions_are_the_c_librarys_and_the_devices_pow_stays_within_an_ulp():
    x = np.array([0.3, 0.9, 1.0, 1.1, 3.7])
    y = ref.CONSTS["R_d"] / ref.CONSTS["cp_d"]
    assert list(ref.libm_pow(x, y)) == [math.pow(v, y) for v in x]
    assert np.all(np.abs(emu_harness.emu_pow(x, y) - ref.libm_pow(x, y)) <= np.spacing(ref.libm_pow(x, y)))
    assert ref.saturation_vapor_pressure(280.0) == 610.94 * math.exp(17.625 * (280.0 - 273.15) / (243.04 + (280.0 - 273.15)))


# ------------------------------------------------------------------------------------------------------------------------------
# the host emulation against the restatement

CASES = [(s, a, f) for s in pc.SHAPES for a in (0, 1) for f in (1, 0)]
CASE_IDS = ["%s-adjust%d-first%d" % ("x".join(map(str, s)), a, f) for s, a, f in CASES]


@pytest.mark.parametrize("shape,adjust,first_step", CASES, ids=CASE_IDS)
def test_emulation_matches_restatement_bit_for_bit(shape, adjust, first_step):
    """both layouts: layout 1 is layout 0 transposed and flipped; the adjusted coupler fields and the iteration counts included"""
    state = pc.make_state(shape)
    want = pc.restated_case(shape, adjust, first_step)
    for layout in (0, 1):
        got = pc.emulated(state, layout, adjust, first_step)
        w0 = {k: want[0][k] for k in ref.PACKED}
        pc.assert_set_equal(got[0], w0 if layout == 0 else ref.to_layout1(w0), ref.PACKED, "pack")
        w1 = {k: v for k, v in want[1].items() if k != "p3_tend_out"}
        pc.assert_set_equal(got[1], w1 if layout == 0 else ref.to_layout1(w1), None, "stand-in")
        pc.assert_set_equal(got[2], want[2], pc.STATE_AFTER, "unpack")
        pc.assert_set_equal(got[3], want[3], pc.ADJUSTED, "adjusted")
        if adjust:
            assert np.array_equal(got[4].reshape(shape[0], -1), want[4]["iters"])
        else:
            assert not got[4].any() and all(pc.same_bits(got[3][k], state[k]) for k in pc.ADJUSTED)


def test_emulation_writes_p3_tend_out_in_layout_0():
    state = pc.make_state((5, 1, 7, 3))
    want = pc.restated(state, 0, 1, pow=emu_harness.emu_pow, num_tend_out=49)
    got = pc.emulated(state, 0, 0, 1, num_tend_out=49)
    assert got[1]["p3_tend_out"].shape == (49, 5, 21) and pc.same_bits(got[1]["p3_tend_out"], want[1]["p3_tend_out"])
    assert np.isnan(got[0]["p3_tend_out"]).all()                              # pack does not touch it


@pytest.mark.parametrize("adjust", [0, 1])
def test_emulation_carries_nans_to_the_same_places(adjust):
    shape = (17, 3, 5, 13)
    state = dict(pc.make_state(shape))
    rng = np.random.default_rng(5)
    for k in ("rho_d", "rho_v", "rho_c", "temp", "q_prev", "t_prev", "nc_nuceat_tend"):
        a = np.array(state[k])
        a[rng.random(shape) < 0.01] = np.nan
        state[k] = a
    state["q"] = [np.where(rng.random(shape) < 0.01, np.nan, x) for x in state["q"]]
    want = pc.restated(state, adjust, 0, pow=emu_harness.emu_pow)
    for layout in (0, 1):
        got = pc.emulated(state, layout, adjust, 0)
        pc.assert_set_equal(got[2], want[2], pc.STATE_AFTER, "unpack")
        pc.assert_set_equal(got[3], want[3], pc.ADJUSTED, "adjusted")
    assert np.isnan(want[2]["temp"]).any() and np.isnan(want[2]["rho_c"]).any() and not np.isnan(want[2]["temp"]).all()


@pytest.mark.parametrize("layout", [0, 1])
def test_wide_index_instances_give_the_same_bits(layout):
    state = pc.make_state((17, 3, 5, 13))
    nout = 49 if layout == 0 else 0
    a, b = pc.emulated(state, layout, 1, 1, num_tend_out=nout), pc.emulated(state, layout, 1, 1, wide=True, num_tend_out=nout)
    for stage in (0, 1, 2, 3):
        pc.assert_set_equal(a[stage], b[stage])


@pytest.mark.parametrize("shape", [s for s in pc.SHAPES if np.prod(s) >= 64], ids=[i for s, i in zip(pc.SHAPES, pc.SHAPE_IDS) if np.prod(s) >= 64])
def test_every_branch_is_reached(shape):
    """a census on the test states: every branch of the adjustment, first_step on and off (by construction of the cases), every clamp of
    unpack on both sides"""
    state = pc.make_state(shape)
    for first_step in (1, 0):
        packed, after, out, adjusted, info = pc.restated_case(shape, 1, first_step)
        assert set(np.unique(info["branch"])) == {0, 1, 2}
        assert info["iters"][info["branch"] > 0].min() >= 1 and not info["iters"][info["branch"] == 0].any()
        rd = ref.columns(state["rho_d"])
        for name in ("qc", "nc", "qr", "nr", "qi", "ni", "qm", "bm", "qv"):
            x = after[name] * rd
            assert (x < 0).any() and (x > 0).any(), name
        assert not pc.same_bits(packed["q_prev"], pc.restated_case(shape, 1, 1 - first_step)[0]["q_prev"])


@pytest.mark.parametrize("shape", pc.SHAPES, ids=pc.SHAPE_IDS)
def test_the_seeds_keep_the_exempt_cells_of_the_device_gate_rare(shape):
    """the GPU test exempts cells whose bisection decision margin is below 1e-12 from bit equality.  None is: the restatement alone
    says that the smallest margin of an adjusted cell of the states the tests use is >= 1e-10 (9.1e-10 over the six shapes, first_step
    on and off)"""
    for first_step in (1, 0):
        info = pc.restated_case(shape, 1, first_step)[4]
        adjusted = info["branch"] > 0
        smallest = float(info["margin"][adjusted].min())
        print("%s first_step %d: smallest margin %.3g" % (shape, first_step, smallest))
        assert smallest >= pc.MIN_MARGIN
        assert not ((info["margin"] < pc.MARGIN) & adjusted).any()


# ------------------------------------------------------------------------------------------------------------------------------
# the flat index by value, nothing allocated

NCOL, NLEV, NOUT = 2 ** 26 + 5, 72, 49


def _index(layout, col, k, ncol, nz, plane=0, nplanes=1):
    return (plane * nz + k) * ncol + col if layout == 0 else (col * nplanes + plane) * nz + (nz - 1 - k)


@pytest.mark.parametrize("layout", [0, 1])
def test_offset_by_value_past_2_to_the_31(layout):
    lib = pc.emu()
    last = NOUT * NLEV * NCOL - 1
    assert last > 2 ** 32
    for col, k, p in [(0, 0, 0), (NCOL - 1, NLEV - 1, NOUT - 1), (NCOL - 1, 0, 0), (0, NLEV - 1, 0), (0, 0, NOUT - 1), (2 ** 26 + 1, 35, 6),
                      (12345, 71, 48)]:
        want = _index(layout, col, k, NCOL, NLEV, p, NOUT)
        assert lib.emu_p3_offset(layout, col, k, NCOL, NLEV, p, NOUT, 1) == want, (col, k, p)
        if want < 2 ** 32:
            assert lib.emu_p3_offset(layout, col, k, NCOL, NLEV, p, NOUT, 0) == want, (col, k, p)
    # the p3_tend_out planes: first and last element
    assert lib.emu_p3_offset(0, 0, 0, NCOL, NLEV, 0, NOUT, 1) == 0 and lib.emu_p3_offset(0, NCOL - 1, NLEV - 1, NCOL, NLEV, NOUT - 1, NOUT, 1) == last
    # a cell array and the flux arrays: the corners; an element between 2^31 and 2^32 in both widths; the flip of layout 1
    for nz in (NLEV, NLEV + 1):
        ktop, kbot = nz - 1, 0
        assert lib.emu_p3_offset(layout, NCOL - 1, ktop if layout == 0 else kbot, NCOL, nz, 0, 1, 1) == nz * NCOL - 1 > 2 ** 32
        assert lib.emu_p3_offset(layout, 0, kbot if layout == 0 else ktop, NCOL, nz, 0, 1, 1) == 0
        col, k = (NCOL - 1, 62) if layout == 0 else (58000000, 0)
        want = _index(layout, col, k, NCOL, nz)
        assert 2 ** 31 < want < 2 ** 32
        for wide in (0, 1):
            assert lib.emu_p3_offset(layout, col, k, NCOL, nz, 0, 1, wide) == want
    # col_location: (3, ncol) / (ncol, 3), not flipped
    assert lib.emu_p3_offset(layout, 3, 0, NCOL, 1, 2, 3, 1) == (2 * NCOL + 3 if layout == 0 else 3 * 3 + 2)
    assert lib.emu_p3_offset(layout, NCOL - 1, 0, NCOL, 1, 2, 3, 1) == 3 * NCOL - 1


def test_the_library_picks_the_wide_instances_before_a_byte_offset_passes_32_bits():
    """COUPLING_NARROW in modules_kernels.hip, shared with the SHOC layer: arrays of 2^29 doubles (4 GiB) and more take the long long
    kernels, p3_tend_out included"""
    text = open(os.path.join(pc.ROOT, "pam_amd", "csrc", "modules_kernels.hip")).read()
    assert len(re.findall(r"COUPLING_NARROW = 1ll << 29;", text)) == 1 and "P3_NARROW" not in text
    assert "std::max<long long>(nout, 1) * nz * ncol" in text
    # one narrow expression on the one constant; pack, unpack and the stand-in hand it P3's largest array
    assert len(re.findall(r"\bcoupling_narrow\(bool force_wide, long long largest\) \{ return !force_wide && largest < COUPLING_NARROW; \}", text)) == 1
    assert len(re.findall(r"coupling_narrow\(g_p3_force_wide, p3_largest\(", text)) == 3
    assert (2 ** 29 - 1) * 8 + 7 < 2 ** 32


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI

NEW_SYMBOLS = ("pam_amd_p3_workspace_create", "pam_amd_p3_workspace_args", "pam_amd_p3_workspace_bytes", "pam_amd_p3_workspace_destroy",
               "pam_amd_p3_pack", "pam_amd_p3_unpack", "pam_amd_p3_main_standin", "pam_amd_p3_debug_wide_index")
ISSUE_MEMBERS = ("qc nc qr nr th_atm qv qi qm ni bm pres dz nc_nuceat_tend nccn_prescribed ni_activated inv_qc_relvar precip_liq_surf "
                 "precip_ice_surf diag_eff_radius_qc diag_eff_radius_qi diag_eff_radius_qr bulk_qi precip_total_tend nevapr qr_evap_tend dpres "
                 "inv_exner qv2qi_depos_tend precip_liq_flux precip_ice_flux cld_frac_r cld_frac_l cld_frac_i p3_tend_out mu_c lamc "
                 "liq_ice_exchange vap_liq_exchange vap_ice_exchange q_prev t_prev col_location").split()


def test_new_entry_points_are_exported_and_declared():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(pc.ROOT, "include", "pam_amd_modules.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pam_amd_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.MODULE_SYMBOLS and name in declared, name
    body = re.search(r"typedef struct pam_amd_p3_args_t \{(.*?)\} pam_amd_p3_args_t;", text, flags=re.S).group(1)
    assert tuple(re.findall(r"\*(\w+)", body)) == ("stream",) + capi.P3_ARRAYS == ("stream",) + tuple(ISSUE_MEMBERS) + ("exner",)
    assert [f[0] for f in capi.P3Args._fields_[:13]] == re.findall(r"\b(\w+)\b(?=\s*[,;])", body.split("double *qc")[0].replace("void *", ""))
    assert re.search(r"typedef int \(\*pam_amd_p3_main_fn\)\(const pam_amd_p3_args_t \*\w+, void \*\w+\);", text)


def _refused(lib, who, call):
    assert call() == -1, who                                    # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
    assert who.encode() in lib.pam_amd_awfl_last_error(), (who, lib.pam_amd_awfl_last_error())


CREATE_BAD = [dict(nens=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(layout=2), dict(layout=-1), dict(nout=-1), dict(nout=50, layout=0),
              dict(nout=1, layout=1), dict(nens=2 ** 20, nx=2 ** 10, ny=2)]


@pytest.mark.parametrize("bad", CREATE_BAD, ids=[str(sorted(b.items())) for b in CREATE_BAD])
def test_workspace_create_refuses(bad):
    lib = capi.load()
    a = dict(nens=4, nx=4, ny=6, nz=3, layout=1, nout=0)
    a.update(bad)
    ws = C.c_void_p(1)
    _refused(lib, "p3_workspace_create", lambda: lib.pam_amd_p3_workspace_create(a["nens"], a["nx"], a["ny"], a["nz"], a["layout"], a["nout"],
                                                                                 C.byref(ws)))
    assert not ws.value


def test_workspace_calls_refuse_what_is_no_workspace():
    lib = capi.load()
    _refused(lib, "p3_workspace_create", lambda: lib.pam_amd_p3_workspace_create(4, 4, 6, 3, 1, 0, None))
    n, a = C.c_longlong(), capi.P3Args()
    _refused(lib, "p3_workspace_args", lambda: lib.pam_amd_p3_workspace_args(None, C.byref(a)))
    _refused(lib, "p3_workspace_bytes", lambda: lib.pam_amd_p3_workspace_bytes(None, C.byref(n)))
    assert lib.pam_amd_p3_workspace_destroy(None) == 0
    fake = (C.c_ulonglong * 64)()                               # readable memory without the workspace's mark
    for who, call in (("p3_workspace_args", lambda: lib.pam_amd_p3_workspace_args(fake, C.byref(a))),
                      ("p3_workspace_bytes", lambda: lib.pam_amd_p3_workspace_bytes(fake, C.byref(n))),
                      ("p3_workspace_destroy", lambda: lib.pam_amd_p3_workspace_destroy(fake))):
        _refused(lib, who, call)


P = 1 << 20                                                     # never dereferenced: validation fails first
PACK_OK = [None] + [P] * 4 + [None] + [P] * 6 + [1, 1, 287.042, 461.505, 1004.64, 1859.0, 4188.0, 1.0e5, 9.80616, None]
UNPACK_OK = [None] + [P] * 3 + [None] + [P] * 8 + [1004.64, 717.598, None]
PACK_BAD = [(i, None) for i in list(range(1, 5)) + list(range(6, 12))] + \
           [(i, v) for i in (14, 15, 16, 18, 19, 20) for v in (0.0, -1.0, math.nan, math.inf)] + [(17, math.nan), (17, math.inf)]
UNPACK_BAD = [(i, None) for i in list(range(1, 4)) + list(range(5, 13))] + [(i, v) for i in (13, 14) for v in (0.0, -1.0, math.nan, math.inf)]


@pytest.mark.parametrize("index,value", PACK_BAD, ids=["%d-%s" % b for b in PACK_BAD])
def test_pack_refuses(index, value):
    lib = capi.load()
    args = list(PACK_OK)
    args[index] = value
    _refused(lib, "p3_pack", lambda: lib.pam_amd_p3_pack(*args))
    assert b"workspace" not in lib.pam_amd_awfl_last_error()    # refused for the argument, before the workspace is looked at


def test_pack_accepts_a_negative_cp_v():
    """cv_v = R_v - cp_v is negative as the reference writes it; cp_v itself only has to be finite: the next check (the workspace) refuses"""
    lib = capi.load()
    args = list(PACK_OK)
    args[17] = -1859.0
    _refused(lib, "p3_pack: not a workspace", lambda: lib.pam_amd_p3_pack(*args))


@pytest.mark.parametrize("index,value", UNPACK_BAD, ids=["%d-%s" % b for b in UNPACK_BAD])
def test_unpack_refuses(index, value):
    lib = capi.load()
    args = list(UNPACK_OK)
    args[index] = value
    _refused(lib, "p3_unpack", lambda: lib.pam_amd_p3_unpack(*args))
    assert b"workspace" not in lib.pam_amd_awfl_last_error()


def test_pack_and_unpack_refuse_what_is_no_workspace():
    lib = capi.load()
    fake = (C.c_ulonglong * 64)()
    for ws in (None, fake):
        _refused(lib, "p3_pack: not a workspace", lambda: lib.pam_amd_p3_pack(ws, *PACK_OK[1:]))
        _refused(lib, "p3_unpack: not a workspace", lambda: lib.pam_amd_p3_unpack(ws, *UNPACK_OK[1:]))


def _standin_args(**kw):
    a = capi.P3Args()
    a.ncol, a.nlev, a.dt, a.layout, a.num_tend_out = 24, 3, 1.0, 0, 2
    for n in capi.P3_ARRAYS:
        setattr(a, n, P)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


STANDIN_BAD = [dict(ncol=0), dict(ncol=2 ** 31 - 64), dict(nlev=0), dict(layout=2), dict(num_tend_out=-1), dict(num_tend_out=50),
               dict(layout=1)] + [{n: None} for n in capi.P3_ARRAYS]


@pytest.mark.parametrize("bad", STANDIN_BAD, ids=[next(iter(b)) + "=" + str(next(iter(b.values()))) for b in STANDIN_BAD])
def test_standin_refuses(bad):
    lib = capi.load()
    _refused(lib, "p3_main_standin", lambda: lib.pam_amd_p3_main_standin(C.byref(_standin_args(**bad)), None))


def test_standin_refuses_null_args():
    lib = capi.load()
    _refused(lib, "p3_main_standin", lambda: lib.pam_amd_p3_main_standin(None, None))


def test_python_class_mirrors_the_reference_members():
    from pam_amd import MicrophysicsP3 as M
    from pam_amd.physics import p3_shapes
    m = M()
    assert m.get_num_tracers() == 9 and m.micro_name() == "p3" and m.layout == 1 and m.num_tend_out == 0 and M(layout=0).num_tend_out == 49
    assert m.get_diffused_tracers_indices() == [M.ID_V, M.ID_C, M.ID_R, M.ID_I] == [8, 0, 2, 4] and m.get_num_diffused_tracers() == 4
    assert M.cv_v == M.R_v - M.cp_v < 0 and M.cp_l == 4188.0 and m.first_step and not m.sgs_shoc
    with pytest.raises(capi.PamAmdError, match="layout"):
        M(layout=2)
    with pytest.raises(capi.PamAmdError, match="num_tend_out"):
        M(layout=1, num_tend_out=3)
    s0, s1 = p3_shapes(6, 4, 0, 49), p3_shapes(6, 4, 1)
    assert tuple(s0) == capi.P3_ARRAYS and s0["qc"] == (4, 6) and s1["qc"] == (6, 4) and s0["precip_liq_flux"] == (5, 6)
    assert s1["precip_ice_flux"] == (6, 5) and s0["col_location"] == (3, 6) and s1["col_location"] == (6, 3) and s0["p3_tend_out"] == (49, 4, 6)
    assert s0["precip_liq_surf"] == (6,) and s1["p3_tend_out"] == (6, 0, 4)


# ------------------------------------------------------------------------------------------------------------------------------
# the boundary of the C++ plug-in class

# the member signatures of physics/micro/p3/Microphysics.h, as written there (:93, :97, :101, :108, :214, :886, :889)
SIGNATURES = ("static int constexpr get_num_tracers()", "static auto constexpr get_diffused_tracers_indices()",
              "static auto constexpr get_num_diffused_tracers()", "void init(pam::PamCoupler &coupler)",
              "void timeStep( pam::PamCoupler &coupler )", "void finalize(pam::PamCoupler &coupler)", "std::string micro_name() const")


def test_plugin_header_calls_only_members_the_reference_has():
    import test_boundary_surface as tb
    coupler, dm = tb._used_members(open(MICRO_H).read())
    assert coupler and dm, "scan found no coupler / DataManager calls"
    assert coupler <= tb.REF_COUPLER, sorted(coupler - tb.REF_COUPLER)
    assert dm <= tb.REF_DM, sorted(dm - tb.REF_DM)
    ours = tb._declared(os.path.join(HOST, "pam_coupler.h"))
    assert (coupler | dm) <= ours, sorted((coupler | dm) - ours)


def test_plugin_header_has_the_reference_members():
    import test_boundary_surface as tb
    from pam_amd import MicrophysicsP3 as M
    text = tb._norm(tb._strip_comments(open(MICRO_H).read()))
    for sig in SIGNATURES:
        assert tb._norm(sig) + "{" in text, sig
    assert tb._norm("void set_p3_main(pam_amd_p3_main_fn fn, void *user = nullptr)") + "{" in text
    raw = tb._strip_comments(open(MICRO_H).read())
    for k, v in dict(R_d=287.042, cp_d=1004.64, R_v=461.505, cp_v=1859, p0=1.e5, grav=9.80616, cp_l=4188.0, latvap=2501000.0,
                     latice=333700.0).items():
        m = re.findall(r"\b%s\s*=\s*(-?[0-9.e+]+)\s*;" % k, raw)
        assert [float(x) for x in m] == [float(v)], (k, m)
    assert re.search(r"cv_v\s*=\s*R_v - cp_v;", raw) and "int layout = 1;" in raw
    registered = re.findall(r'register_and_allocate<real>\(\s*"(\w+)"\s*,\s*"([^"]*)"', raw)
    want = list(M.ARRAYS_4D[:5]) + list(M.ARRAYS_3D) + list(M.ARRAYS_4D[5:])
    assert registered == [tuple(w) for w in want]
    tracers = re.findall(r'add_tracer\("(\w+)"\s*,\s*"([^"]*)"\s*,\s*(true|false)\s*,\s*(true|false)\s*\)', raw)
    assert [(n, d, p == "true", m == "true") for n, d, p, m in tracers] == list(M.TRACERS)
    assert 'set_option<std::string>("micro","p3")' in raw
    for k in ("latvap", "latice", "R_d", "R_v", "cp_d", "cp_v", "grav", "p0"):
        assert re.search(r'set_option<real>\("%s"\s*,\s*%s\s*\)' % (k, k), raw), k
    assert "p3_lookup_data_path" not in raw and "p3_lookup_data_path" in open(MICRO_H).read()


def test_the_signatures_are_the_reference_lines():
    """against digests recorded from the reference's header (tests/golden/p3_extract.json): runs without the reference tree"""
    import test_boundary_surface as tb
    rec = json.load(open(EXTRACT))
    ours = tb._norm(tb._strip_comments(open(MICRO_H).read()))
    lines = dict(zip(SIGNATURES, (93, 97, 101, 108, 214, 886, 889)))
    assert sorted(rec["signature_sha256"]) == sorted("physics/micro/p3/Microphysics.h:%d" % ln for ln in lines.values())
    for sig, ln in lines.items():
        assert tb._digest(tb._norm(sig)) == rec["signature_sha256"]["physics/micro/p3/Microphysics.h:%d" % ln], sig
        assert tb._norm(sig) + "{" in ours, sig


def test_plugin_header_compiles_with_the_shoc_plugin_and_the_workalike(tmp_path):
    """the reference's CI plug-in combination: SHOC as SGS, P3 as Microphysics"""
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "physics/micro/p3_amd/Microphysics.h"\n#include "physics/sgs/shoc_amd/SGS.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  Microphysics micro;\n  SGS sgs;\n  micro.init(coupler);\n  sgs.init(coupler);\n"
                   "  sgs.set_shoc_main(pam_amd_shoc_main_standin);\n  micro.set_p3_main(pam_amd_p3_main_standin);\n  sgs.timeStep(coupler);\n"
                   "  micro.timeStep(coupler);\n  static_assert(Microphysics::get_num_tracers() == 9 && Microphysics::ID_V == 8, \"\");\n"
                   "  static_assert(Microphysics::get_num_diffused_tracers() == 4 && Microphysics::get_diffused_tracers_indices()[0] == 8, \"\");\n"
                   "  micro.finalize(coupler);\n  return (int)micro.micro_name().size() + (int)micro.etime;\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]
