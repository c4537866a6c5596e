"""Explicit scalar momentum transport without a GPU: the closed form of the pressure solve, the mutants of the restatement, the device
bodies under g++ against the restatement (tests/esmt_ref.py) bit for bit, the properties of the contract, the refusals of the C ABI and
the layers above it."""
import math
import os
import subprocess

import numpy as np
import pytest

import esmt_ref as ref
import esmt_cases as ec
from esmt_harness import EmuBackend
from pam_amd import capi
from tools.native_build import cxx_program, syntax_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
BACKENDS = (("restatement", ref.RefBackend), ("emulation", EmuBackend))
RD, RV = ref.RD, ref.RV
EPS = 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the closed form: on a uniform grid with constant rho_mean and linear shear G, w = cos(pi l (k + 1/2) / nz) cos(2 pi m0 i / nx - phi)
# is a discrete eigenvector of the operator, so T = 2 kap^2 G w / (lam_l + kap^2), lam_l = (2 - 2 cos(pi l / nz)) / dz^2

CLOSED = ((8, 6, 0, 1), (8, 6, 2, 4), (7, 5, 1, 3), (65, 12, 3, 5), (32, 60, 7, 16))
CLOSED_GATE = 1.0e-12      # 70 times the worst value a numpy probe of the contract gave (1.4e-14); every mistake this is for gives order one


def closed_form_errors(case, mutant=None):
    """-> max |T - exact| / max |exact| and max over levels of |sum_i T| / max |T|"""
    nx, nz, l, m0 = case
    dz, dx, G, rho = 250.0, 500.0, 3.0e-3, 1.1
    phi = 0.0 if 2 * m0 == nx else 0.7
    k, i = np.arange(nz)[:, None], np.arange(nx)[None, :]
    w = (np.cos(np.pi * l * (k + 0.5) / nz) * np.cos(2.0 * np.pi * m0 * i / nx - phi))[:, :, None]
    z, h = ((np.arange(nz) + 0.5) * dz)[:, None], np.full((nz, 1), dz)
    Ct, St = ref.tables(nx)
    T = ref.force(w, np.full((nz, 1), rho), {"u": G * z}, z, h, Ct, St, dx, nx // 2, mutant)["u"]
    kap, lam = 2.0 * np.pi * m0 / (nx * dx), (2.0 - 2.0 * np.cos(np.pi * l / nz)) / dz ** 2
    exact = 2.0 * kap ** 2 * G * w / (lam + kap ** 2)
    return np.abs(T - exact).max() / np.abs(exact).max(), np.abs(T.sum(axis=1)).max() / np.abs(T).max()


@pytest.mark.parametrize("case", CLOSED, ids=lambda c: "nx%d-nz%d-l%d-m%d" % c)
def test_the_solve_matches_the_closed_form(case):
    err, total = closed_form_errors(case)
    print("closed form", case, "error %.3e" % err, "x sum %.3e" % total)
    assert err <= CLOSED_GATE and total <= CLOSED_GATE


def test_the_closed_form_through_the_emulated_kernels():
    """the same eigenvector through diagnose and the force of the device bodies: esmt_u = rho (G z), one member, no forcing"""
    nx, nz, l, m0 = 8, 6, 2, 3
    dz, dx, G, rho, dt = 250.0, 500.0, 3.0e-3, 1.0, 10.0
    k, i = np.arange(nz)[:, None], np.arange(nx)[None, :]
    w = (np.cos(np.pi * l * (k + 0.5) / nz) * np.cos(2.0 * np.pi * m0 * i / nx - 0.7))[:, None, :, None]
    z = ((np.arange(nz) + 0.5) * dz)[:, None]
    full = (nz, 1, nx, 1)
    Ct, St = ref.tables(nx)
    us = np.broadcast_to((G * z)[:, None, None, :], full)
    case = dict(ec.CONSTANTS, fields={RD: np.full(full, rho), RV: np.zeros(full), "wvel": np.ascontiguousarray(w),
                                      "esmt_u": np.ascontiguousarray(rho * us), "esmt_v": np.zeros(full)},
                zmid=z, dz=np.full((nz, 1), dz), cos=Ct, sin=St, kmax=nx // 2, dx=dx, dt=dt)
    got = EmuBackend().run(case)
    kap, lam = 2.0 * np.pi * m0 / (nx * dx), (2.0 - 2.0 * np.cos(np.pi * l / nz)) / dz ** 2
    exact = rho * us + rho * dt * (2.0 * kap ** 2 * G * w / (lam + kap ** 2))
    assert np.abs(got["esmt_u"] - exact).max() / np.abs(exact - rho * us).max() <= CLOSED_GATE
    assert ref.same_bits(got["esmt_v"], case["fields"]["esmt_v"])


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the mutants of the restatement: each is caught by the closed form or by a bit comparison on a named case

def test_mutants_of_the_restatement_are_caught():
    assert set(ref.MUTANTS) == {"nyquist_scale", "sine_sign", "a_c_swapped", "centred_end_gradient", "k2_not_doubled", "plain_mean"}
    for mutant in ref.MUTANTS:
        by_form = [c for c in CLOSED if max(closed_form_errors(c, mutant)) > CLOSED_GATE]
        by_bits = [s for s in ec.SHAPES if ref.results_differ(ref.pgf(ec.cases(s)["all_on"], mutant), ec.reference(s, "all_on"))]
        assert by_form or by_bits, mutant
        if mutant == "plain_mean":
            assert by_bits and not by_form             # the closed form takes its means as given
            case = ec.cases((5, 65, 70))["all_on"]
            assert ref.results_differ(ref.diagnose(case, mutant=mutant), ref.diagnose(case)) != []
        else:
            assert by_form, mutant
        if mutant == "nyquist_scale":                  # only an even nx has the wavenumber
            assert all(2 * c[3] == c[0] for c in by_form) and all(s[1] % 2 == 0 for s in by_bits)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the device bodies under g++ against the restatement

@pytest.mark.parametrize("wide", (False, True), ids=("narrow", "wide"))
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape, wide):
    """every named case; the index width is the only path that depends on the size"""
    be = EmuBackend(wide)
    for name in ec.CASE_NAMES:
        assert ref.results_differ(be.run(ec.cases(shape)[name]), ec.reference(shape, name), nan_by_place=True) == [], name


@pytest.mark.parametrize("shape", ec.SHAPES, ids=ref.shape_id)
def test_emulated_set_and_diagnose_match_restatement_bit_for_bit(shape):
    case = ec.cases(shape)["all_on"]
    F = case["fields"]
    for feedback in (False, True):
        got, want = EmuBackend().diagnose(case, feedback), ref.diagnose(case, feedback)
        assert sorted(got) == sorted(want) == ["rho_mean", "tend_u", "tend_v", "u_mean", "v_mean"]
        assert ref.results_differ(got, want) == [], feedback
    with_f, with_b = ref.diagnose(case, False), ref.diagnose(case, True)
    assert ref.same_bits(with_f["tend_u"], -with_b["tend_u"])
    without = EmuBackend().diagnose(dict(case, gcm_u=None), False)
    assert "tend_u" not in without and ref.same_bits(without["tend_v"], with_f["tend_v"])
    eu, ev = EmuBackend().set(F[RD], F[RV], case["gcm_u"], case["gcm_v"])
    wu, wv = ref.set_scalars(F[RD], F[RV], case["gcm_u"], case["gcm_v"])
    assert ref.same_bits(eu, wu) and ref.same_bits(ev, wv)


@pytest.mark.parametrize("shape", [s for s in ec.SHAPES if s[2] >= 64], ids=ref.shape_id)
def test_members_split_over_calls_equal_the_whole(shape):
    nens = shape[2]
    for name in ("all_on", "nan_w"):
        case, want = ec.cases(shape)[name], ec.reference(shape, name)
        parts = [EmuBackend().run(ref.members(case, slice(lo, hi))) for lo, hi in ((0, 1), (1, 6), (6, nens))]
        got = {n: np.concatenate([p[n] for p in parts], axis=-1) for n in want}
        assert ref.results_differ(got, want, nan_by_place=True) == [], name


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the properties of the contract, on the named cases, for the restatement and for the emulated kernels

@pytest.mark.parametrize("label,backend", BACKENDS, ids=[b[0] for b in BACKENDS])
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ref.shape_id)
def test_no_shear_and_no_forcing_keeps_every_bit(shape, label, backend):
    case = ec.cases(shape)["no_force"]
    flat_u, flat_v = ec.no_shear(shape[2])
    got = backend().run(case)
    for n, flat in (("esmt_u", flat_u), ("esmt_v", flat_v)):
        assert ref.same_bits(got[n][..., flat], case["fields"][n][..., flat]), n
        if (~flat).any() and shape[1] > 2:
            assert not ref.same_bits(got[n][..., ~flat], case["fields"][n][..., ~flat]), n
    nothing = backend().run(ec.cases(shape)["kmax0_no_force"])
    assert ref.results_differ(nothing, {n: case["fields"][n] for n in ref.SCALARS}) == []


@pytest.mark.parametrize("label,backend", BACKENDS, ids=[b[0] for b in BACKENDS])
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ref.shape_id)
def test_kmax_zero_applies_the_uniform_forcing_alone(shape, label, backend):
    case = ec.cases(shape)["kmax0"]
    F, dt = case["fields"], np.float64(case["dt"])
    rho = F[RD] + F[RV]
    got = backend().run(case)
    for x in "uv":
        assert ref.same_bits(got["esmt_" + x], F["esmt_" + x] + rho * (dt * case["force_" + x])[:, None, None, :]), x


@pytest.mark.parametrize("label,backend", BACKENDS, ids=[b[0] for b in BACKENDS])
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ref.shape_id)
def test_a_nan_stays_in_its_own_member(shape, label, backend):
    k, i, e = ec.nan_place(shape)
    got, clean = backend().run(ec.cases(shape)["nan_w"]), backend().run(ec.cases(shape)["no_force"])
    flat_u, flat_v = ec.no_shear(shape[2])
    others = np.arange(shape[2]) != e
    for n, flat in (("esmt_u", flat_u), ("esmt_v", flat_v)):
        assert np.isnan(got[n][..., e]).all(), n        # 0 NaN is a NaN too: a member without shear does not hide it
        assert ref.same_bits(got[n][..., others], clean[n][..., others]), n


@pytest.mark.parametrize("label,backend", BACKENDS, ids=[b[0] for b in BACKENDS])
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ref.shape_id)
def test_the_force_leaves_the_level_means_alone_and_the_forcing_moves_them_by_dt_f(shape, label, backend):
    be = backend()
    for name in ("no_force", "all_on", "shared_grid"):
        case = ec.cases(shape)[name]
        F, dt = case["fields"], case["dt"]
        rho = F[RD] + F[RV]
        got = be.run(case)
        quiet = ec.reference(shape, "no_force") if name != "shared_grid" else ref.pgf(dict(case, force_u=None, force_v=None))
        T_max = max(np.abs((quiet[n] - F[n]) / (rho * dt)).max() for n in ref.SCALARS)
        bound = ec.mean_bound(case, T_max)
        for x in "uv":
            before, after = ref.level_mean(F["esmt_" + x] / rho), ref.level_mean(got["esmt_" + x] / rho)
            want = dt * case["force_" + x] if case.get("force_" + x) is not None else 0.0
            worst = np.abs(after - before - want).max()
            print(shape, name, x, "drift %.3e" % worst, "bound %.3e" % bound)
            assert worst <= bound, (name, x)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the C ABI: its symbols; refusals before any device is asked for; the answer without a device

def test_capi_symbols_and_the_tables():
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read()
    for s in ("pam_amd_esmt_set", "pam_amd_esmt_diagnose", "pam_amd_esmt_pgf", "pam_amd_esmt_workspace_doubles", "pam_amd_esmt_tables",
              "pam_amd_esmt_debug_wide_index"):
        assert s in capi.MODULE_SYMBOLS and getattr(lib, s) is not None and s + "(" in header
    assert len(capi.MODULE_SYMBOLS["pam_amd_esmt_pgf"][1]) == 24 and len(capi.MODULE_SYMBOLS["pam_amd_esmt_diagnose"][1]) == 18
    assert lib.pam_amd_esmt_debug_wide_index(1) == 0 and lib.pam_amd_esmt_debug_wide_index(0) == 0
    assert lib.pam_amd_esmt_workspace_doubles(70, 60, 16) == 6 * 16 * 60 * 70 <= 3 * 60 * 32 * 70
    assert lib.pam_amd_esmt_workspace_doubles(3, 5, 0) == 0
    for nx in (2, 7, 8, 65):
        cos, sin = np.full(nx + 1, 7.25), np.full(nx + 1, 7.25)
        assert lib.pam_amd_esmt_tables(nx, cos.ctypes.data, sin.ctypes.data) == 0
        Ct, St = ref.tables(nx)
        assert cos[nx] == 7.25 and sin[nx] == 7.25 and cos[0] == 1.0 and sin[0] == 0.0
        assert np.abs(cos[:nx] - Ct).max() <= 2.0 * EPS and np.abs(sin[:nx] - St).max() <= 2.0 * EPS      # two libraries, one ulp at the most
    assert lib.pam_amd_esmt_tables(1, cos.ctypes.data, sin.ctypes.data) == -1
    assert lib.pam_amd_esmt_tables(4, None, sin.ctypes.data) == -1


NENS, NX, NZ, KMAX = 4, 6, 3, 3
CELLS, ROWS = NENS * NX * NZ, NZ * NENS
WORDS = 6 * KMAX * ROWS


def _abi():
    """host arrays filled with a pattern, and the three calls over them with keyword overrides"""
    lib = capi.load()
    names = ("eu", "ev", "w", "rd", "rv", "zmid", "dz", "rm", "um", "vm", "fu", "fv", "cos", "sin", "gu", "gv", "tu", "tv", "su", "sv", "work", "spare")
    arrays = [np.full(max(CELLS, WORDS) + 16, 7.25) for _ in names]
    P = dict(zip(names, [a.ctypes.data for a in arrays]))
    good = dict(nens=NENS, nx=NX, ny=1, nz=NZ, dx=500.0, dt=10.0, gcm_dt=1200.0, kmax=KMAX, words=WORDS, feedback=0, **{n: n for n in names})

    def args(kw):
        a = dict(good)
        a.update(kw)
        return a, lambda key: None if a[key] is None else (P[a[key]] if isinstance(a[key], str) else a[key])

    def pgf(**kw):
        a, p = args(kw)
        return lib.pam_amd_esmt_pgf(a["nens"], a["nx"], a["ny"], a["nz"], p("eu"), p("ev"), p("w"), p("rd"), p("rv"), p("zmid"), p("dz"), p("rm"),
                                    p("um"), p("vm"), p("fu"), p("fv"), p("cos"), p("sin"), a["dx"], a["dt"], a["kmax"], p("work"), a["words"], None)

    def diagnose(**kw):
        a, p = args(kw)
        return lib.pam_amd_esmt_diagnose(a["nens"], a["nx"], a["ny"], a["nz"], p("rd"), p("rv"), p("eu"), p("ev"), p("rm"), p("um"), p("vm"), p("gu"),
                                         p("gv"), a["gcm_dt"], a["feedback"], p("tu"), p("tv"), None)

    def set_(**kw):
        a, p = args(kw)
        return lib.pam_amd_esmt_set(a["nens"], a["nx"], a["ny"], a["nz"], p("rd"), p("rv"), p("su"), p("sv"), p("eu"), p("ev"), None)
    return lib, arrays, P, pgf, diagnose, set_


def test_entry_points_reject_bad_arguments_and_leave_the_arrays_untouched():
    """the pointers are host arrays here: a refusal comes before the first HIP call, so nothing dereferences them, and afterwards every
    array still holds the pattern it was filled with"""
    lib, arrays, P, pgf, diagnose, set_ = _abi()
    bad = (0.0, -1.0, math.nan, math.inf)
    sizes = [dict(ny=2), dict(ny=0), dict(nz=1), dict(nx=1), dict(nens=0), dict(nz=65536)]
    last = 8 * CELLS - 8
    calls = sizes + [dict(kmax=-1), dict(kmax=NX // 2 + 1)]
    calls += [{n: None} for n in ("eu", "ev", "w", "rd", "rv", "zmid", "dz", "rm", "cos", "sin", "work")]
    calls += [dict(um=None), dict(vm=None), dict(um=None, vm=None, fu=None)]                                 # a force without its scalar's mean
    calls += [{n: b} for n in ("dt", "dx") for b in bad]
    calls += [dict(words=WORDS - 1), dict(words=0)]
    calls += [dict(eu="ev"), dict(eu="w"), dict(ev="rd"), dict(eu=P["rv"] + last), dict(ev=P["zmid"] + 8 * ROWS - 8), dict(um="eu"),
              dict(fu=P["ev"] + last), dict(cos=P["eu"] + last), dict(work="eu"), dict(work=P["w"] + last), dict(work=P["sin"] + 8 * NX - 8),
              dict(rm=P["work"] + 8 * WORDS - 8), dict(fv="work")]
    for i, kw in enumerate(calls):
        assert pgf(**kw) == -1, (i, kw)                              # PAM_AMD_EINVAL, not PAM_AMD_ENOGPU: no device was asked
        assert lib.pam_amd_awfl_last_error().startswith(b"esmt_pgf: "), i
        assert all((a == 7.25).all() for a in arrays), i
    calls = sizes + [{n: None} for n in ("rd", "rv", "eu", "ev", "rm", "um", "vm")]
    calls += [dict(gu=None), dict(tv=None), dict(gu=None, tu=None, tv=None)] + [dict(gcm_dt=b) for b in bad]
    calls += [dict(rm="um"), dict(um=P["eu"] + last), dict(tu="tv"), dict(tu="gu"), dict(tv=P["rm"] + 8 * ROWS - 8), dict(vm="rd")]
    for i, kw in enumerate(calls):
        assert diagnose(**kw) == -1, (i, kw)
        assert lib.pam_amd_awfl_last_error().startswith(b"esmt_diagnose: "), i
        assert all((a == 7.25).all() for a in arrays), i
    calls = sizes + [{n: None} for n in ("rd", "rv", "su", "sv", "eu", "ev")] + [dict(eu="ev"), dict(eu="rd"), dict(ev=P["su"] + 8 * ROWS - 8)]
    for i, kw in enumerate(calls):
        assert set_(**kw) == -1, (i, kw)
        assert lib.pam_amd_awfl_last_error().startswith(b"esmt_set: "), i
        assert all((a == 7.25).all() for a in arrays), i


def test_entry_points_answer_without_a_device_and_nothing_to_do_launches_nothing():
    import torch
    lib, arrays, P, pgf, diagnose, set_ = _abi()
    # nothing to do is no error and asks for no device: kmax == 0 (the workspace may be absent) or no mean, and no force
    assert pgf(kmax=0, fu=None, fv=None, work=None, words=0) == 0
    assert pgf(um=None, vm=None, fu=None, fv=None) == 0
    if not torch.cuda.is_available():
        for kw in (dict(), dict(kmax=0, work=None, words=0), dict(fu=None, fv=None), dict(vm=None, fv=None), dict(kmax=1), dict(nx=2, kmax=1)):
            assert pgf(**kw) == -2, kw
            assert lib.pam_amd_awfl_last_error() == b"esmt_pgf: no HIP device available (this library has no CPU path)"
        for kw in (dict(), dict(gu=None, tu=None), dict(gu=None, tu=None, gv=None, tv=None, gcm_dt=0.0), dict(feedback=1)):
            assert diagnose(**kw) == -2, kw
        assert set_() == -2
    assert all((a == 7.25).all() for a in arrays)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the layers above: the Python functions on a host coupler, the C++ module, the driver, the tool, the documents

def _host_coupler(nz=4, ny=1, nx=6, nens=5):
    from pam_amd import PamCoupler
    coupler = PamCoupler("cpu")
    coupler.set_option("crm_dt", 10.0)
    coupler.allocate_coupler_state(nz, ny, nx, nens)
    coupler.set_grid(500.0 * nx, 500.0 * ny, np.linspace(0.0, 4000.0, nz + 1))
    return coupler


def test_init_registers_the_tracers_the_profiles_the_tables_and_the_workspace():
    from pam_amd import modules
    from pam_amd.capi import PamAmdError
    coupler = _host_coupler()
    with pytest.raises(PamAmdError, match="call esmt_init first"):
        modules.esmt_pgf(coupler)
    modules.esmt_init(coupler)
    dm = coupler.get_data_manager_device_readwrite()
    assert coupler.get_tracer_names() == ["esmt_u", "esmt_v"] and coupler.get_option("esmt_kmax") == 3
    for n in modules.ESMT_SCALARS:
        assert coupler.get_tracer_info(n)[1:] == (True, False, False) and tuple(dm.get(n).shape) == (4, 1, 6, 5)
    assert [n for n, _ in modules.ESMT_PROFILES] == ["esmt_rho_mean", "esmt_u_mean", "esmt_v_mean", "esmt_u_forcing", "esmt_v_forcing",
                                                     "esmt_u_tend", "esmt_v_tend"]
    for n, _ in modules.ESMT_PROFILES:
        assert tuple(dm.get(n).shape) == (4, 5) and (dm.get(n) == 0).all()
    Ct, St = ref.tables(6)
    assert np.abs(dm.get("esmt_cos").numpy() - Ct).max() <= 2.0 * EPS and np.abs(dm.get("esmt_sin").numpy() - St).max() <= 2.0 * EPS
    assert dm.get("esmt_workspace").numel() == 6 * 3 * 4 * 5
    with pytest.raises(PamAmdError, match="called twice"):
        modules.esmt_init(coupler)
    coupler = _host_coupler()
    modules.esmt_init(coupler, kmax=1)
    assert coupler.get_option("esmt_kmax") == 1 and coupler.get_data_manager_device_readwrite().get("esmt_workspace").numel() == 6 * 4 * 5
    for kw, shape in ((dict(kmax=4), {}), (dict(kmax=-1), {}), ({}, dict(ny=2)), ({}, dict(nx=1))):
        with pytest.raises(PamAmdError, match="esmt_init"):
            modules.esmt_init(_host_coupler(**shape), **kw)
    with pytest.raises(PamAmdError, match="source must be"):
        modules.esmt_set(coupler, source="nowhere")


def test_cxx_module_compiles(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "pam_coupler.h"\n#include "modules/scalar_momentum.h"\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  modules::esmt_init(coupler);\n  modules::esmt_init(coupler, 3);\n"
                   '  modules::esmt_set(coupler);\n  modules::esmt_set(coupler, "crm");\n  modules::esmt_compute_forcing(coupler);\n'
                   "  modules::esmt_pgf(coupler);\n  modules::esmt_pgf(coupler, 5.0, false);\n  modules::esmt_compute_feedback(coupler);\n  return 0;\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cxx_program_reports_the_refusals_and_the_answer_without_a_device():
    """tests/cxx/scalar_momentum.cpp builds against the header and the library and calls the entry points directly with host arrays: a
    line per refusal, then the three calls that pass every check, PAM_AMD_ENOGPU where there is no device"""
    import torch
    r = subprocess.run([cxx_program("scalar_momentum")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    lines = r.stdout.strip().split("\n")
    refusals = [l for l in lines if l.startswith("### refuse ")]
    assert len(refusals) == 12 and all(l.endswith(" -1") for l in refusals), refusals
    assert "### nothing 0 0" in lines
    if not torch.cuda.is_available():
        assert "### rc -2 -2 -2" in lines


def test_cxx_module_and_python_functions_name_the_same_entries_and_options():
    import inspect
    from pam_amd import modules
    text = open(os.path.join(HOST, "modules", "scalar_momentum.h")).read()
    py = inspect.getsource(modules)
    for n, desc in modules.ESMT_PROFILES:
        assert '"%s"' % n in text and desc in text, n
    for s in ('"esmt_u"', '"esmt_v"', '"esmt_cos"', '"esmt_sin"', '"esmt_workspace"', '"esmt_kmax"', '"gcm_uvel"', '"gcm_vvel"', '"gcm_physics_dt"',
              '"vertical_cell_dz"', "pam_amd_esmt_set(", "pam_amd_esmt_diagnose(", "pam_amd_esmt_pgf(", "pam_amd_esmt_tables(", "pam_amd_msa_diagnose("):
        assert s in text and s in py, s


def test_driver_bench_tool_and_documents_know_esmt():
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert drv.count('"--esmt"') == 1 and drv.count("[--esmt [KMAX]]") >= 2 and "esmt: etime" in drv
    assert drv.index("modules::sponge_layer);") < drv.index("modules::esmt_pgf(c") < drv.index("sgs_smag.timeStep(c)")
    tool = open(os.path.join(ROOT, "tools", "bench_modules.py")).read()
    assert '"esmt"' in tool and "pam_amd_esmt_pgf" in tool and "pam_amd_esmt_diagnose" in tool
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "esmt_pgf" in open(os.path.join(ROOT, doc)).read(), doc
    rows = open(os.path.join(ROOT, "profiles", "r22_esmt_kernel_resources.txt")).read().split("\n")
    kernels = [l.split() for l in rows if l.startswith("esmt_")]
    assert len(kernels) == 8 and all(k[-4] == "0" for k in kernels)      # no scratch
