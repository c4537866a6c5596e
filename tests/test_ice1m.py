"""The one-moment ice microphysics, everything that needs no GPU: the device bodies under g++ (tests/emu/ice1m_emu.cpp) against the numpy
restatement (tests/ice1m_ref.py) bit for bit on every shape and named case, narrow and wide and with the member axis split; the census of
the branches the named states reach; the guarantees of the contract (water budget, per-cell heat, no negative species, dt == 0, a NaN in
its column); the mutants of the restatement; the C ABI's symbols, signature and refusals; the Python class, the species tables, the C++
class, the driver flag, the bench row and the documents."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import ice1m_ref as ref
import ice1m_cases as ic
from ice1m_harness import EmuBackend, run_split
from pam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pam_amd", "csrc", "host")
BACKENDS = (("restatement", ref.RefBackend), ("emulation", EmuBackend))
FINITE_STATES = ic.STATES          # every named state is finite and non-negative
_EMU = {}


def emu(shape, name, wide=False):
    if (shape, name, wide) not in _EMU:
        _EMU[shape, name, wide] = EmuBackend(wide).run(ic.cases(shape)[name])
    return _EMU[shape, name, wide]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the device bodies under g++

@pytest.mark.parametrize("wide", (False, True), ids=("narrow", "wide"))
@pytest.mark.parametrize("shape", ic.SHAPES, ids=ref.shape_id)
def test_emulation_matches_restatement_bit_for_bit(shape, wide):
    for name in ic.CASE_NAMES:
        assert ref.results_differ(emu(shape, name, wide), ic.reference(shape, name), nan_by_place=True) == [], name


@pytest.mark.parametrize("shape", ic.SHAPES, ids=ref.shape_id)
def test_emulated_pre_pass_gives_the_restatements_sub_cycle_count(shape):
    for name in ic.STATES + ("nan_cell",):
        case = ic.cases(shape)[name]
        assert np.array_equal(EmuBackend().sub_cycles(case), ref.sub_cycles(case)), name


@pytest.mark.parametrize("shape", [s for s in ic.SHAPES if s[3] >= 64], ids=ref.shape_id)
def test_members_split_over_calls_equal_the_whole(shape):
    """calls over the members (0,1), (1,37), (37,nens) with the matching slices of zint: nsub is per column, so nothing can differ"""
    for name in ("mixed_a", "deep_fall", "nan_cell"):
        case, want = ic.cases(shape)[name], ic.reference(shape, name)
        for label, backend in BACKENDS:
            got = run_split(backend(), case, (0, 1, 37, shape[3]))
            assert ref.results_differ(got, want, nan_by_place=True) == [], (name, label)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the census

@pytest.mark.parametrize("shape", [s for s in ic.SHAPES if s[0] >= 2], ids=ref.shape_id)
def test_named_states_reach_every_branch(shape):
    census = ic.census(shape)
    assert set(census) == set(ref.COUNTERS)
    assert [n for n in ref.COUNTERS if census[n] < 1] == []


def test_deep_fall_holds_every_sub_cycle_count_in_one_wavefront():
    for shape in [s for s in ic.SHAPES if s[0] >= 2 and s[3] >= 64]:
        n = ic.trace(shape, "deep_fall")["nsub"].reshape(-1)[:64]
        assert (n == 1).any() and ((n >= 2) & (n <= 8)).any() and (n == ref.MAX_SUB).any(), shape


def test_mixed_states_hold_clear_and_precipitating_columns_in_one_wavefront():
    for shape in [s for s in ic.SHAPES if s[3] >= 64]:
        F = ic.cases(shape)["mixed_a"]["fields"]
        falls = ((F["precip_liquid"] + F["precip_ice"] + F["cloud_ice"]) > 0).any(axis=0).reshape(-1)[:64]
        assert falls.any() and not falls.all(), shape


def test_warm_only_and_cold_only_are_what_they_say():
    for shape in ic.SHAPES:
        warm, cold = ic.cases(shape)["warm_only"]["fields"], ic.cases(shape)["cold_only"]["fields"]
        assert (warm["temp"] > ref.T0).all() and not warm["cloud_ice"].any() and not warm["precip_ice"].any()
        assert (cold["temp"] < ref.TH).all()
        out = ic.reference(shape, "warm_only")
        assert not out["cloud_ice"].any() and not out["precip_ice"].any() and not out["preci"].any(), shape


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the guarantees

@pytest.mark.parametrize("shape", ic.SHAPES, ids=ref.shape_id)
def test_no_species_goes_negative_and_everything_stays_finite(shape):
    for name in FINITE_STATES:
        for label, out in (("restatement", ic.reference(shape, name)), ("emulation", emu(shape, name))):
            for n in ref.OUTPUTS:
                assert np.isfinite(out[n]).all() and (out[n] >= 0).all(), (name, label, n)


@pytest.mark.parametrize("shape", ic.SHAPES, ids=ref.shape_id)
def test_column_water_falls_by_the_surface_precipitation_alone(shape):
    """|M_after - M_before + 1000 dt (precl + preci)| <= (33 nsub + 46) W u per column, the bound derived in ice1m_ref"""
    for name in FINITE_STATES:
        case = ic.cases(shape)[name]
        before = ref.column_water(case["fields"], case["zint"])
        nsub = ic.trace(shape, name)["nsub"]
        for label, out in (("restatement", ic.reference(shape, name)), ("emulation", emu(shape, name))):
            after = ref.column_water(out, case["zint"])
            fallen = 1000.0 * case["dt"] * (out["precl"] + out["preci"])
            miss = np.abs((after - before) + fallen)
            assert (miss <= ref.water_bound(before, nsub)).all(), (name, label, float((miss / before).max()))


@pytest.mark.parametrize("shape", ic.SHAPES, ids=ref.shape_id)
def test_local_processes_keep_the_heat_identity_per_cell(shape):
    """cp_d rd dT = Lv d(rc + rr) + Ls d(ri + rs) over the local part, to u (8 cp_d rd Tmax + 40 Ls w)"""
    for name in FINITE_STATES:
        case, out, was = ic.cases(shape)[name], ic.reference(shape, name), ic.trace(shape, name)["settled"]
        rd, cp_d = case["fields"]["density_dry"], case["cp_d"]
        d = {n: out[n] - was[n] for n in ref.WRITTEN}
        lhs = cp_d * rd * d["temp"]
        rhs = ref.LV * (d["cloud_liquid"] + d["precip_liquid"]) + ref.LS * (d["cloud_ice"] + d["precip_ice"])
        water = np.maximum(sum(out[n] for n in ref.SPECIES), sum(was[n] for n in ref.SPECIES))
        bound = ref.heat_bound(cp_d, rd, np.maximum(out["temp"], was["temp"]), water)
        assert (np.abs(lhs - rhs) <= bound).all(), (name, float((np.abs(lhs - rhs) / bound).max()))
        assert np.abs(rhs).max() > 1.0e3 * bound.max() or shape[0] * shape[3] < 8, name      # the identity is not vacuous


@pytest.mark.parametrize("shape", ic.SHAPES, ids=ref.shape_id)
def test_dt_zero_keeps_every_bit(shape):
    case = ic.cases(shape)["dt_zero"]
    for out in (ic.reference(shape, "dt_zero"), emu(shape, "dt_zero"), emu(shape, "dt_zero", True)):
        for n in ref.WRITTEN:
            assert ref.same_bits(out[n], case["fields"][n]), n
        for n in ("precl", "preci"):
            assert ref.same_bits(out[n], np.zeros(shape[1:])), n


@pytest.mark.parametrize("shape", ic.SHAPES, ids=ref.shape_id)
def test_a_nan_stays_in_its_column(shape):
    k, j, i, e = ic.nan_place(shape)
    clean = ic.reference(shape, "mixed_b")
    for out in (ic.reference(shape, "nan_cell"), emu(shape, "nan_cell")):
        assert np.isnan(out["precip_liquid"][k, j, i, e])
        for n in ref.OUTPUTS:
            a, b = out[n].copy(), clean[n].copy()
            a[..., j, i, e] = b[..., j, i, e] = 0.0
            assert ref.same_bits(a, b), n


def test_inputs_are_not_written():
    shape = ic.SHAPES[3]
    case = ic.cases(shape)["mixed_a"]
    keep = {n: a.copy() for n, a in case["fields"].items()}
    zint = case["zint"].copy()
    EmuBackend().run(case)
    ref.time_step(case)
    assert all(ref.same_bits(case["fields"][n], keep[n]) for n in keep) and ref.same_bits(case["zint"], zint)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the mutants of the restatement

MUTANT_CASE = {"melt_order_swapped": "mixed_a", "evaporate_ice_first": "mixed_a", "unclipped_fall_speed": "deep_fall",
               "global_nsub": "deep_fall"}


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_caught_by_its_named_case(mutant):
    assert set(MUTANT_CASE) == set(ref.MUTANTS)
    shape = (5, 1, 4, 64)
    got = ref.time_step(ic.cases(shape)[MUTANT_CASE[mutant]], mutant=mutant)
    assert ref.results_differ(got, ic.reference(shape, MUTANT_CASE[mutant]), nan_by_place=True) != [], mutant


def test_unclipped_fall_speed_empties_a_cell_beyond_what_it_holds():
    """a sub-cycle of a column at the cap takes more than a cell holds: the cell goes negative, and the next sub-cycle's root makes it a NaN"""
    shape = (5, 1, 4, 64)
    got = ref.time_step(ic.cases(shape)["deep_fall"], mutant="unclipped_fall_speed")
    assert any((np.isnan(got[n]) | (got[n] < 0.0)).any() for n in ref.FALLING)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the C ABI

def test_symbols_and_signature():
    lib = capi.load()
    assert capi.MODULE_SYMBOLS["pam_amd_ice1m_time_step"] == (C.c_int, [C.c_int] * 4 + [C.c_void_p] * 10 + [C.c_double] * 3 + [C.c_void_p])
    assert capi.MODULE_SYMBOLS["pam_amd_ice1m_debug_wide_index"] == (C.c_int, [C.c_int])
    assert hasattr(lib, "pam_amd_ice1m_time_step") and hasattr(lib, "pam_amd_ice1m_debug_wide_index")
    header = open(os.path.join(ROOT, "include", "pam_amd_modules.h")).read()
    assert "int pam_amd_ice1m_time_step(int nens, int nx, int ny, int nz, double *rho_v, double *rho_c, double *rho_i, double *rho_r," in header
    assert lib.pam_amd_ice1m_debug_wide_index(1) == 0 and lib.pam_amd_ice1m_debug_wide_index(0) == 0


def test_refusals_come_before_any_device_call():
    lib = capi.load()
    nens, nx, ny, nz = 3, 2, 1, 4
    cells, level = nens * nx * ny * nz, nens * nx * ny
    buf = np.zeros(8 * cells + 2 * level + (nz + 1) * nens)
    base = buf.ctypes.data
    ptrs = [base + 8 * cells * i for i in range(7)]                       # rv rc ri rr rs rd temp
    precl, preci = base + 8 * cells * 7, base + 8 * cells * 7 + 8 * level
    zint = base + 8 * cells * 7 + 16 * level

    def call(sizes=(nens, nx, ny, nz), p=None, dt=10.0, R_v=461.0, cp_d=1003.0):
        p = list(p if p is not None else ptrs + [precl, preci, zint])
        return lib.pam_amd_ice1m_time_step(*sizes, *p, dt, R_v, cp_d, None)

    good = ptrs + [precl, preci, zint]
    refused = [call(sizes=s) for s in ((0, nx, ny, nz), (nens, 0, ny, nz), (nens, nx, -1, nz), (nens, nx, ny, 0))]
    refused += [call(p=good[:i] + [None] + good[i + 1:]) for i in range(10)]
    refused += [call(dt=v) for v in (-1.0, math.nan, math.inf)]
    refused += [call(R_v=0.0), call(cp_d=math.nan)]
    overlap = list(good)
    overlap[2] = good[1] + 8                                               # rho_i inside rho_c
    refused.append(call(p=overlap))
    overlap = list(good)
    overlap[8] = good[7]                                                   # preci is precl
    refused.append(call(p=overlap))
    overlap = list(good)
    overlap[5] = good[0]                                                   # rho_dry is rho_v
    refused.append(call(p=overlap))
    assert refused == [-1] * len(refused)
    assert b"ice1m" in lib.pam_amd_awfl_last_error()
    assert not buf.any()                                                    # nothing written
    import torch
    if not torch.cuda.is_available():
        assert call() == -2 and call(dt=0.0) == -2                          # PAM_AMD_ENOGPU: the arguments pass, a zero dt included


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the layers above

def test_python_class_has_the_members_of_microphysics():
    import pam_amd
    from pam_amd import micro
    assert pam_amd.MicrophysicsIce is micro.MicrophysicsIce
    M = pam_amd.MicrophysicsIce
    assert M.get_num_tracers() == 5 and M.micro_name() == "ice1m"
    for member in ("init", "timeStep", "compute_total_mass", "finalize"):
        assert callable(getattr(M, member)) and callable(getattr(pam_amd.Microphysics, member))
    assert tuple(t[0] for t in M.TRACERS) == ref.SPECIES
    for k in ("R_d", "R_v", "cp_d", "cp_v", "grav", "p0"):
        assert getattr(M, k) == getattr(pam_amd.Microphysics, k)
    assert (M.R_v, M.cp_d) == (ic.CONSTANTS["R_v"], ic.CONSTANTS["cp_d"])


def test_species_tables_have_the_ice1m_row_and_keep_the_others():
    from pam_amd import modules, physics
    assert physics.RadiationGray.CONDENSATE_ICE1M == {"ice1m": (("cloud_liquid",), ("cloud_ice",))}
    assert physics.SGSSmagorinsky.CONDENSATE_ICE1M == {"ice1m": (("cloud_liquid", "cloud_ice"), ("precip_liquid", "precip_ice"))}
    assert modules.SATURATION_CONDENSATE == {"kessler": "cloud_liquid", "p3": "cloud_water", "ice1m": "cloud_liquid"}
    assert modules.MSA_CONDENSATE == {"kessler": ("cloud_liquid", None), "p3": ("cloud_water", "ice"), "none": (None, None),
                                      "ice1m": ("cloud_liquid", "cloud_ice")}
    assert '"preci"' in inspect.getsource(modules._column_diagnostics_names)


CXX_TABLES = ("physics/radiation/gray_amd/radiation.h", "physics/sgs/smag_amd/SGS.h", "modules/saturation_adjustment.h",
              "modules/radiation_aggregate.h", "modules/column_diagnostics.h", "modules/flux_profiles.h", "modules/mean_state_acceleration.h",
              "modules/variance_transport.h", "modules/crm_feedback.h")


@pytest.mark.parametrize("header", CXX_TABLES)
def test_cxx_species_tables_have_the_ice1m_row(header):
    text = open(os.path.join(HOST, header)).read()
    assert '"ice1m"' in text and '"cloud_ice"' in text or '"ice1m"' in text and "cloud_ice" in text, header
    assert '"kessler"' in text and '"p3"' in text, header


def test_shoc_and_p3_keep_refusing_other_schemes():
    for header in ("physics/sgs/shoc_amd/SGS.h", "physics/micro/p3_amd/Microphysics.h"):
        assert "ice1m" not in open(os.path.join(HOST, header)).read(), header
    from pam_amd import physics
    assert "ice1m" not in inspect.getsource(physics.SGSShoc)


def test_cxx_class_driver_tool_and_documents_know_the_scheme(tmp_path):
    from tools.native_build import syntax_check
    cls = os.path.join(HOST, "physics", "micro", "ice_amd", "Microphysics.h")
    text = open(cls).read()
    for s in ("num_tracers = 5", '"ice1m"', "pam_amd_ice1m_time_step(", '"water_vapor"', '"cloud_liquid"', '"cloud_ice"', '"precip_liquid"',
              '"precip_ice"', '"precl"', '"preci"', "compute_total_mass", "finalize", "timeStep", "micro_name"):
        assert s in text, s
    src = tmp_path / "tu.cpp"               # the class under its own name, and beside Kessler's under another, as the driver holds them
    src.write_text('#include "pam_coupler.h"\n#include "physics/micro/kessler_amd/Microphysics.h"\n#define PAM_MICRO_CLASS MicrophysicsIce\n'
                   '#include "physics/micro/ice_amd/Microphysics.h"\n#undef PAM_MICRO_CLASS\n'
                   "int main() {\n  pam::PamCoupler coupler;\n  Microphysics k;\n  MicrophysicsIce m;\n  m.init(coupler);\n  m.timeStep(coupler);\n"
                   "  real w = m.compute_total_mass(coupler);\n  m.finalize(coupler);\n  return m.micro_name() == \"ice1m\" && w >= 0 ? 0 : 1;\n}\n")
    r = syntax_check(src)
    assert r.returncode == 0, r.stderr[-2000:]
    drv = open(os.path.join(ROOT, "examples", "driver.cpp")).read()
    assert drv.count('"--micro-ice"') == 1 and "micro ice:" in drv and drv.count("[--micro-ice]") >= 2
    tool = open(os.path.join(ROOT, "tools", "bench_modules.py")).read()
    assert '"ice1m"' in tool and "pam_amd_ice1m_time_step" in tool
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ice1m" in open(os.path.join(ROOT, doc)).read(), doc
    assert "untuned" in open(os.path.join(ROOT, "README.md")).read().split("ice1m", 1)[1][:3000]


def test_kernel_resource_table_shows_no_scratch():
    """the committed compiler table: both instances, no scratch, no LDS (columns: VGPR AGPR SGPR scratch w/SIMD LDS instr)"""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "r21_ice1m_kernel_resources.txt")):
        if line.startswith("ice1m_kernel"):
            parts = line.split()
            rows[" ".join(parts[:-7])] = [int(v) for v in parts[-7:]]
    assert sorted(rows) == ["ice1m_kernel<long long>", "ice1m_kernel<unsigned int>"], rows
    for name, (vgpr, agpr, sgpr, scratch, waves, lds, instr) in rows.items():
        assert scratch == 0 and lds == 0 and agpr == 0 and 0 < vgpr <= 512 and waves >= 1, (name, rows[name])
