"""The coupler-module kernels at the sizes that select their `long long` instances, and just below them at the edge of the 32-bit ones
(pam_amd/csrc/modules_kernels.hip; DESIGN.md section 8, "Index width").

The reference of a whole-ensemble run is the same entry point run on member chunks [lo, hi): a chunk is a few 1e4 .. 1e5 members, less
than 1/8 of a threshold, so it takes the 32-bit instance far from its edge.  README and DESIGN promise that a member's result does not
depend on how many members the call holds; at these sizes that promise is "long long instance == unsigned instance, bit for bit".
Every output of every chunk is compared with the matching member slice of the whole run with torch.equal, on the device, and the
chunks cover all members.  One more chunk -- the last 70 members, whose cells sit at the highest addresses -- is copied to the host and
gated against the oracle at the tolerances of the small-shape module tests; no other tolerance appears here.  That the reference
arithmetic itself is bit-equal between whole and chunks for these inputs is pinned on the CPU (tests/test_member_chunks_premise.py).

Inputs are generated on the device, every member and column different (tests/wide_index_cases.py), and regenerated per chunk; no large
tensor is copied or moved to the host.  The C ABI is called directly with torch tensors, so that only the fields a module reads exist.
Every test states its peak device memory as arithmetic and skips only when the device has less than that plus 10 % free."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import moist_surface_ref as mref
import statistics_ref as sref
import test_member_chunks_premise as pre
import test_micro_kessler as tk
import test_modules as tm
import test_moist_surface_modules as tms
import wide_index_cases as wi
from oracle import awfl_oracle as ao
from pam_amd import capi
from pam_amd.capi import check

NAN = float("nan")
F64 = 8
SIDES = ["wide", "below"]
GEN_TEMP = 3 * F64 * (1 << 25)      # temporaries of Members.fill: gathered block, factor, product (2^25 elements each)


_stated_peak = []


@pytest.fixture(autouse=True)
def _free_device_memory():
    """frees the device memory of a case, and holds its stated peak to what the allocator measured"""
    _stated_peak.clear()
    yield
    gc.collect()
    if torch.cuda.is_available():
        measured = torch.cuda.max_memory_allocated()
        torch.cuda.empty_cache()
        if _stated_peak:
            print("peak device memory: stated %.1f GB, measured %.1f GB" % (_stated_peak[0] / 1e9, measured / 1e9))
            assert measured <= 1.1 * _stated_peak[0], (measured, _stated_peak[0])


def _need(peak_bytes):
    """skips where the device has less free memory than the case's stated peak + 10 %; nowhere else"""
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < 1.1 * peak_bytes:
        pytest.skip("needs %.1f GB of device memory (peak %.1f GB + 10 %%), %.1f GB of %.1f GB are free"
                    % (1.1 * peak_bytes / 1e9, peak_bytes / 1e9, free / 1e9, total / 1e9))
    torch.cuda.reset_peak_memory_stats()
    _stated_peak.append(peak_bytes)


def _new(shape, fill=NAN):
    return torch.full(tuple(shape), fill, dtype=torch.float64, device="cuda:0")


def _tab(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _stream():
    return torch.cuda.current_stream("cuda:0").cuda_stream


def _whole_vs_chunks(nens, make, run, outs, oracle=None):
    """run(state, members, whole's result or None) on make(0, nens) and on make(lo, hi) of every chunk; every output of every chunk
    equals the whole's member slice; then the oracle-gated chunk.  Returns (whole state, whole result, chunk results)."""
    with torch.cuda.device(0):
        whole = make(0, nens)
        rw = run(whole, nens, None)
        results = []
        for lo, hi in wi.member_chunks(nens):
            part = make(lo, hi)
            results.append(run(part, hi - lo, rw))
            for k in outs:
                wi.assert_same(k, whole[k], part[k], lo, hi)
            del part
        if oracle is not None:
            lo, hi = nens - wi.ORACLE_MEMBERS, nens
            part = make(lo, hi)
            host_in = {k: v.cpu().numpy() for k, v in part.items()}
            rp = run(part, hi - lo, rw)
            for k in outs:
                wi.assert_same(k, whole[k], part[k], lo, hi)
            oracle(host_in, {k: part[k].cpu().numpy() for k in outs}, rw, rp)
    return whole, rw, results


def _assert_side(side, elements, threshold, per_member):
    """the shape is on the side of the threshold (as the source states it) that the case is about"""
    if side == "wide":
        assert elements >= threshold, (elements, threshold)
    else:
        assert threshold - 64 * per_member <= elements < threshold, (elements, threshold)


# ------------------------------------------------------------------------------------------------------------------------------
# Kessler: kessler_column_kernel<SINGLE, IDX>, long long at nz * ncol >= 2^29
KES_NX, KES_NY, KES_NZ = 8, 4, 32          # 1024 cells per member
KES_OUT = ("rho_v", "rho_c", "rho_r", "temp", "precl")


@pytest.mark.gpu
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("heavy,dt", [(False, 5.0), (True, 60.0)], ids=["single", "subcycled"])
def test_kessler_whole_ensemble_equals_member_chunks(heavy, dt, side):
    """wide: 524325 members x 1024 cells = 2^29 + 37888 cells -> kessler_column_kernel<true, long long> (single: one sub-cycle) and
    <false, long long> (subcycled: heavy rain, several sub-cycles, the exner workspace at full size).  below: 524287 members = 2^29 -
    1024 cells -> the <., unsigned> instances one member short of their limit.  Chunks run with the whole's sub-cycle count as hint.
    Peak memory: rho_v, rho_c, rho_r, rho_dry, temp and the workspace, whole + one chunk of 1/13, + precl and zmid of both
        = 8 B x 1024 x 524325 x (6 + 2/32) x (1 + 1/13) + generator temporaries = 28.0 + 0.8 = 28.8 GB"""
    thr = wi.source_thresholds()["kessler"]
    per = KES_NX * KES_NY * KES_NZ
    nens = wi.members_at(thr, per, side)
    _assert_side(side, KES_NZ * (KES_NY * KES_NX * nens), thr, per)
    _need(F64 * per * nens * (6 + 2 / 32) * (1 + 1 / 13) + GEN_TEMP)
    lib = capi.load()
    g = wi.Members(pre.kessler_base(heavy, KES_NX, KES_NY, KES_NZ), "cuda:0")
    c = tk.C0

    def run(st, n, rw):
        st["precl"] = _new((KES_NY, KES_NX, n))
        work = _new((per * n + 1,))
        dt_max, count = C.c_double(), C.c_int()
        check(lib.pam_amd_kessler_max_stable_dt(n, KES_NX, KES_NY, KES_NZ, st["rho_r"].data_ptr(), st["rho_dry"].data_ptr(),
                                                st["zmid"].data_ptr(), dt, work.data_ptr(), _stream(), C.byref(dt_max)))
        check(lib.pam_amd_kessler_time_step(n, KES_NX, KES_NY, KES_NZ, st["rho_v"].data_ptr(), st["rho_c"].data_ptr(),
                                            st["rho_r"].data_ptr(), st["rho_dry"].data_ptr(), st["temp"].data_ptr(),
                                            st["precl"].data_ptr(), st["zmid"].data_ptr(), dt, c["R_d"], c["R_v"], c["cp_d"], c["p0"],
                                            work.data_ptr(), _stream(), 0 if rw is None else rw[0], C.byref(count)))
        torch.cuda.synchronize()
        return count.value, dt_max.value

    def oracle(h, got, rw, rp):
        h["precl"], n = ao.kessler(h["rho_v"], h["rho_c"], h["rho_r"], h["rho_dry"], h["temp"], h["zmid"], dt, c, rainsplit=rw[0])
        assert n == rw[0]
        for k in KES_OUT:      # test_micro_kessler.py: 1e-12 of the field's maximum
            assert np.abs(got[k] - h[k]).max() <= 1e-12 * np.abs(h[k]).max(), k

    whole, (n, dt_max), parts = _whole_vs_chunks(nens, lambda lo, hi: g.make_all(pre.KESSLER_IN, lo, hi), run, KES_OUT, oracle)
    assert (n >= 2) if heavy else (n == 1), n                       # the SINGLE instances resp. the sub-cycled ones
    assert n == max(1, int(np.ceil(dt / dt_max)))
    assert all(p[0] == n for p in parts)
    assert dt_max == min(p[1] for p in parts)                       # the global minimum is the minimum over the chunks, exactly
    assert float(whole["precl"].max()) > 0 and bool(torch.isfinite(whole["temp"]).all())


# ------------------------------------------------------------------------------------------------------------------------------
# GCM forcing: gcm_forcing_compute_kernel<IDX>, gcm_forcing_apply_kernel<IDX> (long long at >= 2^29 cells), gcm_fill_*
GCM_NX, GCM_NY, GCM_NZ = 8, 4, 16          # 512 cells per member
GCM_OUT = tuple(ao.GCM_FORCING_CRM) + tuple(ao.GCM_FORCING_TEND)


@pytest.mark.gpu
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kw,want", tm.GCM_CASES, ids=["no_fill", "level_fill", "whole_crm_fallback"])
def test_gcm_forcing_whole_ensemble_equals_member_chunks(kw, want, side):
    """wide: 1048613 members x 512 cells = 2^29 + 18944 cells -> gcm_forcing_compute_kernel<long long>, then four
    gcm_forcing_apply_kernel<long long> with gcm_fill_level_kernel (level_fill, whole_crm_fallback) and gcm_fill_glob_sum_kernel +
    gcm_fill_glob_kernel (whole_crm_fallback) over the same cells.  below: 1048575 members = 2^29 - 512 cells -> the <unsigned>
    instances.  All ten CRM fields and all fourteen tendencies are compared, and the mask of every application.
    Peak memory: ten CRM fields; ten GCM columns, fourteen tendencies, dz and 6 + 2/16 workspace columns of 1/32 of a field each;
    whole + one chunk of 1/13
        = 8 B x 512 x 1048613 x (10 + 31.2/32) x (1 + 1/13) + generator temporaries = 50.8 + 0.8 = 51.6 GB"""
    thr = wi.source_thresholds()
    assert thr["gcm_compute"] == thr["gcm_apply"]
    per = GCM_NX * GCM_NY * GCM_NZ
    nens = wi.members_at(thr["gcm_apply"], per, side)
    _assert_side(side, GCM_NZ * GCM_NY * GCM_NX * nens, thr["gcm_apply"], per)
    _need(F64 * per * nens * (10 + 31.2 / 32) * (1 + 1 / 13) + GEN_TEMP)
    lib = capi.load()
    g = wi.Members(pre.gcm_base(kw, GCM_NX, GCM_NY, GCM_NZ), "cuda:0")
    dt_gcm, crm_dt = 1200.0, 300.0

    def run(st, n, rw):
        for t in ao.GCM_FORCING_TEND:
            st[t] = _new((GCM_NZ, n))
        work = _new((6 * GCM_NZ * n + 2 * n + 4,))
        crm, gcm = _tab([st[k] for k in ao.GCM_FORCING_CRM]), _tab([st[k] for k in ao.GCM_FORCING_GCM])
        tend = _tab([st[k] for k in ao.GCM_FORCING_TEND])
        check(lib.pam_amd_gcm_forcing_compute(n, GCM_NX, GCM_NY, GCM_NZ, crm, gcm, tend, dt_gcm, _stream()))
        masks = []
        for _ in range(4):
            m = C.c_int(-1)
            check(lib.pam_amd_gcm_forcing_apply(n, GCM_NX, GCM_NY, GCM_NZ, crm, gcm, tend, st["dz"].data_ptr(), crm_dt, dt_gcm,
                                                work.data_ptr(), _stream(), C.byref(m)))
            masks.append(m.value)
        torch.cuda.synchronize()
        return masks

    def oracle(h, got, rw, rp):
        crm = {k: h[k] for k in ao.GCM_FORCING_CRM}
        gcm = {k: h[k] for k in ao.GCM_FORCING_GCM}
        tend = ao.compute_gcm_forcing_tendencies(crm, gcm, dt_gcm)
        assert [ao.apply_gcm_forcing_tendencies(crm, gcm, tend, h["dz"], crm_dt, dt_gcm) for _ in range(4)] == rp
        scale = max(np.abs(v).max() for v in gcm.values()) / dt_gcm        # the tolerances of test_modules.py
        for k in ao.GCM_FORCING_TEND:
            if k[-5:] in ("rho_v", "rho_l", "rho_i"):
                assert np.abs(got[k] - tend[k]).max() <= 1e-13 * 0.015 / dt_gcm, k
            else:
                assert np.abs(got[k] - tend[k]).max() <= 1e-14 * scale, k
        for k in ao.GCM_FORCING_CRM:
            assert np.abs(got[k] - crm[k]).max() <= 1e-12 * max(np.abs(crm[k]).max(), 1e-300), k

    whole, masks, parts = _whole_vs_chunks(nens, lambda lo, hi: g.make_all(pre.GCM_IN, lo, hi), run, GCM_OUT, oracle)
    union = 0
    for m in masks:
        union |= m
    assert union == want, (masks, want)                  # the path of test_modules.py's GCM_CASES ...
    assert all(p == masks for p in parts), (masks, parts)   # ... which every chunk takes too, application by application


# ------------------------------------------------------------------------------------------------------------------------------
# statistics: horizontal_average_kernel<IDX>, time_average_kernel<ZERO, IDX>: long long when the largest field of a launch table has
# >= 2^31 elements
BIG = (16, 4, 8)                           # (nz, ny, nx) of the large field: 512 elements per member


def _stats_table(kind, stats_table):
    """(name, shape without the members) of the fields of one call.  mixed: small, large, small -- one launch, which the large field
    puts on the wide instance.  long: more fields than one launch table holds, the large one in the second launch."""
    if kind == "mixed":
        return [("s0", (1, 2, 4)), ("big", BIG), ("s1", (3, 5))]
    small = [("s%d" % f, (1 + f % 2, 1 + f % 3)) for f in range(stats_table + 1)]
    return small + [("big", BIG)]


def _stats_setup(kind, side):
    thr = wi.source_thresholds()["stats"]
    text = open(wi.SRC).read()
    assert "constexpr int STATS_TABLE = 32;" in text
    table = _stats_table(kind, 32)
    per = int(np.prod(BIG))
    nens = wi.members_at(thr, per, side)
    sizes = [int(np.prod(s)) * nens for _, s in table]
    _assert_side(side, max(sizes), thr, per)
    big_at = [n for n, _ in table].index("big")
    if kind == "long":       # the first launch (fields 0 .. 31) is narrow, the second holds the large field
        assert big_at >= 32 and max(sizes[:32]) < thr and len(table) > 32
    return table, per, nens


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mixed", "long"])
def test_horizontal_average_whole_ensemble_equals_member_chunks(kind):
    """4194341 members: the large field (16, 4, 8, nens) has 2^31 + 18944 elements -> horizontal_average_kernel<long long> for the
    launch that holds it (mixed: the only one; long: the second, fields 32 and 33, after a narrow launch of 32 small fields).
    Peak memory: the large field and the small ones (mixed 23, long 98 elements per member) and the (nz, nens) averages (mixed 20,
    long 65 per member), whole + one chunk of 1/13
        = 8 B x 4194341 x (512 + 98 + 65) x (1 + 1/13) + generator temporaries = 24.4 + 0.8 = 25.2 GB"""
    table, per, nens = _stats_setup(kind, "wide")
    _need(F64 * nens * (per + 98 + 65) * (1 + 1 / 13) + GEN_TEMP)
    lib = capi.load()
    g = wi.Members(pre.stats_base(dict(table)), "cuda:0")
    names = [n for n, _ in table]
    outs = tuple(n + "_havg" for n in names)
    nzs = (C.c_int * len(table))(*[s[0] for _, s in table])
    ncols = (C.c_int * len(table))(*[int(np.prod(s[1:])) for _, s in table])

    def run(st, n, rw):
        for (name, s) in table:
            st[name + "_havg"] = _new((s[0], n))
        check(lib.pam_amd_horizontal_average(n, len(table), nzs, ncols, _tab([st[k] for k in names]), _tab([st[k] for k in outs]),
                                             _stream()))
        torch.cuda.synchronize()

    def oracle(h, got, rw, rp):
        for name in names:   # test_statistics_modules.py: bit for bit
            assert np.array_equal(got[name + "_havg"], sref.horizontal_average(h[name], True)), name

    _whole_vs_chunks(nens, lambda lo, hi: g.make_all(names, lo, hi), run, outs, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,side", [("mixed", "wide"), ("long", "wide"), ("mixed", "below")])
def test_time_average_whole_ensemble_equals_member_chunks(kind, side):
    """wide: 4194341 members, the large field has 2^31 + 18944 elements -> time_average_kernel<true, long long> (zero) and
    <false, long long> (accumulate) for the launch that holds it, as in the horizontal_average test.  below: 4194303 members = 2^31 -
    512 elements -> the <., unsigned> instances.  Zero over an accumulator full of NaN, then two accumulates: the second reads a
    non-zero accumulator and a changed variable.
    Peak memory: variable and accumulator of the large field and of the small ones (mixed 23, long 98 elements per member), whole +
    one chunk of 1/13
        = 8 B x 4194341 x 2 x (512 + 98) x (1 + 1/13) + generator temporaries = 44.1 + 0.8 = 44.9 GB"""
    table, per, nens = _stats_setup(kind, side)
    _need(F64 * nens * 2 * (per + 98) * (1 + 1 / 13) + GEN_TEMP)
    lib = capi.load()
    g = wi.Members(pre.stats_base(dict(table)), "cuda:0")
    names = [n for n, _ in table]
    outs = tuple(n + "_tavg" for n in names)
    factors = (float(sref.time_average_factor(20.0, 900.0)), float(sref.time_average_factor(30.0, 900.0)))

    def run(st, n, rw):
        sizes = (C.c_longlong * len(table))(*[int(np.prod(s)) * n for _, s in table])
        for (name, s) in table:
            st[name + "_tavg"] = _new(tuple(s) + (n,))
        var, tavg = _tab([st[k] for k in names]), _tab([st[k] for k in outs])
        check(lib.pam_amd_time_average_zero(len(table), sizes, tavg, _stream()))
        check(lib.pam_amd_time_average_accumulate(len(table), sizes, var, tavg, factors[0], _stream()))
        for k in names:
            st[k].mul_(0.75)
        check(lib.pam_amd_time_average_accumulate(len(table), sizes, var, tavg, factors[1], _stream()))
        torch.cuda.synchronize()

    def oracle(h, got, rw, rp):
        for name in names:   # test_statistics_modules.py: bit for bit
            t = sref.time_average_accumulate(np.zeros_like(h[name]), h[name], factors[0])
            t = sref.time_average_accumulate(t, h[name] * 0.75, factors[1])
            assert np.array_equal(got[name + "_tavg"], t) and np.abs(t).max() > 0, name

    _whole_vs_chunks(nens, lambda lo, hi: g.make_all(names, lo, hi), run, outs, oracle)


# ------------------------------------------------------------------------------------------------------------------------------
# the untemplated kernels (long long casts throughout) on fields of >= 2^29 elements -- byte offsets past 2^32 -- and, for sponge,
# saturation adjustment and broadcast, on fields of >= 2^31 elements: element indices leave 32 bits too
U_NX, U_NY, U_NZ = 8, 4, 32                # 1024 cells per member
SAT_NZ = 4                                 # saturation adjustment where the oracle (a Python loop per cell) gates a chunk: 128 cells
F_NZ = 3                                   # surface friction: the three levels it reads


def _untemplated_members(power, per):
    thr = wi.source_thresholds()
    assert thr["kessler"] == 1 << 29 and thr["stats"] == 1 << 31
    nens = wi.members_at(1 << power, per, "wide")
    assert per * nens >= 1 << power and F64 * per * nens > 1 << (power + 3)
    return nens


def _sponge_case(nens, oracle):
    lib = capi.load()
    g = wi.Members(pre.sponge_base(U_NX, U_NY, U_NZ), "cuda:0")

    def run(st, n, rw):
        check(lib.pam_amd_sponge_layer(n, U_NX, U_NY, U_NZ, 5, _tab([st[k] for k in pre.SPONGE_F]), st["zint"].data_ptr(),
                                       st["zmid"].data_ptr(), 2.0, 5, 60.0, None, _stream()))
        torch.cuda.synchronize()

    def gate(h, got, rw, rp):
        want = pre.sponge_oracle(h, num_layers=5, time_scale=60.0, crm_dt=2.0)
        for k in pre.SPONGE_F:   # test_modules.py: 1e-14 of the field's maximum
            assert np.abs(got[k] - want[k]).max() <= 1e-14 * max(np.abs(want[k]).max(), 1e-300), k
        assert np.abs(want["temp"] - h["temp"]).max() > 0

    _whole_vs_chunks(nens, lambda lo, hi: g.make_all(pre.SPONGE_IN, lo, hi), run, pre.SPONGE_F, gate if oracle else None)


def _saturation_case(nens, nz, oracle):
    lib = capi.load()
    g = wi.Members(pre.sat_base(U_NX, U_NY, nz), "cuda:0")

    def run(st, n, rw):
        check(lib.pam_amd_saturation_adjustment(n, U_NX, U_NY, nz, st["density_dry"].data_ptr(), st["water_vapor"].data_ptr(),
                                                st["cloud_liquid"].data_ptr(), st["temp"].data_ptr(), 2,
                                                _tab([st["water_vapor"], st["cloud_liquid"]]), tms.R_V, tms.CP_D, tms.CP_V, mref.CP_L,
                                                _stream()))
        torch.cuda.synchronize()

    def gate(h, got, rw, rp):
        want, info = mref.saturation_adjustment(h, pre.SAT_TRACERS, "kessler", tms.R_V, tms.CP_D, tms.CP_V)
        assert np.array_equal(got["density_dry"], h["density_dry"]) and set(np.unique(info["branch"])) == {0, 1, 2}
        # test_moist_surface_modules.py: 1e-12 of the field maximum, except where a decision of the bisection was within 1e-12 of its
        # root (at most 2 tol in rho there, the matching change in T)
        exempt = info["margin"].reshape(h["temp"].shape) < 1e-12
        dT = 2 * mref.TOL * 2.6e6 / (0.5 * tms.CP_D)
        for k, allow in (("water_vapor", 2 * mref.TOL), ("cloud_liquid", 2 * mref.TOL), ("temp", dT)):
            err = np.abs(got[k] - want[k])
            tol = 1e-12 * np.abs(want[k]).max()
            assert np.all(err[~exempt] <= tol), (k, err[~exempt].max(), tol)
            assert np.all(err[exempt] <= allow + tol), k

    _whole_vs_chunks(nens, lambda lo, hi: g.make_all(pre.SAT_IN, lo, hi), run, pre.SAT_IN, gate if oracle else None)


def _broadcast_case(nens, num_fields):
    lib = capi.load()
    rng = np.random.default_rng(3)
    base = {n: rng.uniform(0.5, 1.5, (U_NZ, wi.NB)) for n in ao.BROADCAST_GCM[:num_fields]}
    g = wi.Members(base, "cuda:0")
    with torch.cuda.device(0):
        gcm = g.make_all(ao.BROADCAST_GCM[:num_fields], 0, nens)
        crm = {n: _new((U_NZ, U_NY, U_NX, nens)) for n in ao.BROADCAST_CRM[:num_fields]}
        check(lib.pam_amd_broadcast_initial_gcm_column(nens, U_NX, U_NY, U_NZ, num_fields, _tab(list(gcm.values())),
                                                       _tab(list(crm.values())), _stream()))
        torch.cuda.synchronize()
        for cn, gn in zip(ao.BROADCAST_CRM, ao.BROADCAST_GCM[:num_fields]):
            for lo, hi in wi.member_chunks(nens):       # exact equality with the expanded GCM column, all members
                wi.assert_same(cn, crm[cn], gcm[gn][:, None, None, lo:hi].expand(U_NZ, U_NY, U_NX, hi - lo), lo, hi)


@pytest.mark.gpu
def test_sponge_layer_past_2_32_bytes():
    """524325 members x 1024 cells = 2^29 + 37888 cells per field.  Peak memory: five fields, zint and zmid, whole + one chunk of 1/13
        = 8 B x 1024 x 524325 x (5 + 2/32) x (1 + 1/13) + generator temporaries = 23.4 + 0.8 = 24.2 GB"""
    nens = _untemplated_members(29, U_NX * U_NY * U_NZ)
    _need(F64 * 1024 * nens * (5 + 2 / 32) * (1 + 1 / 13) + GEN_TEMP)
    _sponge_case(nens, oracle=True)


@pytest.mark.gpu
def test_saturation_adjustment_past_2_32_bytes():
    """4194341 members x 128 cells = 2^29 + 4736 cells per field.  Peak memory: four fields, whole + one chunk of 1/13
        = 8 B x 128 x 4194341 x 4 x (1 + 1/13) + generator temporaries = 18.5 + 0.8 = 19.3 GB"""
    nens = _untemplated_members(29, U_NX * U_NY * SAT_NZ)
    _need(F64 * 128 * nens * 4 * (1 + 1 / 13) + GEN_TEMP)
    _saturation_case(nens, SAT_NZ, oracle=True)


@pytest.mark.gpu
def test_perturb_temperature_past_2_32_bytes():
    """the kernel walks the lowest nz/4 levels only, so the field is 5/4 of 2^31 elements: 2621487 members x 1024 cells, whose lowest 8
    of 32 levels end at 2^29 + 134 M elements -- a quarter of what it touches lies past 2^32 bytes.  ids[lo:hi] go with a chunk.
    Peak memory: temp, whole + one chunk of 1/13
        = 8 B x 1024 x 2621487 x (1 + 1/13) + generator temporaries = 23.1 + 0.8 = 23.9 GB"""
    per = U_NX * U_NY * U_NZ
    nens = _untemplated_members(31, per) * 5 // 4 | 1
    assert nens % 64 != 0 and F64 * (U_NZ // 4) * U_NY * U_NX * nens >= (1 << 32) * 5 // 4
    _need(F64 * per * nens * (1 + 1 / 13) + GEN_TEMP)
    lib = capi.load()
    g = wi.Members({"temp": pre.sponge_base(U_NX, U_NY, U_NZ)["temp"]}, "cuda:0")

    def make(lo, hi):
        return {"temp": g.make("temp", lo, hi), "ids": (torch.arange(lo, hi, device="cuda:0") * 3 + 11).to(torch.int32)}

    def run(st, n, rw):
        check(lib.pam_amd_perturb_temperature(n, U_NX, U_NY, U_NZ, st["temp"].data_ptr(), st["ids"].data_ptr(), 0.25, _stream()))
        torch.cuda.synchronize()

    def gate(h, got, rw, rp):
        assert np.array_equal(h["ids"], pre.perturb_ids(nens - wi.ORACLE_MEMBERS, nens))
        want = np.array(h["temp"])
        ao.perturb_temperature(want, h["ids"], 0.25)
        assert np.abs(got["temp"] - want).max() <= 1e-14 * want.max()       # test_modules.py
        assert np.abs(want - h["temp"]).max() > 0.1

    _whole_vs_chunks(nens, make, run, ("temp",), gate)


@pytest.mark.gpu
def test_surface_friction_past_2_32_bytes():
    """surface_friction_init and compute_surface_friction read levels 0 .. 2 only, so the fields have three levels and 5/4 of 2^29
    cells: 6990553 members x (8 x 4 x 3 = 96) cells -- a fifth of level 2 lies past 2^32 bytes.  Peak memory, doubles per member:
    density_dry, water_vapor, uvel, vvel 4 x 96; the fluxes and their copies after the init 4 x 32; zint, zmid, gcm_uvel, gcm_vvel 13;
    tau, bflx, z0, sfc_bflx 4; whole + one chunk of 1/13
        = 8 B x 529 x 6990553 x (1 + 1/13) + generator temporaries = 31.9 + 0.8 = 32.7 GB"""
    per = U_NX * U_NY * F_NZ
    nens = _untemplated_members(29, per) * 5 // 4 | 1
    assert nens % 64 != 0 and F64 * per * nens >= (1 << 32) * 5 // 4
    _need(F64 * 529 * nens * (1 + 1 / 13) + GEN_TEMP)
    lib = capi.load()
    g = wi.Members(pre.friction_base(U_NX, U_NY, F_NZ), "cuda:0")
    outs = ("z0", "sfc_bflx", "flx_u_after_init", "flx_v_after_init", "sfc_mom_flx_u", "sfc_mom_flx_v")

    def run(st, n, rw):
        for k in ("z0", "sfc_bflx"):
            st[k] = _new((n,))
        for k in ("sfc_mom_flx_u", "sfc_mom_flx_v"):
            st[k] = _new((U_NY, U_NX, n))
        p = {k: v.data_ptr() for k, v in st.items()}
        check(lib.pam_amd_surface_friction_init(n, U_NX, U_NY, F_NZ, p["density_dry"], p["water_vapor"], p["zmid"], p["gcm_uvel"],
                                                p["gcm_vvel"], p["tau"], p["bflx"], p["z0"], p["sfc_bflx"], p["sfc_mom_flx_u"],
                                                p["sfc_mom_flx_v"], _stream()))
        st["flx_u_after_init"], st["flx_v_after_init"] = st["sfc_mom_flx_u"].clone(), st["sfc_mom_flx_v"].clone()
        check(lib.pam_amd_surface_friction_compute(n, U_NX, U_NY, F_NZ, p["density_dry"], p["water_vapor"], p["uvel"], p["vvel"],
                                                   p["zmid"], p["zint"], p["z0"], p["sfc_bflx"], p["sfc_mom_flx_u"], p["sfc_mom_flx_v"],
                                                   _stream()))
        torch.cuda.synchronize()

    def gate(h, got, rw, rp):      # test_moist_surface_modules.py: 1e-12 of the maximum; sfc_bflx and the zeroed fluxes exactly
        z0, sb, _, _ = mref.surface_friction_init(h["density_dry"], h["water_vapor"], h["zmid"], h["gcm_uvel"], h["gcm_vvel"], h["tau"],
                                                  h["bflx"])
        assert np.all(np.abs(got["z0"] - z0) <= 1e-12 * np.abs(z0).max())
        assert np.array_equal(got["sfc_bflx"], sb)
        assert not got["flx_u_after_init"].any() and not got["flx_v_after_init"].any()
        fu, fv = mref.compute_surface_friction(h["density_dry"], h["water_vapor"], h["uvel"], h["vvel"], h["zmid"], h["zint"], got["z0"],
                                               got["sfc_bflx"])
        for k, want in (("sfc_mom_flx_u", fu), ("sfc_mom_flx_v", fv)):
            assert np.abs(got[k] - want).max() <= 1e-12 * np.abs(want).max() and np.abs(want).max() > 0, k

    _whole_vs_chunks(nens, lambda lo, hi: g.make_all(pre.FRICTION_IN, lo, hi), run, outs, gate)


@pytest.mark.gpu
def test_broadcast_initial_gcm_column_past_2_32_bytes():
    """all six fields of 524325 members x 1024 cells against the expanded GCM columns.  Peak memory: six fields and their columns +
    the comparison's mask of one chunk
        = 8 B x 1024 x 524325 x (6 + 6/32) + 1024 x 524325 / 13 B + generator temporaries = 26.6 + 0.8 = 27.4 GB"""
    nens = _untemplated_members(29, U_NX * U_NY * U_NZ)
    _need(F64 * 1024 * nens * (6 + 6 / 32) + 1024 * nens / 13 + GEN_TEMP)
    _broadcast_case(nens, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("module", ["broadcast_dry_density", "saturation_adjustment", "sponge_layer"])
def test_single_fields_past_2_31_elements(module):
    """2097189 members x 1024 cells = 2^31 + 37888 elements per field: element indices as well as byte offsets leave 32 bits.  Whole
    against chunks bit for bit (broadcast: against the expanded column); the oracle gates these modules at the 2^29 shape.
    Peak memory, 8 B x 1024 x 2097189 = 17.2 GB per field:
        broadcast_dry_density   1 field + its column (1/32) + the comparison's mask + the temporaries  = 17.9 + 0.8 = 18.7 GB
        saturation_adjustment   4 fields x (1 + 1/13) + generator temporaries                         = 74.0 + 0.8 = 74.8 GB
        sponge_layer            (5 fields + zint, zmid of 1/32 each) x (1 + 1/13) + the temporaries   = 93.7 + 0.8 = 94.5 GB"""
    per = U_NX * U_NY * U_NZ
    nens = _untemplated_members(31, per)
    fields = {"broadcast_dry_density": 1 + 1 / 32 + 1 / 13 / 8, "saturation_adjustment": 4 * (1 + 1 / 13),
              "sponge_layer": (5 + 2 / 32) * (1 + 1 / 13)}[module]
    _need(F64 * per * nens * fields + GEN_TEMP)
    if module == "broadcast_dry_density":
        _broadcast_case(nens, 1)
    elif module == "saturation_adjustment":
        _saturation_case(nens, U_NZ, oracle=False)
    else:
        _sponge_case(nens, oracle=False)
