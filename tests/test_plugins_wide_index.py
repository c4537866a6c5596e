"""radiation_forced_kernel<IDX> and coupler_pressure_kernel<IDX> at the size that selects their `long long` instances, and one member
below it at the edge of the `unsigned` ones (pam_amd/csrc/modules_kernels.hip; DESIGN.md section 8, "Index width").  In its own file,
to be run in its own pytest process like tests/test_modules_wide_index.py: the arrays are large.

Shape: a member has 8 x 4 x 32 = 1024 cells, so 524325 members make 2^29 + 37888 cells (`long long`) and 524287 members 2^29 - 1024
(`unsigned`); the rad grid is 2 x 8 (fy = 2, fx = 4), 128 rad cells per member.  Members come from tests/wide_index_cases.py: no two
members and no two columns hold the same numbers, so an offset that wraps lands on different data.  The whole ensemble equals its 13
member chunks bit for bit (torch.equal on the device), and the last 70 members -- the highest addresses -- equal the CPU restatement.

Peak device memory (fields of 8 B x 2^29 = 4.3 GB):
  radiation   temp + the tendency (1/8 of a field), whole + one chunk of 1/13, + the generator's and the comparison's temporaries
              (under two chunks): 4.3 GB x (9/8) x (14/13) + 0.7 GB = 5.9 GB
  pressure    rho_d, rho_v, temp and the pressure, whole + one chunk of 1/13, + the same temporaries:
              4.3 GB x 4 x (14/13) + 0.7 GB = 19.2 GB"""
import gc
import re

import numpy as np
import pytest
import torch

import plugins_ref as ref
import wide_index_cases as wi
from pam_amd import capi

NZ, NY, NX, RAD_NY, RAD_NX = 8, 4, 32, 2, 8
PER_MEMBER = NZ * NY * NX
CP_D, CRM_DT, R_D, R_V = 1003.0, 20.0, 287.0, 461.0
FIELD = 8 * (1 << 29)
PEAK = {"radiation": FIELD * (9 / 8) * (14 / 13) + 0.7e9, "pressure": FIELD * 4 * (14 / 13) + 0.7e9}


def threshold():
    """the size at which the host switches to the long long instances, read from the dispatch code itself"""
    text = open(wi.SRC).read()
    m = re.findall(r"constexpr long long PLUGINS_NARROW_CELLS = 1ll << (\d+);", text)
    assert len(m) == 1
    for kernel in ("radiation_forced_kernel", "coupler_pressure_kernel"):
        assert len(re.findall(r"if \(ncell < PLUGINS_NARROW_CELLS\)\s*hipLaunchKernelGGL\(\(%s<unsigned>\)" % kernel, text)) == 1, kernel
        assert len(re.findall(r"else\s*hipLaunchKernelGGL\(\(%s<long long>\)" % kernel, text)) == 1, kernel
    return 1 << int(m[0])


def test_threshold_is_read_from_the_dispatch_code():
    assert threshold() == 1 << 29 and max(PEAK.values()) < 30e9


def _need(peak_bytes):
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < 1.1 * peak_bytes:
        pytest.skip("needs %.1f GB of device memory (peak %.1f GB + 10 %%), %.1f GB of %.1f GB are free"
                    % (1.1 * peak_bytes / 1e9, peak_bytes / 1e9, free / 1e9, total / 1e9))
    torch.cuda.reset_peak_memory_stats()


def base_case():
    rng = np.random.default_rng(29)
    shape = (NZ, NY, NX, wi.NB)
    return {"temp": rng.uniform(190.0, 310.0, shape), "rho_d": rng.uniform(0.05, 1.3, shape), "rho_v": rng.uniform(0.0, 0.02, shape),
            "tend": rng.standard_normal((NZ, RAD_NY, RAD_NX, wi.NB)) * 10.0 ** rng.uniform(-3, 1, (NZ, RAD_NY, RAD_NX, wi.NB))}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_radiation(gen, lo, hi):
    """members [lo, hi): radiation applied twice; returns the new temp"""
    temp, tend = gen.make("temp", lo, hi), gen.make("tend", lo, hi)
    for _ in range(2):
        capi.check(capi.load().pam_amd_radiation_forced(hi - lo, NX, NY, NZ, RAD_NX, RAD_NY, temp.data_ptr(), tend.data_ptr(), CP_D, CRM_DT,
                                                        _stream()))
    torch.cuda.synchronize()
    return temp


def run_pressure(gen, lo, hi):
    f = gen.make_all(("rho_d", "rho_v", "temp"), lo, hi)
    p = torch.full((NZ, NY, NX, hi - lo), float("nan"), dtype=torch.float64, device=gen.device)
    capi.check(capi.load().pam_amd_compute_pressure(hi - lo, NX, NY, NZ, f["rho_d"].data_ptr(), f["rho_v"].data_ptr(), f["temp"].data_ptr(),
                                                    R_D, R_V, p.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return p


def restate(kind, gen, lo, hi):
    h = {k: gen.make(k, lo, hi).cpu().numpy() for k in (("temp", "tend") if kind == "radiation" else ("rho_d", "rho_v", "temp"))}
    if kind == "radiation":
        return ref.radiation_forced(ref.radiation_forced(h["temp"], h["tend"], CP_D, CRM_DT), h["tend"], CP_D, CRM_DT)
    return ref.compute_pressure(h["rho_d"], h["rho_v"], h["temp"], R_D, R_V)


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["wide", "below"])
@pytest.mark.parametrize("kind", ["radiation", "pressure"])
def test_whole_ensemble_equals_member_chunks(kind, side):
    thr = threshold()
    nens = wi.members_at(thr, PER_MEMBER, side)
    assert (PER_MEMBER * nens >= thr) == (side == "wide") and nens == (524325 if side == "wide" else 524287)
    _need(PEAK[kind])
    gen = wi.Members(base_case(), "cuda:0")
    run = run_radiation if kind == "radiation" else run_pressure
    whole = run(gen, 0, nens)
    assert bool(torch.isfinite(whole[-1, -1, -1]).all())
    chunks = wi.member_chunks(nens)
    assert len(chunks) == wi.NCHUNK
    for lo, hi in chunks:
        part = run(gen, lo, hi)
        wi.assert_same(kind, whole, part, lo, hi)
        del part
    lo = nens - wi.ORACLE_MEMBERS                                     # the highest addresses, through the restatement
    got = whole[..., lo:].cpu().numpy()
    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(restate(kind, gen, lo, nens)).view(np.uint64))
    got0 = whole[..., :wi.ORACLE_MEMBERS].cpu().numpy()
    assert np.array_equal(got0, restate(kind, gen, 0, wi.ORACLE_MEMBERS))
    del whole
    gc.collect()
    measured = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    print("%s %s: %d members, peak device memory stated %.1f GB, measured %.1f GB" % (kind, side, nens, PEAK[kind] / 1e9, measured / 1e9))
    assert measured <= 1.1 * PEAK[kind]
