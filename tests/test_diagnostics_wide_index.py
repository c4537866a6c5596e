"""pam_amd_field_diagnostics on a field of more than 2^31 elements: the flat index is 64-bit throughout.  One float field of ones with
2^31 + 4160 elements, 8.6 GB; -2.5 at index 2^31 and 3.0 at index 2^31 + 7.  The indices and the extremes are exact, and so is the sum:
every partial of the tree is a multiple of 0.5 below 2^53, so the result is the count-based value whatever the order -- three levels
of the tree are walked.  Run in a pytest process of its own, like the other wide-index files."""
import gc

import numpy as np
import pytest
import torch

N = (1 << 31) + 4160
LOW, HIGH = 1 << 31, (1 << 31) + 7


@pytest.mark.gpu
def test_indices_extremes_and_sum_past_2_31_are_exact():
    """Peak memory: the field, 4 B x (2^31 + 4160) = 8.6 GB (filled in place), and 0.2 GB of scratch for the per-member call."""
    import pam_amd
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    need = 1.15 * 4 * N
    if free < need:
        pytest.skip("needs %.1f GB of device memory, %.1f GB of %.1f GB are free" % (need / 1e9, free / 1e9, total / 1e9))
    t = torch.ones(N, dtype=torch.float32, device="cuda:0")
    t[LOW] = -2.5
    t[HIGH] = 3.0
    out = pam_amd.field_diagnostics([t])
    got = {k: v[0].item() for k, v in out.items()}
    assert got == {"vmin": -2.5, "vmax": 3.0, "vsum": (N - 2) - 2.5 + 3.0, "argmin": LOW, "argmax": HIGH, "nan_count": 0}, got
    # the view that starts one element later: every index one lower, the base no longer 16-byte aligned
    out = pam_amd.field_diagnostics([t[1:]])
    got = {k: v[0].item() for k, v in out.items()}
    assert got == {"vmin": -2.5, "vmax": 3.0, "vsum": (N - 3) - 2.5 + 3.0, "argmin": LOW - 1, "argmax": HIGH - 1, "nan_count": 0}, got
    # per member, 64 members of 2^25 + 65 rows: member 0 holds the -2.5, member 7 the 3.0; every other member's extremes are its row 0
    M, rows = 64, N // 64
    per = pam_amd.field_diagnostics([t], members=M)
    vsum = np.full(M, float(rows))
    vsum[0], vsum[7] = rows - 1 - 2.5, rows - 1 + 3.0
    vmin, vmax, argmin, argmax = np.ones(M), np.ones(M), np.arange(M), np.arange(M)
    vmin[0], argmin[0] = -2.5, LOW
    vmax[7], argmax[7] = 3.0, HIGH
    argmax[0], argmin[7] = 0, 7
    assert np.array_equal(per["vsum"][0], vsum) and not per["nan_count"].any()
    assert np.array_equal(per["vmin"][0], vmin) and np.array_equal(per["vmax"][0], vmax)
    assert np.array_equal(per["argmin"][0], argmin) and np.array_equal(per["argmax"][0], argmax)
    assert float(t[LOW]) == -2.5 and float(t[HIGH]) == 3.0 and float(t[:1 << 20].sum()) == float(1 << 20)
    del t
    torch.cuda.empty_cache()
