"""pam_amd_validate_fields on a field of more than 2^31 elements: the flat index is 64-bit throughout (the reference's `int i` wraps
there, pam_core/DataManager.h:473).  One float field of 2^31 + 4160 elements, 8.6 GB; a negative value at index 2^31 and a NaN at the
last index, nothing else.  Integers only: the comparison is exact.  Run in a pytest process of its own, like the other wide-index
files."""
import gc

import numpy as np
import pytest
import torch

N = (1 << 31) + 4160


@pytest.mark.gpu
def test_first_indices_past_2_31_are_exact():
    """Peak memory: the field, 4 B x (2^31 + 4160) = 8.6 GB (filled in place)."""
    import pam_amd
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    need = 1.1 * 4 * N
    if free < need:
        pytest.skip("needs %.1f GB of device memory, %.1f GB of %.1f GB are free" % (need / 1e9, free / 1e9, total / 1e9))
    t = torch.ones(N, dtype=torch.float32, device="cuda:0")
    t[1 << 31] = -2.5
    t[N - 1] = float("nan")
    count, first = pam_amd.validate_fields([t], [True])
    assert np.array_equal(count, [[1, 0, 1]]), count
    assert np.array_equal(first, [[N - 1, -1, 1 << 31]]), first
    # the view that starts one element later: every index one lower, the base no longer 16-byte aligned
    count, first = pam_amd.validate_fields([t[1:]], [True])
    assert np.array_equal(count, [[1, 0, 1]]) and np.array_equal(first, [[N - 2, -1, (1 << 31) - 1]]), (count, first)
    assert float(t[1 << 31]) == -2.5 and bool(torch.isnan(t[N - 1])) and float(t[:1 << 20].sum()) == float(1 << 20)
    del t
    torch.cuda.empty_cache()
