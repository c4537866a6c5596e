"""pam::VerticalInterp's kernels at the size that selects their `long long` instances, and one member below it at the edge of the
`unsigned` ones (pam_amd/csrc/modules_kernels.hip: the edges array -- the larger one -- has >= 2^31 elements).  In its own file, to be
run in its own pytest process like tests/test_modules_wide_index.py: the arrays are large.

Shape: 15 levels of 1024 x 1024 columns, so a member has 16 x 2^20 = 2^24 edge values: 128 members reach 2^31 exactly (`long long`),
127 members stay 2^24 below it (`unsigned`, the last element at index 2^31 - 2^24 - 1).  Orders 3 and 5, per-member tables (every
member its own stretched column) and the shared table.  The whole ensemble equals its member chunks bit for bit (torch.equal on the
device; a chunk is 32 members, a quarter of the threshold, far from the edge of the 32-bit instance); the last member's first and last
65536 columns -- the lowest and the highest addresses of its slice -- equal the CPU restatement bit for bit (the restatement of a whole
chunk, 5e8 cells of Python-driven numpy, would take a quarter of an hour).

Peak device memory: data 15/16 and edges 16/16 of 8 B x 2^31 = 17.2 GB, whole + one chunk of 1/4, + the comparison's temporaries (a
contiguous copy of the whole's slice and the mask: (8 + 1) B x 2^29)
    = 17.2 GB x (31/16) x (1 + 1/4) + 4.8 GB = 46.4 GB; the tables (15 x 52 x 128 doubles) do not count."""
import gc

import numpy as np
import pytest
import torch

import test_vertical_interp as tv
import vertical_interp_ref as ref

NZ, NY, NX = 15, 1024, 1024
CHUNK = 32
PEAK = 8 * (1 << 31) * (31 / 16) * (1 + 1 / 4) + 9 * (1 << 29)


def _need(peak_bytes):
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < 1.1 * peak_bytes:
        pytest.skip("needs %.1f GB of device memory (peak %.1f GB + 10 %%), %.1f GB of %.1f GB are free"
                    % (1.1 * peak_bytes / 1e9, peak_bytes / 1e9, free / 1e9, total / 1e9))
    torch.cuda.reset_peak_memory_stats()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["stretched", "l60"], ids=["per_member", "shared"])
@pytest.mark.parametrize("nens,ord", [(128, 5), (127, 5), (128, 3)], ids=["wide_ord5", "below_ord5", "wide_ord3"])
def test_whole_ensemble_equals_member_chunks(nens, ord, kind):
    import pam_amd
    elements = (NZ + 1) * NY * NX * nens
    assert (elements >= 1 << 31) == (nens == 128) and elements >= (1 << 31) - (1 << 24)
    assert "const bool narrow = (long long)(h->nz + 1) * ncol * h->nens < IDX32_LIMIT;" in open(tv.ROOT + "/pam_amd/csrc/modules_kernels.hip").read()
    _need(PEAK)
    dev = "cuda:0"
    zint = tv.grid(kind, NZ, nens)
    g = torch.Generator(device=dev)
    g.manual_seed(100 * ord + nens)
    data = torch.empty((NZ, NY, NX, nens), dtype=torch.float64, device=dev)
    data.normal_(generator=g)
    data.mul_(torch.logspace(-3, 3, NX, dtype=torch.float64, device=dev)[None, None, :, None])    # mixed sign and magnitude

    def run(lo, hi, d):
        v = pam_amd.VerticalInterp(ord)
        v.init(torch.from_numpy(np.ascontiguousarray(zint[:, lo:hi])).to(dev))
        assert v.shared_table == (kind == "l60")
        out = torch.full((NZ + 1, NY, NX, hi - lo), float("nan"), dtype=torch.float64, device=dev)
        v.cells_to_edges(d, 1, 0, out=out)
        torch.cuda.synchronize()
        v.finalize()
        return out

    whole = run(0, nens, data)
    assert bool(torch.isfinite(whole[-1, -1, -1]).all())
    for lo in range(0, nens, CHUNK):
        hi = min(lo + CHUNK, nens)
        part = run(lo, hi, data[..., lo:hi].contiguous())
        assert torch.equal(whole[..., lo:hi], part), (lo, hi)
        del part
    # the last member against the restatement: its lowest and highest addresses
    for rows in (slice(0, 64), slice(NY - 64, NY)):
        d = data[:, rows, :, nens - 1:].cpu().numpy()
        want = ref.interp(d, zint[:, nens - 1:], ord, 1, 0)
        assert tv.same_bits(whole[:, rows, :, nens - 1:].cpu().numpy(), want), rows
    del whole, data
    gc.collect()
    measured = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    print("peak device memory: stated %.1f GB, measured %.1f GB" % (PEAK / 1e9, measured / 1e9))
    assert measured <= 1.1 * PEAK
