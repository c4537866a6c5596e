"""Shared pieces of tests/test_modules_wide_index.py (GPU, real sizes) and tests/test_member_chunks_premise.py (CPU, small sizes):
the thresholds as the source states them, ensembles of distinct members generated from a small base case, member chunks, and the
bit comparison of a member chunk with the matching slice of a whole-ensemble run.

Members: member e of a field is base[..., e % nb] * (1 + e * 2^-28), where base holds nb members of one of the suite's small cases and
every column c = j * nx + i of a 4-D base field was scaled by (1 + c * 2^-20) first.  1 + e * 2^-28 is exact for e < 2^28 and the
product is one IEEE multiplication per element, so a member's values do not depend on which range [lo, hi) it was generated in:
make(0, nens)[..., lo:hi] == make(lo, hi) bit for bit, on any device.  No two members and no two columns hold the same numbers, so an
index that wraps lands on different data."""
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pam_amd", "csrc", "modules_kernels.hip")
MEMBER_STEP = 2.0 ** -28
COLUMN_STEP = 2.0 ** -20
NB = 7            # members of a base case
NCHUNK = 13       # member chunks of a whole-ensemble run (plus the oracle-gated chunk)
ORACLE_MEMBERS = 70


def source_thresholds():
    """the sizes at which the host switches to the long long instances, read from the dispatch code itself: a test that asserts its
    shape against these fails when a threshold moves"""
    text = open(SRC).read()
    pats = {
        "kessler": r"const bool narrow = \(long long\)nz \* ncol < \(1ll << (\d+)\);",
        "gcm_compute": r"const bool small = \(long long\)nz \* ny \* nx \* nens < \(1ll << (\d+)\);",
        "gcm_apply": r"if \(ncell < \(1ll << (\d+)\)\)\s*hipLaunchKernelGGL\(gcm_forcing_apply_kernel<unsigned>",
        "stats": r"constexpr long long IDX32_LIMIT = 1LL << (\d+);",
    }
    out = {}
    for k, p in pats.items():
        m = re.findall(p, text)
        assert len(m) == 1, "the dispatch of %s is no longer written as %s" % (k, p)
        out[k] = 1 << int(m[0])
    # horizontal_average and time_average_* both dispatch on the largest field of the table against that one limit
    assert len(re.findall(r"if \(most < IDX32_LIMIT\)", text)) == 2
    return out


def members_at(threshold, per_member, side):
    """a ragged member count whose field of per_member elements per member is at or past the threshold ("wide") or the largest
    convenient one still under it ("below": less than one member short, or two where that count is a multiple of 64)"""
    if side == "wide":
        n = -(-threshold // per_member) + 37
        if n % 64 == 0:
            n += 1
        assert per_member * n >= threshold
    else:
        n = (threshold - 1) // per_member
        if n % 64 == 0:
            n -= 1
        assert per_member * n < threshold and threshold - per_member * n <= 64 * per_member     # within one block of 64 members
    assert n % 64 != 0
    return n


def member_chunks(nens, n=NCHUNK):
    """[lo, hi) ranges of odd length that cover 0 .. nens"""
    size = -(-nens // n) | 1
    ranges = [(lo, min(nens, lo + size)) for lo in range(0, nens, size)]
    assert ranges[0][0] == 0 and ranges[-1][1] == nens and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    return ranges


class Members:
    """the generator of the module docstring over a dict of base arrays whose last dimension is the nb base members"""

    def __init__(self, base, device):
        self.device = torch.device(device)
        self.base = {}
        for k, v in base.items():
            v = np.asarray(v, dtype=np.float64)
            if v.ndim == 4:
                ny, nx = v.shape[1:3]
                v = v * (1.0 + np.arange(ny * nx, dtype=np.float64).reshape(1, ny, nx, 1) * COLUMN_STEP)
            self.base[k] = torch.from_numpy(np.ascontiguousarray(v)).to(self.device)
        nb = {int(v.shape[-1]) for v in self.base.values()}
        assert len(nb) == 1
        self.nb = nb.pop()

    def fill(self, name, out, lo, hi):
        """out[..., 0 : hi-lo] = members lo .. hi of `name`, in blocks of members (the temporaries stay at ~2^25 elements)"""
        b = self.base[name]
        per = max(1, b.numel() // self.nb)
        block = max(1, (1 << 25) // per)
        assert hi <= 1 << 28 and out.shape[-1] == hi - lo
        for b0 in range(lo, hi, block):
            b1 = min(hi, b0 + block)
            e = torch.arange(b0, b1, device=self.device)
            out[..., b0 - lo:b1 - lo] = b.index_select(-1, e % self.nb) * (1.0 + e.to(torch.float64) * MEMBER_STEP)
        return out

    def make(self, name, lo, hi):
        b = self.base[name]
        return self.fill(name, torch.empty(tuple(b.shape[:-1]) + (hi - lo,), dtype=torch.float64, device=self.device), lo, hi)

    def make_all(self, names, lo, hi):
        return {n: self.make(n, lo, hi) for n in names}


def first_difference(field, whole, part, lo, hi):
    """None where members [lo, hi) of `whole` equal `part` bit for bit (torch.equal); otherwise the report: the field, the first
    differing flat index of the whole field with its (k, j, i, e), and on which side of 2^29 and 2^31 it lies"""
    nens = whole.shape[-1]
    w = whole[..., lo:hi]
    assert tuple(w.shape) == tuple(part.shape), (field, tuple(w.shape), tuple(part.shape))
    if torch.equal(w, part):
        return None
    ne = (w != part).reshape(-1)
    count = int(ne.sum())
    flat = int(ne.to(torch.uint8).argmax())
    n = hi - lo
    row, e = flat // n, lo + flat % n
    g = row * nens + e
    idx = tuple(int(x) for x in np.unravel_index(row, tuple(whole.shape[:-1]) or (1,))) + (e,)
    names = ("k", "j", "i", "e") if whole.dim() == 4 else tuple("d%d" % d for d in range(whole.dim() - 1)) + ("e",)
    wv, pv = float(w.reshape(-1)[flat]), float(part.reshape(-1)[flat])
    where = ["past 2^%d" % p if g >= 1 << p else "below 2^%d" % p for p in (29, 31)]
    return ("%s: members [%d, %d) of the whole run differ from the chunk run in %d of %d elements, first at flat index %d = (%s) = %s, "
            "%s and %s (byte offset %d): whole %r, chunk %r" % (field, lo, hi, count, ne.numel(), g, ", ".join(names[-len(idx):]), idx,
                                                                 where[0], where[1], 8 * g, wv, pv))


def assert_same(field, whole, part, lo, hi):
    msg = first_difference(field, whole, part, lo, hi)
    assert msg is None, msg
