#!/usr/bin/env python3
"""Per-polynomial FP64 instruction ledger of the WENO reconstruction (gfx950 device assembly, no GPU needed).

usage: python tools/weno_ledger.py [awfl_kernels.s]
  1. weno5_const and weno5_table (the wave-uniform table, as the C2 z sweep reads it: struct VTable, whose upper polynomial is the
     Cholesky rows of its blended TV and the rows of its even and odd parts), each compiled alone into a kernel that reconstructs ONE
     polynomial: FP64 / all VALU instructions of the kernel (a handful of them are the kernel's own loads / stores).
  2. the loops of the hot kernels (tools/isa_loops.py) in the given assembly of pam_amd/csrc/awfl_kernels.hip, compiled here when no
     file is given:  awfl_flux_kernel<false,true,false,false> (C2's y + z sweeps: the pass-1 loops, then the pair loops, whose
     rows make five trips of two fields per round -- the per-polynomial column divides them by 10) and
     awfl_xupd_kernel<2,false> (the fused x-sweep: its first loop is the main loop, seven polynomials per trip)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_loops  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value"]

SINGLE = r'''
#include <hip/hip_runtime.h>
#include "awfl_device.h"
using namespace pama;
extern "C" __global__ void ledger_const(const double *__restrict__ u, double *__restrict__ out) {
  const long long t = blockIdx.x * blockDim.x + threadIdx.x;
  const WenoConsts wc = weno_consts();
  double w[5], L, R;
  for (int s = 0; s < 5; s++) w[s] = u[t * 5 + s];
  weno5_const(w, wc, L, R);
  out[2 * t] = L; out[2 * t + 1] = R;
}
extern "C" __global__ void ledger_table(const double *__restrict__ u, const double *__restrict__ vz, double *__restrict__ out) {
  const long long t = blockIdx.x * blockDim.x + threadIdx.x;
  const WenoConsts wc = weno_consts();
  double w[5], L, R;
  for (int s = 0; s < 5; s++) w[s] = u[t * 5 + s];
  weno5_table(w, vz, 1, wc, L, R);
  out[2 * t] = L; out[2 * t + 1] = R;
}
'''


def kernel_counts(asm, name):
    text = open(asm).read()
    m = re.search(r"^%s:" % name, text, flags=re.M)
    body = text[m.end():]
    body = body[:body.index("s_endpgm")]
    v = [l for l in body.split("\n") if re.match(r"\s+v_", l)]
    return sum("_f64" in l for l in v), len(v)


def main():
    with tempfile.TemporaryDirectory() as td:
        src, asm = os.path.join(td, "ledger.hip"), os.path.join(td, "ledger.s")
        open(src, "w").write(SINGLE)
        subprocess.run([HIPCC] + FLAGS + ["-I", os.path.join(ROOT, "pam_amd", "csrc"), src, "-o", asm], check=True)
        print("%-44s %6s %6s" % ("one polynomial", "f64", "VALU"))
        for k, label in (("ledger_const", "weno5_const (x, y)"), ("ledger_table", "weno5_table (z, factored wave-uniform table)")):
            f, v = kernel_counts(asm, k)
            print("%-44s %6d %6d" % (label, f, v))
        big = sys.argv[1] if len(sys.argv) > 1 else None
        if big is None:
            big = os.path.join(td, "awfl.s")
            subprocess.run([HIPCC] + FLAGS + [os.path.join(ROOT, "pam_amd", "csrc", "awfl_kernels.hip"), "-o", big], check=True)
        for key, per in (("16awfl_flux_kernelILb0ELb1ELb0ELb0E", 10), ("16awfl_xupd_kernelILi2ELb0E", 7)):
            rows, _ = isa_loops.stats(big, key)
            print("== %s  (f64/poly: f64 / %d)" % (key, per))
            for r in rows:
                print("%-12s instr %5d VALU %5d f64 %5d  f64/poly %6.1f" % (r[0], r[2], r[4], r[6], r[6] / per))


if __name__ == "__main__":
    main()
