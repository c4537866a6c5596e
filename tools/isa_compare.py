#!/usr/bin/env python3
"""Compare the gfx950 code of two versions of a HIP source kernel by kernel (no GPU needed).

usage: python tools/isa_compare.py BASE NEW [KERNEL [LINES]] > profiles/rNN_isa_compare.txt
BASE / NEW: a .hip source (compiled here: hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only) or its assembly (.s).
Kernels are matched by demangled name after mapping the tracer-sweep families that were merged into one
(awfl_xtr_kernel<S, P, A> -> <S, P, 2, A>, awfl_xtrn_kernel<S, P, G> -> awfl_xtr_kernel<S, P, G, false>, awfl_xupd_kernel<S, F[, P]> -> <S, F, P, false>) and the two canary kernels that became coupling_canary_kernel<word>; symbol names and local labels
are normalised.  Per kernel: the resources the compiler reports (VGPRs, AGPRs, SGPRs, scratch, waves per SIMD, LDS) and the instruction
stream -- `identical`, `registers renamed` (the same opcodes in the same order, other register numbers) or `DIFFERENT` (with the
opcode-count deltas).  KERNEL: print a unified diff of that kernel's streams as well (LINES of it, default 80).
Exit status 0 when every kernel is identical or only renamed and the two sides hold the same kernels."""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

RES = ["TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize"]
# the canary kernels of the SHOC and the P3 coupling layer, merged into one template over the word they write
CANARY = {"shoc_canary_kernel": 0x7ff853484f435f5f, "p3_canary_kernel": 0x7ff850335f57535f}


def assembly(path, tmp):
    if path.endswith(".s"):
        return open(path).read()
    out = os.path.join(tmp, "k%d.s" % len(os.listdir(tmp)))
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Wno-unused-value", path, "-o", out], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-3000:])
    return open(out).read()


def canon(d):
    d = d.replace("(anonymous namespace)::", "")
    d = re.sub(r"\(.*", "", d).replace("void ", "")
    m = re.match(r"awfl_xtrn_kernel<(\d+), (\d+), (\d+)>", d)
    if m:
        return "awfl_xtr_kernel<%s, %s, %s, false>" % m.groups()
    m = re.match(r"awfl_xtr_kernel<(\d+), (\d+), (false|true)>", d)
    if m:
        return "awfl_xtr_kernel<%s, %s, 2, %s>" % m.groups()
    m = re.match(r"awfl_xupd_kernel<(\d+), (false|true)(?:, (false|true))?>$", d)      # (PRESSURE and LAZY_SEED default to false)
    if m:
        return "awfl_xupd_kernel<%s, %s, %s, false>" % (m.group(1), m.group(2), m.group(3) or "false")
    if d in CANARY:
        return "coupling_canary_kernel<%dull>" % CANARY[d]
    return d


def kernels(s):
    """canonical name -> (instruction lines, resources) of every .amdhsa_kernel entry"""
    entries = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", s, flags=re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(entries), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for sym, d in zip(entries, dem):
        m = re.search(r"^%s:[^\n]*\n" % re.escape(sym), s, flags=re.M)
        body = s[m.end():]
        end = body.find(".Lfunc_end")
        lines = []
        for l in body[:end].split("\n"):
            l = l.split(";")[0].rstrip()
            if not l.strip() or (l.strip().startswith(".") and not re.match(r"\s*\.LBB", l)):
                continue
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)
            lines.append(re.sub(r"_Z\w+", "SYM", l))
        tail = body[end:end + 4000]
        res = tuple(int(re.search(r"; %s: (\d+)" % k, tail).group(1)) for k in RES)
        out[canon(d)] = (lines, res + (sum(1 for l in lines if l.startswith(("\t", " "))),))
    return len(entries), out


def opcodes(lines):
    return [l.split()[0] for l in lines if l.startswith(("\t", " "))]


def main():
    with tempfile.TemporaryDirectory() as tmp:
        (na, a), (nb, b) = kernels(assembly(sys.argv[1], tmp)), kernels(assembly(sys.argv[2], tmp))
    print("# .amdhsa_kernel entries: %d base, %d new; matched by name: %d" % (na, nb, len(set(a) & set(b))))
    print("%-64s %5s %5s %5s %8s %6s %8s %7s  %s" % ("kernel", "SGPR", "VGPR", "AGPR", "scratch", "w/SIMD", "LDS(st.)", "instr", "instruction stream"))
    count = collections.Counter()
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            verdict = "ONLY IN " + ("base" if k in a else "new")
        else:
            (la, ra), (lb, rb) = a[k], b[k]
            if ra != rb:
                verdict = "DIFFERENT resources (base: %s)" % " ".join(map(str, ra))
            elif la == lb:
                verdict = "identical"
            elif opcodes(la) == opcodes(lb):
                verdict = "registers renamed"
            else:
                oa, ob = collections.Counter(opcodes(la)), collections.Counter(opcodes(lb))
                verdict = "DIFFERENT %s" % dict(sorted((o, ob[o] - oa[o]) for o in set(oa) | set(ob) if oa[o] != ob[o]))
        count[verdict.split()[0] + (" renamed" if verdict == "registers renamed" else "")] += 1
        print("%-64s %5d %5d %5d %8d %6d %8d %7d  %s" % ((k[:64],) + (b.get(k) or a[k])[1] + (verdict,)))
    print("# " + ", ".join("%s: %d" % kv for kv in sorted(count.items())))
    if len(sys.argv) > 3:
        k = sys.argv[3]
        print("\n".join(list(difflib.unified_diff(a[k][0], b[k][0], lineterm="", n=1))[:int(sys.argv[4]) if len(sys.argv) > 4 else 80]))
    ok = na == nb and set(a) == set(b) and set(count) <= {"identical", "registers renamed"}
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
