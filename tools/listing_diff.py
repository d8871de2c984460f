#!/usr/bin/env python3
"""Compare two device listings (hipcc -S --cuda-device-only) kernel by kernel.

    python tools/listing_diff.py parent_gemm.s result_gemm.s

A host-only refactor must leave every kernel's code, kernel descriptor and metadata entry as they were.  hipcc emits template
instantiations in the order the host code first names them, so the ORDER of kernels in a listing may move with host code while no
kernel changes; the function-local label numbers (.LBB<n>_, .Lfunc_end<n>, "Header=BB<n>_") and the column of the comment after
a label move with it.  This tool therefore keys every block by its kernel symbol, drops lines that carry a file path, the compiler ident or the per-source `__hip_cuid_` hash, and reports
  * kernels only in one listing,
  * kernels whose text / descriptor / metadata entry differ,
  * whether the kernels come in the same order, and whether what is outside any kernel block is equal.
Exit status 0: identical in every respect; 2: the same kernels, each identical, in another order; 1: anything else.
"""
import re
import sys

LABEL = re.compile(r"(\.L|=)(BB|func_end|func_begin|tmp)\d+")
DROP = re.compile(r"\.file\b|\.ident\b|__hip_cuid_|/[\w.-]+/[\w./-]+\.(hip|h|cpp)")
BEGIN = re.compile(r"\.globl\s+(\S+)\s*; -- Begin function")


def parse(path):
    lines = [re.sub(r"[ \t]+;", " ;", LABEL.sub(lambda m: m.group(1) + m.group(2), l.rstrip())) for l in open(path) if not DROP.search(l)]
    meta_at = next(i for i, l in enumerate(lines) if l.strip() == ".amdgpu_metadata")
    code, meta = lines[:meta_at], lines[meta_at:]
    kernels, order, rest, cur, in_cs = {}, [], [], None, False
    for i, l in enumerate(code):
        m = BEGIN.search(l)
        if m:
            cur, in_cs = m.group(1), False
            order.append(cur)
            kernels[cur] = [rest.pop()] if rest and ".section" in rest[-1] else []
        elif cur and in_cs and not l.startswith(";"):
            cur = None                                       # the block ends after its ".AMDGPU.csdata" comment lines
        if cur:
            kernels[cur].append(l)
            in_cs = in_cs or ".AMDGPU.csdata" in l
        else:
            rest.append(l)
    entries, key, buf = {}, None, []
    for l in meta:                                           # one "  - " list item per kernel under amdhsa.kernels
        if l.startswith("  - ") or not l.startswith("    "):
            if key:
                entries[key] = buf
            key, buf = None, []
        buf.append(l)
        if l.strip().startswith(".name:"):
            key = l.split()[-1]
    return kernels, order, rest, entries


def main(a, b):
    ka, oa, ra, ma = parse(a)
    kb, ob, rb, mb = parse(b)
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k] or ma.get(k) != mb.get(k))
    print("kernels: %d and %d; only in first: %d, only in second: %d, differing: %d" % (len(ka), len(kb), len(only_a), len(only_b), len(differ)))
    for k in only_a + only_b + differ:
        print("  " + k)
    print("same order: %s; outside the kernel blocks equal: %s" % (oa == ob, ra == rb))
    if only_a or only_b or differ or set(ma) != set(mb) or ra != rb:
        return 1
    return 2 if oa != ob else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
