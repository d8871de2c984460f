#!/usr/bin/env python3
"""Record the sha256 of what every case of tests/dead_rows_cases.py writes.

    python tools/dead_rows_probe.py --run OUT.json          (on the GPU; AC_LIBACAMD_PATH selects the library: the PARENT
                                                             commit's build for the committed tests/data/dead_rows_parent.json)
    python tools/dead_rows_probe.py --compare A.json B.json

The ring cases run under the forced ring configuration; the encoder cases return the CLS vectors.  A refused call is recorded by
its return code (the fp16x2 entry takes no shape under 192 rows)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "adaptive-classifier_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def run(out):
    os.environ.setdefault("AC_TEST_HOOKS", "1")
    import torch
    from adaptive_classifier import _native as nv
    import dead_rows_cases as D
    dev = torch.device("cuda:0")
    rec = {"cus": nv.device_info()["cus"], "cases": {}}

    def put(cid, **kw):
        rec["cases"][cid] = kw
        print("%-52s %s" % (cid, " ".join("%s=%s" % (k, str(v)[:16]) for k, v in kw.items())), flush=True)

    for c in D.ring_cases():
        rc, got, canary = D.run_ring(nv, dev, c, c["cfg"])
        put(c["id"], rc=rc, sha256=D.sha(got) if rc == 0 else None, canary=canary)
    for c in D.LN_CASES:
        got, launches = D.run_ln(nv, c)
        put(c["id"], sha256=D.sha(got.numpy()), fused_launches=launches)
    for c in D.ATTN_FUSED_CASES:
        put(c["id"], sha256=D.sha(D.run_attn_fused(c).numpy()))
    for c in D.ATTN_TILE_CASES:
        got, want = D.run_tile(c)
        put(c["id"], sha256=D.sha(got.numpy()), err=float((got - want).abs().max()))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    bad = [k for k in sorted(set(A["cases"]) | set(B["cases"]))
           if any(A["cases"].get(k, {}).get(f) != B["cases"].get(k, {}).get(f) for f in ("rc", "sha256", "fused_launches"))]
    for k in bad:
        print(k, A["cases"].get(k), B["cases"].get(k))
    print("%d cases, %d differences" % (len(A["cases"]), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.run:
        run(a.run)
    elif a.compare:
        sys.exit(compare(*a.compare))
