"""Record the native call sequence of every case of tests/knn_call_cases.py on the GPU (entry names and marshalled arguments, the
workspace planners included) -> a JSON fixture.  Run once at the commit whose marshalling is the reference:

    python tools/knn_call_probe.py --out tests/data/knn_calls_parent.json

tests/test_knn_calls_gpu.py replays the cases and asserts equality.  --compare FILE prints the cases that differ from FILE."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "adaptive-classifier_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def dump(records, path):
    """one case per line: the fixture stays diffable"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in records.items()) + "\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", default=None)
    args = ap.parse_args()
    import torch
    import knn_call_cases as cases
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    nv.require_gpu()
    records = cases.run_all(nv, ix, torch.device("cuda:0"))
    print(len(records), "cases,", sum(len(r["calls"]) for r in records.values()), "native calls,",
          sum(r["raised"] is not None for r in records.values()), "raised")
    if args.out:
        dump(records, args.out)
    if args.compare:
        want = json.load(open(args.compare))
        bad = [k for k in want if records.get(k) != want[k]]
        print("differ from", args.compare + ":", bad or "none")
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
