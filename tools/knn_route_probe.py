"""Record the routing of every sequence of tests/knn_route_cases.py (CPU; the module-level calls of adaptive_classifier.index are
replaced by recorders) -> a JSON fixture.  Run once at the commit whose routing is the reference:

    python tools/knn_route_probe.py --out tests/data/knn_route_parent.json

tests/test_knn_route_cpu.py replays the sequences and asserts equality."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "adaptive-classifier_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import knn_route_cases as cases
    from adaptive_classifier import index as ix
    records = cases.run_all(ix)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:                 # one sequence per line: the fixture stays diffable
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in records.items()) + "\n}\n")
    print(len(records), "sequences,", sum(len(v) for v in records.values()), "steps")


if __name__ == "__main__":
    main()
