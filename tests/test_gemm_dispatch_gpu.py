"""Every leaf of the GEMM dispatch (csrc/gemm_plan.h) computes what the parent commit computed, bit for bit.

tests/data/gemm_dispatch_parent.json holds, for each case of tests/gemm_dispatch_cases.py, the kernel the PARENT commit's
library launched on MI355X (name, grid, block: tests/test_gemm_plan_cpu.py checks the planner against those) and the sha256
of the bytes it wrote.  Here the same calls run in this process and the hashes must be equal: the same kernel instantiation
with the same grid on the same inputs is deterministic, so any difference is a changed dispatch or a changed launch argument.
The plan depends on the CU count; on a device with another count than the recorded one the hashes need not apply."""
import json
import os

import pytest

import gemm_dispatch_cases as G

pytestmark = pytest.mark.gpu

FIXTURE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "gemm_dispatch_parent.json")))
RECORDED = {c["id"]: c for c in FIXTURE["cases"]}


@pytest.mark.parametrize("case", G.CASES, ids=[c["id"] for c in G.CASES])
def test_output_is_bit_identical_to_the_parents(case, cuda_dev):
    from adaptive_classifier import _native as nv
    cus = nv.device_info()["cus"]
    if cus != FIXTURE["cus"]:
        pytest.skip("fixture recorded on %d CUs, this device has %d: the dispatch depends on the count" % (FIXTURE["cus"], cus))
    want = RECORDED[case["id"]]
    rc, sha = G.run_case(nv, cuda_dev, case)
    assert rc == want["rc"], (rc, nv.lib().ac_last_error())
    assert sha == want["sha256"], want.get("kernel")
