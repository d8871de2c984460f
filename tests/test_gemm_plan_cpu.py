"""csrc/gemm_plan.h, the host-side GEMM dispatch as a pure function, against the launches the parent commit really made.

No GPU: gemm_plan.h is plain C++17, so tests/gemm_plan_cli.cpp is built with the host compiler under AddressSanitizer and
UBSan and run directly as a stand-alone program.
  * every case of tests/data/gemm_dispatch_parent.json (kernel names, grids and blocks from a kernel trace of the parent
    commit's library on MI355X, tools/gemm_dispatch_probe.py) is planned with the recorded CU count: family, compile-time
    selectors, grid and block must equal the trace, and a recorded refusal must be a refusal;
  * a sweep over M in 1..600 x N x K x arithmetic x variant at 256 and 64 CUs: where linear_takes_planes holds the plan
    never refuses operand planes (it refuses result planes exactly when N % 8 != 0, the layout's own condition, as the parent
    does), where it does not hold the plan always refuses them, and pipe_ln_applies' shape half implies the LayerNorm tile
    (checked against the built-in rule and the tile's geometry written out, not against the plan's own cfg);
  * the environment switches (forced tm, forced 8-wave tile, few-tile kernel off), which need no GPU to be covered."""
import json
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "data", "gemm_dispatch_parent.json")
CXX = shutil.which("g++") or shutil.which("clang++")

REFUSE, SMALLM, FEWTILES, RING, PLANES8, PLANES, SPLIT, TILE, DIRECT = range(9)
KEYS = ("family", "J", "tm", "cls", "cfg", "a_planes", "c_planes", "grid_x", "grid_y", "block")


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler (g++ or clang++): the planner cannot be checked"
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_cli")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "gemm_plan_cli.cpp"), "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        return r.stdout.splitlines()
    return run


def plan_line(cus, M, N, K, arith=1, variant=0, force_tm=0, tile256=-1, fewtiles=1, table=None, table_f16=None, a_kmaj=1, b_kmaj=1,
              aligned=1, a_planes=0, w_planes=0, c_planes=0, f16=0, act=0, alpha=1.0, beta=0.0, drop_p=0.0, bias=1, residual=0, mask=0,
              gate=0, entry=0):
    tab = lambda t: "-" if t is None else (t or "empty")
    return " ".join(str(x) for x in ("plan", cus, arith, variant, force_tm, tile256, fewtiles, tab(table), tab(table_f16), M, N, K,
                                     a_kmaj, b_kmaj, aligned, a_planes, w_planes, c_planes, f16, act, alpha, beta, drop_p, bias,
                                     residual, mask, gate, entry))


def parse(out):
    nums, refusal = out.split(" | ")
    return dict(zip(KEYS, (int(x) for x in nums.split())), refusal=refusal)


def case_line(c, cus):
    """The planner's query for a recorded case: what the public entry passes to launch_gemm (csrc/gemm.hip)."""
    kw = dict(arith=c["arith"], variant=c["variant"], table=c["table"], act=c["act"], residual=int(c["res"]))
    if c["entry"] == "gemm_f32":
        kw.update(a_kmaj=int(c["transA"] == 0), b_kmaj=int(c["transB"] != 0), alpha=c["alpha"], beta=c["beta"], bias=0, residual=0)
    elif c["entry"] == "linear_f32":
        kw.update(aligned=int((c["K"] + c["lda_pad"]) % 4 == 0))
    elif c["entry"] == "linear_bf16x3":
        kw.update(a_planes=int("a" in c["planes"]), w_planes=int("w" in c["planes"]), c_planes=int(c["cplanes"]), entry=1)
    else:
        kw.update(f16=1, a_planes=1, w_planes=1, c_planes=int(c["cplanes"]))
    return plan_line(cus, c["M"], c["N"], c["K"], **kw)


def from_trace(kernel):
    """(family, selectors) named by a kernel of the trace, e.g. 'gemm_planes_nt<1, 2, true, false, 2>'"""
    m = re.fullmatch(r"gemm_(\w+?)(?:<(.*)>)?", kernel)
    name, a = m.group(1), [{"true": 1, "false": 0}.get(x.strip(), x.strip()) for x in (m.group(2) or "").split(",") if x.strip()]
    a = [int(x) for x in a]
    if name == "smallm_nt":
        return dict(family=SMALLM, J=a[0])
    if name == "fewtiles_nt":
        return dict(family=FEWTILES)
    if name == "pipe_nt":        # <EPI, TM, TN, WMW, WNW, NS, C_PLANES, PIPE, AR>; cfg = tm tn wmw wnw ns pipe, one digit each
        return dict(family=RING, cls=a[0], cfg=int("%d%d%d%d%d%d" % (a[1], a[2], a[3], a[4], a[5], a[7])), c_planes=a[6])
    if name == "planes_nt":      # <EPI, TM, A_PLANES, C_PLANES, WMW>
        return dict(family=PLANES8 if a[4] == 4 else PLANES, cls=a[0], tm=a[1], a_planes=a[2], c_planes=a[3])
    if name in ("split_nt", "tile_nt"):
        return dict(family=SPLIT if name == "split_nt" else TILE, cls=a[0], tm=a[1])
    assert name == "direct", kernel
    return dict(family=DIRECT)


def test_plan_equals_the_parents_recorded_launches(cli):
    fx = json.load(open(FIXTURE))
    cases = fx["cases"]
    plans = [parse(o) for o in cli([case_line(c, fx["cus"]) for c in cases])]
    assert len(plans) == len(cases)
    seen = set()
    for c, p in zip(cases, plans):
        if c["rc"] != 0:
            assert p["family"] == REFUSE and p["refusal"] != "-", (c["id"], p)
            continue
        want = from_trace(c["kernel"])
        want.update(grid_x=c["grid"][0], grid_y=c["grid"][1], block=c["block"][0])
        assert c["grid"][2] == 1 and c["block"][1:] == [1, 1], c
        assert {k: p[k] for k in want} == want, (c["id"], c["kernel"], p)
        seen.add(p["family"])
    assert seen == {SMALLM, FEWTILES, RING, PLANES8, PLANES, SPLIT, TILE, DIRECT}      # the fixture reaches every family


def test_fixture_is_the_case_list():
    import gemm_dispatch_cases as G
    recorded = json.load(open(FIXTURE))["cases"]
    assert [{k: c[k] for k in G.CASES[0]} for c in recorded] == G.CASES
    assert all((c["rc"] == 0) == (c["sha256"] is not None) for c in recorded)


def test_direct_family_follows_the_transposes():
    fx = json.load(open(FIXTURE))
    for c in fx["cases"]:
        if c["entry"] == "gemm_f32" and "direct" in c["kernel"]:
            assert c["kernel"] == "gemm_direct<%s, %s>" % ("true" if c["transA"] == 0 else "false", "true" if c["transB"] else "false")


@pytest.mark.parametrize("cus", [256, 64])
def test_sweep_planes_predicate_and_plan_agree(cli, cus):
    out = cli(["sweep %d" % cus])
    assert out[-1].startswith("sweep cus %d ln_shapes " % cus) and out[-1].endswith(" violations 0"), out[-12:]
    f = out[-1].split()
    assert int(f[6]) >= 600 * 9 * 7 * 2 * 2 * 4
    assert int(f[4]) >= 400          # the LayerNorm invariant is not vacuous: N = 128 and 768 at K >= 64, M >= 192 (bf16x3, variant 0)


def test_environment_switches(cli):
    P = lambda **kw: parse(cli([plan_line(256, **kw)])[0])
    planes = dict(a_planes=1, w_planes=1)
    # AC_GEMM_TM: 8256 x 1024 x 32 takes the 128-row tile under bf16x3 (520 tiles: one round of 3 per CU); forced to 64 rows and back
    free = P(M=8256, N=1024, K=32)
    assert (free["family"], free["tm"], free["grid_x"]) == (SPLIT, 2, 520)
    forced = P(M=8256, N=1024, K=32, force_tm=1)
    assert (forced["family"], forced["tm"], forced["grid_x"]) == (SPLIT, 1, 1032)
    assert P(M=8256, N=1024, K=32, arith=0)["tm"] == 1 and P(M=8256, N=1024, K=32, arith=0, force_tm=2)["tm"] == 2
    assert P(M=8256, N=1024, K=32, force_tm=3) == free                          # only 1 and 2 are values
    # AC_GEMM_TILE256: the 8-wave tile forced on for a shape far below 3 rounds, and off for one that has them
    small = dict(M=192, N=136, K=32, **planes)
    assert P(**small)["family"] == PLANES
    on = P(tile256=1, **small)
    assert (on["family"], on["tm"], on["grid_x"], on["block"]) == (PLANES8, 2, 2, 512)
    big = dict(M=8192, N=3072, K=32, **planes)
    assert P(**big)["family"] == PLANES8 and P(tile256=0, **big)["family"] == PLANES
    assert P(tile256=1, act=1, **small)["family"] == PLANES                     # (no 8-wave ReLU kernel is built: the switch cannot name one)
    assert P(tile256=1, M=192, N=136, K=64, **planes)["family"] == RING         # the ring is asked first
    # AC_GEMM_FEWTILES=0: the few-tile shapes fall to the direct or the tiled kernels
    assert P(M=65, N=8, K=64)["family"] == FEWTILES and P(M=65, N=8, K=64, fewtiles=0)["family"] == DIRECT
    assert P(M=192, N=128, K=64)["family"] == FEWTILES and P(M=192, N=128, K=64, fewtiles=0)["family"] == SPLIT
    assert P(M=192, N=128, K=64, fewtiles=0, arith=0)["family"] == TILE


def test_refusals_carry_the_messages_of_the_launch_path(cli):
    P = lambda **kw: parse(cli([plan_line(256, **kw)])[0])
    both = dict(a_planes=1, w_planes=1)
    assert "fused GeGLU needs the pre-split kernel" in P(M=192, N=128, K=64, act=3, w_planes=1)["refusal"]
    assert "does not take the pre-split kernel" in P(M=191, N=128, K=64, **both)["refusal"]
    assert "does not take the pre-split kernel" in P(M=192, N=128, K=64, arith=0, **both)["refusal"]
    assert "does not take the pre-split kernel" in P(M=192, N=128, K=64, a_planes=1)["refusal"]          # A planes without W planes
    assert "N %% 64 == 0" in P(M=192, N=136, K=64, act=3, c_planes=1, **both)["refusal"]
    assert "bias / bias+gelu epilogue" in P(M=192, N=136, K=64, residual=1, c_planes=1, **both)["refusal"]
    assert "bias / bias+gelu epilogue" in P(M=192, N=132, K=64, c_planes=1, **both)["refusal"]
    assert P(M=8192, N=3076, K=32, c_planes=1, **both)["refusal"] == "gemm: planes output needs N %% 8 == 0"
    assert "linear_f16x2: %d x %d x %d does not take" in P(M=192, N=136, K=32, f16=1, **both)["refusal"]
    assert "linear_f16x2" in P(M=192, N=136, K=64, f16=1, variant=1, **both)["refusal"]
    ok = P(M=192, N=136, K=64, f16=1, **both)
    assert ok["family"] == RING and ok["cfg"] > 0 and ok["refusal"] == "-"
