// Stand-alone driver of csrc/gemm_plan.h for tests/test_gemm_plan_cpu.py: host compiler only, built with
// -fsanitize=address,undefined and run directly.  Reads commands from stdin, one per line:
//   plan  <cus> <arith> <variant> <force_tm> <force_tile256> <fewtiles> <table> <table_f16>
//         <M> <N> <K> <a_kmaj> <b_kmaj> <aligned> <a_planes> <w_planes> <c_planes> <f16> <act> <alpha> <beta> <drop_p>
//         <bias> <residual> <mask> <gate> <bf16x3_entry>
//       -> family J tm cls cfg a_planes c_planes grid_x grid_y block | refusal
//       (a table is "-" for none, "empty", or "NxK=cfg;..."; bf16x3_entry = 1 applies ac_linear_bf16x3's rule: A planes are
//        dropped when the shape does not take them)
//   sweep <cus>   the planner's invariants over the shape grid of the test (see main): counts of shapes and of violations
#include "../adaptive-classifier_amd/csrc/gemm_plan.h"

#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>

using namespace acg;

static PipeTable parse_table(const std::string& s) {
    PipeTable t;
    if (s == "-") return t;
    t.n = 0;
    if (s == "empty") return t;
    const char* p = s.c_str();
    while (*p && t.n < 16) {
        int N = 0, K = 0, cfg = 0, used = 0;
        if (sscanf(p, "%dx%d=%d%n", &N, &K, &cfg, &used) != 3) break;
        t.rules[t.n++] = {N, K, cfg};
        p += used;
        if (*p == ';') ++p;
    }
    return t;
}

static long long g_checked = 0, g_bad = 0, g_ln_shapes = 0;
static void expect(bool ok, const char* what, const GemmQuery& q, const GemmEnv& e) {
    ++g_checked;
    if (!ok && g_bad++ < 10)
        printf("violation: %s at %d x %d x %d arith %d variant %d cus %d c_planes %d\n", what, q.M, q.N, q.K, e.arith, e.variant, e.cus, (int)q.c_planes);
}

static void sweep(int cus) {
    const int Ns[] = {1, 8, 15, 16, 64, 128, 136, 768, 3072}, Ks[] = {4, 8, 12, 32, 64, 96, 768};
    for (int arith = 0; arith <= 1; ++arith)
        for (int variant = 0; variant <= 1; ++variant) {
            GemmEnv e;
            e.cus = cus; e.arith = arith; e.variant = variant;
            for (int M = 1; M <= 600; ++M)
                for (int N : Ns)
                    for (int K : Ks) {
                        GemmQuery q;
                        q.M = M; q.N = N; q.K = K; q.bias = true; q.a_planes = q.w_planes = true;
                        const bool takes = linear_takes_planes(M, N, K, e);
                        for (int cp = 0; cp <= 1; ++cp) {
                            q.c_planes = cp != 0;
                            const GemmPlan p = gemm_plan(q, e);
                            // result planes hold 8 columns per slot: with N % 8 != 0 the parent refuses them by name, and so does the plan
                            if (takes && cp && (N % 8) != 0) expect(p.family == GEMM_REFUSE && strstr(p.refusal, "N %% 8 == 0"), "planes out with N % 8 != 0 must be refused", q, e);
                            else if (takes) expect(p.family != GEMM_REFUSE && p.grid_x >= 1 && p.block >= 64, "takes planes, but the plan refuses", q, e);
                            else expect(p.family == GEMM_REFUSE, "does not take planes, but the plan accepts them", q, e);
                            if (takes && p.family != GEMM_REFUSE) expect(p.family == GEMM_RING || p.family == GEMM_PLANES8 || p.family == GEMM_PLANES, "planes on a kernel without planes", q, e);
                        }
                        q.c_planes = false; q.residual = true;
                        if (pipe_ln_shape(M, N, K, e)) {         // stated from the kernel's side: split arithmetic, default variant, the built-in
                            ++g_ln_shapes;                       // rule's own choice, one 128 x 128 tile per CU at most, 8 waves, bias + residual
                            const GemmPlan p = gemm_plan(q, e);
                            const unsigned tiles = (unsigned)((M + 127) / 128) * (unsigned)(N / 128);
                            expect(arith != 0 && variant == 0 && M >= 192 && K >= 64 && K % 32 == 0 && N % 128 == 0 && N <= 1024 && (int)tiles <= cus &&
                                       builtin_choose(M, N, EPI_BIAS_RES, false, cus) == 124262 && p.family == GEMM_RING && p.cfg == 124262 &&
                                       p.cls == EPI_BIAS_RES && !p.c_planes && p.grid_x == tiles && p.block == 512,
                                   "LayerNorm fusion without its tile", q, e);
                        }
                        q = GemmQuery();                         // fp32 operands never refuse, and only an NT aligned shape leaves the direct kernel
                        q.M = M; q.N = N; q.K = K; q.bias = true;
                        expect(gemm_plan(q, e).family != GEMM_REFUSE, "fp32 operands refused", q, e);
                        q.aligned = false;
                        expect(gemm_plan(q, e).family == GEMM_DIRECT, "misaligned operands off the direct kernel", q, e);
                    }
        }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, table, table_f16;
        in >> cmd;
        if (cmd == "sweep") {
            int cus = 0;
            in >> cus;
            g_checked = g_bad = g_ln_shapes = 0;
            sweep(cus);
            printf("sweep cus %d ln_shapes %lld checked %lld violations %lld\n", cus, g_ln_shapes, g_checked, g_bad);
        } else if (cmd == "plan") {
            GemmEnv e;
            GemmQuery q;
            int fewtiles, b[14], entry;
            in >> e.cus >> e.arith >> e.variant >> e.force_tm >> e.force_tile256 >> fewtiles >> table >> table_f16 >> q.M >> q.N >> q.K;
            for (int i = 0; i < 7; ++i) in >> b[i];
            in >> q.act >> q.alpha >> q.beta >> q.drop_p;
            for (int i = 7; i < 11; ++i) in >> b[i];
            in >> entry;
            if (!in) { printf("error: cannot parse '%s'\n", line.c_str()); return 2; }
            e.fewtiles = fewtiles != 0; e.table = parse_table(table); e.table_f16 = parse_table(table_f16);
            q.a_kmaj = b[0]; q.b_kmaj = b[1]; q.aligned = b[2]; q.a_planes = b[3]; q.w_planes = b[4]; q.c_planes = b[5]; q.f16 = b[6];
            q.bias = b[7]; q.residual = b[8]; q.mask = b[9]; q.gate = b[10];
            if (entry) q.a_planes = q.a_planes && linear_takes_planes(q.M, q.N, q.K, e);
            const GemmPlan p = gemm_plan(q, e);
            printf("%d %d %d %d %d %d %d %u %u %u | %s\n", p.family, p.J, p.tm, p.cls, p.cfg, (int)p.a_planes, (int)p.c_planes, p.grid_x, p.grid_y,
                   p.block, p.refusal ? p.refusal : "-");
        } else if (!cmd.empty()) {
            printf("error: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
