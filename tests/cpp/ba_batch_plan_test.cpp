// ba_batch_plan_test.cpp -- how eao_local_ba_batch deals its windows (eao_fusion_amd/csrc/ba_batch_plan.h) without a GPU: the plan's invariants over every
// combination of batch size, switches, core count and latency marker a call can meet, and a table of literal plans.  Built by tests/test_ba_batch_plan_cpu.py with
// -fsanitize=address,undefined (group_of and the gStart writes stay inside the G + 1 entries).
#include <cstdio>
#include <vector>

#include "../../eao_fusion_amd/csrc/ba_batch_plan.h"

using namespace eao::lm;

static long check_invariants() {
    long cases = 0, failed = 0;
    BatchPlan P;
    for (int n = 1; n <= 96; n++)
        for (int envThreads = 0; envThreads <= 20; envThreads++)
            for (int envGroups = 0; envGroups <= 9; envGroups++)
                for (int hw : {0, 1, 2, 6, 16, 64, 256})
                    for (int even = 0; even < 2; even++)
                        for (int alive = 0; alive < 2; alive++) {
                            plan_batch(BatchPlanIn{n, envThreads, envGroups, hw, even != 0, alive != 0}, P);
                            cases++;
                            bool ok = 1 <= P.nThreads && P.nThreads <= n && 1 <= P.G && P.G <= P.nThreads && (int)P.gStart.size() == P.G + 1;
                            ok = ok && P.gStart[0] == 0 && P.gStart[P.G] == n;
                            for (int g = 0; ok && g < P.G; g++) {
                                ok = P.gStart[g] < P.gStart[g + 1];                              // no group is empty
                                if (!even && n >= 8) ok = ok && P.gStart[g] % 8 == 0;            // whole rows of eight
                                for (int w = P.gStart[g]; ok && w < P.gStart[g + 1]; w++) ok = P.group_of(w) == g;
                            }
                            if (!ok && failed++ < 10)
                                std::fprintf(stderr, "FAILED invariants: n %d, threads %d, groups %d, hw %d, even %d, latency %d -> nThreads %d, G %d\n", n, envThreads,
                                             envGroups, hw, even, alive, P.nThreads, P.G);
                        }
    std::printf("%ld plans enumerated, %ld break an invariant\n", cases, failed);
    return failed;
}

// Literal plans, written down from the arithmetic as it stood inside eao_local_ba_batch before it moved into the header (hw = 64 unless the row says otherwise): a slip
// in the arithmetic cannot pass by agreeing with itself.
struct Pinned { const char* what; BatchPlanIn in; int nThreads; std::vector<int> sizes; };
static int check_pinned() {
    const int hw = 64;
    const std::vector<Pinned> table = {
        {"default", {1, 0, 0, hw, false, false}, 1, {1}},
        {"default", {7, 0, 0, hw, false, false}, 7, {7}},
        {"default", {8, 0, 0, hw, false, false}, 8, {8}},
        {"default", {11, 0, 0, hw, false, false}, 11, {11}},
        {"default", {12, 0, 0, hw, false, false}, 12, {8, 4}},
        {"default", {15, 0, 0, hw, false, false}, 15, {8, 7}},
        {"default", {17, 0, 0, hw, false, false}, 16, {8, 9}},
        {"default", {20, 0, 0, hw, false, false}, 16, {8, 8, 4}},
        {"default", {24, 0, 0, hw, false, false}, 16, {8, 8, 8}},
        {"default", {25, 0, 0, hw, false, false}, 16, {8, 8, 9}},
        {"default", {28, 0, 0, hw, false, false}, 16, {8, 8, 8, 4}},
        {"default", {33, 0, 0, hw, false, false}, 16, {8, 8, 8, 9}},
        {"default", {40, 0, 0, hw, false, false}, 16, {8, 8, 8, 16}},
        {"default", {64, 0, 0, hw, false, false}, 16, {16, 16, 16, 16}},
        {"latencyAlive", {8, 0, 0, hw, false, true}, 8, {8}},
        {"latencyAlive", {12, 0, 0, hw, false, true}, 12, {8, 4}},
        {"latencyAlive", {25, 0, 0, hw, false, true}, 16, {8, 17}},
        {"latencyAlive", {40, 0, 0, hw, false, true}, 16, {16, 24}},
        {"even", {7, 0, 0, hw, true, false}, 7, {7}},
        {"even", {9, 0, 0, hw, true, false}, 9, {4, 5}},
        {"even", {12, 0, 0, hw, true, false}, 12, {4, 4, 4}},
        {"even", {25, 0, 0, hw, true, false}, 16, {6, 6, 6, 7}},
        {"envThreads = 1", {25, 1, 0, hw, false, false}, 1, {25}},
        {"envGroups = 1", {25, 0, 1, hw, false, false}, 16, {25}},
        {"envGroups = 6", {64, 0, 6, hw, false, false}, 16, {8, 8, 16, 8, 8, 16}},
        {"hw = 2", {25, 0, 0, 2, false, false}, 1, {25}},
        {"hw = 6", {25, 0, 0, 6, false, false}, 3, {8, 8, 9}},
    };
    int failed = 0;
    BatchPlan P;
    for (const Pinned& t : table) {
        plan_batch(t.in, P);
        std::vector<int> sizes;
        for (int g = 0; g + 1 < (int)P.gStart.size(); g++) sizes.push_back(P.gStart[g + 1] - P.gStart[g]);
        if (P.nThreads == t.nThreads && P.G == (int)t.sizes.size() && sizes == t.sizes) continue;
        failed++;
        std::fprintf(stderr, "FAILED pinned plan (%s, n %d): nThreads %d (want %d), groups", t.what, t.in.n, P.nThreads, t.nThreads);
        for (int s : sizes) std::fprintf(stderr, " %d", s);
        std::fprintf(stderr, " (want");
        for (int s : t.sizes) std::fprintf(stderr, " %d", s);
        std::fprintf(stderr, ")\n");
    }
    std::printf("%d pinned plans, %d differ\n", (int)table.size(), failed);
    return failed;
}

int main() {
    const long bad = check_invariants() + check_pinned();
    if (!bad) std::printf("all plans as required\n");
    return bad ? 1 : 0;
}
