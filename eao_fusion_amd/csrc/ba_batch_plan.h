// ba_batch_plan.h -- how eao_local_ba_batch (lm_host.hip) deals its windows: the number of set-up threads, the number of window groups and where each group starts.
// Plain C++17, no HIP, no environment, no clock (the caller reads the switches and the latency marker and passes them in): tests/cpp/ba_batch_plan_test.cpp
// enumerates it under AddressSanitizer + UBSan on a machine without a GPU.
#pragma once

#include <algorithm>
#include <vector>

namespace eao {
namespace lm {

constexpr int kBatchGroups = 4, kBatchGroupMin = 4;     // default number of window groups / fewest windows worth a group

struct BatchPlanIn {
    int n;                   // windows of the call (>= 1)
    int envThreads;          // EAO_BA_BATCH_THREADS (0: unset)
    int envGroups;           // EAO_BA_BATCH_GROUPS (0: unset)
    int hw;                  // std::thread::hardware_concurrency()
    bool even;               // EAO_BA_BATCH_EVEN (A/B switch: the even split of rounds 2-3)
    bool latencyAlive;       // a frame-rate caller is alive in the process: common.h, note_latency_call
};

struct BatchPlan {
    int nThreads = 1, G = 1;
    std::vector<int> gStart;      // G + 1 entries: group g holds the windows [gStart[g], gStart[g + 1]), gStart[G] == n
    int group_of(int w) const { int g = 0; while (gStart[g + 1] <= w) g++; return g; }
};

// ---- The windows are dealt to G groups (contiguous ranges).  A group is a chain of its own on its own stream: its
//      host-side set-up (validation, pinned mirror, active structure, two uploads per window: ~0.1 ms of memcpy and
//      counting each, on a few host threads), then ONE batched enqueue for its windows.  The first group's kernels start
//      while the others are still being set up, and a group's one-workgroup-per-window solver (a tenth of the chip) and
//      the tails of its other launches overlap the other groups' wide kernels.  More than four streams share hardware
//      queues on this runtime and serialise (measured: 5+ groups are 40 % slower than one).
inline void plan_batch(const BatchPlanIn& in, BatchPlan& P) {
    const int n = in.n;
    // (set-up threads make no HIP call any more -- packing and counting only -- so they scale with the host's cores)
    P.nThreads = std::max(1, std::min(n, in.envThreads > 0 ? in.envThreads : std::min(16, std::max(1, in.hw / 2))));
    // Groups hold WHOLE ROWS of eight windows where the batch has them (BA_WIN pins a window to an XCD row by row, and deals an incomplete row over all eight):
    // 25 windows as 8 + 8 + 9 load every XCD with 3.125 windows, as 6 + 6 + 6 + 7 the fullest one with 3.5 (2.6 against 2.8 ms per call).
    const int fullRows = n / 8, rest = n - 8 * fullRows;
    const bool rowGroups = fullRows >= 1 && !in.even;
    const bool restGroup = rowGroups && rest >= kBatchGroupMin;                // an incomplete row large enough to be a group of its own (else it joins the last group)
    // (two groups while a frame-rate caller is alive in the process)
    const int gWant = std::min(in.envGroups > 0 ? in.envGroups : (in.latencyAlive ? 2 : kBatchGroups), P.nThreads);
    const int G = P.G = std::max(1, rowGroups ? std::min(gWant, fullRows + (restGroup ? 1 : 0)) : std::min(gWant, n / kBatchGroupMin));
    P.gStart.assign(G + 1, n);
    for (int g = 0; g < G; g++) {
        if (!rowGroups) P.gStart[g] = (int)((long long)n * g / G);
        else if (restGroup && G > 1) P.gStart[g] = g == G - 1 ? 8 * fullRows : 8 * (int)((long long)fullRows * g / (G - 1));
        else P.gStart[g] = 8 * (int)((long long)fullRows * g / G);
    }
}

}  // namespace lm
}  // namespace eao
