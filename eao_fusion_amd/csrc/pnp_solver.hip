// pnp_solver.hip -- PnPsolver (reference src/PnPsolver.cc, include/PnPsolver.h): the EPnP RANSAC of Tracking::Relocalization (src/Tracking.cc:2786-2940).
//
// One call is one PnPsolver::iterate (:165-258): one upload, four kernels on the calling thread's latency-class stream, one wait, one download.
//   k_pnp_hypotheses  grid (hypothesis, problem), one wavefront each: compute_pose (:477-525) over the sampled set, CheckInliers (:308-339) with the lanes striding
//                     over all N correspondences, counts by __ballot / __popcll, flags as 64-bit words.
//   k_pnp_scan        one workgroup per problem, integers only: the records -- hypotheses with mnInliersi >= min_inliers and mnInliersi > mnBestInliers, the
//                     best being the running value (:209-224; strict >).
//   k_pnp_refine      grid (slot, problem), one wavefront each: Refine (:260-305) of slot 0 = the set the state carries in, slot r = the chunk's r-th record.
//                     Upstream calls Refine on mvbBestInliers at EVERY hypothesis that passes the >= gate; Refine is deterministic and that set changes only at
//                     a record, so one evaluation per set gives the same verdicts.  pnp_internal.h keeps every sum inside one lane in index order (upstream's
//                     order): no atomics, no tree, bytes independent of the launch -- so one wavefront per record does what a workgroup would.
//   k_pnp_finish      the sequential rule over counts and verdicts, the new state, the flags of what returns.
// The arithmetic and its two deviations from upstream: pnp_internal.h, include/eao_fusion.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnp_internal.h"

using namespace eao;

namespace {

constexpr int kWave = 64;
constexpr int kKernels = 4;

struct HypOut {
    double R[9], t[3], rep[3];
    int choice, inliers;
};
struct RecOut {
    double R[9], t[3];
    int inliers, ok;
};
struct Out {
    int iterations, best_inliers;
    float best_Tcw[16];
    int best_changed, returned, refined, n_inliers, no_more, n_rec;      // n_rec: records of the chunk (slots 1 .. n_rec); k_pnp_finish trims it to those the call reached
    float Tcw[16];
};

// one problem on the device (all arrays device pointers)
struct Rec {
    int n, n_hyp, min_set, min_inliers, max_its, words, has_carried, iterations, best_inliers, pad;
    float best_Tcw[16];
    double fu, fv, uc, vc;
    const float* p3d;                        // n*3
    const float* p2d;                        // n*2
    const float* max_error;                  // n: mvMaxError
    const int* sets;                         // n_hyp*min_set
    const unsigned long long* carried;       // words: the state's best_inlier
    HypOut* hyp;                             // n_hyp
    unsigned long long* hyp_mask;            // n_hyp*words
    RecOut* rec;                             // n_hyp+1 slots
    unsigned long long* rec_mask;            // (n_hyp+1)*words
    int* rec_hyp;                            // n_hyp+1: the hypothesis of a slot (slot 0: -1)
    double* work;                            // (n_hyp+1) slots of 8 n doubles: alphas, pcs, tmp
    int* work_idx;                           // (n_hyp+1) slots of n ints: Refine's vIndices
    Out* out;
    unsigned char* inlier;                   // n
    unsigned char* best_inlier;              // n
};

// CheckInliers over all correspondences by the lanes of one wave; returns mnInliersi to every lane
__device__ inline int check_inliers(const Rec& P, const double* R, const double* t, unsigned long long* mask, int lane) {
    int count = 0;
    for (int base = 0; base < P.n; base += kWave) {
        const int i = base + lane;
        bool in = false;
        if (i < P.n) in = pnp::is_inlier(R, t, P.p3d + 3 * i, P.p2d + 2 * i, P.fu, P.fv, P.uc, P.vc, P.max_error[i]);
        const unsigned long long m = __ballot(in);
        if (lane == 0) mask[base / kWave] = m;
        count += __popcll(m);
    }
    return count;
}

__global__ __launch_bounds__(kWave) void k_pnp_hypotheses(const Rec* __restrict__ W) {
    const Rec& P = W[blockIdx.y];
    const int h = blockIdx.x, lane = threadIdx.x;
    if (h >= P.n_hyp) return;      // (uniform over the wave)
    __shared__ pnp::Ws ws;
    __shared__ double lists[8 * pnp::kMinSetHi];
    pnp::Pts L;
    L.p3d = P.p3d; L.p2d = P.p2d; L.idx = P.sets + (size_t)h * P.min_set; L.n = P.min_set;
    L.fu = P.fu; L.fv = P.fv; L.uc = P.uc; L.vc = P.vc;
    L.alphas = lists; L.pcs = lists + 4 * pnp::kMinSetHi; L.tmp = lists + 7 * pnp::kMinSetHi;
    pnp::compute_pose(ws, L, lane);
    const int count = check_inliers(P, ws.R, ws.t, P.hyp_mask + (size_t)h * P.words, lane);
    if (lane == 0) {
        HypOut& o = P.hyp[h];
        for (int k = 0; k < 9; k++) o.R[k] = ws.R[k];
        for (int k = 0; k < 3; k++) { o.t[k] = ws.t[k]; o.rep[k] = ws.rep[k + 1]; }
        o.choice = ws.choice;
        o.inliers = count;
    }
}

__global__ __launch_bounds__(kWave) void k_pnp_scan(const Rec* __restrict__ W) {
    const Rec& P = W[blockIdx.x];
    if (threadIdx.x != 0) return;
    int n_rec = 0;
    P.rec_hyp[0] = -1;
    if (P.n >= P.min_inliers) {
        int best = P.best_inliers;
        for (int k = 0; k < P.n_hyp; k++) {
            const int c = P.hyp[k].inliers;
            if (c >= P.min_inliers && c > best) {
                best = c;
                P.rec_hyp[++n_rec] = k;
            }
        }
    }
    P.out->n_rec = n_rec;
}

__global__ __launch_bounds__(kWave) void k_pnp_refine(const Rec* __restrict__ W) {
    const Rec& P = W[blockIdx.y];
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot > P.n_hyp) return;
    if (slot == 0 ? !P.has_carried : slot > P.out->n_rec) return;      // (uniform over the wave)
    const unsigned long long* set = slot == 0 ? P.carried : P.hyp_mask + (size_t)P.rec_hyp[slot] * P.words;
    __shared__ pnp::Ws ws;
    __shared__ int sh_n;
    int* idx = P.work_idx + (size_t)slot * P.n;
    if (lane == 0) {      // vIndices (:262-271)
        int m = 0;
        for (int i = 0; i < P.n; i++)
            if ((set[i >> 6] >> (i & 63)) & 1ull) idx[m++] = i;
        sh_n = m;
    }
    wave_sync();
    pnp::Pts L;
    L.p3d = P.p3d; L.p2d = P.p2d; L.idx = idx; L.n = sh_n;
    L.fu = P.fu; L.fv = P.fv; L.uc = P.uc; L.vc = P.vc;
    double* work = P.work + (size_t)slot * 8 * P.n;
    L.alphas = work; L.pcs = work + 4 * (size_t)P.n; L.tmp = work + 7 * (size_t)P.n;
    pnp::compute_pose(ws, L, lane);
    const int count = check_inliers(P, ws.R, ws.t, P.rec_mask + (size_t)slot * P.words, lane);
    if (lane == 0) {
        RecOut& o = P.rec[slot];
        for (int k = 0; k < 9; k++) o.R[k] = ws.R[k];
        for (int k = 0; k < 3; k++) o.t[k] = ws.t[k];
        o.inliers = count;
        o.ok = count > P.min_inliers ? 1 : 0;      // (:292, strict)
    }
}

// Rcw.convertTo(CV_32F) into an eye(4, 4) (:217-223, :294-300)
__device__ inline void pose_to_float(const double* R, const double* t, float* T) {
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[3 * i + j];
        T[4 * i + 3] = (float)t[i];
        T[12 + i] = 0.f;
    }
    T[15] = 1.f;
}

__global__ __launch_bounds__(kWave) void k_pnp_finish(const Rec* __restrict__ W) {
    const Rec& P = W[blockIdx.x];
    __shared__ int sh_ret_slot, sh_best_hyp, sh_returned, sh_refined;
    if (threadIdx.x == 0) {
        Out o = *P.out;      // (n_rec is k_pnp_scan's)
        o.iterations = P.iterations; o.best_inliers = P.best_inliers;
        for (int k = 0; k < 16; k++) { o.best_Tcw[k] = P.best_Tcw[k]; o.Tcw[k] = 0.f; }
        o.best_changed = 0; o.returned = -1; o.refined = 0; o.n_inliers = 0; o.no_more = 0;
        int ret_slot = -1, best_hyp = -1;
        if (P.n < P.min_inliers) {
            o.no_more = 1;      // (:173-177)
        } else {
            int cur = P.has_carried ? 0 : -1, next = 1;
            for (int k = 0; k < P.n_hyp; k++) {
                o.iterations++;
                const int c = P.hyp[k].inliers;
                if (c >= P.min_inliers) {
                    if (next <= o.n_rec && P.rec_hyp[next] == k) {
                        cur = next++;
                        o.best_inliers = c;
                        best_hyp = k;
                    }
                    if (cur >= 0 && P.rec[cur].ok) {
                        o.returned = k; o.refined = 1;
                        ret_slot = cur;
                        break;
                    }
                }
            }
            o.n_rec = next - 1;      // records past the hypothesis that ended the call leave no trace
            if (best_hyp >= 0) {
                pose_to_float(P.hyp[best_hyp].R, P.hyp[best_hyp].t, o.best_Tcw);
                o.best_changed = 1;
            }
            if (o.returned >= 0) {
                o.n_inliers = P.rec[ret_slot].inliers;
                pose_to_float(P.rec[ret_slot].R, P.rec[ret_slot].t, o.Tcw);
            } else if (o.iterations >= P.max_its) {      // (:241-255)
                o.no_more = 1;
                if (o.best_inliers >= P.min_inliers) {
                    o.returned = best_hyp >= 0 ? best_hyp : P.n_hyp;
                    o.n_inliers = o.best_inliers;
                    for (int k = 0; k < 16; k++) o.Tcw[k] = o.best_Tcw[k];
                }
            }
        }
        *P.out = o;
        sh_ret_slot = ret_slot; sh_best_hyp = best_hyp; sh_returned = o.returned; sh_refined = o.refined;
    }
    __syncthreads();
    const unsigned long long* best = sh_best_hyp >= 0 ? P.hyp_mask + (size_t)sh_best_hyp * P.words : P.carried;
    const unsigned long long* ret = sh_returned < 0 ? nullptr : (sh_refined ? P.rec_mask + (size_t)sh_ret_slot * P.words : best);
    for (int i = threadIdx.x; i < P.n; i += kWave) {
        P.best_inlier[i] = (unsigned char)((best[i >> 6] >> (i & 63)) & 1ull);
        P.inlier[i] = ret ? (unsigned char)((ret[i >> 6] >> (i & 63)) & 1ull) : 0;
    }
}

// ---------------------------------------------------------------------- host side
struct PnpCtx : ThreadStream {
    DevBuf<unsigned char> dev;
    std::vector<unsigned char> host;
    KernelClock<kKernels> clock;      // EAO_PNP_EVENTS=1 (tools/bench_pnp_solver.py)
};
thread_local PnpCtx g_pnp;

struct Call {
    const eao_pnp_solver_problem* p;
    int min_inliers, max_its, min_set;
    eao_pnp_solver_state* state;
    const int32_t* sets;
    int n_hyp;
    eao_pnp_solver_result* r;
    int n_eval;      // 0 when n < min_inliers
    size_t offIn, offCarried, offHyp, offHypMask, offRec, offRecMask, offRecHyp, offInl, offBest, offWork, offIdx;
};

eao_status check_call(Call& c) {
    EAO_REQUIRE(c.p && c.state && c.r, "null argument");
    const eao_pnp_solver_problem& p = *c.p;
    EAO_REQUIRE(p.n >= 0, "bad problem: n = %d", p.n);
    EAO_REQUIRE(c.min_set >= pnp::kMinSetLo && c.min_set <= pnp::kMinSetHi, "bad call: min_set = %d (%d .. %d)", c.min_set, pnp::kMinSetLo, pnp::kMinSetHi);
    EAO_REQUIRE(c.n_hyp >= 0 && c.n_hyp <= 65534 && c.max_its >= 0 && c.min_inliers >= 0, "bad call: n_hyp %d, max_its %d, min_inliers %d", c.n_hyp, c.max_its, c.min_inliers);
    EAO_REQUIRE(p.n == 0 || (p.p3d_w && p.p2d && p.sigma2), "bad problem: missing arrays");
    EAO_REQUIRE(std::isfinite(p.fx) && std::isfinite(p.fy) && std::isfinite(p.cx) && std::isfinite(p.cy) && std::isfinite(p.th2), "bad problem: non-finite intrinsic or th2");
    for (size_t i = 0; i < (size_t)3 * p.n; i++) EAO_REQUIRE(std::isfinite(p.p3d_w[i]), "bad problem: point %zu is not finite", i / 3);
    for (size_t i = 0; i < (size_t)2 * p.n; i++) EAO_REQUIRE(std::isfinite(p.p2d[i]), "bad problem: observation %zu is not finite", i / 2);
    for (int i = 0; i < p.n; i++) EAO_REQUIRE(std::isfinite(p.sigma2[i]), "bad problem: sigma2 of correspondence %d is not finite", i);
    EAO_REQUIRE(c.state->iterations >= 0 && c.state->best_inliers >= 0, "bad state: iterations %d, best_inliers %d", c.state->iterations, c.state->best_inliers);
    for (int k = 0; k < 16; k++) EAO_REQUIRE(std::isfinite(c.state->best_Tcw[k]), "bad state: best_Tcw is not finite");
    c.n_eval = 0;
    if (p.n < c.min_inliers) return EAO_OK;      // iterate returns before it draws (:173-177): neither the sets nor the state are read
    EAO_REQUIRE(p.n >= c.min_set, "bad call: n = %d < min_set = %d", p.n, c.min_set);
    EAO_REQUIRE(c.state->best_inlier && c.r->inlier, "bad call: state->best_inlier and result->inlier are written");
    EAO_REQUIRE(c.n_hyp == 0 || c.sets, "bad call: sets missing");
    for (size_t k = 0; k < (size_t)c.n_hyp * c.min_set; k++)
        EAO_REQUIRE(c.sets[k] >= 0 && c.sets[k] < p.n, "bad call: set index %d at %zu, n = %d", c.sets[k], k, p.n);
    int set = 0;
    for (int i = 0; i < p.n; i++) set += c.state->best_inlier[i] ? 1 : 0;
    EAO_REQUIRE(set == c.state->best_inliers, "bad state: %d flags set in best_inlier, best_inliers = %d", set, c.state->best_inliers);
    c.n_eval = c.n_hyp;
    return EAO_OK;
}

eao_status run_solver(std::vector<Call>& calls) {
    const int nb = (int)calls.size();
    for (Call& c : calls) {
        eao_status st = check_call(c);
        if (st) return st;
    }
    PnpCtx& ctx = g_pnp;
    eao_status st = ctx.ready(StreamClass::Latency);      // Tracking's thread waits for the call
    if (st) return st;
    // layout: [records][per problem: 6 n floats, the sets, the carried mask] | [Out][per problem: inlier n, best_inlier n, HypOut, masks, RecOut, masks, rec_hyp] | [work]
    size_t off = align256(sizeof(Rec) * nb);
    int maxEval = 0;
    for (Call& c : calls) {
        const size_t n = (size_t)c.p->n, words = (n + 63) / 64;
        c.offIn = off;
        off = align256(off + n * 6 * sizeof(float) + (size_t)c.n_eval * c.min_set * sizeof(int));
        c.offCarried = off;
        off = align256(off + words * 8);
        maxEval = std::max(maxEval, c.n_eval);
    }
    const size_t inEnd = off, offOut = off;
    off = align256(off + sizeof(Out) * nb);
    for (Call& c : calls) {
        const size_t n = (size_t)c.p->n, words = (n + 63) / 64, slots = (size_t)c.n_eval + 1;
        c.offInl = off; off += n;
        c.offBest = off; off = align256(off + n);
        c.offHyp = off; off = align256(off + sizeof(HypOut) * c.n_eval);
        c.offHypMask = off; off = align256(off + 8 * words * c.n_eval);
        c.offRec = off; off = align256(off + sizeof(RecOut) * slots);
        c.offRecMask = off; off = align256(off + 8 * words * slots);
        c.offRecHyp = off; off = align256(off + sizeof(int) * slots);
    }
    const size_t outEnd = off;
    for (Call& c : calls) {
        const size_t n = (size_t)c.p->n, slots = (size_t)c.n_eval + 1;
        c.offWork = off; off = align256(off + 8 * n * sizeof(double) * slots);
        c.offIdx = off; off = align256(off + n * sizeof(int) * slots);
    }
    const size_t total = std::max<size_t>(off, 256);
    if ((st = ctx.dev.reserve(total))) return st;
    if (ctx.host.size() < outEnd) ctx.host.resize(outEnd);
    unsigned char* h = ctx.host.data();
    unsigned char* d = ctx.dev.p;
    Rec* recs = (Rec*)h;
    for (int b = 0; b < nb; b++) {
        const Call& c = calls[b];
        const eao_pnp_solver_problem& p = *c.p;
        const size_t n = (size_t)p.n, words = (n + 63) / 64;
        float* p3d = (float*)(h + c.offIn);
        float* p2d = p3d + 3 * n;
        float* maxe = p2d + 2 * n;
        int* sets = (int*)(maxe + n);
        if (n) {
            std::memcpy(p3d, p.p3d_w, 12 * n);
            std::memcpy(p2d, p.p2d, 8 * n);
        }
        for (size_t i = 0; i < n; i++) maxe[i] = p.sigma2[i] * p.th2;      // mvMaxError (:154-156)
        if (c.n_eval) std::memcpy(sets, c.sets, (size_t)c.n_eval * c.min_set * sizeof(int));
        unsigned long long* carried = (unsigned long long*)(h + c.offCarried);
        for (size_t k = 0; k < words; k++) carried[k] = 0;
        const bool live = p.n >= c.min_inliers;
        if (live)
            for (size_t i = 0; i < n; i++)
                if (c.state->best_inlier[i]) carried[i >> 6] |= 1ull << (i & 63);
        Rec& R = recs[b];
        std::memset(&R, 0, sizeof(R));
        R.n = p.n; R.n_hyp = c.n_eval; R.min_set = c.min_set; R.min_inliers = c.min_inliers; R.max_its = c.max_its; R.words = (int)words;
        R.has_carried = live && c.state->best_inliers > 0;
        R.iterations = c.state->iterations; R.best_inliers = c.state->best_inliers;
        std::memcpy(R.best_Tcw, c.state->best_Tcw, sizeof(R.best_Tcw));
        R.fu = p.fx; R.fv = p.fy; R.uc = p.cx; R.vc = p.cy;      // (:104-107: float -> double)
        R.p3d = (const float*)(d + c.offIn);
        R.p2d = R.p3d + 3 * n;
        R.max_error = R.p2d + 2 * n;
        R.sets = (const int*)(R.max_error + n);
        R.carried = (const unsigned long long*)(d + c.offCarried);
        R.hyp = (HypOut*)(d + c.offHyp);
        R.hyp_mask = (unsigned long long*)(d + c.offHypMask);
        R.rec = (RecOut*)(d + c.offRec);
        R.rec_mask = (unsigned long long*)(d + c.offRecMask);
        R.rec_hyp = (int*)(d + c.offRecHyp);
        R.work = (double*)(d + c.offWork);
        R.work_idx = (int*)(d + c.offIdx);
        R.out = (Out*)(d + offOut) + b;
        R.inlier = d + c.offInl;
        R.best_inlier = d + c.offBest;
    }
    static const bool envEvents = getenv("EAO_PNP_EVENTS") && atoi(getenv("EAO_PNP_EVENTS"));
    if (envEvents != ctx.clock.armed()) ctx.clock.arm(envEvents);
    const Rec* dW = (const Rec*)d;
    Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    EAO_HIP(hipMemsetAsync(d + offOut, 0, outEnd - offOut, ctx.stream));      // slots and hypotheses no kernel writes read as zero
    ctx.clock.mark(0, ctx.stream);
    if (maxEval > 0) hipLaunchKernelGGL(k_pnp_hypotheses, dim3(maxEval, nb), dim3(kWave), 0, ctx.stream, dW);
    ctx.clock.mark(1, ctx.stream);
    hipLaunchKernelGGL(k_pnp_scan, dim3(nb), dim3(kWave), 0, ctx.stream, dW);
    ctx.clock.mark(2, ctx.stream);
    hipLaunchKernelGGL(k_pnp_refine, dim3(maxEval + 1, nb), dim3(kWave), 0, ctx.stream, dW);
    ctx.clock.mark(3, ctx.stream);
    hipLaunchKernelGGL(k_pnp_finish, dim3(nb), dim3(kWave), 0, ctx.stream, dW);
    ctx.clock.mark(4, ctx.stream);
    EAO_HIP(hipGetLastError());
    EAO_HIP(hipMemcpyAsync(h + offOut, d + offOut, outEnd - offOut, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(Drain::Latency));
    ctx.clock.collect();
    const Out* outs = (const Out*)(h + offOut);
    for (int b = 0; b < nb; b++) {
        const Call& c = calls[b];
        const Out& o = outs[b];
        const size_t n = (size_t)c.p->n, words = (n + 63) / 64;
        eao_pnp_solver_result& r = *c.r;
        c.state->iterations = o.iterations; c.state->best_inliers = o.best_inliers;
        std::memcpy(c.state->best_Tcw, o.best_Tcw, sizeof(o.best_Tcw));
        if (o.best_changed) std::memcpy(c.state->best_inlier, h + c.offBest, n);
        r.returned = o.returned; r.refined = o.refined; r.n_inliers = o.n_inliers; r.no_more = o.no_more;
        std::memcpy(r.Tcw, o.Tcw, sizeof(r.Tcw));
        if (o.returned >= 0) std::memcpy(r.inlier, h + c.offInl, n);
        const bool carried = c.p->n >= c.min_inliers && recs[b].has_carried;
        r.n_records = o.n_rec + (carried ? 1 : 0);
        const HypOut* hyp = (const HypOut*)(h + c.offHyp);
        const unsigned long long* hm = (const unsigned long long*)(h + c.offHypMask);
        for (int k = 0; k < c.n_hyp; k++) {
            const bool ev = k < c.n_eval;      // (nothing is evaluated when n < min_inliers)
            const HypOut z = {};
            const HypOut& q = ev ? hyp[k] : z;
            if (r.hyp_R) std::memcpy(r.hyp_R + 9 * (size_t)k, q.R, 72);
            if (r.hyp_t) std::memcpy(r.hyp_t + 3 * (size_t)k, q.t, 24);
            if (r.hyp_rep_err) std::memcpy(r.hyp_rep_err + 3 * (size_t)k, q.rep, 24);
            if (r.hyp_choice) r.hyp_choice[k] = q.choice;
            if (r.hyp_inliers) r.hyp_inliers[k] = q.inliers;
            if (r.hyp_inlier)
                for (size_t i = 0; i < n; i++) r.hyp_inlier[(size_t)k * n + i] = ev ? (unsigned char)((hm[(size_t)k * words + (i >> 6)] >> (i & 63)) & 1ull) : 0;
        }
        const RecOut* rec = (const RecOut*)(h + c.offRec);
        const unsigned long long* rm = (const unsigned long long*)(h + c.offRecMask);
        const int* rh = (const int*)(h + c.offRecHyp);
        for (int k = 0; k <= c.n_hyp; k++) {      // entry k: slot k + (carried ? 0 : 1)
            const int slot = k + (carried ? 0 : 1);
            const bool ev = k < r.n_records;
            const RecOut z = {};
            const RecOut& q = ev ? rec[slot] : z;
            if (r.rec_hyp) r.rec_hyp[k] = ev ? rh[slot] : 0;
            if (r.rec_R) std::memcpy(r.rec_R + 9 * (size_t)k, q.R, 72);
            if (r.rec_t) std::memcpy(r.rec_t + 3 * (size_t)k, q.t, 24);
            if (r.rec_inliers) r.rec_inliers[k] = q.inliers;
            if (r.rec_inlier)
                for (size_t i = 0; i < n; i++) r.rec_inlier[(size_t)k * n + i] = ev ? (unsigned char)((rm[(size_t)slot * words + (i >> 6)] >> (i & 63)) & 1ull) : 0;
        }
    }
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_pnp_solver_iterate(const eao_pnp_solver_problem* problem, int32_t min_inliers, int32_t max_its, int32_t min_set, eao_pnp_solver_state* state,
                                  const int32_t* sets, int32_t n_hyp, eao_pnp_solver_result* result) {
    std::vector<Call> calls(1);
    calls[0] = Call{};
    calls[0].p = problem; calls[0].min_inliers = min_inliers; calls[0].max_its = max_its; calls[0].min_set = min_set;
    calls[0].state = state; calls[0].sets = sets; calls[0].n_hyp = n_hyp; calls[0].r = result;
    return run_solver(calls);
}

eao_status eao_pnp_solver_iterate_batch(int32_t n_problems, const eao_pnp_solver_problem* problems, const int32_t* min_inliers, const int32_t* max_its,
                                        const int32_t* min_set, eao_pnp_solver_state* states, const int32_t* const* sets, const int32_t* n_hyp,
                                        eao_pnp_solver_result* results) {
    EAO_REQUIRE(n_problems >= 0 && (n_problems == 0 || (problems && min_inliers && max_its && min_set && states && sets && n_hyp && results)), "bad batch");
    if (n_problems == 0) return EAO_OK;
    std::vector<Call> calls(n_problems);
    for (int b = 0; b < n_problems; b++) {
        calls[b] = Call{};
        calls[b].p = &problems[b]; calls[b].min_inliers = min_inliers[b]; calls[b].max_its = max_its[b]; calls[b].min_set = min_set[b];
        calls[b].state = &states[b]; calls[b].sets = sets[b]; calls[b].n_hyp = n_hyp[b]; calls[b].r = &results[b];
    }
    return run_solver(calls);
}

eao_status eao_pnp_solver_last_kernel_ms(float* kernel_ms) {
    EAO_REQUIRE(kernel_ms, "null argument");
    return g_pnp.clock.read(kernel_ms, "no measurement on this thread: EAO_PNP_EVENTS=1 and a call of eao_pnp_solver_iterate come first");
}

}  // extern "C"
