// keyframe.hip -- keyframe handles for MI355X (gfx950): upload once, search many.
//
// LocalMapping::CreateNewMapPoints and SearchInNeighbors (reference src/LocalMapping.cc:211-290, 458-520) and LoopClosing hit the SAME keyframes again and
// again -- ten or twenty neighbours per new keyframe, the same neighbours for the next one.  The host-array entry points of csrc/search.hip upload every frame
// with every call, put it into grid order on the host and replay the selection there; on a 1000-keypoint problem three of them were slower than ONE CPU thread
// (VERDICT r4 weak #7).  An eao_keyframe owns what the searches read of a keyframe (or of a Frame that is a search target) in HBM: keypoints, octaves, angles,
// uRight, descriptors, the grid order Frame / KeyFrame::GetFeaturesInArea walks (PosInGrid + counting sort, once), the DBoW2 feature vector, the occupancy
// (GetMapPoint(k) != NULL) and the scale tables.  On top of it:
//   * the vocabulary-node searches -- SearchByBoW (KF, Frame) / (KF, KF), src/ORBmatcher.cc:159-288, 522-655, and SearchForTriangulation, :657-823 with
//     CheckDistEpipolarLine :140-157 -- run WHOLLY on the device: a wavefront per common vocabulary node walks the node's side-1 features in upstream's order,
//     the lanes share the side-2 features (two smallest (distance, position) keys = "first of equal distances wins", the node-local "already matched" set as a
//     per-lane bit mask -- a keypoint lies in ONE node, so upstream's greedy rule never reaches across nodes), a second small launch per problem applies the
//     rotation histogram and writes the match table into mapped host memory: two launches and one synchronisation per call, whatever the number of neighbours;
//   * the search half of Fuse (:825-975, 977-1100) likewise: a wavefront per (target keyframe, map point) projects the point, walks its grid window in the
//     resident grid order and keeps the best gated candidate -- no candidate lists, no host replay (a point's search does not depend on other points');
//   * the list-based searches (loop / relocalisation projection, initialisation, SearchBySim3) keep their host replay (csrc/search.hip) but take the frame from
//     the handle: only the queries travel.
// Results are those of the host-array entry points, entry for entry (tests/test_gpu_search.py runs every case through both and against the CPU restatement).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"
#include "match_internal.h"
#include "search_internal.h"
#include "triangulate_internal.h"

namespace {

constexpr int TH_LOW = refc::TH_LOW, HISTO = refc::HISTO_LENGTH;
constexpr int kMaxProb = 16;      // problems (neighbours / targets) per launch: their records travel in the kernel arguments

struct KfDev {      // what the kernels read of one keyframe: device addresses inside the handle's block
    int n, no, nNodes, nlevels;
    const float* kx; const float* ky; const float* ur; const float* ang; const int* oct; const uint4* desc;
    const int* order; const unsigned short* cellx; const unsigned short* celly; const int* colStart;
    const unsigned char* occ;
    const unsigned* nodeId; const int* nodeStart; const unsigned* index;
    const float* sf; const float* s2; const float* is2;
    float minX, minY, maxX, maxY, invW, invH, logScale;
    int cols, rows;
};

__device__ __forceinline__ int dist256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// Smallest value of the wave, on the VALU's data-parallel primitives: four row_shr steps leave lane 15 of every row of 16 with the row's minimum, row_bcast15 /
// row_bcast31 carry it across the rows into lane 63, one v_readlane hands it to everybody.  (A shuffle butterfly -- six dependent ds_bpermute round trips per
// key, ~150 cycles each -- made every step of the node walk 0.5 us: 976 ticks of 10 ns for 20 features, EAO_DEBUG_STAMPS.)
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    constexpr int kId = (int)0xFFFFFFFFu;      // lanes without a source (row edges, rows outside the mask) read the identity
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(kId, (int)v, 0x111, 0xF, 0xF, false));   // row_shr:1
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(kId, (int)v, 0x112, 0xF, 0xF, false));   // row_shr:2
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(kId, (int)v, 0x114, 0xF, 0xF, false));   // row_shr:4
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(kId, (int)v, 0x118, 0xF, 0xF, false));   // row_shr:8
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(kId, (int)v, 0x142, 0xA, 0xF, false));   // row_bcast15 into rows 1 and 3
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(kId, (int)v, 0x143, 0xC, 0xF, false));   // row_bcast31 into rows 2 and 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// ---------------------------------------------------------------------------------------------------------------- vocabulary-node searches
struct NodeProb { const KfDev* k2; float F[9]; float ex, ey; };
struct NodesArgs {
    KfDev K1;                     // side 1 by value: one dependent load less at the head of every wave
    int nProb, onlyStereo;
    float nnratio;
    const unsigned char* valid1; const unsigned char* valid2;      // BoW: mapped host arrays (gathered once per wave); triangulation: unused
    int2* match;                  // per (problem, side-1 keypoint): {generation stamp, side-2 keypoint}
    int gen, n1;
    NodeProb P[kMaxProb];
    // ONE problem (nProb == 1) whose side 1 has at most kPairCap nodes: side 2 travels by value too and the host has merged the two node-id lists already
    // (pairB[a] = the node of side 2 with the id of side 1's node a, or -1) -- the wave's head loses its chain of dependent loads (struct, node id, six probes)
    long long* dbg;               // EAO_DEBUG_STAMPS=1: shader-clock stamps of the wave that owns side-1 node 0 (diagnostic runs only)
    int single;
    KfDev K2v;
    short pairB[512];
};
constexpr int kPairCap = 512;

// MODE 0: SearchByBoW(KeyFrame*, Frame&), 1: SearchByBoW(KeyFrame*, KeyFrame*), 2: SearchForTriangulation
template <int MODE>
__global__ __launch_bounds__(256) void k_kf_nodes(NodesArgs A) {
    const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6), pb = blockIdx.y;
    const KfDev& K1 = A.K1;
    if (a >= K1.nNodes) return;
    const bool stamp = A.dbg && a == 0 && pb == 0 && lane == 0;
    if (stamp) A.dbg[0] = wall_clock64();
    const NodeProb& PB = A.P[pb];
    KfDev K2;
    int lo;
    if (A.single) {
        lo = A.pairB[a];
        if (lo < 0) return;
        K2 = A.K2v;
    } else {
        K2 = *PB.k2;
        // the node of side 1 in side 2's vector (both ascending: std::map order; upstream's merge walk with lower_bound, :175-262)
        const unsigned id = K1.nodeId[a];
        lo = 0;
        int hi = K2.nNodes;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (K2.nodeId[mid] < id) lo = mid + 1; else hi = mid;
        }
        if (lo >= K2.nNodes || K2.nodeId[lo] != id) return;
    }
    const int s1 = K1.nodeStart[a], c1 = K1.nodeStart[a + 1] - s1, s2 = K2.nodeStart[lo], c2 = K2.nodeStart[lo + 1] - s2;
    if (c1 <= 0 || c2 <= 0) return;
    // side 2, first 64 entries of the node in registers (a node rarely holds more; the rest is read from memory in every round)
    int idx2 = -1, oct2 = 0;
    uint4 f0 = make_uint4(0, 0, 0, 0), f1 = f0;
    float x2 = 0, y2 = 0;
    bool stereo2 = false, skip2 = true;
    auto load2 = [&](int p, int& i2, uint4& g0, uint4& g1, float& xx, float& yy, int& oc, bool& st2) -> bool {      // false: upstream `continue`s at this entry
        i2 = (int)K2.index[s2 + p];
        bool skip;
        if (MODE == 0) skip = false;
        else if (MODE == 1) skip = !A.valid2[i2];
        else skip = K2.occ[i2] || (A.onlyStereo && !(K2.ur[i2] >= 0));
        if (skip) return false;
        g0 = K2.desc[2 * (size_t)i2]; g1 = K2.desc[2 * (size_t)i2 + 1];
        if (MODE == 2) { xx = K2.kx[i2]; yy = K2.ky[i2]; oc = K2.oct[i2]; st2 = K2.ur[i2] >= 0; }
        return true;
    };
    if (stamp) { A.dbg[1] = wall_clock64(); A.dbg[6] = c1; A.dbg[7] = c2; }
    if (lane < c2) skip2 = !load2(lane, idx2, f0, f1, x2, y2, oct2, stereo2);
    if (A.dbg) __builtin_amdgcn_s_waitcnt(0);      // (diagnostic runs: the stamp below then includes the loads' latency)
    if (stamp) { A.dbg[2] = wall_clock64() + (f0.x & 0); }
    unsigned long long taken = 0;      // bit j: list position lane + 64 j of the node's side 2 has been matched (BoW)
    int matched = 0;
    for (int a0 = 0; a0 < c1; a0 += 64) {
        // side 1, 64 entries at a time: lane aa loads entry a0 + aa -- index, "does upstream look at it" (a ballot), descriptor, and for the triangulation its
        // coordinates -- all 64 in flight at once; the walk below fetches them lane by lane with v_readlane (the walk's counter is wave-uniform).  Loading each
        // descriptor when its turn came made every step of the walk a cache miss: 19.9 us per launch on the 1000-keypoint scene.
        int myIdx1 = 0;
        bool ok1 = false;
        uint4 m0 = make_uint4(0, 0, 0, 0), m1d = m0;
        float mx1 = 0, my1 = 0, mur1 = -1;
        if (a0 + lane < c1) {
            myIdx1 = (int)K1.index[s1 + a0 + lane];
            if (MODE == 2) { mur1 = K1.ur[myIdx1]; ok1 = !(K1.occ[myIdx1] || (A.onlyStereo && !(mur1 >= 0))); }
            else ok1 = A.valid1[myIdx1] != 0;
            if (ok1) {
                m0 = K1.desc[2 * (size_t)myIdx1]; m1d = K1.desc[2 * (size_t)myIdx1 + 1];
                if (MODE == 2) { mx1 = K1.kx[myIdx1]; my1 = K1.ky[myIdx1]; }
            }
        }
        const unsigned long long m1 = __ballot(ok1);
        if (A.dbg) __builtin_amdgcn_s_waitcnt(0);
        if (stamp && a0 == 0) A.dbg[3] = wall_clock64() + (m0.x & 0);
        const int cnt = min(64, c1 - a0);
        for (int aa = 0; aa < cnt; aa++) {
            if (!((m1 >> aa) & 1)) continue;
            const int idx1 = __builtin_amdgcn_readlane(myIdx1, aa);
            uint4 d0, d1;
            d0.x = __builtin_amdgcn_readlane(m0.x, aa); d0.y = __builtin_amdgcn_readlane(m0.y, aa); d0.z = __builtin_amdgcn_readlane(m0.z, aa); d0.w = __builtin_amdgcn_readlane(m0.w, aa);
            d1.x = __builtin_amdgcn_readlane(m1d.x, aa); d1.y = __builtin_amdgcn_readlane(m1d.y, aa); d1.z = __builtin_amdgcn_readlane(m1d.z, aa); d1.w = __builtin_amdgcn_readlane(m1d.w, aa);
            float la = 0, lb = 0, lc = 0, den = 0;
            bool stereo1 = false;
            if (MODE == 2) {      // the epipolar line of keypoint 1 in image 2 (CheckDistEpipolarLine, :140-157)
                const float x1 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(mx1), aa)), y1 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my1), aa));
                stereo1 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(mur1), aa)) >= 0;
                la = x1 * PB.F[0] + y1 * PB.F[3] + PB.F[6];
                lb = x1 * PB.F[1] + y1 * PB.F[4] + PB.F[7];
                lc = x1 * PB.F[2] + y1 * PB.F[5] + PB.F[8];
                den = la * la + lb * lb;
            }
            unsigned k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;
            auto offer = [&](int p, const uint4& g0, const uint4& g1, float xx, float yy, int oc, bool st2) {
                const unsigned d = (unsigned)dist256(d0, d1, g0, g1);
                unsigned key;
                if (MODE == 2) {
                    // upstream (:722-757): d <= TH_LOW and d <= the best so far, then the epipole and epipolar-line gates, then "best = this one" -- i.e. the smallest
                    // distance among the gated candidates, the LAST of equal ones: position enters the key inverted
                    if (d > (unsigned)TH_LOW) return;
                    if (!stereo1 && !st2) {
                        const float dex = PB.ex - xx, dey = PB.ey - yy;
                        if (dex * dex + dey * dey < 100 * K2.sf[oc]) return;
                    }
                    const float num = la * xx + lb * yy + lc;
                    if (den == 0) return;
                    const float dsqr = num * num / den;
                    if (!(dsqr < refc::EPIPOLAR_CHI2 * K2.s2[oc])) return;
                    key = (d << 16) | (unsigned)(0xFFFF - p);
                } else {
                    key = (d << 16) | (unsigned)p;      // first of equal distances wins (strict '<' upstream, :206-215)
                }
                if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
            };
            if (!skip2 && !(taken & 1)) offer(lane, f0, f1, x2, y2, oct2, stereo2);
            for (int p = lane + 64, j = 1; p < c2; p += 64, j++) {
                if ((taken >> j) & 1) continue;
                int i2, oc = 0; uint4 g0, g1; float xx = 0, yy = 0; bool st2 = false;
                if (!load2(p, i2, g0, g1, xx, yy, oc, st2)) continue;
                offer(p, g0, g1, xx, yy, oc, st2);
            }
            // the wave's two smallest keys (all distinct: the position is part of the key): the minimum, then the minimum again with its owner's runner-up in its place
            {
                const unsigned b1 = wave_min_u32(k1);
                if (b1 == 0xFFFFFFFFu) continue;
                const unsigned b2 = (MODE == 2) ? 0xFFFFFFFFu : wave_min_u32(k1 == b1 ? k2 : k1);      // (the triangulation has no ratio test)
                k1 = b1; k2 = b2;
            }
            const int best1 = (int)(k1 >> 16), best2 = k2 == 0xFFFFFFFFu ? 256 : (int)(k2 >> 16);
            bool accept;
            int p;
            if (MODE == 2) { accept = true; p = 0xFFFF - (int)(k1 & 0xFFFFu); }
            else {
                p = (int)(k1 & 0xFFFFu);
                accept = (MODE == 0 ? best1 <= TH_LOW : best1 < TH_LOW) && (float)best1 < A.nnratio * (float)best2;
            }
            if (!accept) continue;
            if (MODE != 2 && (p & 63) == lane) taken |= 1ull << (p >> 6);      // (triangulation never consumes side 2: upstream does not set vbMatched2)
            // (the winner's keypoint index sits in lane p's register for the node's first 64 entries: a load here would stall every matching step of the walk
            //  for a cache round trip -- 0.45 us per step, EAO_DEBUG_STAMPS)
            const int win = p < 64 ? __builtin_amdgcn_readlane(idx2, p) : (int)K2.index[s2 + p];
            if (lane == 0) {
                A.match[(size_t)pb * A.n1 + idx1] = make_int2(A.gen, win);
                matched++;
            }
        }
    }
    (void)matched;
    if (stamp) A.dbg[4] = wall_clock64();
}

// rotation histogram + ComputeThreeMaxima (src/ORBmatcher.cc:1603-1644) over a problem's matches, the table and its count into mapped host memory
struct FinishArgs {
    const float* ang1;
    int nProb, n1, gen, checkOrientation;
    const int2* match;
    int* out;        // mapped host: nProb x n1
    int* nm;         // mapped host: nProb
    // the call's LAST finish launch publishes a done word the host polls (as the tracker's chain does, csrc/lm.hip pose_publish): every workgroup fences its
    // stores to host memory at system scope, reads one of its own words back over PCIe (a read pushes posted writes) and takes a ticket; the last one stores
    // the word.
    int* ticket; int ticketLast; int* done; int doneSeq;
    const float* ang2[kMaxProb];
};
__global__ __launch_bounds__(256) void k_kf_finish(FinishArgs A) {
    __shared__ int s_hist[HISTO], s_keep[3], s_nm;
    const int pb = blockIdx.x, t = threadIdx.x;
    const float* ang1 = A.ang1;
    const float* ang2 = A.ang2[pb];
    const float factor = 1.0f / HISTO;
    if (t < HISTO) s_hist[t] = 0;
    if (t == 0) { s_nm = 0; s_keep[0] = s_keep[1] = s_keep[2] = -1; }
    __syncthreads();
    const int2* M = A.match + (size_t)pb * A.n1;
    auto bin_of = [&](int i, int m) {
        float rot = ang1[i] - ang2[m];
        if (rot < 0.0) rot += 360.0f;
        int b = (int)roundf(rot * factor);
        if (b == HISTO) b = 0;
        return b;
    };
    // up to kFinPer x 256 keypoints: a thread's matches and their bins stay in registers between the vote and the verdict (one pass over memory)
    constexpr int kFinPer = 8;
    int mm[kFinPer], bb[kFinPer];
    const bool inRegs = A.n1 <= kFinPer * 256;
#pragma unroll
    for (int u = 0; u < kFinPer; u++) {
        const int i = t + 256 * u;
        mm[u] = -1; bb[u] = -1;
        if (inRegs && i < A.n1) {
            const int2 e = M[i];
            if (e.x == A.gen) {
                mm[u] = e.y;
                if (A.checkOrientation) { bb[u] = bin_of(i, e.y); if (bb[u] >= 0 && bb[u] < HISTO) atomicAdd(&s_hist[bb[u]], 1); }
            }
        }
    }
    if (A.checkOrientation) {
        if (!inRegs)
            for (int i = t; i < A.n1; i += 256) {
                const int2 e = M[i];
                if (e.x != A.gen) continue;
                const int b = bin_of(i, e.y);
                if (b >= 0 && b < HISTO) atomicAdd(&s_hist[b], 1);
            }
        __syncthreads();
        if (t == 0) {
            int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
            for (int i = 0; i < HISTO; i++) {
                const int s = s_hist[i];
                if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
                else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
                else if (s > max3) { max3 = s; ind3 = i; }
            }
            if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
            else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
            s_keep[0] = ind1; s_keep[1] = ind2; s_keep[2] = ind3;
        }
        __syncthreads();
    }
    int kept = 0;
    if (inRegs) {
#pragma unroll
        for (int u = 0; u < kFinPer; u++) {
            const int i = t + 256 * u;
            if (i >= A.n1) continue;
            int m = mm[u];
            if (m >= 0 && A.checkOrientation && bb[u] != s_keep[0] && bb[u] != s_keep[1] && bb[u] != s_keep[2]) m = -1;
            A.out[(size_t)pb * A.n1 + i] = m;
            kept += m >= 0;
        }
    } else {
        for (int i = t; i < A.n1; i += 256) {
            const int2 e = M[i];
            int m = e.x == A.gen ? e.y : -1;
            if (m >= 0 && A.checkOrientation) {
                const int b = bin_of(i, m);
                if (b != s_keep[0] && b != s_keep[1] && b != s_keep[2]) m = -1;
            }
            A.out[(size_t)pb * A.n1 + i] = m;
            kept += m >= 0;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) kept += __shfl_xor(kept, o);
    if ((t & 63) == 0 && kept) atomicAdd(&s_nm, kept);
    __syncthreads();
    if (t == 0) A.nm[pb] = s_nm;
    __threadfence_system();
    __syncthreads();
    if (t == 0) {
        const int back = __hip_atomic_load(&A.nm[pb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // (cannot pass this workgroup's posted writes)
        const int tk = atomicAdd(A.ticket, 1);
        if (tk == A.ticketLast && back == s_nm) __hip_atomic_store(A.done, A.doneSeq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---------------------------------------------------------------------------------------------------------------- Fuse
struct PtsDev { int n; const unsigned char* active; const float* Xw; const float* normal; const float* dmin; const float* dmax; const float* draw; const uint4* desc; };
struct FuseTarget { const KfDev* k; float R[9], t[3], Ow[3]; };
struct FuseArgs {
    int nKf, useSim3;
    float fx, fy, cx, cy, bf, th;
    PtsDev P;
    int* out;            // mapped host: nKf x P.n
    FuseTarget T[kMaxProb];
};
// one wavefront per (target keyframe, map point): upstream's loop body (:851-971 / :1003-1096) up to "bestDist <= TH_LOW"
__global__ __launch_bounds__(256) void k_kf_fuse(FuseArgs A) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6), f = blockIdx.y;
    if (i >= A.P.n) return;
    int* out = A.out + (size_t)f * A.P.n + i;
    const FuseTarget& T = A.T[f];
    const KfDev K = *T.k;
    if (!A.P.active[i]) { if (lane == 0) *out = -1; return; }
    // the projection with the range / viewing-angle tests (cv::Mat float semantics: A x + b accumulates in double and rounds once; cv::norm and Mat::dot
    // accumulate in double) -- the same statements as shoot() in csrc/search.hip
    const float X0 = A.P.Xw[3 * i], X1 = A.P.Xw[3 * i + 1], X2 = A.P.Xw[3 * i + 2];
    float pc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double s = (double)T.R[r * 3] * (double)X0 + (double)T.R[r * 3 + 1] * (double)X1 + (double)T.R[r * 3 + 2] * (double)X2;
        pc[r] = (float)(1.0 * s + (double)T.t[r]);
    }
    bool ok = !(pc[2] < 0.0f);
    float invz = 0, u = 0, v = 0;
    int level = 0;
    if (ok) {
        invz = A.useSim3 ? (float)(1.0 / pc[2]) : 1 / pc[2];
        const float x = pc[0] * invz, y = pc[1] * invz;
        u = A.fx * x + A.cx; v = A.fy * y + A.cy;
        ok = u >= K.minX && u < K.maxX && v >= K.minY && v < K.maxY;      // KeyFrame::IsInImage
    }
    if (ok) {
        const float PO0 = X0 - T.Ow[0], PO1 = X1 - T.Ow[1], PO2 = X2 - T.Ow[2];
        const float dist = (float)sqrt((double)PO0 * PO0 + (double)PO1 * PO1 + (double)PO2 * PO2);
        if (dist < A.P.dmin[i] || dist > A.P.dmax[i]) ok = false;
        if (ok) {
            const double dot = (double)PO0 * A.P.normal[3 * i] + (double)PO1 * A.P.normal[3 * i + 1] + (double)PO2 * A.P.normal[3 * i + 2];
            if (dot < 0.5 * dist) ok = false;
        }
        if (ok) {      // MapPoint::PredictScale (src/MapPoint.cc:385-394): float log, float division, ceil -- the float logarithm as in frustum_point (chain_internal.h)
            const float ratio = A.P.draw[i] / dist;
            const float lg = (float)log((double)ratio);
            level = (int)ceilf(lg / K.logScale);
            ok = level >= 0 && level < K.nlevels;
        }
    }
    if (!ok) { if (lane == 0) *out = -1; return; }
    const float r = A.th * K.sf[level];
    // KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:608-647), the float expressions as written upstream
    const int x0 = max(0, (int)floorf((u - K.minX - r) * K.invW));
    const int x1 = min(K.cols - 1, (int)ceilf((u - K.minX + r) * K.invW));
    const int y0 = max(0, (int)floorf((v - K.minY - r) * K.invH));
    const int y1 = min(K.rows - 1, (int)ceilf((v - K.minY + r) * K.invH));
    if (x0 >= K.cols || x1 < 0 || y0 >= K.rows || y1 < 0) { if (lane == 0) *out = -1; return; }
    const uint4 d0 = A.P.desc[2 * (size_t)i], d1 = A.P.desc[2 * (size_t)i + 1];
    const float ur = u - A.bf * invz;
    const int oBeg = K.colStart[x0], oEnd = min(K.colStart[x1 + 1], K.no);
    unsigned best = 0xFFFFFFFFu;
    for (int o0 = oBeg; o0 < oEnd; o0 += 64) {
        const int o = o0 + lane;
        if (o >= oEnd) continue;
        const int cx = K.cellx[o], cy = K.celly[o];
        if (cx < x0 || cx > x1 || cy < y0 || cy > y1) continue;
        const int k = K.order[o];
        const float kx = K.kx[k], ky = K.ky[k];
        if (!(fabsf(kx - u) < r && fabsf(ky - v) < r)) continue;
        const int kl = K.oct[k];
        if (kl < level - 1 || kl > level) continue;
        if (!A.useSim3) {      // reprojection gates of the pose overload (:915-941)
            const float exx = u - kx, eyy = v - ky;
            const float kur = K.ur[k];
            if (kur >= 0) {
                const float er = ur - kur;
                const float e2 = exx * exx + eyy * eyy + er * er;
                if (e2 * K.is2[kl] > refc::FUSE_CHI2_STEREO) continue;
            } else {
                const float e2 = exx * exx + eyy * eyy;
                if (e2 * K.is2[kl] > refc::FUSE_CHI2_MONO) continue;
            }
        }
        const unsigned d = (unsigned)dist256(d0, d1, K.desc[2 * (size_t)k], K.desc[2 * (size_t)k + 1]);
        best = min(best, (d << 16) | (unsigned)o);      // candidates come in grid order: the first of equal distances wins (strict '<' upstream)
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = min(best, (unsigned)__shfl_xor(best, o));
    if (lane == 0) *out = (best != 0xFFFFFFFFu && (int)(best >> 16) <= TH_LOW) ? K.order[best & 0xFFFFu] : -1;
}

// 16 bytes per lane from mapped pinned host memory into HBM, on the searches' own stream (an SDMA copy in front of a kernel costs a cross-engine hand-over)
__global__ __launch_bounds__(256) void k_kf_upload(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

using PinBuf = eao::PinBuf<hipHostMallocMapped>;   // kernels read and write it in place through .d
struct Ctx : eao::ThreadStream {   // per host thread, grow-only
    PinBuf in, out;
    eao::DevBuf<int2> match;
    eao::DevBuf<unsigned char> dev;
    eao::DevBuf<int> ticket;       // finish workgroups of all calls so far take their tickets here (a device counter that only grows)
    int ticketNext = 0;
    PinBuf doneWord;
    PinBuf tri;                    // eao_kf_create_new_map_points: [verdicts | points] in mapped host memory
    eao::KernelClock<1> triClock;  // EAO_TRI_EVENTS=1: around the triangulation launches (tools/bench_triangulation.py)
    eao::DevBuf<long long> dbg;
    int seq = 0;
    int gen = 0;
};
thread_local Ctx g_kctx;

using eao::align256;

}  // namespace

struct eao_keyframe {
    // host copies: the list-based searches replay their selection over them, and the handle outlives the caller's arrays
    std::vector<float> kx, ky, ang, ur, sf, s2, is2;
    std::vector<int32_t> oct, nodeStart;
    std::vector<uint8_t> desc, occ;
    std::vector<uint32_t> nodeId, index;
    eao_frame_view view;
    eao_feature_vector fv;
    bool hasFv = false, fvUnique = true;
    unsigned char* dev = nullptr;      // one device block: [KfDev | arrays]
    size_t oOcc = 0;
    // eao_keyframe_set_depth: mvDepth and mvKeys[i].pt (host copies, and one more device block [depth | raw_x | raw_y])
    std::vector<float> depth, rawx, rawy;
    unsigned char* devDepth = nullptr;
    const float* dDepth = nullptr; const float* dRawx = nullptr; const float* dRawy = nullptr;
    KfDev D;
    eao::match::Resident res;
};

extern "C" {

eao_status eao_keyframe_create(const eao_frame_view* F, const eao_feature_vector* fv, eao_keyframe** out) {
    EAO_REQUIRE(F && out, "null argument");
    *out = nullptr;
    eao_status st = eao::require_device();
    if (st) return st;
    const int n = F->n;
    EAO_REQUIRE(n >= 0 && n < 65536, "a keyframe holds 0..65535 keypoints (indices are packed in 16 bits)");
    EAO_REQUIRE(n == 0 || (F->kp_x && F->kp_y && F->kp_octave && F->kp_angle && F->u_right && F->descriptors), "incomplete frame view");
    EAO_REQUIRE(F->scale_factors && F->nlevels > 0 && F->nlevels <= 64 && F->grid_cols > 0 && F->grid_rows > 0 && (long long)F->grid_cols * F->grid_rows < (1 << 24), "bad geometry");
    for (int i = 0; i < n; i++) {
        EAO_REQUIRE(F->kp_octave[i] >= 0 && F->kp_octave[i] < F->nlevels, "keypoint %d: octave %d lies outside the %d levels", i, F->kp_octave[i], F->nlevels);
        EAO_REQUIRE(std::isfinite(F->kp_x[i]) && std::isfinite(F->kp_y[i]), "keypoint %d: NaN / Inf coordinate", i);
    }
    if (fv) EAO_REQUIRE(eao::search::feature_vector_ok(fv, n), "malformed feature vector");
    eao_keyframe* h = new eao_keyframe();
    h->kx.assign(F->kp_x, F->kp_x + n); h->ky.assign(F->kp_y, F->kp_y + n); h->ang.assign(F->kp_angle, F->kp_angle + n); h->ur.assign(F->u_right, F->u_right + n);
    h->oct.assign(F->kp_octave, F->kp_octave + n); h->desc.assign(F->descriptors, F->descriptors + 32 * (size_t)n);
    h->occ.assign(n, 0);
    if (F->occupied) h->occ.assign(F->occupied, F->occupied + n);
    const int nl = F->nlevels;
    h->sf.assign(F->scale_factors, F->scale_factors + nl);
    h->s2.assign(nl, 0.f); h->is2.assign(nl, 0.f);
    if (F->level_sigma2) h->s2.assign(F->level_sigma2, F->level_sigma2 + nl);
    if (F->inv_level_sigma2) h->is2.assign(F->inv_level_sigma2, F->inv_level_sigma2 + nl);
    h->view = *F;
    h->view.kp_x = h->kx.data(); h->view.kp_y = h->ky.data(); h->view.kp_octave = h->oct.data(); h->view.kp_angle = h->ang.data(); h->view.u_right = h->ur.data();
    h->view.descriptors = h->desc.data(); h->view.occupied = h->occ.data(); h->view.scale_factors = h->sf.data();
    h->view.level_sigma2 = F->level_sigma2 ? h->s2.data() : nullptr; h->view.inv_level_sigma2 = F->inv_level_sigma2 ? h->is2.data() : nullptr;
    int nn = 0;
    if (fv) {
        nn = fv->n_nodes;
        h->hasFv = true;
        h->nodeId.assign(fv->node_id, fv->node_id + nn);
        h->nodeStart.assign(fv->node_start, fv->node_start + nn + 1);
        h->index.assign(fv->index, fv->index + (nn ? fv->node_start[nn] : 0));
        std::vector<uint8_t> seen(n, 0);      // DBoW2 files a feature under ONE node; a vector that lists a keypoint twice takes the host path (upstream's greedy rule would reach across nodes)
        for (uint32_t k : h->index) { if (seen[k]) h->fvUnique = false; seen[k] = 1; }
        //  k_kf_nodes marks side-2 entries already matched in ONE 64-bit mask per lane: 64 x 64 = 4096 entries of a node at most.  A node beyond that (DBoW2's
        // level-4 nodes of a 1000-feature frame hold tens) takes the host path like a non-unique vector.
        for (int a = 0; a < nn; a++) if (h->nodeStart[a + 1] - h->nodeStart[a] > 4096) h->fvUnique = false;
    }
    if (h->nodeStart.empty()) h->nodeStart.assign(1, 0);
    h->fv.n_nodes = nn; h->fv.node_id = h->nodeId.data(); h->fv.node_start = h->nodeStart.data(); h->fv.index = h->index.data();
    // grid order: PosInGrid (src/Frame.cc:751-761 / KeyFrame's copy of the grid) then cell column-major, insertion (= index) order inside a cell
    const int cols = F->grid_cols, rows = F->grid_rows;
    const size_t nCells = (size_t)cols * rows;
    std::vector<int> cellOf(n), cellStart(nCells + 1, 0);
    for (int i = 0; i < n; i++) {
        const int px = (int)std::round((F->kp_x[i] - F->min_x) * F->grid_inv_w);
        const int py = (int)std::round((F->kp_y[i] - F->min_y) * F->grid_inv_h);
        const bool in = px >= 0 && px < cols && py >= 0 && py < rows;
        cellOf[i] = in ? px * rows + py : -1;
        if (in) cellStart[cellOf[i] + 1]++;
    }
    for (size_t q = 0; q < nCells; q++) cellStart[q + 1] += cellStart[q];
    const int no = cellStart[nCells];
    std::vector<int> order(std::max(no, 1)), colStart(cols + 1);
    std::vector<unsigned short> cellx(std::max(no, 1)), celly(std::max(no, 1));
    for (int x = 0; x <= cols; x++) colStart[x] = cellStart[(size_t)std::min(x, cols) * rows];
    {
        std::vector<int> cur(cellStart.begin(), cellStart.end() - 1);
        for (int i = 0; i < n; i++)
            if (cellOf[i] >= 0) { const int o = cur[cellOf[i]]++; order[o] = i; cellx[o] = (unsigned short)(cellOf[i] / rows); celly[o] = (unsigned short)(cellOf[i] % rows); }
    }
    // one device block
    const size_t n1 = std::max(n, 1), no1 = std::max(no, 1), nn1 = std::max(nn, 1), ni = std::max<size_t>(h->index.size(), 1);
    size_t off = align256(sizeof(KfDev));
    const size_t oKx = off; off = align256(off + 4 * n1);
    const size_t oKy = off; off = align256(off + 4 * n1);
    const size_t oUr = off; off = align256(off + 4 * n1);
    const size_t oAn = off; off = align256(off + 4 * n1);
    const size_t oOc = off; off = align256(off + 4 * n1);
    const size_t oDe = off; off = align256(off + 32 * n1);
    const size_t oOr = off; off = align256(off + 4 * no1);
    const size_t oCx = off; off = align256(off + 2 * no1);
    const size_t oCy = off; off = align256(off + 2 * no1);
    const size_t oCs = off; off = align256(off + 4 * (size_t)(cols + 1));
    const size_t oOcc = off; off = align256(off + n1);
    const size_t oNi = off; off = align256(off + 4 * nn1);
    const size_t oNs = off; off = align256(off + 4 * (nn1 + 1));
    const size_t oIx = off; off = align256(off + 4 * ni);
    const size_t oSf = off; off = align256(off + 4 * (size_t)nl);
    const size_t oS2 = off; off = align256(off + 4 * (size_t)nl);
    const size_t oI2 = off; off = align256(off + 4 * (size_t)nl);
    std::vector<unsigned char> hb(off, 0);
    if (hipMalloc((void**)&h->dev, off) != hipSuccess) { delete h; eao::set_error("hipMalloc of %zu bytes failed", off); return EAO_ERR_NO_DEVICE; }
    unsigned char* dv = h->dev;
    KfDev& D = h->D;
    D.n = n; D.no = no; D.nNodes = nn; D.nlevels = nl;
    D.kx = (const float*)(dv + oKx); D.ky = (const float*)(dv + oKy); D.ur = (const float*)(dv + oUr); D.ang = (const float*)(dv + oAn);
    D.oct = (const int*)(dv + oOc); D.desc = (const uint4*)(dv + oDe); D.order = (const int*)(dv + oOr);
    D.cellx = (const unsigned short*)(dv + oCx); D.celly = (const unsigned short*)(dv + oCy); D.colStart = (const int*)(dv + oCs);
    D.occ = dv + oOcc; D.nodeId = (const unsigned*)(dv + oNi); D.nodeStart = (const int*)(dv + oNs); D.index = (const unsigned*)(dv + oIx);
    D.sf = (const float*)(dv + oSf); D.s2 = (const float*)(dv + oS2); D.is2 = (const float*)(dv + oI2);
    D.minX = F->min_x; D.minY = F->min_y; D.maxX = F->max_x; D.maxY = F->max_y; D.invW = F->grid_inv_w; D.invH = F->grid_inv_h; D.logScale = F->log_scale_factor;
    D.cols = cols; D.rows = rows;
    std::memcpy(hb.data(), &D, sizeof(D));
    if (n) {
        std::memcpy(&hb[oKx], h->kx.data(), 4 * (size_t)n); std::memcpy(&hb[oKy], h->ky.data(), 4 * (size_t)n); std::memcpy(&hb[oUr], h->ur.data(), 4 * (size_t)n);
        std::memcpy(&hb[oAn], h->ang.data(), 4 * (size_t)n); std::memcpy(&hb[oOc], h->oct.data(), 4 * (size_t)n); std::memcpy(&hb[oDe], h->desc.data(), 32 * (size_t)n);
        std::memcpy(&hb[oOcc], h->occ.data(), n);
    }
    if (no) { std::memcpy(&hb[oOr], order.data(), 4 * (size_t)no); std::memcpy(&hb[oCx], cellx.data(), 2 * (size_t)no); std::memcpy(&hb[oCy], celly.data(), 2 * (size_t)no); }
    std::memcpy(&hb[oCs], colStart.data(), 4 * (size_t)(cols + 1));
    if (nn) { std::memcpy(&hb[oNi], h->nodeId.data(), 4 * (size_t)nn); std::memcpy(&hb[oIx], h->index.data(), 4 * h->index.size()); }
    std::memcpy(&hb[oNs], h->nodeStart.data(), 4 * h->nodeStart.size());
    std::memcpy(&hb[oSf], h->sf.data(), 4 * (size_t)nl); std::memcpy(&hb[oS2], h->s2.data(), 4 * (size_t)nl); std::memcpy(&hb[oI2], h->is2.data(), 4 * (size_t)nl);
    if (hipMemcpy(dv, hb.data(), off, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(h->dev); delete h; eao::set_error("upload of the keyframe failed"); return EAO_ERR_NO_DEVICE; }
    h->oOcc = oOcc;
    eao::match::Resident& R = h->res;
    R.kx = D.kx; R.ky = D.ky; R.ur = D.ur; R.oct = D.oct; R.desc = (const uint8_t*)D.desc; R.order = D.order; R.cellx = D.cellx; R.celly = D.celly; R.colStart = D.colStart;
    R.n = n; R.no = no;
    *out = h;
    return EAO_OK;
}

eao_status eao_keyframe_update_points(eao_keyframe* h, const uint8_t* occupied) {
    EAO_REQUIRE(h, "null handle");
    if (h->D.n == 0) return EAO_OK;
    if (occupied) std::memcpy(h->occ.data(), occupied, h->D.n);
    else std::fill(h->occ.begin(), h->occ.end(), 0);
    EAO_HIP(hipMemcpy(h->dev + h->oOcc, h->occ.data(), h->D.n, hipMemcpyHostToDevice));
    return EAO_OK;
}

void eao_keyframe_destroy(eao_keyframe* h) {
    if (!h) return;
    if (h->dev) (void)hipFree(h->dev);
    if (h->devDepth) (void)hipFree(h->devDepth);
    delete h;
}

eao_status eao_keyframe_set_depth(eao_keyframe* h, const float* depth, const float* raw_x, const float* raw_y) {
    EAO_REQUIRE(h, "null handle");
    const size_t n = (size_t)h->D.n;
    EAO_REQUIRE(n == 0 || depth, "depth missing");
    EAO_REQUIRE(!raw_x == !raw_y, "raw_x and raw_y come together");
    const size_t seg = align256(4 * std::max<size_t>(n, 1));
    if (!h->devDepth && hipMalloc((void**)&h->devDepth, 3 * seg) != hipSuccess) { h->devDepth = nullptr; eao::set_error("hipMalloc of %zu bytes failed", 3 * seg); return EAO_ERR_NO_DEVICE; }
    h->depth.assign(depth, depth + n);
    if (raw_x) { h->rawx.assign(raw_x, raw_x + n); h->rawy.assign(raw_y, raw_y + n); }
    else { h->rawx = h->kx; h->rawy = h->ky; }
    if (n) {
        EAO_HIP(hipMemcpy(h->devDepth, h->depth.data(), 4 * n, hipMemcpyHostToDevice));
        EAO_HIP(hipMemcpy(h->devDepth + seg, h->rawx.data(), 4 * n, hipMemcpyHostToDevice));
        EAO_HIP(hipMemcpy(h->devDepth + 2 * seg, h->rawy.data(), 4 * n, hipMemcpyHostToDevice));
    }
    h->dDepth = (const float*)h->devDepth; h->dRawx = (const float*)(h->devDepth + seg); h->dRawy = (const float*)(h->devDepth + 2 * seg);
    return EAO_OK;
}

int32_t eao_keyframe_size(const eao_keyframe* h) { return h ? h->D.n : -1; }

}  // extern "C"

namespace {

// eao_kf_create_new_map_points: the triangulation of csrc/triangulate.hip enqueued behind the search's last launch, over the table the finish kernel wrote
struct TriTail { const eao_tri_camera* cam1; const eao_tri_camera* cams2; float ratioFactor; int32_t* verdict; float* x3d; };

eao::tri::Side tri_side(const eao_keyframe* k) {
    eao::tri::Side S;
    S.n = k->D.n; S.nlevels = k->D.nlevels;
    S.kx = k->D.kx; S.ky = k->D.ky; S.ur = k->D.ur; S.depth = k->dDepth; S.rawx = k->dRawx; S.rawy = k->dRawy; S.oct = k->D.oct; S.sf = k->D.sf; S.s2 = k->D.s2;
    return S;
}

// the shared driver of the vocabulary-node searches: MODE as in k_kf_nodes; problems in chunks of kMaxProb per launch pair, ONE synchronisation
// (tail: the triangulation kernels follow on the same stream and the one wait is the stream's, behind them)
eao_status run_nodes(int mode, const eao_keyframe* k1, int nProb, const eao_keyframe* const* k2s, const float* F12s, const float* exs, const float* eys,
                     const uint8_t* valid1, const uint8_t* valid2, float nnratio, int onlyStereo, int checkOrientation, int32_t* match12, int32_t* nmatches,
                     const TriTail* tail = nullptr) {
    Ctx& c = g_kctx;
    eao_status st = c.ready(eao::StreamClass::Latency);
    if (st) return st;
    const int n1 = k1->D.n;
    if (n1 == 0 || nProb == 0) { for (int p = 0; p < nProb; p++) nmatches[p] = 0; return EAO_OK; }
    const size_t cells = (size_t)nProb * n1;
    eao::Drain drain(c.stream);
    if (c.match.n < cells) {
        if ((st = c.match.reserve(cells + (cells >> 2)))) return st;
        EAO_HIP(hipMemsetAsync(c.match.p, 0, c.match.n * sizeof(int2), c.stream));      // (fresh memory may hold anything: no stamp of it may equal a generation)
        c.gen = 0;
    }
    if (c.gen == 0x7FFFFFFF) { EAO_HIP(hipMemsetAsync(c.match.p, 0, c.match.n * sizeof(int2), c.stream)); c.gen = 0; }
    c.gen++;
    // mapped input block: the BoW validity flags; mapped output block: [counts | tables]
    const size_t oV1 = 0, oV2 = align256((size_t)n1), inBytes = oV2 + align256(valid2 ? (size_t)k2s[0]->D.n : 1);
    if ((st = c.in.reserve(inBytes))) return st;
    if (valid1) std::memcpy(c.in.p + oV1, valid1, n1);
    if (valid2) std::memcpy(c.in.p + oV2, valid2, k2s[0]->D.n);
    const size_t oTab = align256(4 * (size_t)nProb);
    if ((st = c.out.reserve(oTab + 4 * cells))) return st;
    const size_t oX3 = align256(4 * cells);
    if (tail && (st = c.tri.reserve(oX3 + 12 * cells))) return st;
    if (!c.ticket.p) {
        if ((st = c.ticket.reserve(1))) return st;
        EAO_HIP(hipMemsetAsync(c.ticket.p, 0, sizeof(int), c.stream));
        c.ticketNext = 0;
        if ((st = c.doneWord.reserve(64))) return st;
    }
    if (c.ticketNext > 0x70000000) { EAO_HIP(hipMemsetAsync(c.ticket.p, 0, sizeof(int), c.stream)); c.ticketNext = 0; }
    const int seq = ++c.seq;
    volatile int* doneHost = reinterpret_cast<volatile int*>(c.doneWord.p);
    *doneHost = 0;
    for (int p0 = 0; p0 < nProb; p0 += kMaxProb) {
        const int np = std::min(kMaxProb, nProb - p0);
        NodesArgs A;
        A.K1 = k1->D; A.nProb = np; A.onlyStereo = onlyStereo; A.nnratio = nnratio;
        A.valid1 = valid1 ? c.in.d + oV1 : nullptr; A.valid2 = valid2 ? c.in.d + oV2 : nullptr;
        A.match = c.match.p + (size_t)p0 * n1; A.gen = c.gen; A.n1 = n1;
        static const bool envStamps = getenv("EAO_DEBUG_STAMPS") && atoi(getenv("EAO_DEBUG_STAMPS"));
        if (envStamps && (st = c.dbg.reserve(64))) return st;
        A.dbg = c.dbg.p;
        A.single = 0;
        if (nProb == 1 && k1->D.nNodes <= kPairCap && k2s[0]->D.nNodes < 32768) {
            A.single = 1;
            A.K2v = k2s[0]->D;
            const eao_keyframe* k2 = k2s[0];
            int b = 0;
            for (int a = 0; a < k1->D.nNodes; a++) {
                while (b < k2->D.nNodes && k2->nodeId[b] < k1->nodeId[a]) b++;
                A.pairB[a] = (short)((b < k2->D.nNodes && k2->nodeId[b] == k1->nodeId[a]) ? b : -1);
            }
        }
        FinishArgs B;
        B.ang1 = k1->D.ang; B.nProb = np; B.n1 = n1; B.gen = c.gen; B.checkOrientation = checkOrientation; B.match = A.match;
        B.out = (int*)(c.out.d + oTab) + (size_t)p0 * n1; B.nm = (int*)c.out.d + p0;
        const bool lastChunk = p0 + np >= nProb;
        B.ticket = c.ticket.p; B.done = (int*)c.doneWord.d; B.doneSeq = seq; B.ticketLast = -1;
        if (lastChunk) B.ticketLast = c.ticketNext + nProb - 1;      // the last workgroup of the call's LAST launch: every earlier one has taken its ticket
        else B.doneSeq = 0;                                          // (earlier chunks take tickets and confirm their stores; they never see ticketLast)
        for (int q = 0; q < np; q++) {
            A.P[q].k2 = (const KfDev*)k2s[p0 + q]->dev;
            if (F12s) { std::memcpy(A.P[q].F, F12s + 9 * (size_t)(p0 + q), 36); A.P[q].ex = exs[p0 + q]; A.P[q].ey = eys[p0 + q]; }
            else { std::memset(A.P[q].F, 0, 36); A.P[q].ex = A.P[q].ey = 0; }
            B.ang2[q] = k2s[p0 + q]->D.ang;
        }
        const dim3 grid(eao::cdiv(std::max(k1->D.nNodes, 1), 4), np);
        if (mode == 0) hipLaunchKernelGGL(k_kf_nodes<0>, grid, dim3(256), 0, c.stream, A);
        else if (mode == 1) hipLaunchKernelGGL(k_kf_nodes<1>, grid, dim3(256), 0, c.stream, A);
        else hipLaunchKernelGGL(k_kf_nodes<2>, grid, dim3(256), 0, c.stream, A);
        hipLaunchKernelGGL(k_kf_finish, dim3(np), dim3(256), 0, c.stream, B);
    }
    bool seen = false;
    //  a rejected launch would leave the device ticket counter behind ticketNext for the rest of the thread's life (every later call would spin out its
    // 50 ms): on any launch error, and after a poll that timed out, the counter and its host twin start again from zero
    const hipError_t launchErr = hipGetLastError();
    if (launchErr != hipSuccess) {
        (void)drain.wait_more(eao::Drain::Block);
        (void)hipMemsetAsync(c.ticket.p, 0, sizeof(int), c.stream);      // (the guard waits for it)
        c.ticketNext = 0;
        eao::set_error("keyframe search launch failed: %s", hipGetErrorString(launchErr));
        return EAO_ERR_NO_DEVICE;
    }
    c.ticketNext += nProb;
    if (tail) {
        static const bool envEvents = getenv("EAO_TRI_EVENTS") && atoi(getenv("EAO_TRI_EVENTS"));
        if (envEvents != c.triClock.armed()) c.triClock.arm(envEvents);
        c.triClock.mark(0, c.stream);
        const eao::tri::Side S1 = tri_side(k1);
        for (int p0 = 0; p0 < nProb; p0 += eao::tri::kMaxProb) {
            const int np = std::min(eao::tri::kMaxProb, nProb - p0);
            eao::tri::Prob P[eao::tri::kMaxProb];
            for (int q = 0; q < np; q++) {
                P[q].K2 = tri_side(k2s[p0 + q]);
                P[q].cam2 = tail->cams2[p0 + q];
                P[q].match = (const int*)(c.out.d + oTab) + (size_t)(p0 + q) * n1;      // where k_kf_finish left the row
            }
            eao::tri::launch(c.stream, S1, *tail->cam1, tail->ratioFactor, np, P, (int*)c.tri.d + (size_t)p0 * n1, (float*)(c.tri.d + oX3) + (size_t)p0 * n1 * 3);
        }
        EAO_HIP(hipGetLastError());
        c.triClock.mark(1, c.stream);
        EAO_HIP(drain.wait_more(eao::Drain::Latency));
        c.triClock.collect();
        seen = true;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0; !seen && !(seen = *doneHost == seq); spins++)
        if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
    std::atomic_thread_fence(std::memory_order_acquire);
    if (seen) drain.disarm();      // (the done word is the last store of the stream's last kernel; the tail's wait came behind its own kernels)
    else {
        EAO_HIP(drain.wait_more(eao::Drain::Latency));
        EAO_HIP(hipMemsetAsync(c.ticket.p, 0, sizeof(int), c.stream)); EAO_HIP(drain.wait(eao::Drain::Latency)); c.ticketNext = 0;
    }
    EAO_HIP(hipGetLastError());
    if (c.dbg.p) {
        long long st[8];
        EAO_HIP(hipMemcpy(st, c.dbg.p, sizeof(st), hipMemcpyDeviceToHost));
        fprintf(stderr, "[eao kf nodes stamps] node 0 (%lld x %lld features): head %lld, side 2 in registers %lld, side 1 in registers %lld, walk %lld ticks of 10 ns\n", st[6], st[7],
                st[1] - st[0], st[2] - st[1], st[3] - st[2], st[4] - st[3]);
    }
    std::memcpy(nmatches, c.out.p, 4 * (size_t)nProb);
    std::memcpy(match12, c.out.p + oTab, 4 * cells);
    if (tail) {
        std::memcpy(tail->verdict, c.tri.p, 4 * cells);
        std::memcpy(tail->x3d, c.tri.p + oX3, 12 * cells);
    }
    return EAO_OK;
}

bool finite_n(const float* v, int n) {
    for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace

extern "C" {

eao_status eao_kf_search_by_bow(int32_t mode, const eao_keyframe* kf1, const uint8_t* valid1, const eao_keyframe* kf2, const uint8_t* valid2, float nnratio,
                                int32_t check_orientation, int32_t* match12, int32_t* nmatches) {
    EAO_REQUIRE((mode == 0 || mode == 1) && kf1 && kf2 && match12 && nmatches, "bad argument");
    EAO_REQUIRE(kf1->hasFv && kf2->hasFv, "both handles need their feature vector (eao_keyframe_create with fv)");
    EAO_REQUIRE(kf1->D.n == 0 || valid1, "valid1 missing");
    EAO_REQUIRE(mode == 0 || kf2->D.n == 0 || valid2, "valid2 missing (mode 1)");
    if (!kf1->fvUnique || !kf2->fvUnique)      // a keypoint filed under two nodes: upstream's walk order matters across nodes -- the host replay keeps it
        return eao_search_by_bow(mode, kf1->D.n, kf1->desc.data(), kf1->ang.data(), valid1, &kf1->fv, kf2->D.n, kf2->desc.data(), kf2->ang.data(), valid2, &kf2->fv,
                                 nnratio, check_orientation, match12, nmatches);
    return run_nodes(mode, kf1, 1, &kf2, nullptr, nullptr, nullptr, valid1, mode == 1 ? valid2 : nullptr, nnratio, 0, check_orientation, match12, nmatches);
}

eao_status eao_kf_search_for_triangulation(const eao_keyframe* kf1, int32_t n_nb, const eao_keyframe* const* kf2s, const float* F12s, const float* exs,
                                           const float* eys, int32_t only_stereo, int32_t check_orientation, int32_t* match12, int32_t* nmatches) {
    EAO_REQUIRE(kf1 && n_nb >= 0 && (n_nb == 0 || (kf2s && F12s && exs && eys && match12 && nmatches)), "bad argument");
    if (n_nb == 0) return EAO_OK;
    EAO_REQUIRE(kf1->hasFv, "the handle needs its feature vector (eao_keyframe_create with fv)");
    bool unique = kf1->fvUnique;
    for (int k = 0; k < n_nb; k++) {
        EAO_REQUIRE(kf2s[k] && kf2s[k]->hasFv && kf2s[k]->view.level_sigma2, "neighbour %d: no handle, no feature vector or no level_sigma2 in its view", k);
        EAO_REQUIRE(finite_n(F12s + 9 * (size_t)k, 9), "neighbour %d: F12 holds a NaN / Inf", k);      // (the epipole may: a keyframe against itself projects its own centre -- upstream's comparison with it is then false, here too)
        unique = unique && kf2s[k]->fvUnique;
    }
    if (!unique) {
        std::vector<const eao_frame_view*> vs(n_nb);
        std::vector<const eao_feature_vector*> fs(n_nb);
        for (int k = 0; k < n_nb; k++) { vs[k] = &kf2s[k]->view; fs[k] = &kf2s[k]->fv; }
        return eao_search_for_triangulation_batch(&kf1->view, &kf1->fv, n_nb, vs.data(), fs.data(), F12s, exs, eys, only_stereo, check_orientation, match12, nmatches);
    }
    return run_nodes(2, kf1, n_nb, kf2s, F12s, exs, eys, nullptr, nullptr, 0.f, only_stereo, check_orientation, match12, nmatches);
}

eao_status eao_kf_create_new_map_points(const eao_keyframe* kf1, const eao_tri_camera* cam1, int32_t n_nb, const eao_keyframe* const* kf2s,
                                        const eao_tri_camera* cams2, const float* F12s, const float* exs, const float* eys, int32_t only_stereo,
                                        int32_t check_orientation, float ratio_factor, int32_t* match12, int32_t* nmatches, int32_t* verdict, float* x3d) {
    EAO_REQUIRE(kf1 && cam1 && n_nb >= 0 && (n_nb == 0 || (kf2s && cams2 && F12s && exs && eys && match12 && nmatches && verdict && x3d)), "bad argument");
    if (n_nb == 0) return EAO_OK;
    EAO_REQUIRE(kf1->hasFv, "the handle needs its feature vector (eao_keyframe_create with fv)");
    EAO_REQUIRE(kf1->dDepth && kf1->view.level_sigma2, "keyframe 1: no depth (eao_keyframe_set_depth) or no level_sigma2 in its view");
    bool unique = kf1->fvUnique;
    for (int k = 0; k < n_nb; k++) {
        EAO_REQUIRE(kf2s[k] && kf2s[k]->hasFv && kf2s[k]->view.level_sigma2, "neighbour %d: no handle, no feature vector or no level_sigma2 in its view", k);
        EAO_REQUIRE(kf2s[k]->dDepth, "neighbour %d: no depth (eao_keyframe_set_depth)", k);
        EAO_REQUIRE(finite_n(F12s + 9 * (size_t)k, 9), "neighbour %d: F12 holds a NaN / Inf", k);
        unique = unique && kf2s[k]->fvUnique;
    }
    if (!unique) {      // the host replay of the search (as eao_kf_search_for_triangulation), then the triangulation over host arrays
        std::vector<const eao_frame_view*> vs(n_nb);
        std::vector<const eao_feature_vector*> fs(n_nb);
        std::vector<const float*> dp(n_nb), rx(n_nb), ry(n_nb);
        for (int k = 0; k < n_nb; k++) { vs[k] = &kf2s[k]->view; fs[k] = &kf2s[k]->fv; dp[k] = kf2s[k]->depth.data(); rx[k] = kf2s[k]->rawx.data(); ry[k] = kf2s[k]->rawy.data(); }
        eao_status st = eao_search_for_triangulation_batch(&kf1->view, &kf1->fv, n_nb, vs.data(), fs.data(), F12s, exs, eys, only_stereo, check_orientation, match12, nmatches);
        if (st) return st;
        return eao_triangulate_matches_batch(&kf1->view, cam1, kf1->depth.data(), kf1->rawx.data(), kf1->rawy.data(), n_nb, vs.data(), cams2, dp.data(), rx.data(), ry.data(),
                                             match12, ratio_factor, verdict, x3d);
    }
    const TriTail tail{cam1, cams2, ratio_factor, verdict, x3d};
    return run_nodes(2, kf1, n_nb, kf2s, F12s, exs, eys, nullptr, nullptr, 0.f, only_stereo, check_orientation, match12, nmatches, &tail);
}

eao_status eao_kf_last_triangulation_ms(float* ms) {
    EAO_REQUIRE(ms, "null argument");
    return g_kctx.triClock.read(ms, "no measurement on this thread: EAO_TRI_EVENTS=1 and a call of eao_kf_create_new_map_points come first");
}

eao_status eao_kf_fuse_search(int32_t n_kf, const eao_keyframe* const* kfs, int32_t use_sim3, const float* poses, float fx, float fy, float cx, float cy, float bf,
                              const eao_map_points* pts, float th, int32_t* best_kp, int32_t* nfused) {
    EAO_REQUIRE(n_kf >= 0 && (n_kf == 0 || (kfs && poses && best_kp && nfused)), "bad argument");
    EAO_REQUIRE(pts && pts->n >= 0 && (pts->n == 0 || (pts->active && pts->Xw && pts->normal && pts->min_dist_inv && pts->max_dist_inv && pts->max_dist && pts->desc)),
                "incomplete map points");
    if (n_kf == 0) return EAO_OK;
    const int n = pts->n, plen = use_sim3 ? 16 : 15;
    for (int f = 0; f < n_kf; f++) {
        EAO_REQUIRE(kfs[f] && (use_sim3 || kfs[f]->view.inv_level_sigma2), "target %d: no handle, or no inv_level_sigma2 in its view", f);
        EAO_REQUIRE(finite_n(poses + (size_t)plen * f, plen), "target %d: the pose holds a NaN / Inf", f);
        nfused[f] = 0;
    }
    if (n == 0) return EAO_OK;
    Ctx& c = g_kctx;
    eao_status st = c.ready(eao::StreamClass::Latency);
    if (st) return st;
    // the points: one staging block in mapped memory, one upload kernel
    const size_t N = n;
    const size_t oAc = 0, oXw = align256(N), oNr = align256(oXw + 12 * N), oMn = align256(oNr + 12 * N), oMx = align256(oMn + 4 * N), oDr = align256(oMx + 4 * N), oDe = align256(oDr + 4 * N),
                 bytes = align256(oDe + 32 * N);
    if ((st = c.in.reserve(bytes))) return st;
    if ((st = c.dev.reserve(bytes))) return st;
    unsigned char* hb = c.in.p;
    std::memcpy(hb + oAc, pts->active, N); std::memcpy(hb + oXw, pts->Xw, 12 * N); std::memcpy(hb + oNr, pts->normal, 12 * N);
    std::memcpy(hb + oMn, pts->min_dist_inv, 4 * N); std::memcpy(hb + oMx, pts->max_dist_inv, 4 * N); std::memcpy(hb + oDr, pts->max_dist, 4 * N);
    std::memcpy(hb + oDe, pts->desc, 32 * N);
    if ((st = c.out.reserve(4 * N * (size_t)n_kf))) return st;
    const size_t n16 = bytes / 16;
    eao::Drain drain(c.stream);
    hipLaunchKernelGGL(k_kf_upload, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 256)), dim3(256), 0, c.stream, (const uint4*)c.in.d, (uint4*)c.dev.p, n16);
    for (int f0 = 0; f0 < n_kf; f0 += kMaxProb) {
        const int nf = std::min(kMaxProb, n_kf - f0);
        FuseArgs A;
        A.nKf = nf; A.useSim3 = use_sim3; A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.bf = bf; A.th = th;
        unsigned char* dv = c.dev.p;
        A.P.n = n; A.P.active = dv + oAc; A.P.Xw = (const float*)(dv + oXw); A.P.normal = (const float*)(dv + oNr); A.P.dmin = (const float*)(dv + oMn);
        A.P.dmax = (const float*)(dv + oMx); A.P.draw = (const float*)(dv + oDr); A.P.desc = (const uint4*)(dv + oDe);
        A.out = (int*)c.out.d + (size_t)f0 * N;
        for (int q = 0; q < nf; q++) {
            FuseTarget& T = A.T[q];
            T.k = (const KfDev*)kfs[f0 + q]->dev;
            const float* pose = poses + (size_t)plen * (f0 + q);
            if (use_sim3) {      // src/ORBmatcher.cc:980-986 (the same statements as decompose_sim3, csrc/search.hip)
                const float scw = (float)std::sqrt((double)pose[0] * pose[0] + (double)pose[1] * pose[1] + (double)pose[2] * pose[2]);
                for (int r = 0; r < 3; r++) { for (int cc = 0; cc < 3; cc++) T.R[r * 3 + cc] = pose[r * 4 + cc] / scw; T.t[r] = pose[r * 4 + 3] / scw; }
                for (int i = 0; i < 3; i++) {
                    double s = 0;
                    for (int k = 0; k < 3; k++) s += (double)T.R[k * 3 + i] * (double)T.t[k];
                    T.Ow[i] = (float)(-s);
                }
            } else { std::memcpy(T.R, pose, 36); std::memcpy(T.t, pose + 9, 12); std::memcpy(T.Ow, pose + 12, 12); }
        }
        hipLaunchKernelGGL(k_kf_fuse, dim3(eao::cdiv(n, 4), nf), dim3(256), 0, c.stream, A);
    }
    EAO_HIP(drain.wait(eao::Drain::Latency));
    EAO_HIP(hipGetLastError());
    std::memcpy(best_kp, c.out.p, 4 * N * (size_t)n_kf);
    for (int f = 0; f < n_kf; f++) {
        int nf = 0;
        const int32_t* b = best_kp + (size_t)f * N;
        for (int i = 0; i < n; i++) nf += b[i] >= 0;
        nfused[f] = nf;
    }
    return EAO_OK;
}

// ---- the list-based searches over a resident frame: the frame's view is the handle's host copy, its occupancy the caller's (it differs from search to search)
eao_status eao_kf_search_by_projection_sim3(const eao_keyframe* kf, const uint8_t* occupied, const float* Scw, float fx, float fy, float cx, float cy,
                                            const eao_map_points* pts, int32_t th, int32_t* kp_match, int32_t* nmatches) {
    EAO_REQUIRE(kf, "null handle");
    eao_frame_view v = kf->view;
    v.occupied = occupied;
    return eao::search::projection_sim3(&v, &kf->res, Scw, fx, fy, cx, cy, pts, th, kp_match, nmatches);
}
eao_status eao_kf_search_by_projection_kf(const eao_keyframe* cur, const uint8_t* occupied, const float* Tcw, float fx, float fy, float cx, float cy,
                                          const eao_map_points* pts, const float* kf_angle, float th, int32_t orb_dist, int32_t check_orientation, int32_t* cur_match,
                                          int32_t* nmatches) {
    EAO_REQUIRE(cur, "null handle");
    eao_frame_view v = cur->view;
    v.occupied = occupied;
    return eao::search::projection_kf(&v, &cur->res, Tcw, fx, fy, cx, cy, pts, kf_angle, th, orb_dist, check_orientation, cur_match, nmatches);
}
eao_status eao_kf_search_for_initialization(int32_t n1, const int32_t* octave1, const float* angle1, const uint8_t* desc1, const eao_keyframe* f2, float* prev_matched,
                                            int32_t window, float nnratio, int32_t check_orientation, int32_t* match12, int32_t* nmatches) {
    EAO_REQUIRE(f2, "null handle");
    return eao::search::initialization(n1, octave1, angle1, desc1, &f2->view, &f2->res, prev_matched, window, nnratio, check_orientation, match12, nmatches);
}
eao_status eao_kf_search_by_sim3(const eao_keyframe* k1, const float* T1w, const eao_map_points* pts1, const eao_keyframe* k2, const float* T2w,
                                 const eao_map_points* pts2, float fx, float fy, float cx, float cy, float s12, const float* R12, const float* t12, float th,
                                 int32_t* match12, int32_t* nfound) {
    EAO_REQUIRE(k1 && k2, "null handle");
    return eao::search::by_sim3(&k1->view, &k1->res, T1w, pts1, &k2->view, &k2->res, T2w, pts2, fx, fy, cx, cy, s12, R12, t12, th, match12, nfound);
}

}  // extern "C"
