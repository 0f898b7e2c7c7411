// iforest.hip -- Object_Map::IsolationForestDeleteOutliers on the device (reference src/Object.cc:1239-1348, include/isolation_forest.h): the 50-tree isolation
// forest over an object's map points, bit for bit what the reference's header computes under libstdc++ (csrc/iforest_internal.h names the algorithms).
//
//   k_iforest_build   one wavefront per (object, tree).  The tree's generator (std::mt19937, 624 words) lives in LDS: the seeding recurrence runs on one lane, the
//                     twist in lane-parallel chunks of 64, every draw is a broadcast read.  std::shuffle's draws are reduced 64 at a time, its swaps run on one lane over 16-bit ids; the first
//                     sample_size ids are the sample.  Node::Build's recursion is a depth-first walk with an explicit stack of pending right children; per node a
//                     wave min/max reduction, the two draws, and a partition by ballot and prefix counts (the left child is the SET of elements below the split,
//                     so no sort is needed).  Nodes are emitted in preorder as Node::Serialize writes them, each with the index of its right child.
//   k_iforest_score   one wavefront per point, one lane per tree: each lane walks its tree to double(depth) + C[size], C from the host's libm table; lane 0 adds
//                     them in tree order.
//
// The host finishes (total / trees, pow with libm, the threshold and the rules of :1241-1257) and draws the tree seeds.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"
#include "iforest_internal.h"

namespace {

using namespace eao::iforest;

static_assert(kTreeCount == EAO_OBJECT_IFOREST_TREES && kSeed == EAO_OBJECT_IFOREST_SEED && kMinPoints == EAO_OBJECT_IFOREST_MIN_POINTS &&
                  kMaxPoints == EAO_IFOREST_MAX_POINTS && kExemptClasses[0] == EAO_OBJECT_IFOREST_EXEMPT_CLASS_A &&
                  kExemptClasses[1] == EAO_OBJECT_IFOREST_EXEMPT_CLASS_B && kExemptClasses[2] == EAO_OBJECT_IFOREST_EXEMPT_CLASS_C,
              "include/eao_fusion.h and iforest_internal.h state the same rules");

constexpr int kStackSlots = 20;      // pending right children: one per level, maxDepth <= 16

// ---- std::mt19937 in LDS.  p and every draw are wave-uniform: all lanes run the same scalar code, stores are lane 0's.
__device__ __forceinline__ void mt_seed(unsigned* x, unsigned seed, int lane) {
    if (lane == 0) {
        unsigned v = seed;
        x[0] = v;
        for (unsigned i = 1; i < kMtN; i++) {
            v = 1812433253u * (v ^ (v >> 30)) + i;
            x[i] = v;
        }
    }
    eao::wave_sync();
}

// x[k] needs the OLD x[k+1] and x[k+397] (k < 227) and the NEW x[k-227] (k >= 227) and, at k = 623, the NEW x[0]: chunks of 64 in ascending order, each read
// whole before it is written, give exactly that (227 >= 64).
__device__ __forceinline__ void mt_twist(unsigned* x, int lane) {
    for (unsigned base = 0; base < kMtN; base += 64) {
        const unsigned k = base + lane;
        const bool on = k < kMtN;
        unsigned nv = 0;
        if (on) {
            const unsigned k1 = k + 1 == kMtN ? 0 : k + 1;
            const unsigned km = k + kMtM >= kMtN ? k + kMtM - kMtN : k + kMtM;
            const unsigned y = (x[k] & 0x80000000u) | (x[k1] & 0x7fffffffu);
            nv = x[km] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        eao::wave_sync();
        if (on) x[k] = nv;
        eao::wave_sync();
    }
}

struct Gen {
    unsigned* x;
    unsigned p;
    int lane;
    __device__ __forceinline__ unsigned draw() {
        if (p >= kMtN) {
            mt_twist(x, lane);
            p = 0;
        }
        unsigned z = __builtin_amdgcn_readfirstlane(x[p]);
        p++;
        z ^= z >> 11;
        z ^= (z << 7) & 0x9d2c5680u;
        z ^= (z << 15) & 0xefc60000u;
        z ^= z >> 18;
        return z;
    }
    // uniform_int_distribution(0, range - 1), bits/uniform_int_dist.h _S_nd
    __device__ __forceinline__ unsigned lemire(unsigned range) {
        unsigned long long product = (unsigned long long)draw() * range;
        unsigned low = (unsigned)product;
        if (low < range) {
            const unsigned threshold = (0u - range) % range;
            while (low < threshold) {
                product = (unsigned long long)draw() * range;
                low = (unsigned)product;
            }
        }
        return (unsigned)(product >> 32);
    }
    // uniform_real_distribution<float>(a, b): generate_canonical<float, 24> is one draw over 2^32, clamped below 1; then u * (b - a) + a, each operation rounded
    __device__ __forceinline__ float uniform_real(float a, float b) {
        const float r = (float)draw() / 4294967296.0f;
        const float u = r >= 1.0f ? 0x1.fffffep-1f : r;
        const float w = b - a;
        const float m = u * w;
        return m + a;
    }
};

// std::iter_swap(ids + i, ids + j) at step i of the shuffle, j <= i: no earlier step touched ids[i], so it still holds i and is never initialised
__device__ __forceinline__ void swap_ids(unsigned short* ids, unsigned i, unsigned j, int lane) {
    const unsigned short vj = j == i ? (unsigned short)i : ids[j];
    eao::wave_sync();
    if (lane == 0) {
        ids[i] = vj;
        ids[j] = (unsigned short)i;
    }
    eao::wave_sync();
}

__device__ __forceinline__ float wave_min(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ unsigned uni(unsigned v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float unif(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); }
__device__ __forceinline__ unsigned below(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

__global__ __launch_bounds__(64) void k_iforest_build(const ObjDev* __restrict__ objs, const unsigned* __restrict__ treeObj, const unsigned* __restrict__ seeds,
                                                      const float* __restrict__ xyz, NodeDev* __restrict__ nodes, unsigned* __restrict__ nodeCount,
                                                      unsigned* __restrict__ failed, unsigned short* __restrict__ ws, unsigned long long* __restrict__ stamps) {
    __shared__ unsigned mt[kMtN];
    __shared__ unsigned stk[kStackSlots * 4];
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];

    const int lane = threadIdx.x;
    const unsigned g = blockIdx.x;
    const unsigned obj = treeObj[g];
    const ObjDev o = objs[obj];
    const unsigned tree = g - o.treeBase;
    if (tree >= o.treeCount) return;      // (uniform) an object of a chain that the rules skip: its trees are launched before its size is known
    const unsigned N = o.n, S = o.sampleSize, maxDepth = o.maxDepth;
    const float* pin = xyz + (size_t)o.ptStart * 3;
    NodeDev* out = nodes + o.nodeBase + (size_t)tree * o.stride;

    // the working set (iforest_internal.h lds_plan): ids, then in LDS the sample's coordinates by slot
    unsigned short* ids;
    const float* pts;
    unsigned dimStride, idStride;
    if (o.inLds) {
        ids = (unsigned short*)dyn;
        pts = (const float*)(dyn + o.idsBytes);
        dimStride = S;
        idStride = 1;
    } else {
        ids = ws + o.wsBase + (size_t)tree * (o.idsBytes / 2);
        pts = pin;
        dimStride = 1;
        idStride = 3;
    }

    // (profiling only: the constant 100 MHz clock at the four stage boundaries of this tree, for tools/bench_isolation_forest.py)
    if (stamps && lane == 0) stamps[(size_t)g * 4] = wall_clock64();
    Gen gen{mt, kMtN, lane};
    mt_seed(mt, seeds[g], lane);
    if (stamps && lane == 0) stamps[(size_t)g * 4 + 1] = wall_clock64();

    // ---- IsolationTree::Build :314-322: ids 0 .. N-1, std::shuffle (two swaps per draw; an even count swaps one element first)
    if (lane == 0) ids[0] = 0;
    eao::wave_sync();
    {
        unsigned i = 1;
        if (N > 1 && (N & 1u) == 0) {
            swap_ids(ids, i, gen.lemire(2), lane);
            i++;
        }
        // The draws do not depend on the swaps: up to 64 lanes temper one state word each and reduce it to the two partners of their pair of elements; the
        // swaps then run in order on one lane.  A rejected draw (rare) ends the chunk in front of its pair, which goes through the sequential form.
        while (i < N) {
            if (gen.p >= kMtN) {
                mt_twist(mt, lane);
                gen.p = 0;
            }
            const unsigned pairsLeft = (N - i) >> 1, wordsLeft = kMtN - gen.p;
            const unsigned m = min(64u, min(pairsLeft, wordsLeft));
            unsigned ab = 0;
            bool rejected = false;
            if ((unsigned)lane < m) {
                const unsigned ik = i + 2 * lane, b1 = ik + 2, range = (ik + 1) * b1;
                unsigned z = mt[gen.p + lane];
                z ^= z >> 11;
                z ^= (z << 7) & 0x9d2c5680u;
                z ^= (z << 15) & 0xefc60000u;
                z ^= z >> 18;
                const unsigned long long product = (unsigned long long)z * range;
                const unsigned low = (unsigned)product;
                if (low < range) rejected = low < (0u - range) % range;
                const unsigned x = (unsigned)(product >> 32), a = x / b1;
                ab = (a << 16) | (x - a * b1);      // (both partners are at most i + 1 <= 65534)
            }
            const unsigned long long rm = __ballot(rejected);
            const unsigned good = rm ? (unsigned)__ffsll((long long)rm) - 1u : m;
            for (unsigned q = 0; q < good; q++) {
                const unsigned v = __builtin_amdgcn_readlane(ab, q);
                swap_ids(ids, i, v >> 16, lane);
                swap_ids(ids, i + 1, v & 0xffffu, lane);
                i += 2;
            }
            gen.p += good;
            if (good < m) {
                const unsigned b1 = i + 2;
                const unsigned x = gen.lemire((i + 1) * b1);
                const unsigned a = x / b1, b = x - a * b1;
                swap_ids(ids, i, a, lane);
                swap_ids(ids, i + 1, b, lane);
                i += 2;
            }
        }
    }
    // ---- the sample: the first S ids (:327-330).  In LDS its coordinates are copied by slot and the ids become slots.
    if (o.inLds) {
        float* c = (float*)(dyn + o.idsBytes);
        for (unsigned s = lane; s < S; s += 64) {
            const unsigned id = ids[s];
            c[s] = pin[3 * id];
            c[S + s] = pin[3 * id + 1];
            c[2 * S + s] = pin[3 * id + 2];
        }
        eao::wave_sync();
        for (unsigned s = lane; s < S; s += 64) ids[s] = (unsigned short)s;
        eao::wave_sync();
    }
    if (stamps && lane == 0) stamps[(size_t)g * 4 + 2] = wall_clock64();
    unsigned short* tmp = ids + S;      // the partition's scratch: S entries behind the sample (idsEntries = max(N, 2 S))

    // ---- Node::Build :165-224 as a depth-first walk, left subtree first, one generator down the whole walk
    unsigned first = 0, last = S - 1, depth = 0, k = 0, sp = 0;
    bool bad = false;
    for (;;) {
        for (;;) {
            const unsigned me = k++, count = last - first + 1;
            if (me >= o.stride) { bad = true; break; }
            if (count == 1 || depth >= maxDepth) {      // :172-176, nothing drawn
                if (lane == 0) out[me] = NodeDev{0u, 0.0f, count, 0u};
                break;
            }
            const unsigned dim = gen.lemire(3);      // :178-180
            const float* pd = pts + (size_t)dim * dimStride;
            float lo = INFINITY, hi = -INFINITY;
            unsigned short id0 = 0;
            float v0 = 0.0f;
            const bool small = count <= 64;
            if (small) {
                if ((unsigned)lane < count) {
                    id0 = ids[first + lane];
                    v0 = pd[(size_t)id0 * idStride];
                    lo = hi = v0;
                }
            } else {
                for (unsigned i = first + lane; i <= last; i += 64) {
                    const float v = pd[(size_t)ids[i] * idStride];
                    lo = fminf(lo, v);
                    hi = fmaxf(hi, v);
                }
            }
            lo = unif(wave_min(lo));
            hi = unif(wave_max(hi));
            if (lo == hi) {      // :187-191: m_dimId stays set
                if (lane == 0) out[me] = NodeDev{dim, 0.0f, count, 0u};
                break;
            }
            const float split = gen.uniform_real(lo, hi);      // :193
            // the left child: the elements below the split (:196-202 after the sort), kept in their order; the rest behind them
            unsigned nl = 0;
            if (small) {
                const bool on = (unsigned)lane < count;
                const bool left = on && v0 < split;
                const unsigned long long lm = __ballot(left), rm = __ballot(on && !left);
                nl = (unsigned)__popcll(lm);
                eao::wave_sync();
                if (on) ids[first + (left ? below(lm, lane) : nl + below(rm, lane))] = id0;
                eao::wave_sync();
            } else {
                unsigned nr = 0;
                for (unsigned base = first; base <= last; base += 64) {
                    const unsigned i = base + lane;
                    const bool on = i <= last;
                    unsigned short id = 0;
                    bool left = false;
                    if (on) {
                        id = ids[i];
                        left = pd[(size_t)id * idStride] < split;
                    }
                    const unsigned long long lm = __ballot(left), rm = __ballot(on && !left);
                    eao::wave_sync();
                    if (on) {
                        if (left) ids[first + nl + below(lm, lane)] = id;      // (at or before this chunk's first element: read already)
                        else tmp[nr + below(rm, lane)] = id;
                    }
                    nl += (unsigned)__popcll(lm);
                    nr += (unsigned)__popcll(rm);
                    eao::wave_sync();
                }
                for (unsigned j = lane; j < nr; j += 64) ids[first + nl + j] = tmp[j];
                eao::wave_sync();
            }
            nl = uni(nl);
            if (nl == 0) {      // :204-208: m_dimId and m_dimSplitValue stay set
                if (lane == 0) out[me] = NodeDev{dim, split, count, 0u};
                break;
            }
            if (nl == count) { bad = true; break; }      // the split came out above the maximum: upstream's right child is an empty range and Build fails (:167)
            if (lane == 0) {
                out[me] = NodeDev{dim, split, 0u, 0u};
                stk[sp * 4 + 0] = first + nl;
                stk[sp * 4 + 1] = last;
                stk[sp * 4 + 2] = depth + 1;
                stk[sp * 4 + 3] = me;
            }
            eao::wave_sync();
            sp++;
            last = first + nl - 1;
            depth++;
        }
        if (bad || sp == 0) break;
        sp--;
        first = uni(stk[sp * 4 + 0]);
        last = uni(stk[sp * 4 + 1]);
        depth = uni(stk[sp * 4 + 2]);
        const unsigned parent = uni(stk[sp * 4 + 3]);
        eao::wave_sync();
        if (lane == 0) out[parent].right = k;
    }
    if (lane == 0) {
        if (stamps) stamps[(size_t)g * 4 + 3] = wall_clock64();
        nodeCount[g] = k;
        if (bad) atomicOr(&failed[obj], 1u);
    }
}

// Node::GetPathLen (:272-287) and the sum of IsolationForest::GetAnomalyScores (:515-522): one wavefront per point, one lane per tree; lane 0 adds the path
// lengths in tree order, as upstream's loop does
constexpr int kScoreWaves = 4;
__global__ __launch_bounds__(64 * kScoreWaves) void k_iforest_score(const ObjDev* __restrict__ objs, const float* __restrict__ xyz, const NodeDev* __restrict__ nodes,
                                                                     const double* __restrict__ cTable, const unsigned* __restrict__ failed,
                                                                     double* __restrict__ totals) {
    __shared__ double pl[kScoreWaves][64];
    const ObjDev o = objs[blockIdx.y];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned i = blockIdx.x * kScoreWaves + wave;
    if (i >= o.n || failed[blockIdx.y]) return;      // (per wavefront: nothing below waits for another one)
    const float* p = xyz + ((size_t)o.ptStart + i) * 3;
    const float px = p[0], py = p[1], pz = p[2];
    const double* c = cTable + o.cBase;
    double total = 0.0;
    for (unsigned base = 0; base < o.treeCount; base += 64) {
        const unsigned t = base + lane;
        if (t < o.treeCount) {
            const NodeDev* nd = nodes + o.nodeBase + (size_t)t * o.stride;
            unsigned k = 0, depth = 0;
            NodeDev r = nd[0];
            while (r.size == 0) {
                const float v = r.dim == 0 ? px : (r.dim == 1 ? py : pz);
                k = v < r.split ? k + 1 : r.right;
                r = nd[k];
                depth++;
            }
            pl[wave][lane] = (double)depth + c[r.size];
        }
        eao::wave_sync();
        if (lane == 0) {
            const unsigned m = o.treeCount - base < 64u ? o.treeCount - base : 64u;
            for (unsigned q = 0; q < m; q++) total += pl[wave][q];
        }
        eao::wave_sync();
    }
    if (lane == 0) totals[(size_t)o.ptStart + i] = total;
}

}  // namespace

namespace eao {
namespace iforest {

hipError_t enqueue_build(hipStream_t stream, const ObjDev* objs, const unsigned* treeObj, const unsigned* seeds, const float* xyz, NodeDev* nodes, unsigned* nodeCount,
                         unsigned* failed, unsigned short* ws, unsigned long long* stamps, unsigned n_trees, size_t dyn_lds) {
    hipLaunchKernelGGL(k_iforest_build, dim3(n_trees), dim3(64), dyn_lds, stream, objs, treeObj, seeds, xyz, nodes, nodeCount, failed, ws, stamps);
    return hipGetLastError();
}

hipError_t enqueue_score(hipStream_t stream, const ObjDev* objs, const float* xyz, const NodeDev* nodes, const double* cTable, const unsigned* failed, double* totals,
                         unsigned max_n, unsigned n_obj) {
    hipLaunchKernelGGL(k_iforest_score, dim3(eao::cdiv((int)max_n, kScoreWaves), n_obj), dim3(64 * kScoreWaves), 0, stream, objs, xyz, nodes, cTable, failed, totals);
    return hipGetLastError();
}

}  // namespace iforest
}  // namespace eao

namespace {

struct Job {
    const float* xyz;      // n * 3, host
    uint32_t n, treeCount, seed, sampleSize;
};

struct ForestCtx : eao::ThreadStream {
    eao::DevBuf<unsigned char> dev;
    eao::DevBuf<NodeDev> nodes;
    eao::DevBuf<unsigned short> ws;
    eao::PinBuf<hipHostMallocDefault> host;
    eao::DevBuf<unsigned long long> stamps;
    eao::KernelClock<2> clock;          // k_iforest_build, k_iforest_score; armed, the build kernel also stamps its stages
    bool staged = false;
    double stageUs[3] = {0, 0, 0};      // seeding, shuffle and sample, the walk: mean over the trees of the last call
};
thread_local ForestCtx g_forest;

struct Built {
    std::vector<ObjDev> objs;
    std::vector<uint32_t> count;      // nodes per tree
    std::vector<uint32_t> failed;     // per job
    std::vector<double> totals;       // per point, jobs back to back
    std::vector<NodeDev> nodes;       // only when wanted
};

// Every job is valid (the callers checked).  One upload, the two kernels, one copy back.
eao_status run_forests(const std::vector<Job>& jobs, bool wantNodes, Built& B) {
    ForestCtx& ctx = g_forest;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const size_t nJobs = jobs.size();
    B.objs.assign(nJobs, ObjDev{});
    size_t nPts = 0, nTrees = 0, nNodes = 0, nWs = 0, nC = 0, dynLds = 0;
    uint32_t maxN = 0;
    for (size_t j = 0; j < nJobs; j++) {
        const Job& J = jobs[j];
        ObjDev& o = B.objs[j];
        const LdsPlan plan = lds_plan(J.n, J.sampleSize);
        o.ptStart = (uint32_t)nPts; o.n = J.n; o.sampleSize = J.sampleSize; o.maxDepth = max_depth(J.sampleSize);
        o.treeBase = (uint32_t)nTrees; o.treeCount = J.treeCount; o.inLds = plan.inLds ? 1u : 0u; o.idsBytes = (uint32_t)plan.idsBytes;
        o.nodeBase = nNodes; o.wsBase = nWs; o.cBase = (uint32_t)nC; o.stride = max_nodes(J.sampleSize);
        nPts += J.n;
        nTrees += J.treeCount;
        nNodes += (size_t)J.treeCount * o.stride;
        if (plan.inLds) dynLds = std::max(dynLds, plan.bytes);
        else nWs += (size_t)J.treeCount * (plan.idsBytes / 2);
        nC += (size_t)J.sampleSize + 1;
        maxN = std::max(maxN, J.n);
    }
    EAO_REQUIRE(nPts < (1u << 30) && nTrees < (1u << 30) && nC < (1u << 30) && nJobs <= 65535, "the batch is too large (points, trees or objects)");
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = eao::align256(off + bytes); return at; };
    const size_t oXyz = take(nPts * 12), oObj = take(nJobs * sizeof(ObjDev)), oTo = take(nTrees * 4), oSeed = take(nTrees * 4), oC = take(nC * 8),
                 oFail = take(nJobs * 4), inEnd = off;
    const size_t oTot = take(nPts * 8), oCnt = take(nTrees * 4), end = off;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    if ((st = ctx.nodes.reserve(nNodes))) return st;
    if ((st = ctx.ws.reserve(std::max<size_t>(nWs, 1)))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    for (size_t j = 0; j < nJobs; j++) {
        const Job& J = jobs[j];
        const ObjDev& o = B.objs[j];
        std::memcpy(h + oXyz + (size_t)o.ptStart * 12, J.xyz, (size_t)J.n * 12);
        uint32_t* to = (uint32_t*)(h + oTo) + o.treeBase;
        for (uint32_t t = 0; t < J.treeCount; t++) to[t] = (uint32_t)j;
        tree_seeds(J.seed, J.treeCount, (uint32_t*)(h + oSeed) + o.treeBase);
        double* c = (double*)(h + oC) + o.cBase;
        for (uint32_t s = 0; s <= J.sampleSize; s++) c[s] = c_of(s);
    }
    std::memcpy(h + oObj, B.objs.data(), nJobs * sizeof(ObjDev));
    std::memset(h + oFail, 0, nJobs * 4);
    const bool profiling = ctx.clock.armed();
    if (profiling && (st = ctx.stamps.reserve(nTrees * 4))) return st;
    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    ctx.clock.mark(0, ctx.stream);
    // (the scores are not launched over trees that were not built)
    EAO_HIP(enqueue_build(ctx.stream, (const ObjDev*)(d + oObj), (const unsigned*)(d + oTo), (const unsigned*)(d + oSeed), (const float*)(d + oXyz), ctx.nodes.p,
                          (unsigned*)(d + oCnt), (unsigned*)(d + oFail), ctx.ws.p, profiling ? ctx.stamps.p : nullptr, (unsigned)nTrees, dynLds));
    ctx.clock.mark(1, ctx.stream);
    EAO_HIP(enqueue_score(ctx.stream, (const ObjDev*)(d + oObj), (const float*)(d + oXyz), (const NodeDev*)ctx.nodes.p, (const double*)(d + oC), (const unsigned*)(d + oFail),
                          (double*)(d + oTot), maxN, (unsigned)nJobs));
    ctx.clock.mark(2, ctx.stream);
    EAO_HIP(hipMemcpyAsync(h + oFail, d + oFail, end - oFail, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    ctx.clock.collect();
    if (profiling) {
        std::vector<unsigned long long> t(nTrees * 4);
        EAO_HIP(hipMemcpy(t.data(), ctx.stamps.p, t.size() * 8, hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; k++) {
            double sum = 0;
            for (size_t g = 0; g < nTrees; g++) sum += (double)(t[g * 4 + k + 1] - t[g * 4 + k]);
            ctx.stageUs[k] = sum / (double)nTrees / 100.0;      // 100 MHz ticks
        }
        ctx.staged = true;
    }
    B.failed.assign((const uint32_t*)(h + oFail), (const uint32_t*)(h + oFail) + nJobs);
    B.totals.assign((const double*)(h + oTot), (const double*)(h + oTot) + nPts);
    B.count.assign((const uint32_t*)(h + oCnt), (const uint32_t*)(h + oCnt) + nTrees);
    if (wantNodes) {
        B.nodes.resize(nNodes);
        if (nNodes) EAO_HIP(hipMemcpy(B.nodes.data(), ctx.nodes.p, nNodes * sizeof(NodeDev), hipMemcpyDeviceToHost));
    }
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_iforest_scores_batch(int32_t n_obj, const int32_t* start, const float* xyz, const int32_t* tree_count, const uint32_t* seed,
                                    const int32_t* sample_size, double* scores, double* total_path_len, uint8_t* stream, int64_t stream_cap,
                                    int64_t* stream_start) {
    EAO_REQUIRE(n_obj >= 0, "n_obj < 0");
    if (n_obj == 0) {
        if (stream_start) stream_start[0] = 0;
        return EAO_OK;
    }
    EAO_REQUIRE(start && xyz && tree_count && seed && sample_size && scores, "null argument");
    EAO_REQUIRE(!stream || stream_start, "stream without stream_start");
    EAO_REQUIRE(start[0] >= 0, "start[0] < 0");
    std::vector<Job> jobs((size_t)n_obj);
    for (int j = 0; j < n_obj; j++) {
        EAO_REQUIRE(start[j] <= start[j + 1], "start does not ascend at object %d", j);
        const int64_t n = (int64_t)start[j + 1] - start[j];
        const char* why = refusal(n, sample_size[j], tree_count[j]);
        EAO_REQUIRE(!why, "object %d: %s", j, why);
        EAO_REQUIRE(all_finite(xyz + (size_t)start[j] * 3, (size_t)n), "object %d has a non-finite coordinate", j);
        jobs[j] = Job{xyz + (size_t)start[j] * 3, (uint32_t)n, (uint32_t)tree_count[j], seed[j], (uint32_t)sample_size[j]};
    }
    Built B;
    const eao_status st = run_forests(jobs, stream_start != nullptr && stream != nullptr, B);
    if (st) return st;
    for (int j = 0; j < n_obj; j++)
        EAO_REQUIRE(!B.failed[j], "object %d: a split came out above the maximum of its range; upstream's Build fails there (include/isolation_forest.h:167)", j);
    if (stream_start) {
        std::vector<int64_t> at((size_t)n_obj + 1, 0);
        for (int j = 0; j < n_obj; j++) {
            size_t nodes = 0;
            for (uint32_t t = 0; t < jobs[j].treeCount; t++) nodes += B.count[B.objs[j].treeBase + t];
            at[j + 1] = at[j] + (int64_t)stream_bytes(jobs[j].treeCount, nodes);
        }
        if (stream && at[n_obj] > stream_cap) {
            std::memcpy(stream_start, at.data(), at.size() * 8);      // (what the caller needs to size the buffer; nothing else is written)
            eao::set_error("the streams take %lld bytes, the buffer holds %lld", (long long)at[n_obj], (long long)stream_cap);
            return EAO_ERR_CAPACITY;
        }
        std::memcpy(stream_start, at.data(), at.size() * 8);
        if (stream)
            for (int j = 0; j < n_obj; j++)
                write_stream(stream + at[j], jobs[j].treeCount, jobs[j].sampleSize, B.nodes.data() + B.objs[j].nodeBase, B.objs[j].stride,
                             B.count.data() + B.objs[j].treeBase);
    }
    for (int j = 0; j < n_obj; j++) {
        const double cS = c_of(jobs[j].sampleSize);
        const double* tot = B.totals.data() + B.objs[j].ptStart;
        for (uint32_t i = 0; i < jobs[j].n; i++) scores[(size_t)start[j] + i] = finish_score(tot[i], jobs[j].treeCount, cS);
        if (total_path_len) std::memcpy(total_path_len + (size_t)start[j], tot, (size_t)jobs[j].n * 8);
    }
    return EAO_OK;
}

eao_status eao_object_iforest_outliers_batch(int32_t n_obj, const int32_t* start, const float* xyz, const int32_t* class_id, int32_t bi_forest, uint8_t* flags,
                                             int32_t* removed, double* scores) {
    EAO_REQUIRE(n_obj >= 0, "n_obj < 0");
    if (n_obj == 0) return EAO_OK;
    EAO_REQUIRE(start && class_id && flags && removed, "null argument");
    EAO_REQUIRE(start[0] >= 0, "start[0] < 0");
    std::vector<Job> jobs;
    std::vector<int> owner;
    for (int j = 0; j < n_obj; j++) {
        EAO_REQUIRE(start[j] <= start[j + 1], "start does not ascend at object %d", j);
        const int64_t n = (int64_t)start[j + 1] - start[j];
        if (!object_runs(bi_forest != 0, class_id[j], (size_t)n)) continue;
        EAO_REQUIRE(xyz, "xyz is NULL");
        const int64_t sampleSize = n / kSampleDivisor;
        const char* why = refusal(n, sampleSize, kTreeCount);
        EAO_REQUIRE(!why, "object %d: %s", j, why);
        EAO_REQUIRE(all_finite(xyz + (size_t)start[j] * 3, (size_t)n), "object %d has a non-finite coordinate", j);
        jobs.push_back(Job{xyz + (size_t)start[j] * 3, (uint32_t)n, kTreeCount, kSeed, (uint32_t)sampleSize});
        owner.push_back(j);
    }
    Built B;
    if (!jobs.empty()) {
        const eao_status st = run_forests(jobs, false, B);
        if (st) return st;
    }
    const size_t total = (size_t)start[n_obj] - start[0];
    std::memset(flags + start[0], 0, total);
    for (int j = 0; j < n_obj; j++) removed[j] = 0;
    if (scores)
        for (size_t i = 0; i < total; i++) scores[(size_t)start[0] + i] = -1.0;      // (an object the rules skip has no forest: GetAnomalyScore's own answer, :483-486)
    for (size_t q = 0; q < jobs.size(); q++) {
        if (B.failed[q]) continue;      // upstream prints "Failed to build Isolation Forest." and returns (:1296-1300)
        const int j = owner[q];
        const double cS = c_of(jobs[q].sampleSize), th = object_threshold(class_id[j]);
        const double* tot = B.totals.data() + B.objs[q].ptStart;
        const size_t at = (size_t)start[j];
        for (uint32_t i = 0; i < jobs[q].n; i++) {
            const double s = finish_score(tot[i], kTreeCount, cS);
            if (scores) scores[at + i] = s;
            if (s > th) {      // :1317
                flags[at + i] = 1;
                removed[j]++;
            }
        }
    }
    return EAO_OK;
}

eao_status eao_iforest_set_profiling(int32_t on) {
    g_forest.clock.arm(on != 0);
    g_forest.staged = false;
    return EAO_OK;
}

eao_status eao_iforest_last_kernel_ms(float* kernel_ms) {
    EAO_REQUIRE(kernel_ms, "null argument");
    return g_forest.clock.read(kernel_ms, "no measurement on this thread: eao_iforest_set_profiling(1) and a forest call come first");
}

eao_status eao_iforest_last_stage_us(double* stage_us) {
    EAO_REQUIRE(stage_us, "null argument");
    EAO_REQUIRE(g_forest.staged, "no measurement on this thread: eao_iforest_set_profiling(1) and a forest call come first");
    for (int k = 0; k < 3; k++) stage_us[k] = g_forest.stageUs[k];
    return EAO_OK;
}

}  // extern "C"
