// vocabulary.hip -- ORBVocabulary on the device: the DBoW2 tree descent, the BowVector / FeatureVector assembly and L1 scoring
// (include/eao_fusion.h, "ORBVocabulary"; reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1138-1271, BowVector.cpp, FeatureVector.cpp, ScoringObject.cpp:23-68).
//
// Two kernels per transform call, whatever the number of frames:
//   k_voc_descend   16 lanes per descriptor (four descriptors per wavefront): each lane takes one child of the current node (two 16-byte loads, xor + popcount over
//                   8 words), the group's argmin over (distance, child position) goes through shuffles; a node with more than 16 children is walked in chunks.
//                   The levels of one descent are dependent loads; what hides them is the number of descents in flight (1000 features = 250 wavefronts).
//   k_voc_assemble  one workgroup per frame: a bitonic sort of (node id, feature index) keys in LDS gives the FeatureVector, one of (word id, feature index) the
//                   BowVector; segment heads become the CSR arrays; ONE lane walks a word's segment with upstream's c - 1 sequential additions, and one lane sums
//                   the norm in ascending word id.  No atomics on doubles anywhere: every double is a single IEEE operation in upstream's order.
// k_bow_score_l1: one wavefront per stored vector; every lane looks one of its entries up in the query (binary search), the terms of the common words are then
// added in ascending word id (the same sequence in every lane).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "bow_intersect.h"
#include "common.h"
#include "vocabulary_internal.h"

using eao::voc::NodeMeta;

struct eao_vocabulary {
    int32_t n_nodes = 0, n_words = 0, depth = 0, max_children = 0, weighting = 0, norm = 0;
    eao::DevBuf<uint4> desc;       // 2 per slot
    eao::DevBuf<int4> meta;        // NodeMeta per slot
    eao::DevBuf<double> weight;    // per slot
};

namespace {

typedef unsigned long long u64;
constexpr int kGroup = 16;              // lanes per descriptor
constexpr int kDescendBlock = 256;      // 16 descriptors per workgroup
constexpr u64 kNoKey = ~0ull;           // a stopped feature / padding: sorts behind every key

struct DescendArgs {
    const uint4* nodeDesc;
    const int4* meta;
    const double* weight;
    const uint4* desc;          // the features, 2 x uint4 each
    const int* frameStart;      // n_frames + 1
    const int* dN;              // NULL, or the device-resident count of frame 0
    int nidLevel;               // depth - levelsup
    unsigned* fword;
    unsigned* fnode;
    unsigned char* fstop;
    double* fweight;
};

__device__ __forceinline__ int frame_count(const int* frameStart, const int* dN, int f, bool* bad) {
    int n = frameStart[f + 1] - frameStart[f];
    *bad = false;
    if (dN) {
        const int dn = *dN;
        *bad = dn < 0 || dn > n;
        n = *bad ? 0 : dn;
    }
    return n;
}

__global__ __launch_bounds__(kDescendBlock) void k_voc_descend(DescendArgs a) {
    const int f = blockIdx.y;
    bool bad;
    const int n = frame_count(a.frameStart, a.dN, f, &bad);
    const int sub = threadIdx.x & (kGroup - 1);
    const int i = blockIdx.x * (kDescendBlock / kGroup) + (threadIdx.x >> 4);
    if (i >= n) return;      // (a whole group leaves together)
    const size_t gi = (size_t)a.frameStart[f] + i;
    const uint4 q0 = a.desc[gi * 2], q1 = a.desc[gi * 2 + 1];
    int cur = 0, level = 0;
    unsigned nid = 0;
    bool have = a.nidLevel <= 0;      // :1239: the root
    int4 m = a.meta[0];
    while (m.y > 0) {      // :1244-1266, until a node without children
        level++;
        u64 best = kNoKey;
        for (int c0 = 0; c0 < m.y; c0 += kGroup) {
            const int c = c0 + sub;
            if (c < m.y) {
                const uint4* d = a.nodeDesc + (size_t)(m.x + c) * 2;
                const uint4 d0 = d[0], d1 = d[1];
                const unsigned dist = __popc(q0.x ^ d0.x) + __popc(q0.y ^ d0.y) + __popc(q0.z ^ d0.z) + __popc(q0.w ^ d0.w) + __popc(q1.x ^ d1.x) +
                                      __popc(q1.y ^ d1.y) + __popc(q1.z ^ d1.z) + __popc(q1.w ^ d1.w);
                const u64 key = ((u64)dist << 32) | (unsigned)c;      // the smaller position wins among equal distances: strict < in id order (:1256)
                best = key < best ? key : best;
            }
        }
#pragma unroll
        for (int o = kGroup / 2; o > 0; o >>= 1) {
            const unsigned hi = __shfl_xor((unsigned)(best >> 32), o, kGroup), lo = __shfl_xor((unsigned)best, o, kGroup);
            const u64 other = ((u64)hi << 32) | lo;
            best = other < best ? other : best;
        }
        cur = m.x + (int)(unsigned)best;
        m = a.meta[cur];
        if (level == a.nidLevel) {      // :1263
            nid = (unsigned)m.z;
            have = true;
        }
    }
    if (sub == 0) {
        const double w = a.weight[cur];
        unsigned char st = w > 0 ? 0 : 1;      // :1169 `if(w > 0)`: a NaN weight is stopped too
        if (!have) {      // the leaf lies above nid_level: upstream's nid is uninitialised here; defined as the leaf's id and flagged
            nid = (unsigned)m.z;
            st |= 2;
        }
        a.fword[gi] = (unsigned)m.w;
        a.fnode[gi] = nid;
        a.fstop[gi] = st;
        a.fweight[gi] = w;
    }
}

struct AssembleArgs {
    const int* frameStart;
    const int* dN;
    int weighting, norm, n2;      // n2: the power of two the keys are padded to
    const unsigned* fword;
    const unsigned* fnode;
    const unsigned char* fstop;
    const double* fweight;
    unsigned* wordId;
    double* wordVal;
    unsigned* nodeId;
    int* nodeStart;      // frame f's n + 1 entries start at frameStart[f] + f
    unsigned* index;
    int* hdr;            // per frame: n_words, n_fv_nodes, n_features, status
};

__device__ void voc_fill_keys(u64* keys, int n2, int n, const unsigned* key32, const unsigned char* fstop) {
    for (int p = threadIdx.x; p < n2; p += blockDim.x) keys[p] = (p < n && !(fstop[p] & 1)) ? (((u64)key32[p] << 32) | (unsigned)p) : kNoKey;
    __syncthreads();
}

// the keys are distinct but for the padding, so the order is the stable order of (key32, feature index)
__device__ void voc_sort(u64* keys, int n2) {
    for (int size = 2; size <= n2; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n2 >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const bool up = (i & size) == 0;
                const u64 x = keys[i], y = keys[l];
                if ((x > y) == up && x != y) {
                    keys[i] = y;
                    keys[l] = x;
                }
            }
            __syncthreads();
        }
}

// Thread t owns positions t * e .. t * e + e - 1 of the sorted keys.  Returns the number of segment heads (a position whose high word differs from its
// predecessor's) before its first position; *total = all heads.
__device__ int voc_heads_before(const u64* keys, int kept, int e, int* sWave, int* total) {
    const int p0 = threadIdx.x * e;
    int cnt = 0;
    for (int p = p0; p < p0 + e && p < kept; p++) cnt += (p == 0 || (unsigned)(keys[p] >> 32) != (unsigned)(keys[p - 1] >> 32)) ? 1 : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    __syncthreads();      // (sWave may still be read from the previous scan)
    if (lane == 63) sWave[wave] = incl;
    __syncthreads();
    int base = 0, all = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) {
        const int v = sWave[w];
        if (w < wave) base += v;
        all += v;
    }
    *total = all;
    return base + incl - cnt;
}

__global__ __launch_bounds__(1024) void k_voc_assemble(AssembleArgs a) {
    extern __shared__ __align__(16) unsigned char vsm[];
    __shared__ int sWave[16];
    __shared__ int sKept;
    __shared__ int sDivide;
    __shared__ double sNorm;
    u64* keys = (u64*)vsm;
    double* vals = (double*)(vsm + (size_t)a.n2 * 8);
    const int f = blockIdx.x, s0 = a.frameStart[f];
    bool bad;
    const int n = frame_count(a.frameStart, a.dN, f, &bad);
    const int e = a.n2 / (int)blockDim.x;

    // ---- FeatureVector (FeatureVector.cpp:31-45): node ids ascend, each node's indices ascend
    if (threadIdx.x == 0) sKept = 0;
    voc_fill_keys(keys, a.n2, n, a.fnode + s0, a.fstop + s0);
    voc_sort(keys, a.n2);
    for (int p = threadIdx.x; p < a.n2; p += blockDim.x)
        if (keys[p] != kNoKey && (p + 1 == a.n2 || keys[p + 1] == kNoKey)) sKept = p + 1;
    __syncthreads();
    const int kept = sKept;
    int total;
    int ord = voc_heads_before(keys, kept, e, sWave, &total);
    for (int p = threadIdx.x * e; p < threadIdx.x * e + e && p < kept; p++) {
        const u64 k = keys[p];
        a.index[s0 + p] = (unsigned)k;
        if (p == 0 || (unsigned)(k >> 32) != (unsigned)(keys[p - 1] >> 32)) {
            a.nodeId[s0 + ord] = (unsigned)(k >> 32);
            a.nodeStart[s0 + f + ord] = p;
            ord++;
        }
    }
    if (threadIdx.x == 0) {
        a.nodeStart[s0 + f + total] = kept;
        a.hdr[f * 4 + 1] = total;
        a.hdr[f * 4 + 2] = n;
        a.hdr[f * 4 + 3] = bad ? 1 : 0;
    }
    __syncthreads();

    // ---- BowVector: word ids ascend (std::map order); a word's value is built by ONE lane in feature order
    voc_fill_keys(keys, a.n2, n, a.fword + s0, a.fstop + s0);
    voc_sort(keys, a.n2);
    ord = voc_heads_before(keys, kept, e, sWave, &total);
    const bool tf = a.weighting <= 1;      // TF_IDF, TF: addWeight; IDF, BINARY: addIfNotExist
    for (int p = threadIdx.x * e; p < threadIdx.x * e + e && p < kept; p++) {
        const u64 k = keys[p];
        const unsigned wid = (unsigned)(k >> 32);
        if (p == 0 || wid != (unsigned)(keys[p - 1] >> 32)) {
            const double w = a.fweight[s0 + (int)(unsigned)k];      // (every feature of the word carries the word's weight)
            double v = w;
            if (tf)
                for (int q = p + 1; q < kept && (unsigned)(keys[q] >> 32) == wid; q++) v += w;      // BowVector.cpp:40: ((w + w) + w) + ...
            a.wordId[s0 + ord] = wid;
            vals[ord] = v;
            ord++;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.hdr[f * 4 + 0] = total;
        double nv = 0.0;
        int divide = 0;
        if (a.norm == 0) {
            if (tf && total > 0) {      // :1176-1182
                nv = (double)total;
                divide = 1;
            }
        } else {
            if (a.norm == 1) {
#pragma unroll 8
                for (int o = 0; o < total; o++) nv += fabs(vals[o]);      // BowVector.cpp:69-70
            } else {
#pragma unroll 8
                for (int o = 0; o < total; o++) nv += vals[o] * vals[o];      // :74-76
                nv = sqrt(nv);
            }
            divide = nv > 0.0 ? 1 : 0;      // :79
        }
        sNorm = nv;
        sDivide = divide;
    }
    __syncthreads();
    const double nv = sNorm;
    const bool divide = sDivide != 0;
    for (int o = threadIdx.x; o < total; o += blockDim.x) a.wordVal[s0 + o] = divide ? vals[o] / nv : vals[o];
}

__global__ __launch_bounds__(256) void k_bow_score_l1(int nq, const unsigned* qId, const double* qVal, int nDb, const int* dbStart, const unsigned* dbId,
                                                      const double* dbVal, double* scores) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= nDb) return;      // (a whole wavefront leaves together)
    const int b = dbStart[j], e = dbStart[j + 1];
    int common = 0;
    unsigned firstWord = 0;
    const double s = eao::bow_l1_pair<false>(nq, qId, qVal, dbId, dbVal, b, e, lane, common, firstWord);
    if (lane == 0) scores[j] = -s / 2.0;      // :65 (no common word: -0.0)
}

struct VocCtx : eao::ThreadStream {
    eao::DevBuf<unsigned char> dev;
    eao::PinBuf<hipHostMallocDefault> host;
};
thread_local VocCtx g_voc;

struct Layout {
    size_t desc, fs, fweight, outBegin, fword, fnode, fstop, wid, wval, nid, nst, idx, hdr, end, inEnd;
    Layout(size_t N, size_t nf, bool hostDesc) {
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t at = o; o = eao::align256(o + bytes); return at; };
        desc = take(hostDesc ? N * 32 : 0);
        fs = take((nf + 1) * 4);
        inEnd = o;
        fweight = take(N * 8);
        outBegin = o;
        fword = take(N * 4);
        fnode = take(N * 4);
        fstop = take(N);
        wid = take(N * 4);
        wval = take(N * 8);
        nid = take(N * 4);
        nst = take((N + nf) * 4);
        idx = take(N * 4);
        hdr = take(nf * 16);
        end = o;
    }
};

void write_empty(eao_bow_result* r, int n) {
    r->n_words = 0;
    r->n_fv_nodes = 0;
    if (r->node_start) r->node_start[0] = 0;
    if (r->feat_word && n > 0) std::memset(r->feat_word, 0, (size_t)n * 4);
    if (r->feat_node && n > 0) std::memset(r->feat_node, 0, (size_t)n * 4);
    if (r->feat_stopped && n > 0) std::memset(r->feat_stopped, 0, (size_t)n);
}

// the common path: nf frames over host descriptors (desc) or ONE frame over device descriptors (dDesc, dN; frameStart = {0, cap})
eao_status transform(const eao_vocabulary* voc, int nf, const uint8_t* desc, const uint8_t* dDesc, const int32_t* dN, const int32_t* frameStart, int32_t levelsup,
                     eao_bow_result* results, hipStream_t callerStream, bool useCallerStream) {
    EAO_REQUIRE(voc, "voc is NULL");
    EAO_REQUIRE(levelsup >= 0, "levelsup < 0");
    EAO_REQUIRE(nf >= 0 && (nf == 0 || (frameStart && results)), "bad argument");
    if (nf == 0) return EAO_OK;
    EAO_REQUIRE(frameStart[0] == 0, "frame_start[0] != 0");
    int maxn = 0;
    for (int f = 0; f < nf; f++) {
        const long long n = (long long)frameStart[f + 1] - frameStart[f];
        EAO_REQUIRE(n >= 0, "frame_start does not ascend at frame %d", f);
        EAO_REQUIRE(n <= EAO_VOCABULARY_MAX_FEATURES, "frame %d has %lld features; at most %d per frame are supported", f, n, EAO_VOCABULARY_MAX_FEATURES);
        EAO_REQUIRE(results[f].node_start, "results[%d].node_start is NULL", f);
        EAO_REQUIRE(n == 0 || (results[f].word_id && results[f].word_value && results[f].node_id && results[f].index), "a result array of frame %d is NULL", f);
        maxn = std::max(maxn, (int)n);
    }
    const size_t N = (size_t)frameStart[nf];
    EAO_REQUIRE(N == 0 || desc || dDesc, "descriptors are NULL");
    EAO_REQUIRE(!dDesc || (dN && ((uintptr_t)dDesc & 15) == 0), "device descriptors must be 16-byte aligned and come with their count");
    if (voc->n_nodes == 0 || N == 0) {      // empty() (:1146) / nothing to transform
        for (int f = 0; f < nf; f++) write_empty(&results[f], frameStart[f + 1] - frameStart[f]);
        return EAO_OK;
    }
    VocCtx& ctx = g_voc;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const hipStream_t stream = useCallerStream ? callerStream : ctx.stream;
    const Layout L(N, (size_t)nf, desc != nullptr);
    if ((st = ctx.dev.reserve(L.end))) return st;
    if ((st = ctx.host.reserve(L.end))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    int n2 = 128;
    while (n2 < maxn) n2 <<= 1;
    const int block = std::min(1024, std::max(64, n2 / 2));
    const size_t lds = (size_t)n2 * 16;
    static std::once_flag once;
    static hipError_t attrErr = hipSuccess;
    std::call_once(once, [] { attrErr = hipFuncSetAttribute((const void*)k_voc_assemble, hipFuncAttributeMaxDynamicSharedMemorySize, EAO_VOCABULARY_MAX_FEATURES * 16); });
    EAO_HIP(attrErr);

    if (desc) std::memcpy(h + L.desc, desc, N * 32);
    std::memcpy(h + L.fs, frameStart, ((size_t)nf + 1) * 4);
    eao::Drain drain(stream);
    EAO_HIP(hipMemcpyAsync(d, h, L.inEnd, hipMemcpyHostToDevice, stream));
    DescendArgs da;
    da.nodeDesc = voc->desc.p;
    da.meta = voc->meta.p;
    da.weight = voc->weight.p;
    da.desc = desc ? (const uint4*)(d + L.desc) : (const uint4*)dDesc;
    da.frameStart = (const int*)(d + L.fs);
    da.dN = dN;
    da.nidLevel = voc->depth - levelsup;
    da.fword = (unsigned*)(d + L.fword);
    da.fnode = (unsigned*)(d + L.fnode);
    da.fstop = d + L.fstop;
    da.fweight = (double*)(d + L.fweight);
    AssembleArgs aa;
    aa.frameStart = da.frameStart;
    aa.dN = dN;
    aa.weighting = voc->weighting;
    aa.norm = voc->norm;
    aa.n2 = n2;
    aa.fword = da.fword;
    aa.fnode = da.fnode;
    aa.fstop = da.fstop;
    aa.fweight = da.fweight;
    aa.wordId = (unsigned*)(d + L.wid);
    aa.wordVal = (double*)(d + L.wval);
    aa.nodeId = (unsigned*)(d + L.nid);
    aa.nodeStart = (int*)(d + L.nst);
    aa.index = (unsigned*)(d + L.idx);
    aa.hdr = (int*)(d + L.hdr);
    {
        eao::Range r("vocabulary_transform");
        hipLaunchKernelGGL(k_voc_descend, dim3(eao::cdiv(maxn, kDescendBlock / kGroup), nf), dim3(kDescendBlock), 0, stream, da);
        hipLaunchKernelGGL(k_voc_assemble, dim3(nf), dim3(block), lds, stream, aa);
    }
    EAO_HIP(hipGetLastError());
    EAO_HIP(hipMemcpyAsync(h + L.outBegin, d + L.outBegin, L.end - L.outBegin, hipMemcpyDeviceToHost, stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));

    const int* hdr = (const int*)(h + L.hdr);
    for (int f = 0; f < nf; f++) EAO_REQUIRE(hdr[f * 4 + 3] == 0, "the device-resident count is outside 0 .. cap = %d", frameStart[f + 1] - frameStart[f]);
    for (int f = 0; f < nf; f++) {
        eao_bow_result& r = results[f];
        const size_t s0 = (size_t)frameStart[f];
        const int nw = hdr[f * 4 + 0], nn = hdr[f * 4 + 1], n = hdr[f * 4 + 2];
        const int* nst = (const int*)(h + L.nst) + s0 + f;
        r.n_words = nw;
        r.n_fv_nodes = nn;
        if (nw > 0) {
            std::memcpy(r.word_id, (const unsigned*)(h + L.wid) + s0, (size_t)nw * 4);
            std::memcpy(r.word_value, (const double*)(h + L.wval) + s0, (size_t)nw * 8);
        }
        std::memcpy(r.node_start, nst, ((size_t)nn + 1) * 4);
        if (nn > 0) {
            std::memcpy(r.node_id, (const unsigned*)(h + L.nid) + s0, (size_t)nn * 4);
            std::memcpy(r.index, (const unsigned*)(h + L.idx) + s0, (size_t)nst[nn] * 4);
        }
        if (n > 0) {
            if (r.feat_word) std::memcpy(r.feat_word, (const unsigned*)(h + L.fword) + s0, (size_t)n * 4);
            if (r.feat_node) std::memcpy(r.feat_node, (const unsigned*)(h + L.fnode) + s0, (size_t)n * 4);
            if (r.feat_stopped) std::memcpy(r.feat_stopped, h + L.fstop + s0, (size_t)n);
        }
    }
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_vocabulary_create(const eao_vocabulary_desc* desc, eao_vocabulary** out) {
    EAO_REQUIRE(out, "out is NULL");
    eao::voc::Table t;
    std::string err;
    EAO_REQUIRE(eao::voc::flatten(desc, t, err), "eao_vocabulary_create: %s", err.c_str());
    eao_vocabulary* v = new eao_vocabulary;
    v->n_nodes = t.n_nodes;
    v->n_words = t.n_words;
    v->depth = t.depth;
    v->max_children = t.max_children;
    v->weighting = t.weighting;
    v->norm = t.norm;
    if (t.n_nodes > 0) {
        eao_status st = eao::require_device();
        const size_t slots = (size_t)t.n_nodes + 1;
        if (!st) st = v->desc.reserve(slots * 2);
        if (!st) st = v->meta.reserve(slots);
        if (!st) st = v->weight.reserve(slots);
        hipError_t e = hipSuccess;
        if (!st) e = hipMemcpy(v->desc.p, t.descriptor.data(), slots * 32, hipMemcpyHostToDevice);
        if (!st && e == hipSuccess) e = hipMemcpy(v->meta.p, t.meta.data(), slots * sizeof(NodeMeta), hipMemcpyHostToDevice);
        if (!st && e == hipSuccess) e = hipMemcpy(v->weight.p, t.weight.data(), slots * 8, hipMemcpyHostToDevice);
        if (st || e != hipSuccess) {
            delete v;
            if (st) return st;
            EAO_HIP(e);
        }
    }
    *out = v;
    return EAO_OK;
}

void eao_vocabulary_destroy(eao_vocabulary* voc) { delete voc; }

eao_status eao_vocabulary_info(const eao_vocabulary* voc, int32_t* n_nodes, int32_t* n_words, int32_t* depth, int32_t* max_children) {
    EAO_REQUIRE(voc, "voc is NULL");
    if (n_nodes) *n_nodes = voc->n_nodes;
    if (n_words) *n_words = voc->n_words;
    if (depth) *depth = voc->depth;
    if (max_children) *max_children = voc->max_children;
    return EAO_OK;
}

eao_status eao_vocabulary_transform(const eao_vocabulary* voc, const uint8_t* desc, int32_t n, int32_t levelsup, eao_bow_result* result) {
    EAO_REQUIRE(n >= 0 && result, "bad argument");
    const int32_t fs[2] = {0, n};
    return transform(voc, 1, desc, nullptr, nullptr, fs, levelsup, result, nullptr, false);
}

eao_status eao_vocabulary_transform_batch(const eao_vocabulary* voc, int32_t n_frames, const uint8_t* desc, const int32_t* frame_start, int32_t levelsup,
                                          eao_bow_result* results) {
    return transform(voc, n_frames, desc, nullptr, nullptr, frame_start, levelsup, results, nullptr, false);
}

eao_status eao_vocabulary_transform_device(const eao_vocabulary* voc, const uint8_t* d_desc, const int32_t* d_n, int32_t cap, int32_t levelsup,
                                           eao_bow_result* result, void* stream) {
    EAO_REQUIRE(cap >= 0 && result && d_desc && d_n, "bad argument");
    const int32_t fs[2] = {0, cap};
    return transform(voc, 1, nullptr, d_desc, d_n, fs, levelsup, result, (hipStream_t)stream, true);
}

eao_status eao_bow_score_l1(int32_t nq, const uint32_t* q_id, const double* q_val, int32_t n_db, const int32_t* db_start, const uint32_t* db_id,
                            const double* db_val, double* scores) {
    EAO_REQUIRE(nq >= 0 && n_db >= 0 && (nq == 0 || (q_id && q_val)) && (n_db == 0 || (db_start && scores)), "bad argument");
    for (int i = 1; i < nq; i++) EAO_REQUIRE(q_id[i - 1] < q_id[i], "the query's word ids do not ascend strictly at entry %d", i);
    if (n_db == 0) return EAO_OK;
    EAO_REQUIRE(db_start[0] >= 0, "db_start[0] < 0");
    for (int j = 0; j < n_db; j++) {
        EAO_REQUIRE(db_start[j] <= db_start[j + 1], "db_start does not ascend at vector %d", j);
        EAO_REQUIRE(db_start[j] == db_start[j + 1] || (db_id && db_val), "db_id / db_val are NULL");
        for (int c = db_start[j] + 1; c < db_start[j + 1]; c++) EAO_REQUIRE(db_id[c - 1] < db_id[c], "the word ids of stored vector %d do not ascend strictly", j);
    }
    VocCtx& ctx = g_voc;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const size_t b0 = (size_t)db_start[0], M = (size_t)db_start[n_db] - b0;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = eao::align256(o + bytes); return at; };
    const size_t oQi = take((size_t)nq * 4), oQv = take((size_t)nq * 8), oSt = take(((size_t)n_db + 1) * 4), oDi = take(M * 4), oDv = take(M * 8), inEnd = o;
    const size_t oSc = take((size_t)n_db * 8), end = o;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    if (nq > 0) {
        std::memcpy(h + oQi, q_id, (size_t)nq * 4);
        std::memcpy(h + oQv, q_val, (size_t)nq * 8);
    }
    int* hs = (int*)(h + oSt);
    for (int j = 0; j <= n_db; j++) hs[j] = db_start[j] - (int)b0;
    if (M > 0) {
        std::memcpy(h + oDi, db_id + b0, M * 4);
        std::memcpy(h + oDv, db_val + b0, M * 8);
    }
    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    hipLaunchKernelGGL(k_bow_score_l1, dim3(eao::cdiv(n_db, 4)), dim3(256), 0, ctx.stream, nq, (const unsigned*)(d + oQi), (const double*)(d + oQv), n_db,
                       (const int*)(d + oSt), (const unsigned*)(d + oDi), (const double*)(d + oDv), (double*)(d + oSc));
    EAO_HIP(hipGetLastError());
    EAO_HIP(hipMemcpyAsync(h + oSc, d + oSc, (size_t)n_db * 8, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    std::memcpy(scores, h + oSc, (size_t)n_db * 8);
    return EAO_OK;
}

}  // extern "C"
