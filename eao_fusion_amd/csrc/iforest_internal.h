// iforest_internal.h -- the host half of the isolation forest of Object_Map::IsolationForestDeleteOutliers (reference src/Object.cc:1239-1348,
// include/isolation_forest.h).  HIP-free: csrc/iforest.hip includes it for the rules, the tables and the stream layout; tools/isolation_forest_walk.cpp
// includes it alone, builds the forest on the host with it and runs under the sanitizers.
//
// The result upstream computes is defined by libstdc++ (g++ 11) as much as by the reference header, so the algorithms are restated here by name:
//   Mt19937        std::mt19937: seeding recurrence, twist, tempering (bits/random.tcc)
//   lemire         uniform_int_distribution, downscaling branch over a 32-bit engine (bits/uniform_int_dist.h _S_nd): 64-bit product, reject while the low half
//                  is below -range % range
//   shuffle_ids    std::shuffle's two-swaps-per-draw path (bits/stl_algo.h, __gen_two_uniform_ints); it holds while N * N <= 2^32, hence kMaxPoints
//   canonical      generate_canonical<float, 24>: ONE draw converted to float, divided by 2^32, clamped to nextafter(1, 0)
//   uniform_real   u * (b - a) + a in float, rounded operation by operation (-ffp-contract=off)
// The kernels of iforest.hip restate the same five for the device; tests/isolation_forest_reference.py restates them in Python.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define EAO_IF_HD __host__ __device__ inline
#else
#define EAO_IF_HD inline
#endif

namespace eao {
namespace iforest {

// ---- Object_Map::IsolationForestDeleteOutliers' literals (tests/golden/isolation_forest_constants.json holds them to the reference text)
constexpr uint32_t kTreeCount = 50;         // src/Object.cc:1296
constexpr uint32_t kSeed = 12345;           // :1296
constexpr uint32_t kSampleDivisor = 2;      // :1296
constexpr uint32_t kMinPoints = 30;         // :1256
constexpr int kExemptClasses[3] = {75, 64, 65};      // :1245
constexpr float kThreshold = 0.6f;          // :1248
constexpr int kThresholdClass = 62;         // :1249
constexpr float kThresholdOfClass = 0.65f;  // :1250
constexpr double kEuler = 0.5772156649;     // include/isolation_forest.h:99

constexpr uint32_t kMaxPoints = 65535;      // above it libstdc++'s shuffle takes its one-swap-per-draw path
constexpr uint32_t kMtN = 624, kMtM = 397;

inline bool object_runs(bool biForest, int classId, size_t n) {
    if (!biForest) return false;
    for (int c : kExemptClasses)
        if (classId == c) return false;
    return n >= kMinPoints;
}
// `float th`, promoted to double in `anomaly_scores[i] > th`
inline double object_threshold(int classId) { return (double)(classId == kThresholdClass ? kThresholdOfClass : kThreshold); }

struct Mt19937 {
    uint32_t x[kMtN];
    uint32_t p;
    explicit Mt19937(uint32_t seed) {
        x[0] = seed;
        for (uint32_t i = 1; i < kMtN; i++) x[i] = 1812433253u * (x[i - 1] ^ (x[i - 1] >> 30)) + i;
        p = kMtN;
    }
    void twist() {
        for (uint32_t k = 0; k < kMtN; k++) {
            const uint32_t y = (x[k] & 0x80000000u) | (x[(k + 1) % kMtN] & 0x7fffffffu);
            x[k] = x[(k + kMtM) % kMtN] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        p = 0;
    }
    uint32_t operator()() {
        if (p >= kMtN) twist();
        uint32_t z = x[p++];
        z ^= z >> 11;
        z ^= (z << 7) & 0x9d2c5680u;
        z ^= (z << 15) & 0xefc60000u;
        z ^= z >> 18;
        return z;
    }
};

// uniform_int_distribution(0, range - 1), 2 <= range < 2^32
inline uint32_t lemire(Mt19937& g, uint32_t range) {
    uint64_t product = (uint64_t)g() * range;
    uint32_t low = (uint32_t)product;
    if (low < range) {
        const uint32_t threshold = (0u - range) % range;
        while (low < threshold) {
            product = (uint64_t)g() * range;
            low = (uint32_t)product;
        }
    }
    return (uint32_t)(product >> 32);
}

inline float canonical(uint32_t draw) {
    const float r = (float)draw / 4294967296.0f;
    return r >= 1.0f ? 0x1.fffffep-1f : r;
}
inline float uniform_real(Mt19937& g, float a, float b) {
    const float u = canonical(g());
    const float w = b - a;
    const float m = u * w;
    return m + a;
}

inline void shuffle_ids(Mt19937& g, uint16_t* ids, uint32_t n) {
    if (n == 0) return;
    uint32_t i = 1;
    if ((n % 2) == 0) {
        std::swap(ids[i], ids[lemire(g, 2)]);
        i++;
    }
    while (i != n) {
        const uint32_t b1 = i + 2;      // swap_range + 1
        const uint32_t x = lemire(g, (i + 1) * b1);
        std::swap(ids[i], ids[x / b1]);
        i++;
        std::swap(ids[i], ids[x % b1]);
        i++;
    }
}

// IsolationForest::Build (:463-470): the seed of tree i is uniform_int_distribution<uint32_t>(0, UINT32_MAX)(gen): the whole range, one draw
inline void tree_seeds(uint32_t seed, uint32_t treeCount, uint32_t* out) {
    Mt19937 g(seed);
    for (uint32_t i = 0; i < treeCount; i++) out[i] = g();
}

// IsolationTree::Build (:340)
inline uint32_t max_depth(uint32_t sampleSize) { return (uint32_t)std::ceil(std::log2((double)sampleSize)); }
// The same number without libm, for a sample size that only the device knows (csrc/object_chain.hip): the bits of sampleSize - 1.  log2 of a power of two is
// exact and log2 is monotonic, so ceil(log2(S)) is the smallest d with 2^d >= S wherever log2(S) does not round up to an integer from below; a double has 53
// bits and S < 2^32, so it does not.  tests/test_object_chain_reference_cpu.py holds the two forms equal for every S in 1 .. 32767.
EAO_IF_HD uint32_t max_depth_int(uint32_t sampleSize) {
    uint32_t d = 0;
    for (uint32_t v = sampleSize - 1; v != 0 && sampleSize != 0; v >>= 1) d++;
    return d;
}

// CalculateC (:103-118), with libm's log: the scorer reads a table of these, so its sums are upstream's
inline double c_of(uint32_t n) {
    if (n > 2) {
        const double h = std::log((double)(n - 1)) + kEuler;
        return double(2.0 * h) - (double(2.0 * (n - 1)) / double(n));
    }
    return n == 2 ? 1.0 : 0.0;
}
// (:524-526)
inline double finish_score(double totalPathLen, uint32_t treeCount, double cOfSample) {
    const double avgPathLen = totalPathLen / double(treeCount);
    // upstream's object code calls libm's pow.  A compiler that sees the literal base may call exp2 instead (clang does at -O1 and above), whose last bit can
    // differ: the base goes through a volatile so that every build of this header calls pow.
    volatile double two = 2.0;
    return std::pow(two, -avgPathLen / cOfSample);
}

// One record of Node::Serialize (:226-243): size == 0 on inner nodes
struct NodeRec {
    uint32_t dim;
    float split;
    uint32_t size;
};
static_assert(sizeof(NodeRec) == 12, "the record Node::Serialize writes");
// What the build kernel writes per node: the record and the preorder index of the right child (the left child is the next node)
struct NodeDev {
    uint32_t dim;
    float split;
    uint32_t size;
    uint32_t right;
};
constexpr size_t kForestHeaderBytes = 16, kTreeHeaderBytes = 12;
inline size_t stream_bytes(uint32_t treeCount, size_t totalNodes) { return kForestHeaderBytes + kTreeHeaderBytes * treeCount + sizeof(NodeRec) * totalNodes; }
EAO_IF_HD uint32_t max_nodes(uint32_t sampleSize) { return 2 * sampleSize - 1; }

// IsolationForest::Serialize (:532-560) over the kernel's node arrays: tree t owns nodes[t * stride .. + count[t])
inline void write_stream(uint8_t* out, uint32_t treeCount, uint32_t sampleSize, const NodeDev* nodes, size_t stride, const uint32_t* count) {
    const uint64_t dims = 3;
    std::memcpy(out, &dims, 8);
    std::memcpy(out + 8, &treeCount, 4);
    std::memcpy(out + 12, &sampleSize, 4);
    out += kForestHeaderBytes;
    for (uint32_t t = 0; t < treeCount; t++) {
        std::memcpy(out, &dims, 8);
        std::memcpy(out + 8, &sampleSize, 4);
        out += kTreeHeaderBytes;
        for (uint32_t k = 0; k < count[t]; k++, out += sizeof(NodeRec)) std::memcpy(out, &nodes[t * stride + k], sizeof(NodeRec));
    }
}

// What the entry points refuse (include/eao_fusion.h); nullptr = accepted
inline const char* refusal(int64_t n, int64_t sampleSize, int64_t treeCount) {
    if (n > (int64_t)kMaxPoints) return "more than 65535 points (libstdc++'s shuffle takes another path there)";
    if (treeCount <= 0) return "tree_count == 0";
    if (sampleSize <= 0) return "sample_size == 0";
    if (sampleSize > n) return "sample_size above the number of points";
    return nullptr;
}
inline bool all_finite(const float* xyz, size_t n) {
    for (size_t i = 0; i < 3 * n; i++)
        if (!std::isfinite(xyz[i])) return false;
    return true;
}

// ---- the working set of one tree in the build kernel: ids (uint16, max(N, 2 S): the shuffled ids, later the sample's slots and the partition's scratch) and the
// sample's coordinates (3 floats per slot).  It lives in LDS while it fits the budget; above it the ids go to a global workspace and the coordinates are read
// from the caller's points in place.
constexpr size_t kLdsBudget = 59392;      // dynamic LDS of k_iforest_build: 58 KB, beside 2.6 KB of static state under the 64 KB a workgroup may take
struct LdsPlan {
    uint32_t idsEntries;      // max(N, 2 S)
    size_t idsBytes;          // rounded to 16
    size_t bytes;             // ids + coordinates
    bool inLds;
};
EAO_IF_HD LdsPlan lds_plan(uint32_t n, uint32_t sampleSize) {
    LdsPlan p;
    p.idsEntries = n > 2 * sampleSize ? n : 2 * sampleSize;
    p.idsBytes = ((size_t)p.idsEntries * 2 + 15) & ~(size_t)15;
    p.bytes = p.idsBytes + (size_t)sampleSize * 12;
    p.inLds = p.bytes <= kLdsBudget;
    return p;
}

// ---- what the kernels of csrc/iforest.hip read per object from device memory, for the callers that enqueue them: the file's own entries write it on the host,
// the plan kernel of csrc/object_chain.hip on the device.  Tree g of the launch belongs to object treeObj[g]; a tree at or above treeCount leaves at once.
struct ObjDev {
    uint32_t ptStart, n, sampleSize, maxDepth;
    uint32_t treeBase, treeCount, inLds, idsBytes;
    uint64_t nodeBase;      // in NodeDev
    uint64_t wsBase;        // in uint16
    uint32_t cBase, stride; // C table offset in doubles; NodeDev per tree
    uint32_t pad[2];
};
static_assert(sizeof(ObjDev) == 64, "ObjDev layout");

#if defined(__HIPCC__)
// dyn_lds: the largest LdsPlan::bytes among the objects whose plan is inLds; ws: the ids of those whose plan is not
hipError_t enqueue_build(hipStream_t stream, const ObjDev* objs, const unsigned* treeObj, const unsigned* seeds, const float* xyz, NodeDev* nodes, unsigned* nodeCount,
                         unsigned* failed, unsigned short* ws, unsigned long long* stamps, unsigned n_trees, size_t dyn_lds);
// max_n: the largest n among the objects (at least 1)
hipError_t enqueue_score(hipStream_t stream, const ObjDev* objs, const float* xyz, const NodeDev* nodes, const double* cTable, const unsigned* failed, double* totals,
                         unsigned max_n, unsigned n_obj);
#endif

// ---- the forest on the host, in the sort-free form the kernel uses (tools/isolation_forest_walk.cpp; the timing tool's host baseline).
// Returns false where Node::Build does (:167: a split above the maximum leaves the right child an empty range).
inline bool build_tree(uint32_t treeSeed, const float* xyz, uint32_t n, uint32_t sampleSize, std::vector<NodeDev>& nodes) {
    nodes.clear();
    Mt19937 g(treeSeed);
    std::vector<uint16_t> ids(std::max(n, 2 * sampleSize));
    for (uint32_t i = 0; i < n; i++) ids[i] = (uint16_t)i;
    shuffle_ids(g, ids.data(), n);
    uint16_t* tmp = ids.data() + sampleSize;      // (the ids past the sample are dead once it is drawn)
    const uint32_t maxDepth = max_depth(sampleSize);
    struct Pending { uint32_t first, last, depth, parent; };
    std::vector<Pending> stack;
    stack.push_back({0, sampleSize - 1, 0, UINT32_MAX});
    while (!stack.empty()) {
        Pending c = stack.back();
        stack.pop_back();
        if (c.parent != UINT32_MAX) nodes[c.parent].right = (uint32_t)nodes.size();
        for (;;) {
            const uint32_t me = (uint32_t)nodes.size(), count = c.last - c.first + 1;
            if (count == 1 || c.depth >= maxDepth) {
                nodes.push_back({0, 0.0f, count, 0});
                break;
            }
            const uint32_t dim = lemire(g, 3);
            float lo = xyz[3 * ids[c.first] + dim], hi = lo;
            for (uint32_t i = c.first + 1; i <= c.last; i++) {
                const float v = xyz[3 * ids[i] + dim];
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            if (lo == hi) {
                nodes.push_back({dim, 0.0f, count, 0});
                break;
            }
            const float split = uniform_real(g, lo, hi);
            uint32_t nl = 0, nr = 0;
            for (uint32_t i = c.first; i <= c.last; i++) {
                const uint16_t id = ids[i];
                if (xyz[3 * id + dim] < split) ids[c.first + nl++] = id;
                else tmp[nr++] = id;
            }
            for (uint32_t i = 0; i < nr; i++) ids[c.first + nl + i] = tmp[i];
            if (nl == 0) {
                nodes.push_back({dim, split, count, 0});
                break;
            }
            if (nl == count) return false;
            nodes.push_back({dim, split, 0, 0});
            stack.push_back({c.first + nl, c.last, c.depth + 1, me});
            c.last = c.first + nl - 1;
            c.depth++;
        }
    }
    return true;
}

// Node::GetPathLen (:272-287) over one tree, as the scorer walks it
inline double path_len(const NodeDev* nodes, const float* p, const double* cTable) {
    uint32_t k = 0, depth = 0;
    while (nodes[k].size == 0) {
        k = p[nodes[k].dim] < nodes[k].split ? k + 1 : nodes[k].right;
        depth++;
    }
    return double(depth) + cTable[nodes[k].size];
}

struct HostForest {
    uint32_t treeCount = 0, sampleSize = 0;
    std::vector<std::vector<NodeDev>> trees;
    std::vector<double> cTable;
    bool build(uint32_t treeCount_, uint32_t seed, const float* xyz, uint32_t n, uint32_t sampleSize_) {
        treeCount = treeCount_;
        sampleSize = sampleSize_;
        std::vector<uint32_t> seeds(treeCount);
        tree_seeds(seed, treeCount, seeds.data());
        trees.resize(treeCount);
        for (uint32_t t = 0; t < treeCount; t++)
            if (!build_tree(seeds[t], xyz, n, sampleSize, trees[t])) return false;
        cTable.resize((size_t)sampleSize + 1);
        for (uint32_t s = 0; s <= sampleSize; s++) cTable[s] = c_of(s);
        return true;
    }
    double total(const float* p) const {
        double t = 0;
        for (const auto& tree : trees) t += path_len(tree.data(), p, cTable.data());
        return t;
    }
    double score(const float* p) const { return finish_score(total(p), treeCount, cTable[sampleSize]); }
    std::vector<uint8_t> stream() const {
        size_t total = 0, stride = 0;
        for (const auto& t : trees) { total += t.size(); stride = std::max(stride, t.size()); }
        std::vector<NodeDev> flat(stride * treeCount);
        std::vector<uint32_t> count(treeCount);
        for (uint32_t t = 0; t < treeCount; t++) {
            count[t] = (uint32_t)trees[t].size();
            std::copy(trees[t].begin(), trees[t].end(), flat.begin() + t * stride);
        }
        std::vector<uint8_t> out(stream_bytes(treeCount, total));
        write_stream(out.data(), treeCount, sampleSize, flat.data(), stride, count.data());
        return out;
    }
};

// The removal of src/Object.cc:1324-1347 as the adapter performs it: the indices to erase, ascending.  Upstream's loop reads outliernum[numMOutpoint] one past
// the end after the last outlier (:1336); this list is walked with a bound instead.
inline std::vector<uint32_t> flagged_indices(const uint8_t* flags, size_t n) {
    std::vector<uint32_t> out;
    for (size_t i = 0; i < n; i++)
        if (flags[i]) out.push_back((uint32_t)i);
    return out;
}

}  // namespace iforest
}  // namespace eao
