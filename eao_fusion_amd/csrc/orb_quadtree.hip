// orb_quadtree.hip -- k_quadtree: ORBextractor::DistributeOctTree (src/ORBextractor.cc:537-763) for one (frame, level) per workgroup, and its launch.
// (Split from orb.hip in round 6, a pure move; the file header of orb.hip describes the kernel.)
#include "orb_internal.h"

using namespace eao::orb;

namespace {

// ---------------------------------------------------------------------------------------------- quad-tree
// In-place exclusive scan of a[0..n) by the whole kQT-thread block; returns the total.  Caller guarantees a[]
// is fully written and visible (barrier) before the call; the function ends with a barrier.
template <int kQT>
__device__ int block_excl_scan(int* a, int n, int* wtmp) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int per = (n + kQT - 1) / kQT;
    const int b = min(t * per, n), e = min(b + per, n);
    int ssum = 0;
    for (int i = b; i < e; i++) ssum += a[i];
    // inclusive scan over the wave on the VALU (DPP row shifts inside the rows of 16, then the row broadcasts 15 / 31) instead
    // of six ds_bpermute round trips: the quad-tree calls this scan some thirty times per level, each on its critical path
    int v = ssum;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);   // row_bcast15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);   // row_bcast31 into rows 2 and 3
    __syncthreads();  // protect wtmp from the previous call's readers
    if (lane == 63) wtmp[wv] = v;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kQT / 64; w++) {
        const int x = wtmp[w];
        if (w < wv) woff += x;
        total += x;
    }
    int run = woff + v - ssum;
    for (int i = b; i < e; i++) {
        const int x = a[i];
        a[i] = run;
        run += x;
    }
    __syncthreads();
    return total;
}

// The same exclusive scan by ONE wave, in place, without a workgroup barrier (the caller fences at wavefront scope).
__device__ __forceinline__ int wave_excl_scan(int* a, int n, int lane) {
    const int per = (n + 63) >> 6;
    const int b = min(lane * per, n), e = min(b + per, n);
    int ssum = 0;
    for (int i = b; i < e; i++) ssum += a[i];
    int v = ssum;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);   // row_bcast15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);   // row_bcast31 into rows 2 and 3
    const int total = __builtin_amdgcn_readlane(v, 63);
    int run = v - ssum;
    for (int i = b; i < e; i++) {
        const int x = a[i];
        a[i] = run;
        run += x;
    }
    eao::wave_sync();
    return total;
}

// Inclusive sum over the wave of one value per lane, on the VALU (the DPP steps of the scans above); lane 63 holds the total.
__device__ __forceinline__ int wave_incl_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);   // row_bcast15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);   // row_bcast31 into rows 2 and 3
    return v;
}
// Minimum over the wave (uniform result) by the same steps; a lane without a source takes the identity.
__device__ __forceinline__ int wave_min(int v) {
    constexpr int kTop = 0x7FFFFFFF;
    v = min(v, __builtin_amdgcn_update_dpp(kTop, v, 0x111, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(kTop, v, 0x112, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(kTop, v, 0x114, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(kTop, v, 0x118, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(kTop, v, 0x142, 0xA, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(kTop, v, 0x143, 0xC, 0xF, false));
    return __builtin_amdgcn_readlane(v, 63);
}

constexpr unsigned kQtLeaf = 0xFFFFFFFFu;         // mid of an entry that holds one key (every key then maps to quadrant 0)
__device__ __forceinline__ unsigned box_mid(short4 bx) {
    return (unsigned)(bx.x + ((bx.z - bx.x + 1) >> 1)) | ((unsigned)(bx.y + ((bx.w - bx.y + 1) >> 1)) << 16);
}
__device__ __forceinline__ int quadrant_mid(unsigned key, unsigned mid) {
    const unsigned x = key & 0xFFF, y = (key >> 12) & 0xFFF;
    return (x < (mid & 0xFFFFu) ? 0 : 1) + (y < (mid >> 16) ? 0 : 2);
}
__device__ __forceinline__ int quadrant(unsigned key, short4 bx) {
    const int x = key & 0xFFF, y = (key >> 12) & 0xFFF;
    const int mx = bx.x + ((bx.z - bx.x + 1) >> 1);   // UL.x + ceil((UR.x-UL.x)/2)
    const int my = bx.y + ((bx.w - bx.y + 1) >> 1);
    return (x < mx ? 0 : 1) + (y < my ? 0 : 2);
}

// The one sweep of a pass over the M candidates, by the whole workgroup: every candidate moves to the list position that
// wave 0 has just laid out for its child (childpos, split point of the OLD entry in mid) and, when another pass follows
// (`count`, uniform), is counted in the NEXT pass's child histogram under the split point of its new entry (nmid; cc zeroed
// by the caller, complete at the caller's barrier).  The sweep that re-homed in pass i and the one that histogrammed in pass
// i + 1 walked the same candidates with the same key, and the second looked up the node the first had just stored.
// The candidates are in spatial order (cells row-major, corners row-major inside a cell), so neighbouring lanes mostly
// hit the same (node, quadrant) bin: one LDS atomic per RUN of equal bins in the wave instead of one per candidate
// (while the tree is shallow, thousands of atomics would otherwise queue on a handful of words).
// (FOUR rows of kQT candidates per trip: every link of the chain node -> split point -> new node -> its split point is fetched for
//  all four before any of them is used -- as one row per trip a sweep was a chain of dependent LDS reads and an atomic, twelve times over for level 0)
// With one wave per SIMD a sweep is bound by that wave's own instruction stream (profiles/orb_quadtree_sweep_ab.txt): what counts is the
// number of instructions per candidate and that the four rows' loads really are in flight together.
// One trip of the sweep: rows k0, k0 + kQT, .. of kNR <= 4 rows.  Only the last row of a trip that is not kFull may end inside the row.
template <int kQT, int kNR, bool kFull, class KeyPtr, class NofPtr>
__device__ __forceinline__ void rehome_and_count_rows(KeyPtr keys, NofPtr nof, int M, int k0, const unsigned* mid, const int* childpos, const unsigned* nmid, int* cc, bool count) {
    const int t = threadIdx.x, lane = t & 63;
    // (No load of the chain is conditional: a lane past the last candidate reads the last one's key and node, and entry 0 in the place of
    //  whatever that gives it -- every address stays inside its array, whatever another wave has stored to nof[M - 1] by then -- and
    //  neither stores nor counts.  Behind `k < M ? load : x` every load sat in a branch of its own with a full wait in front of it.)
    int nd[kNR], bin[kNR];
    unsigned ky[kNR], md[kNR];
    bool in[kNR];
#pragma unroll
    for (int u = 0; u < kNR; u++) {
        const int k = k0 + u * kQT + t;
        in[u] = kFull || u < kNR - 1 || k < M;
        const int kk = in[u] ? k : M - 1;
        const int n = (int)nof[kk];
        ky[u] = keys[kk];
        nd[u] = in[u] ? n : 0;
    }
#pragma unroll
    for (int u = 0; u < kNR; u++) md[u] = mid[nd[u]];
#pragma unroll
    for (int u = 0; u < kNR; u++) { const int n = childpos[4 * nd[u] + quadrant_mid(ky[u], md[u])]; nd[u] = in[u] ? n : 0; }
#pragma unroll
    for (int u = 0; u < kNR; u++) { const int k = k0 + u * kQT + t; if (in[u]) nof[k] = (unsigned short)nd[u]; }
    if (!count) return;                            // (uniform: the tree has ended, the best-response step needs the nodes alone)
#pragma unroll
    for (int u = 0; u < kNR; u++) md[u] = nmid[nd[u]];
#pragma unroll
    for (int u = 0; u < kNR; u++) bin[u] = in[u] && md[u] != kQtLeaf ? 4 * nd[u] + quadrant_mid(ky[u], md[u]) : -1;
#pragma unroll
    for (int u = 0; u < kNR; u++) {
        const int prev = __builtin_amdgcn_update_dpp(-2, bin[u], 0x138, 0xF, 0xF, false);   // wave_shr:1 (lane 0 keeps -2): VALU, not the LDS crossbar
        const bool head = bin[u] != prev;
        const unsigned long long hm = __ballot(head);
        if (head && bin[u] >= 0) {
            const unsigned long long rest = lane == 63 ? 0ull : (hm >> (lane + 1));
            const int run = rest ? __ffsll((long long)rest) : 64 - lane;
            atomicAdd(&cc[bin[u]], run);
        }
    }
}

template <int kQT, class KeyPtr, class NofPtr>
__device__ __forceinline__ void rehome_and_count(KeyPtr keys, NofPtr nof, int M, const unsigned* mid, const int* childpos, const unsigned* nmid, int* cc, bool count) {
    int k0 = 0;
    for (; k0 + 4 * kQT <= M; k0 += 4 * kQT) rehome_and_count_rows<kQT, 4, true>(keys, nof, M, k0, mid, childpos, nmid, cc, count);
    // the rest, fewer than four rows: as many rows as it has (level 0 of the benchmark frames: 3095 candidates, 23 of them in a fourth trip of 256 x 4)
    const int rest = M - k0;
    if (rest > 3 * kQT) rehome_and_count_rows<kQT, 4, false>(keys, nof, M, k0, mid, childpos, nmid, cc, count);
    else if (rest > 2 * kQT) rehome_and_count_rows<kQT, 3, false>(keys, nof, M, k0, mid, childpos, nmid, cc, count);
    else if (rest > kQT) rehome_and_count_rows<kQT, 2, false>(keys, nof, M, k0, mid, childpos, nmid, cc, count);
    else if (rest > 0) rehome_and_count_rows<kQT, 1, false>(keys, nof, M, k0, mid, childpos, nmid, cc, count);
}

// One workgroup per (level, frame).  List entries are (box, count, creation rank); `nodeof[k]` is the list
// position of candidate k's node.  Every pass (a) picks, from the child histograms of all multi-key nodes, the set
// of nodes that upstream would split in this pass and their processing order, (b) lays out the new list exactly
// as upstream's push_front/erase sequence would leave it, (c) moves the candidates and histograms the next pass's children.
struct QtArgs {
    const Geom* g; const unsigned* cellcand; const int* cellcnt; unsigned* levelkps; int* levelcnt; int f, l, M;
    long long* dbg;
    unsigned* candOut;   // global copy of the gathered candidates (read back by eao_orb_level_candidates)
};

// The gather's loads of one round: sixteen lanes to a cell, each with corners gl and gl + 16 of eight cells.  No address depends on the
// cell counts (a row holds cellCap words whatever its count; a group past the last cell takes the last cell's row).
constexpr int kQtGL = 16, kQtGC = 8;
constexpr int kQtCU = 4;   // entries per trip of a careful pass's rank loop (register form)
template <int kQT>
__device__ __forceinline__ void gather_row_loads(const unsigned* cellcand, long long cslot, int nCells, int cellCap, int c0, unsigned (&va)[kQtGC], unsigned (&vb)[kQtGC]) {
    const int grp = threadIdx.x / kQtGL, gl = threadIdx.x % kQtGL;
#pragma unroll
    for (int u = 0; u < kQtGC; u++) {
        const unsigned* srcc = cellcand + (cslot + min(c0 + u * (kQT / kQtGL) + grp, nCells - 1)) * cellCap;
        va[u] = srcc[min(gl, cellCap - 1)];
        vb[u] = srcc[min(gl + kQtGL, cellCap - 1)];
    }
}

// The candidate keys and their node index live in LDS when the level's M candidates fit the launch's LDS budget
// (g->qtLdsCand; always at the default 1000-feature settings), else in the global scratch arrays: the body is inlined
// once per placement.  kRegs: the node lists are in LDS (every launch but the global fallback, quadtree_global, which stays as it
// was): the set-up of a level with one initial node, the first round of row loads issued by the caller (pa, pb) and the register
// form of the list logic.
template <int kQT, bool kRegs, class KeyPtr, class NofPtr>
__device__ __forceinline__ void quadtree_body(const QtArgs& A, unsigned char* smem, int* wtmp, int* shv, KeyPtr keys, NofPtr nof, const unsigned (&pa)[kQtGC], const unsigned (&pb)[kQtGC]) {
    const Geom* __restrict__ g = A.g;
    int& sh_S = shv[0]; int& sh_phase = shv[1]; int& sh_done = shv[2]; int& sh_rstar = shv[3]; int& sh_nexp = shv[4];
    long long* dbg = A.dbg;
    // (phase stamps of diagnostic runs, thread 0 only, kept in LDS: as per-thread registers they cost 22 VGPRs of a kernel that
    //  spills at 1024 threads)
    __shared__ long long dacc[11];
    if (dbg && threadIdx.x == 0) { for (int i = 0; i < 10; i++) dacc[i] = 0; dacc[10] = clock64(); }
#define QSTAMP(i) do { if (dbg && threadIdx.x == 0) { const long long now_ = clock64(); dacc[i] += now_ - dacc[10]; dacc[10] = now_; } } while (0)
    const int t = threadIdx.x, lane = t & 63;
    const int l = A.l, f = A.f, M = A.M;
    const LevelGeom L = g->L[l];
    const int LC = L.listCap, N = L.quota;
    // ---- LDS carve-up
    short4* box0 = reinterpret_cast<short4*>(smem);
    short4* box1 = box0 + LC;
    int* cnt0 = reinterpret_cast<int*>(box1 + LC);
    int* cnt1 = cnt0 + LC;
    int* crk0 = cnt1 + LC;
    int* crk1 = crk0 + LC;
    unsigned* mid0 = reinterpret_cast<unsigned*>(crk1 + LC);   // split point of a multi-key entry (mx | my << 16), kQtLeaf otherwise
    unsigned* mid1 = mid0 + LC;
    int* childcnt0 = reinterpret_cast<int*>(mid1 + LC);         // 4 per entry, twice: the sweep of a pass fills the next pass's histogram while this pass's childpos is read
    int* childcnt1 = childcnt0 + 4 * LC;
    int* childpos = childcnt1 + 4 * LC; // 4 per entry
    unsigned long long* rkey = reinterpret_cast<unsigned long long*>(childpos);   // sort keys of a careful pass (before childpos is filled)
    int* order = childpos + 4 * LC;
    int* vlist = order + LC;
    int* procRank = vlist + LC;
    int* scanB = procRank + LC;
    int* scanA = scanB + LC;            // g->scanCap entries (>= LC and >= nCells); holds the exclusive cell prefix on entry

    // ---- gather this level's candidates in upstream order: cells row-major, corners row-major inside a cell.  Sixteen
    // lanes to a cell, each with corners j and j + 16 of eight cells in flight (a cell of the benchmark frames holds ~11 corners,
    // few more than 32): a load instruction reads 64-byte pieces of four cells' rows, and the loads of 128 cells (256 threads) wait
    // together.  (As one thread per cell a load instruction touched 64 cache lines for 64 words, sixteen times over, and the 280
    // cells of level 0 took two rounds of it.)
    // A level with ONE initial node (every frame up to 3:2) needs no initial assignment: node 0 holds all M candidates and its box,
    // hence its split point, follows from the geometry alone.  The gather then writes nof[k] = 0 beside the key it stores and
    // counts the key in the first child histogram (per thread: keys right of the split, below it, both; summed per wave with the
    // DPP scan, one LDS word per wave and bin) -- no nof fill, no initial sweep, and none of the barriers around them.
    const long long cslot = (long long)f * g->totalCells + L.cellBase;
    const int nIni = L.nIni;
    const bool direct = kRegs && nIni == 1;
    const short4 bx0 = make_short4(0, 0, (short)(int)(L.hX * 1.0f), (short)L.boxH);
    const unsigned m0 = box_mid(bx0);
    __shared__ int wq[4 * (kQT / 64)];
    {
        constexpr int kGL = kQtGL, kGC = kQtGC, kGroups = kQT / kGL;
        const int grp = t / kGL, gl = t % kGL;
        const int cellCap = g->cellCap;
        int nx = 0, ny = 0, nxy = 0, nall = 0;   // of this thread's keys: x >= split, y >= split, both, all
        auto put = [&](int k, unsigned v) {
            keys[k] = v; A.candOut[k] = v;
            if (direct) {
                nof[k] = 0;
                const bool hx = (v & 0xFFF) >= (m0 & 0xFFFFu), hy = ((v >> 12) & 0xFFF) >= (m0 >> 16);
                nx += hx; ny += hy; nxy += hx && hy; nall++;
            }
        };
        for (int c0 = 0; c0 < L.nCells; c0 += kGroups * kGC) {
            int o[kGC], n[kGC];
            unsigned va[kGC], vb[kGC];
#pragma unroll
            for (int u = 0; u < kGC; u++) {   // (a group past the last cell takes the last cell's row and stores nothing)
                const int c = c0 + u * kGroups + grp, cc = min(c, L.nCells - 1);
                o[u] = scanA[cc];
                const int e = cc + 1 < L.nCells ? scanA[cc + 1] : M;
                n[u] = c < L.nCells ? e - o[u] : 0;
            }
            // (unconditional: a row holds cellCap words, whatever its count.  The first round's loads were issued by the caller, before the
            //  scan of the cell counts: their addresses do not depend on it, only the store offsets below do)
            if (kRegs && c0 == 0) {
#pragma unroll
                for (int u = 0; u < kGC; u++) { va[u] = pa[u]; vb[u] = pb[u]; }
            } else gather_row_loads<kQT>(A.cellcand, cslot, L.nCells, cellCap, c0, va, vb);
#pragma unroll
            for (int u = 0; u < kGC; u++) {
                if (gl < n[u]) put(o[u] + gl, va[u]);
                if (gl + kGL < n[u]) put(o[u] + gl + kGL, vb[u]);
            }
#pragma unroll
            for (int u = 0; u < kGC; u++) {   // (the rest of a crowded cell)
                if (n[u] <= 2 * kGL) continue;
                const unsigned* srcc = A.cellcand + (cslot + c0 + u * kGroups + grp) * cellCap;
                if constexpr (kRegs) {   // (unrolled, with the counters, the copy of this loop for keys in global memory spilled 600 registers)
#pragma unroll 1
                    for (int j = gl + 2 * kGL; j < n[u]; j += kGL) put(o[u] + j, srcc[j]);
                } else {
                    for (int j = gl + 2 * kGL; j < n[u]; j += kGL) put(o[u] + j, srcc[j]);
                }
            }
        }
        if (direct) {   // quadrants 0..3 = (x low, y low), (x high, y low), (x low, y high), (x high, y high), as quadrant_mid
            const int s0 = wave_incl_sum(nall - nx - ny + nxy), s1 = wave_incl_sum(nx - nxy), s2 = wave_incl_sum(ny - nxy), s3 = wave_incl_sum(nxy);
            if (lane == 63) { int* w = wq + 4 * (t >> 6); w[0] = s0; w[1] = s1; w[2] = s2; w[3] = s3; }
        }
    }
    __syncthreads();
    // ---- initial nodes
    int S = 1, phase = 0, done = 0;
    if (direct) {
        if (t < 4) {   // (a lone key is a leaf: nothing counted)
            int s = 0;
            for (int w = 0; w < kQT / 64; w++) s += wq[4 * w + t];
            childcnt0[t] = M > 1 ? s : 0;
        }
        if (t == 0) {
            box0[0] = bx0; cnt0[0] = M; crk0[0] = 0; mid0[0] = M > 1 ? m0 : kQtLeaf;
            procRank[0] = -1;
            sh_S = 1; sh_phase = 0; sh_done = 0; sh_rstar = 0x7FFFFFFF; sh_nexp = 0;
        }
        __syncthreads();
        QSTAMP(0);
        QSTAMP(2);
    } else {
    if (t < nIni) {
        box0[t] = make_short4((short)(int)(L.hX * (float)t), 0, (short)(int)(L.hX * (float)(t + 1)), (short)L.boxH);
        cnt0[t] = 0;
        crk0[t] = t;
        // (the first sweep below moves the candidates like any pass's: from an "old" entry without a split point, whose every key
        //  maps to quadrant 0, through childpos to the entry's place among the non-empty ones)
        mid1[t] = kQtLeaf;
        procRank[t] = -1;
        childcnt0[4 * t] = 0; childcnt0[4 * t + 1] = 0; childcnt0[4 * t + 2] = 0; childcnt0[4 * t + 3] = 0;
    }
    __syncthreads();
    if (nIni == 1) {   // (the global fallback alone comes here with one node: min((int)(x / hX), 0) is node 0 for every candidate -- no division, no count)
        for (int k = t; k < M; k += kQT) nof[k] = 0;
        if (t == 0) cnt0[0] = M;
    } else
    for (int k0 = 0; k0 < M; k0 += kQT) {   // (every candidate lands in one of <= 16 nodes: count by ballot, not by 3000 atomics on one word)
        const int k = k0 + t;
        int ini = -1;
        if (k < M) {
            ini = min((int)((float)(keys[k] & 0xFFF) / L.hX), nIni - 1);
            nof[k] = (unsigned short)ini;
        }
        for (int i = 0; i < nIni; i++) {
            const unsigned long long m = __ballot(ini == i);
            if (m && (t & 63) == 0) atomicAdd(&cnt0[i], __popcll(m));
        }
    }
    __syncthreads();
    if (t == 0) {  // drop empty initial nodes (nIni <= 16)
        int S = 0;
        for (int i = 0; i < nIni; i++) {
            childpos[4 * i] = S;
            if (cnt0[i] > 0) { box0[S] = box0[i]; cnt0[S] = cnt0[i]; crk0[S] = S; mid0[S] = cnt0[i] > 1 ? box_mid(box0[i]) : kQtLeaf; S++; }
        }
        sh_S = S; sh_phase = 0; sh_done = 0; sh_rstar = 0x7FFFFFFF; sh_nexp = 0;
    }
    __syncthreads();
    QSTAMP(0);
    // (wave 0 alone rewrites sh_S / sh_phase / sh_done, behind the NEXT barrier: everyone takes its copies between the two)
    S = sh_S; phase = sh_phase;
    // the list is final only now, with the empty nodes dropped: the first pass's child histogram
    rehome_and_count<kQT>(keys, nof, M, mid1, childpos, mid0, childcnt0, true);
    __syncthreads();
    QSTAMP(2);
    }

    int diters = 0;
    short4* box = box0; short4* nbox = box1;
    unsigned* mid = mid0; unsigned* nmid = mid1;
    int* cnt = cnt0; int* ncnt = cnt1;
    int* crk = crk0; int* ncrk = crk1;
    int* childcnt = childcnt0; int* nchildcnt = childcnt1;
    // Every pass: the list logic over the S <= N nodes, then ONE sweep over the M candidates by the whole workgroup, which moves
    // them to their new nodes and histograms the children of the next pass (rehome_and_count).  The list logic runs in WAVE 0
    // ALONE, wave-synchronously (DPP scans, wavefront-scope fences, no workgroup barrier): as a sequence of block-wide steps it
    // was ~20 barriers per pass with a handful of instructions between them -- 43 k of level 0's 132 k cycles.  Meanwhile the
    // other waves zero the next histogram.  Two barriers per pass remain, one behind the list logic and one behind the sweep
    // (four in a careful pass of the general form, whose O(n^2) ranking stays block-wide; the register form has two in every pass).
#define QT_WAVE_FENCE() eao::wave_sync()
    const int wv = t >> 6;
    for (int iter = 0; iter < 64 && !done; iter++) {
        if (kRegs && S <= 64) {
            // The list fits one entry per lane of wave 0 (workgroup-uniform; every pass of a tree of up to four passes from one initial
            // node): the list logic in registers.  Ranks and prefixes come from ballots, one DPP scan and, in a careful pass, one
            // uniform loop of readlanes -- no index array in LDS (scanA, vlist, order, procRank, scanB), no fence, and no
            // block-wide ranking with its two barriers.  The steps and their results are those of the general form below.
            if (wv == 0) {
                // (1) the entry of this lane, every load issued before any is used (a lane past the list reads entry 0 and owns nothing)
                const bool have = lane < S;
                const int li = have ? lane : 0;
                const int c = cnt[li];
                const int2 ca = *reinterpret_cast<const int2*>(childcnt + 4 * li), cb = *reinterpret_cast<const int2*>(childcnt + 4 * li + 2);
                const short4 b = box[li];
                const int ck = crk[li];
                const unsigned md = mid[li];
                const int cq[4] = {ca.x, ca.y, cb.x, cb.y};
                const bool multi = have && c > 1;
                const int ne = multi ? (cq[0] > 0) + (cq[1] > 0) + (cq[2] > 0) + (cq[3] > 0) : 0;
                const unsigned long long mm = __ballot(multi);
                const unsigned long long below = (1ull << lane) - 1;
                const int nCand = __popcll(mm);
                QSTAMP(1);
                QSTAMP(3);
                // (3) + (4) rank r in processing order and growth prefix (the children of the entries processed before this one)
                int r, pre, nProc = nCand, totalChildren;
                if (phase == 0) {   // list order
                    r = __popcll(mm & below);
                    const int inc = wave_incl_sum(ne);
                    pre = inc - ne;
                    totalChildren = __builtin_amdgcn_readlane(inc, 63);
                } else {
                    // (size, creation rank) descending.  The pairs are unique, so ne can ride below the creation rank in the low word
                    // without changing the order: two readlanes per entry hand every lane that entry's key and ne.
                    // (Over the lanes of the list, kQtCU to a trip, not over the set bits of mm: a bit loop was fourteen dependent
                    //  instructions per entry, 6.5 k cycles for a list of 64, and longer trips spill.  The key of an entry that is not
                    //  multi is 0 and above nobody's.  One accumulator: rank in the bits from 9, prefix (<= 4 x 63) below.  The bound
                    //  through readfirstlane: as a vector value the loop ran on exec masks.)
                    const unsigned klo = ((unsigned)ck << 3) | (unsigned)ne;
                    const unsigned long long key = multi ? ((unsigned long long)(unsigned)c << 32) | klo : 0ull;
                    int acc = 0;
                    const int Su = __builtin_amdgcn_readfirstlane(S);
                    for (int j0 = 0; j0 < Su; j0 += kQtCU)
#pragma unroll
                    for (int u = 0; u < kQtCU; u++) {
                        const int j = j0 + u;
                        const unsigned jlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)key, j);
                        const unsigned long long jkey = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(key >> 32), j) << 32) | jlo;
                        acc += jkey > key ? (int)((jlo & 7u) | 0x200u) : 0;
                    }
                    r = acc >> 9; pre = acc & 0x1FF;
                    // the careful pass stops at the first entry whose children bring the list to N
                    const int rstar = wave_min(multi && S + pre + ne - (r + 1) >= N ? r : 0x7FFFFFFF);
                    if (rstar != 0x7FFFFFFF) nProc = rstar + 1;
                    const unsigned long long lastm = __ballot(multi && r == nProc - 1);
                    totalChildren = lastm ? __builtin_amdgcn_readlane(pre + ne, __ffsll((long long)lastm) - 1) : 0;
                }
                QSTAMP(4);
                const bool proc = multi && r < nProc;
                const int keep = __popcll(__ballot(have && !proc) & below);   // untouched entries ahead of this one
                QSTAMP(5);
                // (5) new list: children of the LAST processed node first (each as n4,n3,n2,n1), untouched entries after
                int myexp = 0;
                if (have) {
                    if (!proc) {
                        const int p = totalChildren + keep;
                        nbox[p] = b; ncnt[p] = c; ncrk[p] = ck; nmid[p] = md;
                        *reinterpret_cast<int2*>(childpos + 4 * lane) = make_int2(p, p);       // (every key of an untouched entry moves with it)
                        *reinterpret_cast<int2*>(childpos + 4 * lane + 2) = make_int2(p, p);
                    } else {
                        const short mx = (short)(b.x + ((b.z - b.x + 1) >> 1)), my = (short)(b.y + ((b.w - b.y + 1) >> 1));
                        int p = totalChildren - (pre + ne);
#pragma unroll
                        for (int q = 3; q >= 0; q--) {
                            const int cc = cq[q];
                            if (cc > 0) {
                                short4 nb;
                                nb.x = (q & 1) ? mx : b.x; nb.z = (q & 1) ? b.z : mx;
                                nb.y = (q & 2) ? my : b.y; nb.w = (q & 2) ? b.w : my;
                                nbox[p] = nb; ncnt[p] = cc; ncrk[p] = 4 * r + q; nmid[p] = cc > 1 ? box_mid(nb) : kQtLeaf;
                                childpos[4 * lane + q] = p;
                                p++;
                                myexp += cc > 1;
                            }
                        }
                    }
                }
                myexp = __builtin_amdgcn_readlane(wave_incl_sum(myexp), 63);
                // (7) upstream's termination tests (src/ORBextractor.cc:660-737)
                if (lane == 0) {
                    const int S2 = totalChildren + S - nProc;
                    sh_S = S2;
                    if (S2 >= N || S2 == S) sh_done = 1;
                    else if (phase == 0 && S2 + 3 * myexp > N) sh_phase = 1;
                }
            } else {
                const int nz = 4 * min(LC, 4 * S);
                for (int i = t - 64; i < nz; i += kQT - 64) nchildcnt[i] = 0;
            }
        } else {
        // (1) the multi-key entries in list order (childcnt of this pass is complete, procRank[0, S) is -1: the sweep before the barrier saw to both)
        int nCand = 0;
        if (wv == 0) {
            for (int i = lane; i < S; i += 64) scanA[i] = cnt[i] > 1 ? 1 : 0;
            QT_WAVE_FENCE();
            nCand = wave_excl_scan(scanA, S, lane);
            for (int i = lane; i < S; i += 64)
                if (cnt[i] > 1) vlist[scanA[i]] = i;
            QT_WAVE_FENCE();
        }
        QSTAMP(1);
        // (3) processing order: list order (full pass) or (size, creation rank) descending (careful pass)
        if (phase == 1) {
            // rank by (size, creation rank) descending, block-wide: the two sort fields are packed into one 64-bit key per node
            // (size << 32 | creation rank; the pairs are unique) and laid out densely (childpos is free here, 8-byte aligned),
            // so that the counting loop is one broadcast LDS read and one compare per node.  When there are fewer nodes than
            // threads, 2 / 4 / ... adjacent lanes share a node's loop and add their counts with DPP shuffles.
            if (wv == 0) {
                for (int j = lane; j < nCand; j += 64) { const int me = vlist[j]; rkey[j] = ((unsigned long long)(unsigned)cnt[me] << 32) | (unsigned)crk[me]; }
                if (lane == 0) sh_nexp = nCand;         // (nCand lives in wave 0's registers: hand it to the others; reset below)
            }
            __syncthreads();
            const int nC2 = sh_nexp;
            int sl = 1;
            while (2 * sl * nC2 <= kQT && sl < 16) sl *= 2;
            for (int j0 = 0; j0 < nC2; j0 += kQT / sl) {
                const int j = j0 + t / sl, part = t & (sl - 1);
                int r = 0;
                if (j < nC2) {
                    const unsigned long long mk = rkey[j];
#pragma unroll 8
                    for (int u = part; u < nC2; u += sl) r += rkey[u] > mk;
                }
                for (int d = sl >> 1; d >= 1; d >>= 1) r += __shfl_xor(r, d);
                if (j < nC2 && part == 0) order[r] = vlist[j];
            }
            __syncthreads();
            if (t == 0) sh_nexp = 0;
        }
        QSTAMP(3);
        if (wv == 0) {
            if (phase == 0) {
                for (int j = lane; j < nCand; j += 64) order[j] = vlist[j];
                QT_WAVE_FENCE();
            }
            // (4) growth prefix in processing order; the careful pass stops at the first prefix reaching N
            for (int r = lane; r < nCand; r += 64) {
                const int i = order[r];
                scanA[r] = (childcnt[4 * i] > 0) + (childcnt[4 * i + 1] > 0) + (childcnt[4 * i + 2] > 0) + (childcnt[4 * i + 3] > 0);
            }
            QT_WAVE_FENCE();
            wave_excl_scan(scanA, nCand, lane);
            int rstar = 0x7FFFFFFF;
            if (phase == 1) {
                for (int r = lane; r < nCand; r += 64) {
                    const int i = order[r];
                    const int ne = (childcnt[4 * i] > 0) + (childcnt[4 * i + 1] > 0) + (childcnt[4 * i + 2] > 0) + (childcnt[4 * i + 3] > 0);
                    if (S + scanA[r] + ne - (r + 1) >= N) rstar = min(rstar, r);
                }
                for (int d = 32; d >= 1; d >>= 1) rstar = min(rstar, __shfl_xor(rstar, d));
            }
            QSTAMP(4);
            const int nProc = (phase == 1 && rstar != 0x7FFFFFFF) ? rstar + 1 : nCand;
            int totalChildren = 0;
            if (nProc > 0) {
                const int i = order[nProc - 1];
                totalChildren = scanA[nProc - 1] + (childcnt[4 * i] > 0) + (childcnt[4 * i + 1] > 0) + (childcnt[4 * i + 2] > 0) + (childcnt[4 * i + 3] > 0);
            }
            for (int r = lane; r < nProc; r += 64) procRank[order[r]] = r;
            QT_WAVE_FENCE();
            for (int i = lane; i < S; i += 64) scanB[i] = procRank[i] < 0 ? 1 : 0;
            QT_WAVE_FENCE();
            wave_excl_scan(scanB, S, lane);
            QSTAMP(5);
            // (5) new list: children of the LAST processed node first (each as n4,n3,n2,n1), untouched entries after
            int myexp = 0;
            for (int i = lane; i < S; i += 64) {
                const int r = procRank[i];
                if (r < 0) {
                    const int p = totalChildren + scanB[i];
                    nbox[p] = box[i]; ncnt[p] = cnt[i]; ncrk[p] = crk[i]; nmid[p] = mid[i];
                    childpos[4 * i] = p; childpos[4 * i + 1] = p; childpos[4 * i + 2] = p; childpos[4 * i + 3] = p;   // (every key of an untouched entry moves with it)
                } else {
                    const short4 b = box[i];
                    const short mx = (short)(b.x + ((b.z - b.x + 1) >> 1)), my = (short)(b.y + ((b.w - b.y + 1) >> 1));
                    const int ne = (childcnt[4 * i] > 0) + (childcnt[4 * i + 1] > 0) + (childcnt[4 * i + 2] > 0) + (childcnt[4 * i + 3] > 0);
                    int p = totalChildren - (scanA[r] + ne);
                    for (int q = 3; q >= 0; q--) {
                        const int c = childcnt[4 * i + q];
                        if (c > 0) {
                            short4 nb;
                            nb.x = (q & 1) ? mx : b.x; nb.z = (q & 1) ? b.z : mx;
                            nb.y = (q & 2) ? my : b.y; nb.w = (q & 2) ? b.w : my;
                            nbox[p] = nb; ncnt[p] = c; ncrk[p] = 4 * r + q; nmid[p] = c > 1 ? box_mid(nb) : kQtLeaf;
                            childpos[4 * i + q] = p;
                            p++;
                            myexp += c > 1;
                        }
                    }
                }
            }
            for (int d = 32; d >= 1; d >>= 1) myexp += __shfl_xor(myexp, d);
            // (7) upstream's termination tests (src/ORBextractor.cc:660-737)
            if (lane == 0) {
                const int S2 = totalChildren + S - nProc;
                sh_S = S2;
                if (S2 >= N || S2 == S) sh_done = 1;
                else if (phase == 0 && S2 + 3 * myexp > N) sh_phase = 1;
            }
        } else {
            // the other waves, beside the list logic: zero the histogram that this pass's sweep fills (a pass leaves at most 4 S entries;
            // its last reader was wave 0 of the pass before, two barriers back)
            const int nz = 4 * min(LC, 4 * S);
            for (int i = t - 64; i < nz; i += kQT - 64) nchildcnt[i] = 0;
        }
        }
        __syncthreads();
        QSTAMP(6);
        // (6) re-home the candidates and count the next pass's children; procRank of the new list back to "not processed"
        S = sh_S; phase = sh_phase; done = sh_done;
        for (int i = t; i < S; i += kQT) procRank[i] = -1;
        rehome_and_count<kQT>(keys, nof, M, mid, childpos, nmid, nchildcnt, !done);
        __syncthreads();
        QSTAMP(7);
        diters++;
        short4* tb = box; box = nbox; nbox = tb;
        unsigned* tm = mid; mid = nmid; nmid = tm;
        int* ti = cnt; cnt = ncnt; ncnt = ti;
        ti = crk; crk = ncrk; ncrk = ti;
        ti = childcnt; childcnt = nchildcnt; nchildcnt = ti;
    }
#undef QT_WAVE_FENCE
    // ---- best response per node, first candidate wins ties (strict '>' at src/ORBextractor.cc:752)
    unsigned* best = reinterpret_cast<unsigned*>(scanB);
    for (int i = t; i < S; i += kQT) best[i] = 0;
    __syncthreads();
    for (int k = t; k < M; k += kQT) atomicMax(&best[nof[k]], ((keys[k] >> 24) << 20) | (0xFFFFFu - (unsigned)k));
    __syncthreads();
    unsigned* out = A.levelkps + (long long)f * g->totalKpCap + L.kpBase;
    for (int i = t; i < S; i += kQT) {
        const unsigned k = 0xFFFFFu - (best[i] & 0xFFFFFu);
        out[i] = keys[k];
    }
    if (t == 0) A.levelcnt[f * g->nlevels + l] = S;
    QSTAMP(8);
    if (dbg && t == 0 && A.dbg) {
        long long* o = dbg + 16 * l;
        for (int i = 0; i < 9; i++) o[i] = dacc[i];
        o[9] = diters; o[10] = M; o[11] = S;
    }
#undef QSTAMP
}

template <int kQT>
__device__ __noinline__ void quadtree_global(const Geom* __restrict__ g, const unsigned* cellcand, const int* cellcnt, unsigned* cand, unsigned short* nodeof,
                                             unsigned* levelkps, int* levelcnt, int* candcnt, int f, int l, unsigned char* base, long long* dbg, int* wtmp, int* shv) {
    const int t = threadIdx.x;
    const LevelGeom L = g->L[l];
    int* scanA = reinterpret_cast<int*>(base + (size_t)L.listCap * (2 * sizeof(short4) + sizeof(int) * kQtNodeInts));
    const long long cslot = (long long)f * g->totalCells + L.cellBase;
    for (int i = t; i < L.nCells; i += kQT) scanA[i] = cellcnt[cslot + i];
    __syncthreads();
    const int M = block_excl_scan<kQT>(scanA, L.nCells, wtmp);
    if (t == 0) candcnt[f * g->nlevels + l] = M;
    if (M == 0) {
        if (t == 0) levelcnt[f * g->nlevels + l] = 0;
        return;
    }
    const unsigned pa[kQtGC] = {}, pb[kQtGC] = {};   // (no loads ahead of the scan here)
    QtArgs A = {g, cellcand, cellcnt, levelkps, levelcnt, f, l, M, dbg, cand + (long long)f * g->totalCandCap + L.candBase};
    quadtree_body<kQT, false>(A, base, wtmp, shv, cand + (long long)f * g->totalCandCap + L.candBase, nodeof + (long long)f * g->totalCandCap + L.candBase, pa, pb);
}

template <int kQT>
__global__ __launch_bounds__(kQT, kQT == 256 ? 4 : 1) void k_quadtree(const Geom* __restrict__ g, const unsigned* __restrict__ cellcand,
                                                  const int* __restrict__ cellcnt, unsigned* __restrict__ cand,
                                                  unsigned short* __restrict__ nodeof, unsigned* __restrict__ levelkps,
                                                  int* __restrict__ levelcnt, int* __restrict__ candcnt, int f0, long long* dbg, int l0,
                                                  unsigned char* __restrict__ qtnodes) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int wtmp[kQT / 64];
    __shared__ int shv[8];
    const int t = threadIdx.x;
    // level-major dispatch (frames fastest): the long level-0 workgroups of EVERY frame start first and the short top levels
    // fill the gaps behind them -- with the levels of a frame dispatched together the last frames' level 0 was the tail
    const int l = blockIdx.y + l0, f = blockIdx.x + f0;   // the launch covers levels l0 .. l0 + gridDim.y - 1
    const LevelGeom L = g->L[l];
    if (g->qtNodesGlobal) {   // node lists too large for LDS: the same algorithm over a global workspace (slower, never refused)
        quadtree_global<kQT>(g, cellcand, cellcnt, cand, nodeof, levelkps, levelcnt, candcnt, f, l, qtnodes + (long long)f * g->qtNodeFrameBytes + L.nodeOff,
                        (dbg && f == f0) ? dbg : nullptr, wtmp, shv);
        return;
    }
    int* scanA = reinterpret_cast<int*>(smem + (size_t)L.listCap * (2 * sizeof(short4) + sizeof(int) * kQtNodeInts));
    const long long cslot = (long long)f * g->totalCells + L.cellBase;
    for (int i = t; i < L.nCells; i += kQT) scanA[i] = cellcnt[cslot + i];
    // the gather's first round of row loads, in flight across the scan of the cell counts (consumed in quadtree_body)
    unsigned pa[kQtGC] = {}, pb[kQtGC] = {};
    if (L.nCells > 0) gather_row_loads<kQT>(cellcand, cslot, L.nCells, g->cellCap, 0, pa, pb);
    __syncthreads();
    const int M = block_excl_scan<kQT>(scanA, L.nCells, wtmp);
    if (t == 0) candcnt[f * g->nlevels + l] = M;
    if (M == 0) {
        if (t == 0) levelcnt[f * g->nlevels + l] = 0;
        return;
    }
    QtArgs A = {g, cellcand, cellcnt, levelkps, levelcnt, f, l, M, (dbg && f == f0) ? dbg : nullptr, cand + (long long)f * g->totalCandCap + L.candBase};
    if (M <= g->qtLdsCand) {
        unsigned* keysL = reinterpret_cast<unsigned*>(smem + g->qtKeysOff);
        quadtree_body<kQT, true>(A, smem, wtmp, shv, keysL, reinterpret_cast<unsigned short*>(keysL + g->qtLdsCand), pa, pb);
    } else {
        quadtree_body<kQT, true>(A, smem, wtmp, shv, cand + (long long)f * g->totalCandCap + L.candBase, nodeof + (long long)f * g->totalCandCap + L.candBase, pa, pb);
    }
}

}  // namespace

void eao::orb::launch_quadtree(const eao_orb* h, hipStream_t str, int nb, int f0, int lFirst, int nLev) {
    if (nb < 36) hipLaunchKernelGGL(k_quadtree<kQTSmall>, dim3(nb, nLev), dim3(kQTSmall), h->quadLds, str, h->d_geom.p, h->d_cellcand.p, h->d_cellcnt.p, h->d_cand.p,
                       h->d_nodeof.p, h->d_levelkps.p, h->d_levelcnt.p, h->d_candcnt.p, f0, h->d_dbg, lFirst, h->d_qtnodes.p);
    else hipLaunchKernelGGL(k_quadtree<kQTLarge>, dim3(nb, nLev), dim3(kQTLarge), h->quadLds, str, h->d_geom.p, h->d_cellcand.p, h->d_cellcnt.p, h->d_cand.p,
                       h->d_nodeof.p, h->d_levelkps.p, h->d_levelcnt.p, h->d_candcnt.p, f0, h->d_dbg, lFirst, h->d_qtnodes.p);
}

eao_status eao::orb::quadtree_reserve_lds(size_t bytes) {      // per-function, process-wide state: only ever raised (another handle with a larger nfeatures may be in use)
    static std::atomic<int> cur{0};
    int have = cur.load();
    while ((int)bytes > have) {
        EAO_HIP(hipFuncSetAttribute((const void*)k_quadtree<kQTSmall>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        EAO_HIP(hipFuncSetAttribute((const void*)k_quadtree<kQTLarge>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        if (cur.compare_exchange_weak(have, (int)bytes)) break;
    }
    return EAO_OK;
}
