// ba_setup.h -- the host set-up of a bundle adjustment that needs no device: validation and counts of the edge list, the map-scale path's covisibility structure
// (observer lists, camera lists, pairs), the active structure and the launch order of the pair kernels -- the stages BAJob::prepare (lm_host.hip) runs in this order.
// Plain C++17, no HIP: tests/cpp/ba_setup_test.cpp holds every stage to a naive reference under AddressSanitizer / ThreadSanitizer on a machine without a GPU.
// Every stage returns false after eao::set_error (the library's definition: api_common.hip; the test brings its own); the caller's status is EAO_ERR_INVALID.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "host_crew.h"

namespace eao {
void set_error(const char* fmt, ...);

namespace lm {

#define BA_SETUP_REQUIRE(cond, ...)      \
    do {                                 \
        if (!(cond)) {                   \
            eao::set_error(__VA_ARGS__); \
            return false;                \
        }                                \
    } while (0)

// The caller's lists as the set-up reads them: landmarks = points then planes, edges = point edges then plane edges.
struct EdgeView {
    int nC = 0, nPo = 0, nPl = 0, Ept = 0, Epl = 0;
    const int* edge_cam = nullptr; const int* edge_point = nullptr;
    const int* pedge_cam = nullptr; const int* pedge_plane = nullptr;
    const uint8_t* cam_fixed = nullptr;
    int nP() const { return nPo + nPl; }
    int E() const { return Ept + Epl; }
    int cam(int e) const { return e < Ept ? edge_cam[e] : pedge_cam[e - Ept]; }
    int lm(int e) const { return e < Ept ? edge_point[e] : nPo + pedge_plane[e - Ept]; }
};

// Everything the stages keep from call to call (no allocation per call) and hand to each other.  ONE object per host thread: the caller takes a reference once per
// call, and the passes work through plain pointers captured by value (in a shared library every use of a thread_local object is a call into the TLS runtime).
struct SetupScratch {
    // count_edges, chunked form (kQ chunks of the edge list): chunk boundaries as edges / as landmarks, per chunk its free observers, pair entries, first finding,
    // per chunk and camera its edge count (then: where the chunk's edges go inside the camera's list) and the last landmark seen
    std::vector<int> cb, cl, chunkFree, camCntQ, camLastQ, chunkBad, chunkBase, ccF;
    std::vector<long long> chunkEnt;
    // build_observer_lists: free cameras with an edge, renumbered; per landmark its free observers (by camera) and their edges; per free camera its landmarks
    // (ascending), the position of its own entry in each landmark's list and, parallel form only, the edge
    std::vector<int> fidx, lmOff, lmCam, lmEdge, cmOff, cmLm, cmU, cmE, pcur;
    // build_pairs: the pairs (prA <= prB) in camera order, where each pair's entries start, where each camera's pairs start; per chunk of cameras its partners / counts
    std::vector<int> prA, prB, prStart, cmPairStart;
    std::vector<std::vector<int>> chB, chCnt;
    // build_active_structure (last landmark per camera) and deal_launch_order (one class of pairs, dealt to the eight XCDs)
    std::vector<int> camLast, cls, grp[8];
    size_t lpEntries = 0;             // (pair, landmark) entries of the covisibility structure
    bool edgesByLandmark = true;      // the edge list is grouped landmark by landmark, ascending (what the adapters and every generator produce): ptEdges is then the identity
    bool countedInChunks = false;     // count_edges took the chunked form: chunk tables valid, no duplicate edge, landmarks strictly ascending
    int nFa = 0;                      // free cameras with at least one edge
};

// Host phases of the set-up in ms since the start of the call (EAO_DEBUG_STAMPS): slots 0 - 4 the caller's, 5 - 10 the covisibility stages'.
struct Laps {
    bool on = false;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double t[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    void lap(int k) { if (on) t[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Who runs the passes of one set-up.  A map-scale call runs them as a SESSION of the host crew (HostCrew: one wake-up, then passes handed over through one polled
// word), open from here to the end of the set-up.  EAO_BA_SETUP_THREADS (read per call): 1 = the serial walks, n > 1 = a session of n threads on any map (the
// tests), unset = a session from 20 000 edges on.  Never from a crew thread (a map-scale window inside a batch call).
struct Workers {
    bool open = false;      // this call owns a crew session
    int envT = 0;
    Workers(bool mapScale, int nEdges) {
        const char* const e = getenv("EAO_BA_SETUP_THREADS");
        envT = e ? atoi(e) : 0;
        if (mapScale && !t_inCrew && envT != 1 && (nEdges >= 20000 || envT > 1)) {
            const int hw = (int)std::thread::hardware_concurrency();
            const int nT = envT > 1 ? envT : std::max(2, std::min(12, hw / 2));
            open = host_crew().session_begin(nT - 1);
        }
    }
    ~Workers() { if (open) host_crew().session_end(); }
    Workers(const Workers&) = delete;
    Workers& operator=(const Workers&) = delete;
    // chunk(0 .. nChunks-1): a pass of the session; without one a run of the crew when `work` is worth it (or the switch says so); else the serial loop
    void pass(size_t work, int nChunks, const std::function<void(int)>& chunk) {
        if (open) { host_crew().session_pass(nChunks, chunk); return; }
        const int hw = (int)std::thread::hardware_concurrency();
        const int nT = t_inCrew || envT == 1 || (work < 200000 && envT <= 0) ? 1 : std::max(1, std::min(envT > 0 ? envT : std::min(12, hw / 2), nChunks));
        if (nT == 1) { for (int q = 0; q < nChunks; q++) chunk(q); return; }
        std::atomic<int> next(0);
        auto body = [&]() { for (int q; (q = next.fetch_add(1)) < nChunks;) chunk(q); };
        host_crew().run(nT - 1, [&](int) { body(); }, body);
    }
};

constexpr int kSetupChunks = 48;      // chunks of the edge list in the parallel forms of count_edges / build_observer_lists

// ---- count_edges, parallel form (sessions; no plane edges): chunks of the edge list cut at landmark boundaries.  Every chunk validates its edges, checks that the
//      landmarks ascend, counts each landmark's edges (a landmark's run belongs to one chunk) and its own edges per camera, looks for a camera that appears twice in a
//      landmark, and counts what the covisibility structure needs (free observers, pair entries).  Anything unexpected -- an index out of range, a landmark out of
//      order -- leaves S.countedInChunks false and the counters zero: the serial form then runs instead (and words the error).
inline bool count_edges_in_chunks(const EdgeView& v, SetupScratch& S, int* camCnt, int* ptCnt) {
    constexpr int kQ = kSetupChunks;
    const int nC = v.nC, Ept = v.Ept;
    const int* const ecam = v.edge_cam; const int* const ept = v.edge_point; const uint8_t* const fixedp = v.cam_fixed;
    std::vector<int>& cb = S.cb;
    cb.assign(kQ + 1, Ept);
    for (int q = 0; q < kQ; q++) {      // chunk q = edges [cb[q], cb[q + 1]); boundaries moved forward to the end of a run of equal landmarks
        int e = (int)((long long)Ept * q / kQ);
        while (e > 0 && e < Ept && ept[e] == ept[e - 1]) e++;
        cb[q] = std::min(e, Ept);
    }
    cb[0] = 0;
    for (int q = 1; q <= kQ; q++) cb[q] = std::max(cb[q], cb[q - 1]);      // (monotone; an empty chunk is harmless)
    S.chunkFree.assign(kQ, 0); S.chunkEnt.assign(kQ, 0); S.chunkBad.assign(2 * kQ, -1);
    S.camCntQ.assign((size_t)kQ * nC, 0); S.camLastQ.assign((size_t)kQ * nC, -1);
    {
        int* const cfp = S.chunkFree.data(); long long* const cep = S.chunkEnt.data(); int* const ccq = S.camCntQ.data(); int* const clq = S.camLastQ.data();
        const int* const cbp = cb.data(); int* const bad = S.chunkBad.data();
        const int nC_ = nC, nPo_ = v.nPo;
        host_crew().session_pass(kQ, [=](int q) {
            int* const cc = ccq + (size_t)q * nC_; int* const last = clq + (size_t)q * nC_;
            int freeN = 0; long long ent = 0;
            const int e1 = cbp[q + 1];
            int prev = cbp[q] > 0 ? ept[cbp[q] - 1] : -1;
            for (int e = cbp[q]; e < e1;) {
                const int lmk = ept[e];
                // (unsigned: `prev` of a chunk q > 0 is the caller's own, unvalidated entry in front of the chunk -- a negative landmark behind a more negative one ascends too)
                if ((unsigned)lmk >= (unsigned)nPo_ || lmk <= prev) { bad[2 * q] = -2; return; }
                int m = 0, run = 0;
                for (; e < e1 && ept[e] == lmk; e++, run++) {
                    const int ec = ecam[e];
                    if ((unsigned)ec >= (unsigned)nC_) { bad[2 * q] = -2; return; }
                    if (last[ec] == lmk && bad[2 * q] == -1) { bad[2 * q] = ec; bad[2 * q + 1] = lmk; }
                    last[ec] = lmk;
                    cc[ec]++;
                    m += fixedp[ec] ? 0 : 1;
                }
                __atomic_store_n(&ptCnt[lmk], run, __ATOMIC_RELAXED);      // (a landmark out of order could be written by two chunks: the serial pass then starts over)
                freeN += m; ent += (long long)m * (m + 1) / 2;
                prev = lmk;
            }
            cfp[q] = freeN; cep[q] = ent;
        });
    }
    bool clean = true;
    for (int q = 0; q < kQ; q++) clean = clean && S.chunkBad[2 * q] != -2;
    if (!clean) { std::fill(camCnt, camCnt + nC + v.nP(), 0); return true; }
    for (int q = 0; q < kQ; q++)
        if (S.chunkBad[2 * q] >= 0) { eao::set_error("two edges join camera %d and point %d", S.chunkBad[2 * q], S.chunkBad[2 * q + 1]); return false; }
    for (int i = 0; i < nC; i++) {      // a camera's count; per chunk: where the chunk's edges go inside the camera's list
        int run = 0;
        for (int q = 0; q < kQ; q++) { const int c0 = S.camCntQ[(size_t)q * nC + i]; S.camCntQ[(size_t)q * nC + i] = run; run += c0; }
        camCnt[i] = run;
    }
    S.countedInChunks = true;
    return true;
}

// Validation of the edge list and, in the same pass, the edge counts per camera and per landmark the active structure starts from: cnt = camCnt[nC] then ptCnt[nP].
inline bool count_edges(const EdgeView& v, Workers& crew, SetupScratch& S, std::vector<int>& cnt) {
    const int nC = v.nC, nPo = v.nPo, nPl = v.nPl, Ept = v.Ept, Epl = v.Epl;
    cnt.assign((size_t)nC + v.nP(), 0);
    int* const camCnt = cnt.data(); int* const ptCnt = camCnt + nC;
    S.edgesByLandmark = true; S.countedInChunks = false;
    if (crew.open && Epl == 0 && Ept > 0 && !count_edges_in_chunks(v, S, camCnt, ptCnt)) return false;
    if (S.countedInChunks) return true;
    bool byLandmark = true;
    for (int e = 0, prev = 0; e < Ept; e++) {
        const int ec = v.edge_cam[e], ep = v.edge_point[e];
        BA_SETUP_REQUIRE(ec >= 0 && ec < nC && ep >= 0 && ep < nPo, "edge %d out of range", e);
        byLandmark = byLandmark && ep >= prev; prev = ep;
        camCnt[ec]++; ptCnt[ep]++;
    }
    for (int e = 0, prev = 0; e < Epl; e++) {
        const int ec = v.pedge_cam[e], ep = v.pedge_plane[e];
        BA_SETUP_REQUIRE(ec >= 0 && ec < nC && ep >= 0 && ep < nPl, "plane edge %d out of range", e);
        byLandmark = byLandmark && ep >= prev; prev = ep;
        camCnt[ec]++; ptCnt[nPo + ep]++;
    }
    S.edgesByLandmark = byLandmark;
    return true;
}

// observers [first, end) of one landmark by camera, each with its edge (insertion sort: a handful per landmark, mostly in order already)
inline void sort_observers(int* lc, int* le, int first, int end) {
    for (int u = first + 1; u < end; u++) {
        const int cf = lc[u], ce = le[u];
        int v = u;
        for (; v > first && lc[v - 1] > cf; v--) { lc[v] = lc[v - 1]; le[v] = le[v - 1]; }
        lc[v] = cf; le[v] = ce;
    }
}

// ---- build_observer_lists, parallel form (after count_edges_in_chunks: the edges come landmark by landmark, so a chunk of the edge list owns its landmarks).  The
//      counting pass has counted every chunk's free observers, pair entries and edges per camera; the pass here writes the observer lists (sorted by camera) and files
//      every entry under its camera at the position the chunks before it left -- a camera's list comes out in ascending landmark order, the same arrays as the
//      serial form, element for element, and the camera's edge list of the active structure (cmE -> camEdges) with it.
inline bool observer_lists_from_chunks(const EdgeView& v, Workers& crew, SetupScratch& S, const int* camCnt, Laps& laps) {
    constexpr int Q = kSetupChunks;
    const int nC = v.nC, nP = v.nP(), Ept = v.Ept, nFa = S.nFa;
    const int* const ecam = v.edge_cam; const int* const ept = v.edge_point;
    S.cl.assign(Q + 1, nP);
    S.cl[0] = 0;
    for (int q = 1; q < Q; q++) S.cl[q] = S.cb[q] < Ept ? ept[S.cb[q]] : nP;
    // chunk bases; per camera the start of its list and, per chunk, where the chunk's entries go
    S.chunkBase.assign(Q + 1, 0);
    for (int q = 0; q < Q; q++) { S.chunkBase[q + 1] = S.chunkBase[q] + S.chunkFree[q]; S.lpEntries += (size_t)S.chunkEnt[q]; }
    BA_SETUP_REQUIRE(S.lpEntries < ((size_t)1 << 31), "covisibility structure too large (%zu pair entries)", S.lpEntries);
    laps.lap(8);
    const int total = S.chunkBase[Q];
    S.lmCam.resize((size_t)total + 1); S.lmEdge.resize((size_t)total + 1);
    S.cmOff.assign((size_t)nFa + 1, 0);
    for (int i = 0; i < nC; i++) if (S.fidx[i] >= 0) S.cmOff[S.fidx[i] + 1] = camCnt[i];
    for (int f = 0; f < nFa; f++) S.cmOff[f + 1] += S.cmOff[f];
    S.cmLm.resize(S.cmOff[nFa]); S.cmU.resize(S.cmOff[nFa]); S.cmE.resize(S.cmOff[nFa]);
    laps.lap(9);
    S.ccF.resize((size_t)Q * nFa);      // per chunk and free camera: where the chunk's entries go inside the camera's list (camCntQ, renumbered)
    for (int q = 0; q < Q; q++)
        for (int i = 0; i < nC; i++) if (S.fidx[i] >= 0) S.ccF[(size_t)q * nFa + S.fidx[i]] = S.camCntQ[(size_t)q * nC + i];
    int* const lmOffp = S.lmOff.data(); int* const lc = S.lmCam.data(); int* const le = S.lmEdge.data(); const int* const fi = S.fidx.data();
    const int* const cbp = S.cb.data(); const int* const clp = S.cl.data(); const int* const basep = S.chunkBase.data();
    const int* const cmOffp = S.cmOff.data(); int* const cmLmp = S.cmLm.data(); int* const cmUp = S.cmU.data(); int* const cmEp = S.cmE.data();
    int* const ccFp = S.ccF.data();
    crew.pass((size_t)Ept * 8, Q, [=](int q) {
        int* const cc = ccFp + (size_t)q * nFa;
        int at = basep[q], e = cbp[q];
        const int lEnd = clp[q + 1];
        for (int lmk = clp[q]; lmk < lEnd; lmk++) {
            lmOffp[lmk] = at;      // (a landmark without edges: an empty list)
            const int first = at;
            for (; e < cbp[q + 1] && ept[e] == lmk; e++) { const int f = fi[ecam[e]]; if (f >= 0) { lc[at] = f; le[at] = e; at++; } }
            sort_observers(lc, le, first, at);
            for (int u = first; u < at; u++) { const int f = lc[u], pos = cmOffp[f] + cc[f]++; cmLmp[pos] = lmk; cmUp[pos] = u; cmEp[pos] = le[u]; }
        }
    });
    S.lmOff[nP] = total;
    laps.lap(10);
    return true;
}

// ---- build_observer_lists, serial form (any edge order, plane edges): a counting sort of the edges by landmark -- a filtered copy when the edges come landmark by
//      landmark -- then per free camera its landmarks in ascending order, by camera ranges on the crew.
inline bool observer_lists_serial(const EdgeView& v, Workers& crew, SetupScratch& S, Laps& laps) {
    const int nP = v.nP(), Ept = v.Ept, E = v.E(), nFa = S.nFa;
    std::vector<int>& lmOff = S.lmOff; std::vector<int>& lmCam = S.lmCam; std::vector<int>& lmEdge = S.lmEdge; std::vector<int>& cmOff = S.cmOff;
    bool byLandmark = true;        // the edges come landmark by landmark (the adapters and every generator list them so): the observer lists are then a filtered copy
    for (int e = 0, prev = 0; e < E; e++) { const int lmk = v.lm(e); byLandmark = byLandmark && lmk >= prev; prev = lmk; if (S.fidx[v.cam(e)] >= 0) lmOff[lmk + 1]++; }
    for (int i = 0; i < nP; i++) {
        const int m = lmOff[i + 1];
        S.lpEntries += (size_t)m * (m + 1) / 2;
        lmOff[i + 1] += lmOff[i];
    }
    BA_SETUP_REQUIRE(S.lpEntries < ((size_t)1 << 31), "covisibility structure too large (%zu pair entries)", S.lpEntries);
    laps.lap(8);
    lmCam.resize((size_t)lmOff[nP] + 1); lmEdge.resize((size_t)lmOff[nP] + 1);      // (+ 1: the branch-free append writes one slot ahead)
    cmOff.assign((size_t)nFa + 1, 0);
    if (byLandmark) {
        // (plain pointers and a branch-free append: the loop is a stream of 2 E loads and at most 2 E stores)
        int* const lc = lmCam.data(); int* const le = lmEdge.data(); int* const co = cmOff.data() + 1; const int* const fi = S.fidx.data();
        const int* const ecam = v.edge_cam; const int* const pcam = v.pedge_cam;
        int at = 0;
        for (int e = 0; e < Ept; e++) { const int f = fi[ecam[e]]; lc[at] = f; le[at] = e; const int ok = f >= 0; at += ok; if (ok) co[f]++; }
        for (int e = Ept; e < E; e++) { const int f = fi[pcam[e - Ept]]; lc[at] = f; le[at] = e; const int ok = f >= 0; at += ok; if (ok) co[f]++; }
    } else {
        S.pcur.assign(lmOff.begin(), lmOff.end() - 1);
        for (int e = 0; e < E; e++) {
            const int f = S.fidx[v.cam(e)];
            if (f < 0) continue;
            const int at = S.pcur[v.lm(e)]++;
            lmCam[at] = f; lmEdge[at] = e; cmOff[f + 1]++;
        }
    }
    laps.lap(9);
    for (int i = 0; i < nP; i++) sort_observers(lmCam.data(), lmEdge.data(), lmOff[i], lmOff[i + 1]);
    laps.lap(10);
    // per free camera: its landmarks in ascending order (a counting sort over the landmarks, walked in ascending order), each with the position of the
    // camera's own entry in that landmark's list
    for (int f = 0; f < nFa; f++) cmOff[f + 1] += cmOff[f];
    S.cmLm.resize(cmOff[nFa]); S.cmU.resize(cmOff[nFa]);
    // (camera ranges on the crew: every worker walks all observer lists and files the entries of ITS cameras -- a camera's list is written by one worker, in landmark order)
    const int nRanges = std::max(1, std::min(16, nFa / 32));
    const int* const lmOffp = lmOff.data(); const int* const lmCamp = lmCam.data(); const int* const cmOffp = cmOff.data();
    int* const cmLmp = S.cmLm.data(); int* const cmUp = S.cmU.data();
    crew.pass(S.lpEntries, nRanges, [=](int q) {
        const int f0 = (int)((long long)nFa * q / nRanges), f1 = (int)((long long)nFa * (q + 1) / nRanges);
        static thread_local std::vector<int> curv;
        curv.assign(cmOffp + f0, cmOffp + f1);
        int* const cur = curv.data();
        for (int i = 0; i < nP; i++)
            for (int u = lmOffp[i]; u < lmOffp[i + 1]; u++) {
                const int f = lmCamp[u];
                if (f < f0 || f >= f1) continue;
                const int at = cur[f - f0]++;
                cmLmp[at] = i; cmUp[at] = u;
            }
    });
    return true;
}

// ---- the covisibility structure of the map-scale path, CAMERA-MAJOR, first half.  Free cameras with at least one edge are numbered in ascending order (fidx: the
//      numbering the active structure gives them, camIdx).  Per landmark: its free observers and their edges, sorted by camera (lmOff / lmCam / lmEdge); per free
//      camera: the landmarks it observes in ascending order, each with the position of the camera's own entry in that landmark's list (cmOff / cmLm / cmU) -- a
//      camera's partners i2 >= i1 in a landmark are then the SUFFIX behind its own entry.  Counts the pair entries (S.lpEntries).  camCnt: count_edges'.
inline bool build_observer_lists(const EdgeView& v, Workers& crew, SetupScratch& S, const int* camCnt, Laps& laps) {
    S.fidx.assign((size_t)v.nC, -1);
    S.lmOff.assign((size_t)v.nP() + 1, 0);
    S.lpEntries = 0;
    int nFa = 0;
    for (int i = 0; i < v.nC; i++) if (camCnt[i] && !v.cam_fixed[i]) S.fidx[i] = nFa++;
    S.nFa = nFa;
    const bool ok = S.countedInChunks ? observer_lists_from_chunks(v, crew, S, camCnt, laps) : observer_lists_serial(v, crew, S, laps);
    laps.lap(5);
    return ok;
}

// ---- second half: the pairs of every camera and their entry counts.  For every free camera i1 (ascending) and each of its landmarks, the observers i2 >= i1: the
//      pairs (i1, i2) of camera i1 are counted in a counter array of nFa entries that stays in the cache and come out sorted; their entries are later written into
//      ONE contiguous range per camera, in ascending landmark order -- the order the assembly's fixed-order sums need.  Chunks of kChunkCams cameras on the crew,
//      each into lists of its own (a camera's pairs are its own: no two workers write the same word), joined in camera order: prA / prB / prStart / cmPairStart.
inline bool build_pairs(Workers& crew, SetupScratch& S, Laps& laps) {
    constexpr int kChunkCams = 4;
    const int nFa = S.nFa;
    const int nChunks = (nFa + kChunkCams - 1) / kChunkCams;
    S.chB.resize(nChunks); S.chCnt.resize(nChunks);
    S.cmPairStart.assign((size_t)nFa + 1, 0);
    {
        int* const pairsOfCam = S.cmPairStart.data() + 1;
        const int* const lmOffp = S.lmOff.data(); const int* const lmCamp = S.lmCam.data(); const int* const cmOffp = S.cmOff.data();
        const int* const cmLmp = S.cmLm.data(); const int* const cmUp = S.cmU.data();
        std::vector<int>* const chBp = S.chB.data(); std::vector<int>* const chCntp = S.chCnt.data();
        crew.pass(S.lpEntries, nChunks, [=](int q) {
            // (the per-thread scratch through plain pointers: in a shared library every use of a thread_local object is a call into the TLS runtime,
            //  and the two loops below made one per observer -- the pass took 0.57 ms where the walk itself needs 0.15)
            static thread_local std::vector<int> cnt2v, touchedv;
            cnt2v.assign((size_t)nFa, 0); touchedv.resize((size_t)nFa);
            int* const cnt2 = cnt2v.data(); int* const touched = touchedv.data();
            std::vector<int>& oB = chBp[q]; std::vector<int>& oC = chCntp[q];
            oB.clear(); oC.clear();
            for (int i1 = q * kChunkCams; i1 < std::min(nFa, (q + 1) * kChunkCams); i1++) {
                int nt = 0;
                for (int k = cmOffp[i1]; k < cmOffp[i1 + 1]; k++)
                    for (int u = cmUp[k], ue = lmOffp[cmLmp[k] + 1]; u < ue; u++) { const int i2 = lmCamp[u]; if (cnt2[i2]++ == 0) touched[nt++] = i2; }
                std::sort(touched, touched + nt);
                for (int k = 0; k < nt; k++) { const int i2 = touched[k]; oB.push_back(i2); oC.push_back(cnt2[i2]); cnt2[i2] = 0; }
                pairsOfCam[i1] = nt;
            }
        });
    }
    laps.lap(6);
    S.prA.clear(); S.prB.clear(); S.prStart.clear();
    int run = 0;
    for (int q = 0; q < nChunks; q++) {
        size_t at = 0;
        for (int i1 = q * kChunkCams; i1 < std::min(nFa, (q + 1) * kChunkCams); i1++) {
            const int np = S.cmPairStart[i1 + 1];
            for (int k = 0; k < np; k++, at++) { S.prA.push_back(i1); S.prB.push_back(S.chB[q][at]); S.prStart.push_back(run); run += S.chCnt[q][at]; }
            S.cmPairStart[i1 + 1] = (int)S.prA.size();
        }
    }
    S.prStart.push_back(run);
    BA_SETUP_REQUIRE((size_t)run == S.lpEntries, "internal: covisibility count mismatch (%d entries counted, %zu expected)", run, S.lpEntries);
    laps.lap(7);
    return true;
}

// The active structure (SparseOptimizer::initializeOptimization(level 0) + buildIndexMapping), written into the caller's arrays: free cameras with an edge and
// landmarks with an edge, renumbered (camIdx / ptIdx, -1 = not active; actCam / actPt the way back), and their edge lists as CSR (camStart / camEdges, ptStart / ptEdges).
struct ActiveStructure {
    int* camIdx; int* ptIdx; int* actCam; int* actPt;      // nC, nP, nC, nP
    int* ptStart; int* ptEdges; int* camStart; int* camEdges;      // nP + 1, E, nC + 1, E
    int nF = 0, nL = 0;
};

// cnt: count_edges' counters (consumed: they become fill cursors).  Refuses two edges between one camera and one landmark (the device's edge table has one slot
// per pair), in one of three forms: found by count_edges_in_chunks already; on the fly while the edges come landmark by landmark; in a walk over ptEdges otherwise.
inline bool build_active_structure(const EdgeView& v, Workers& crew, SetupScratch& S, bool mapScale, std::vector<int>& cnt, ActiveStructure& A) {
    const int nC = v.nC, nP = v.nP(), E = v.E();
    int* const camCnt = cnt.data(); int* const ptCnt = camCnt + nC;      // 1. edges per camera / per landmark
    int nF = 0, nL = 0;
    for (int i = 0; i < nC; i++) { A.camIdx[i] = -1; if (camCnt[i] && !v.cam_fixed[i]) { A.actCam[nF] = i; A.camIdx[i] = nF++; } }
    A.ptStart[0] = 0;
    for (int i = 0; i < nP; i++) { A.ptIdx[i] = -1; if (ptCnt[i]) { A.actPt[nL] = i; A.ptIdx[i] = nL; A.ptStart[nL + 1] = A.ptStart[nL] + ptCnt[i]; nL++; } }
    A.camStart[0] = 0;
    for (int i = 0; i < nF; i++) A.camStart[i + 1] = A.camStart[i] + camCnt[A.actCam[i]];
    A.nF = nF; A.nL = nL;
    int* const camCursor = camCnt; int* const ptCursor = ptCnt;          // 2. the same words as fill cursors into camEdges / ptEdges (active ones only)
    for (int i = 0; i < nL; i++) ptCursor[A.actPt[i]] = A.ptStart[i];
    for (int i = 0; i < nF; i++) camCursor[A.actCam[i]] = A.camStart[i];
    int* const ptEdges = A.ptEdges; int* const camEdges = A.camEdges;
    if (S.countedInChunks && mapScale) {      // (sessions: the duplicate test rode along with the validation pass, a camera's edges came with its landmark list -- cmE)
        BA_SETUP_REQUIRE((int)S.cmE.size() == A.camStart[nF], "internal: camera edge lists built for another set of free keyframes");
        const int* const cmEp = S.cmE.data();
        const int tot = A.camStart[nF];
        crew.pass((size_t)E, 16, [=](int q) {
            for (int e = (int)((long long)E * q / 16), e1 = (int)((long long)E * (q + 1) / 16); e < e1; e++) ptEdges[e] = e;
            const int k0 = (int)((long long)tot * q / 16), k1 = (int)((long long)tot * (q + 1) / 16);
            std::memcpy(camEdges + k0, cmEp + k0, (size_t)(k1 - k0) * sizeof(int));
        });
        return true;
    }
    if (S.edgesByLandmark) {      // (the landmarks' edge lists, concatenated in landmark order, ARE the edge list; the one-edge-per-pair test rides along)
        S.camLast.assign((size_t)nC, -1);
        for (int e = 0; e < E; e++) {
            const int cam = v.cam(e), lmk = v.lm(e);
            ptEdges[e] = e;
            if (A.camIdx[cam] >= 0) camEdges[camCursor[cam]++] = e;
            if (S.camLast[cam] == lmk) { eao::set_error("two edges join camera %d and point %d", cam, lmk); return false; }
            S.camLast[cam] = lmk;
        }
        return true;
    }
    for (int e = 0; e < E; e++) {
        const int cam = v.cam(e);
        ptEdges[ptCursor[v.lm(e)]++] = e;
        if (A.camIdx[cam] >= 0) camEdges[camCursor[cam]++] = e;
    }
    int* const lastSeen = camCnt;                                        // 3. the camera words again: the last active landmark seen with this camera
    for (int i = 0; i < nC; i++) lastSeen[i] = -1;
    for (int l = 0; l < nL; l++)
        for (int k = A.ptStart[l]; k < A.ptStart[l + 1]; k++) {
            const int cam = v.cam(ptEdges[k]);
            if (lastSeen[cam] == l) { eao::set_error("two edges join camera %d and point %d", cam, A.actPt[l]); return false; }
            lastSeen[cam] = l;
        }
    return true;
}

// Launch order of the pair kernels: long pairs (more than kLong entries) first; and inside each class the pairs are dealt to the eight XCDs by camera range --
// workgroup b runs on XCD b % 8, a pair list is sorted by its first camera, and the pairs of neighbouring cameras share their landmarks: dealt round-robin, every
// landmark's blocks were pulled into all eight L2s (the assembly re-reads each block once per pair of its landmark: 570 MB per launch on the banded 1000-keyframe
// map); with one contiguous camera range per XCD (equal shares of the entries) they stay in one or two.  A slot of -1 is an idle workgroup.
// lpStart[nz + 1] / lpPair[2 nz]: the pair CSR; lpOrder: room for `cap` slots.  One camera holding most of the pairs would not fit: plain order then.
inline void deal_launch_order(const int* lpStart, const int* lpPair, int nz, int kLong, size_t cap, SetupScratch& S, int* lpOrder, int& nPairsLong, int& nPairsSlots) {
    std::vector<int>& cls = S.cls; std::vector<int>* const grp = S.grp;
    size_t at = 0;
    bool fits = true;
    auto deal = [&](bool longOnes) -> int {
        cls.clear();
        long long tot = 0;
        for (int k = 0; k < nz; k++) if ((lpStart[k + 1] - lpStart[k] > kLong) == longOnes) { cls.push_back(k); tot += lpStart[k + 1] - lpStart[k]; }
        if (cls.empty()) return 0;
        for (int q = 0; q < 8; q++) grp[q].clear();
        long long run = 0;
        int x = 0, lastCam = -1;
        for (int k : cls) {      // a new XCD only at a camera boundary, once the running share of the entries is reached
            const int cam = lpPair[2 * k];
            if (cam != lastCam && x < 7 && run * 8 >= tot * (x + 1)) x++;
            lastCam = cam;
            grp[x].push_back(k);
            run += lpStart[k + 1] - lpStart[k];
        }
        size_t len = 0;
        for (int q = 0; q < 8; q++) len = std::max(len, grp[q].size());
        if (at + 8 * len > cap) { fits = false; return 0; }
        for (size_t sl = 0; sl < len; sl++)
            for (int q = 0; q < 8; q++) lpOrder[at++] = sl < grp[q].size() ? grp[q][sl] : -1;
        return (int)(8 * len);
    };
    nPairsLong = deal(true);
    nPairsSlots = nPairsLong + deal(false);
    if (!fits) {      // (one camera holds most of the pairs: plain order)
        at = 0;
        for (int k = 0; k < nz; k++) if (lpStart[k + 1] - lpStart[k] > kLong) lpOrder[at++] = k;
        nPairsLong = (int)at;
        for (int k = 0; k < nz; k++) if (lpStart[k + 1] - lpStart[k] <= kLong) lpOrder[at++] = k;
        nPairsSlots = (int)at;
    }
}

#undef BA_SETUP_REQUIRE

}  // namespace lm
}  // namespace eao
