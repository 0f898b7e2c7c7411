// ba_setup_test.cpp -- the host set-up of a bundle adjustment (eao_fusion_amd/csrc/ba_setup.h) without a GPU: every stage against a naive reference written here, the
// serial / crew-run / crew-session forms against each other array by array, the malformed edge lists the library refuses, and the launch order of the pair kernels.
// Built by tests/test_ba_setup_cpu.py twice: with -fsanitize=address,undefined (no stage may write in front of or behind its arrays, malformed lists included) and
// with -fsanitize=thread (the passes of a session share nothing but what they are handed).
#include <cstdarg>
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../eao_fusion_amd/csrc/ba_setup.h"

static std::string g_err;      // what the library would report through eao_last_error
namespace eao {
void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}
}  // namespace eao

using namespace eao::lm;
using ivec = std::vector<int>;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                             \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            std::fprintf(stderr, "FAILED (%s:%d) %s: ", __FILE__, __LINE__, #cond);                  \
            std::fprintf(stderr, __VA_ARGS__);                                                       \
            std::fprintf(stderr, "\n");                                                              \
            g_failed++;                                                                              \
            return false;                                                                            \
        }                                                                                            \
    } while (0)

// ---- maps: banded covisibility, a few fixed cameras, one free camera without an edge, a landmark without an edge, one seen by fixed cameras only, one seen by one
//      free camera; the edges landmark by landmark (ascending), the cameras of a landmark distinct and in random order
struct Map {
    int nC = 0, nPo = 0, nPl = 0;
    std::vector<uint8_t> fixed;
    ivec ecam, ept, pcam, ppl;
    EdgeView view() const {
        EdgeView v;
        v.nC = nC; v.nPo = nPo; v.nPl = nPl; v.Ept = (int)ecam.size(); v.Epl = (int)pcam.size();
        v.edge_cam = ecam.data(); v.edge_point = ept.data(); v.pedge_cam = pcam.data(); v.pedge_plane = ppl.data(); v.cam_fixed = fixed.data();
        return v;
    }
};

static Map make_map(int nFreeSeen, int nPts, int band, int perLandmark, unsigned seed) {
    std::mt19937 rng(seed);
    Map m;
    const ivec fixedAt = {0, 7, 8};
    const int idle = 3;      // the free camera nobody sees
    m.nC = nFreeSeen + (int)fixedAt.size() + 1;
    m.fixed.assign(m.nC, 0);
    for (int i : fixedAt) m.fixed[i] = 1;
    m.nPo = nPts;
    ivec seenFree;
    for (int i = 0; i < m.nC; i++) if (!m.fixed[i] && i != idle) seenFree.push_back(i);
    for (int l = 0; l < nPts; l++) {
        ivec cams;
        if (l == 5) continue;                                          // no edge
        else if (l == 9) cams = {8, 0};                                // fixed cameras only
        else if (l == 11) cams = {seenFree[seenFree.size() / 2]};      // one free camera
        else {
            const int c0 = (int)((long long)l * (m.nC - band + 1) / nPts);
            for (int i = c0; i < c0 + band && i < m.nC; i++) if (i != idle) cams.push_back(i);
            std::shuffle(cams.begin(), cams.end(), rng);
            cams.resize(std::min<size_t>(cams.size(), 1 + rng() % perLandmark));
        }
        for (int cam : cams) { m.ecam.push_back(cam); m.ept.push_back(l); }
    }
    return m;
}

static Map shuffled(const Map& m, unsigned seed) {
    std::mt19937 rng(seed);
    ivec order(m.ecam.size());
    for (size_t e = 0; e < order.size(); e++) order[e] = (int)e;
    std::shuffle(order.begin(), order.end(), rng);
    Map s = m;
    for (size_t e = 0; e < order.size(); e++) { s.ecam[e] = m.ecam[order[e]]; s.ept[e] = m.ept[order[e]]; }
    return s;
}

// ---- one set-up, stage by stage as BAJob::prepare runs them
enum Form { SERIAL, RUN, SESSION };
struct Out {
    bool ok = false, countedInChunks = false, sessionOpen = false;
    std::string err;
    int nFa = 0, nF = 0, nL = 0, nPairsLong = 0, nPairsSlots = 0;
    size_t lpEntries = 0;
    ivec fidx, lmOff, lmCam, lmEdge, cmOff, cmLm, cmU, prA, prB, prStart, cmPairStart;
    ivec camIdx, ptIdx, actCam, actPt, ptStart, ptEdges, camStart, camEdges, lpOrder;
};
static SetupScratch g_scratch;      // kept from call to call, as the library's is: a stage must not depend on what the call before left

static Out run_setup(const Map& m, Form form, int threads, int kLong = 6) {
    Out o;
    g_err.clear();
    setenv("EAO_BA_SETUP_THREADS", form == SERIAL ? "1" : std::to_string(threads).c_str(), 1);
    const EdgeView v = m.view();
    SetupScratch& S = g_scratch;
    Workers crew(form != RUN, form == RUN ? 0 : v.E());
    o.sessionOpen = crew.open;
    Laps laps;
    ivec cnt;
    const int nC = v.nC, nP = v.nP(), E = v.E();
    // (exact sizes: AddressSanitizer sees a write one element out)
    o.camIdx.assign(nC, -7); o.ptIdx.assign(nP, -7); o.actCam.assign(nC, -7); o.actPt.assign(nP, -7);
    o.ptStart.assign(nP + 1, -7); o.ptEdges.assign(E, -7); o.camStart.assign(nC + 1, -7); o.camEdges.assign(E, -7);
    ActiveStructure A{o.camIdx.data(), o.ptIdx.data(), o.actCam.data(), o.actPt.data(), o.ptStart.data(), o.ptEdges.data(), o.camStart.data(), o.camEdges.data()};
    o.ok = count_edges(v, crew, S, cnt) && build_observer_lists(v, crew, S, cnt.data(), laps) && build_pairs(crew, S, laps) && build_active_structure(v, crew, S, true, cnt, A);
    o.err = g_err;
    if (!o.ok) return o;
    o.countedInChunks = S.countedInChunks; o.nFa = S.nFa; o.lpEntries = S.lpEntries; o.nF = A.nF; o.nL = A.nL;
    o.fidx = S.fidx; o.lmOff = S.lmOff; o.cmOff = S.cmOff; o.cmLm = S.cmLm; o.cmU = S.cmU;
    o.lmCam.assign(S.lmCam.begin(), S.lmCam.begin() + S.lmOff[nP]); o.lmEdge.assign(S.lmEdge.begin(), S.lmEdge.begin() + S.lmOff[nP]);      // (the vectors carry one spare slot)
    o.prA = S.prA; o.prB = S.prB; o.prStart = S.prStart; o.cmPairStart = S.cmPairStart;
    const int nz = (int)S.prA.size();
    ivec lpPair(2 * (size_t)nz);
    for (int k = 0; k < nz; k++) { lpPair[2 * k] = S.prA[k]; lpPair[2 * k + 1] = S.prB[k]; }
    o.lpOrder.assign(2 * (size_t)nz + 64, -7);
    deal_launch_order(S.prStart.data(), lpPair.data(), nz, kLong, o.lpOrder.size(), S, o.lpOrder.data(), o.nPairsLong, o.nPairsSlots);
    return o;
}

// ---- the naive reference: observer lists from a sort, camera lists from a scan, pairs and entry counts from a map filled landmark by landmark
static bool check_against_reference(const Map& m, const Out& o, const char* what) {
    const EdgeView v = m.view();
    const int nC = v.nC, nP = v.nP(), E = v.E();
    CHECK(o.ok, "%s: refused: %s", what, o.err.c_str());
    ivec camEdgesN(nC, 0), fidx(nC, -1);
    for (int e = 0; e < E; e++) camEdgesN[v.cam(e)]++;
    int nFa = 0;
    for (int i = 0; i < nC; i++) if (camEdgesN[i] && !m.fixed[i]) fidx[i] = nFa++;
    CHECK(o.nFa == nFa && o.fidx == fidx, "%s: free cameras", what);
    std::vector<std::vector<std::pair<int, int>>> obs(nP);      // per landmark (free camera, edge)
    for (int e = 0; e < E; e++) if (fidx[v.cam(e)] >= 0) obs[v.lm(e)].push_back({fidx[v.cam(e)], e});
    ivec lmOff(nP + 1, 0), lmCam, lmEdge;
    std::vector<ivec> cmLm(nFa), cmU(nFa);
    std::map<std::pair<int, int>, int> pairs;
    size_t lpEntries = 0;
    for (int l = 0; l < nP; l++) {
        std::sort(obs[l].begin(), obs[l].end());
        for (size_t a = 0; a < obs[l].size(); a++) {
            cmLm[obs[l][a].first].push_back(l); cmU[obs[l][a].first].push_back((int)lmCam.size());
            lmCam.push_back(obs[l][a].first); lmEdge.push_back(obs[l][a].second);
            for (size_t b = a; b < obs[l].size(); b++) { pairs[{obs[l][a].first, obs[l][b].first}]++; lpEntries++; }
        }
        lmOff[l + 1] = (int)lmCam.size();
    }
    CHECK(o.lmOff == lmOff && o.lmCam == lmCam && o.lmEdge == lmEdge, "%s: observer lists", what);
    for (int l = 0; l < nP; l++)
        for (int u = o.lmOff[l] + 1; u < o.lmOff[l + 1]; u++) CHECK(o.lmCam[u - 1] < o.lmCam[u], "%s: observers of landmark %d not ascending", what, l);
    CHECK((int)o.cmOff.size() == nFa + 1 && o.cmOff[0] == 0, "%s: camera list offsets", what);
    for (int f = 0; f < nFa; f++) {
        CHECK(o.cmOff[f + 1] - o.cmOff[f] == (int)cmLm[f].size(), "%s: camera %d list length", what, f);
        for (int k = o.cmOff[f]; k < o.cmOff[f + 1]; k++) {
            CHECK(o.cmLm[k] == cmLm[f][k - o.cmOff[f]] && o.cmU[k] == cmU[f][k - o.cmOff[f]], "%s: camera %d list entry", what, f);
            CHECK(k == o.cmOff[f] || o.cmLm[k - 1] < o.cmLm[k], "%s: landmarks of camera %d not ascending", what, f);
            CHECK(o.cmU[k] >= o.lmOff[o.cmLm[k]] && o.cmU[k] < o.lmOff[o.cmLm[k] + 1] && o.lmCam[o.cmU[k]] == f, "%s: cmU of camera %d is not its own entry", what, f);
        }
    }
    ivec prA, prB, prStart, cmPairStart(nFa + 1, 0);
    int run = 0;
    for (const auto& kv : pairs) { prA.push_back(kv.first.first); prB.push_back(kv.first.second); prStart.push_back(run); run += kv.second; cmPairStart[kv.first.first + 1]++; }
    prStart.push_back(run);
    for (int f = 0; f < nFa; f++) cmPairStart[f + 1] += cmPairStart[f];
    CHECK(o.prA == prA && o.prB == prB && o.prStart == prStart && o.cmPairStart == cmPairStart && o.lpEntries == lpEntries, "%s: pairs", what);
    // the active structure: a CSR of the edge list over the active cameras / landmarks (points then planes), edges ascending inside a list
    ivec lmEdgesN(nP, 0);
    for (int e = 0; e < E; e++) lmEdgesN[v.lm(e)]++;
    int nF = 0, nL = 0;
    for (int i = 0; i < nC; i++) {
        const bool act = camEdgesN[i] && !m.fixed[i];
        CHECK(o.camIdx[i] == (act ? nF : -1), "%s: camIdx[%d]", what, i);
        if (!act) continue;
        CHECK(o.actCam[nF] == i && o.camStart[nF + 1] - o.camStart[nF] == camEdgesN[i], "%s: camera %d", what, i);
        int k = o.camStart[nF];
        for (int e = 0; e < E; e++) if (v.cam(e) == i) { CHECK(o.camEdges[k] == e, "%s: camEdges of camera %d", what, i); k++; }
        nF++;
    }
    for (int l = 0; l < nP; l++) {
        CHECK(o.ptIdx[l] == (lmEdgesN[l] ? nL : -1), "%s: ptIdx[%d]", what, l);
        if (!lmEdgesN[l]) continue;
        CHECK(o.actPt[nL] == l && o.ptStart[nL + 1] - o.ptStart[nL] == lmEdgesN[l], "%s: landmark %d", what, l);
        int k = o.ptStart[nL];
        for (int e = 0; e < E; e++) if (v.lm(e) == l) { CHECK(o.ptEdges[k] == e, "%s: ptEdges of landmark %d", what, l); k++; }
        nL++;
    }
    CHECK(o.nF == nF && o.nL == nL && o.nF == nFa && o.camStart[0] == 0 && o.ptStart[0] == 0 && o.ptStart[nL] == E, "%s: active counts", what);
    return true;
}

static bool same_arrays(const Out& a, const Out& b, const char* what, bool lmEdgeToo = true) {
    CHECK(a.ok && b.ok, "%s: refused: %s / %s", what, a.err.c_str(), b.err.c_str());
    CHECK(a.nFa == b.nFa && a.lpEntries == b.lpEntries && a.fidx == b.fidx && a.lmOff == b.lmOff && a.lmCam == b.lmCam && a.cmOff == b.cmOff && a.cmLm == b.cmLm && a.cmU == b.cmU,
          "%s: lists differ", what);
    CHECK(a.prA == b.prA && a.prB == b.prB && a.prStart == b.prStart && a.cmPairStart == b.cmPairStart, "%s: pairs differ", what);
    CHECK(a.lpOrder == b.lpOrder && a.nPairsLong == b.nPairsLong && a.nPairsSlots == b.nPairsSlots, "%s: launch order differs", what);
    if (!lmEdgeToo) return true;
    CHECK(a.lmEdge == b.lmEdge, "%s: lmEdge differs", what);
    CHECK(a.nF == b.nF && a.nL == b.nL && a.camIdx == b.camIdx && a.ptIdx == b.ptIdx && a.actCam == b.actCam && a.actPt == b.actPt && a.ptStart == b.ptStart &&
          a.ptEdges == b.ptEdges && a.camStart == b.camStart && a.camEdges == b.camEdges, "%s: active structure differs", what);
    return true;
}

// long pairs before short ones, every pair once, slots a multiple of 8 padded with -1, a camera's pairs in one XCD column or two adjacent ones
static bool check_launch_order(const Out& o, int kLong, const char* what) {
    const int nz = (int)o.prA.size();
    ivec seen(nz, 0);
    CHECK(o.nPairsLong % 8 == 0 && o.nPairsSlots % 8 == 0 && o.nPairsLong <= o.nPairsSlots && (size_t)o.nPairsSlots <= o.lpOrder.size(), "%s: slot counts", what);
    int nLong = 0;
    for (int k = 0; k < nz; k++) nLong += o.prStart[k + 1] - o.prStart[k] > kLong ? 1 : 0;
    CHECK(nLong > 0 && nLong < nz, "%s: both classes must be non-empty for this check (%d of %d long)", what, nLong, nz);
    std::vector<std::pair<int, int>> cols(2 * (size_t)o.nFa, {8, -1});      // per class and camera: first and last XCD column
    for (int sl = 0; sl < o.nPairsSlots; sl++) {
        const int k = o.lpOrder[sl];
        if (k == -1) continue;
        CHECK(k >= 0 && k < nz, "%s: slot %d holds %d", what, sl, k);
        const bool isLong = o.prStart[k + 1] - o.prStart[k] > kLong;
        CHECK(isLong == (sl < o.nPairsLong), "%s: pair %d in the wrong class", what, k);
        seen[k]++;
        auto& c = cols[2 * (size_t)o.prA[k] + (isLong ? 1 : 0)];
        c.first = std::min(c.first, sl % 8); c.second = std::max(c.second, sl % 8);
    }
    for (int k = 0; k < nz; k++) CHECK(seen[k] == 1, "%s: pair %d appears %d times", what, k, seen[k]);
    for (const auto& c : cols) CHECK(c.second - c.first <= 1, "%s: a camera's pairs span XCD columns %d .. %d", what, c.first, c.second);
    return true;
}

static bool check_map(const Map& m, const char* name, int wantFree, bool wantAllChunks, int wantRanges, int kLong) {
    const EdgeView v = m.view();
    const Out serial = run_setup(m, SERIAL, 1, kLong);
    if (!check_against_reference(m, serial, name)) return false;
    CHECK(!serial.sessionOpen && !serial.countedInChunks, "%s: the serial form took a session", name);
    CHECK(serial.nFa == wantFree, "%s: %d free cameras with edges, %d wanted", name, serial.nFa, wantFree);
    CHECK(std::max(1, std::min(16, serial.nFa / 32)) == wantRanges, "%s: %d free cameras do not give %d camera ranges", name, serial.nFa, wantRanges);
    if (kLong > 0 && !check_launch_order(serial, kLong, name)) return false;
    for (int threads : {2, 5, 12}) {
        const std::string tag = std::string(name) + ", " + std::to_string(threads) + " threads";
        const Out run = run_setup(m, RUN, threads, kLong);
        CHECK(!run.sessionOpen, "%s: the run form opened a session", tag.c_str());
        if (!same_arrays(serial, run, (tag + ", crew run").c_str())) return false;
        const Out session = run_setup(m, SESSION, threads, kLong);
        CHECK(session.sessionOpen && session.countedInChunks, "%s: no session / no chunked count", tag.c_str());
        if (!same_arrays(serial, session, (tag + ", crew session").c_str())) return false;
    }
    int nonEmpty = 0;      // (the chunk table of the last session form)
    for (int q = 0; q < kSetupChunks; q++) nonEmpty += g_scratch.cb[q + 1] > g_scratch.cb[q] ? 1 : 0;
    CHECK(wantAllChunks ? nonEmpty == kSetupChunks : nonEmpty < kSetupChunks, "%s: %d of %d chunks non-empty (%d edges)", name, nonEmpty, kSetupChunks, v.E());
    return true;
}

static bool check_refusal(const Map& bad, const std::string& want, const char* what) {
    for (Form form : {SERIAL, SESSION}) {
        const Out o = run_setup(bad, form, 5);
        CHECK(!o.ok && o.err == want, "%s (%s form): \"%s\" where \"%s\" was expected", what, form == SERIAL ? "serial" : "session", o.ok ? "accepted" : o.err.c_str(), want.c_str());
        CHECK(form == SERIAL || o.sessionOpen, "%s: no session", what);
    }
    return true;
}

int main() {
    // map 1: 45 free cameras with edges (not a multiple of the pair stage's four cameras per chunk), all 48 chunks of the edge list non-empty, one camera range
    const Map m1 = make_map(45, 600, 9, 5, 101);
    if (!check_map(m1, "map 1", 45, true, 1, 6)) return 1;
    // map 2: 70 free cameras: two camera ranges in the serial camera scatter
    const Map m2 = make_map(70, 500, 7, 4, 202);
    if (!check_map(m2, "map 2", 70, true, 2, 5)) return 1;
    // map 3: fewer edges than chunks
    const Map m3 = make_map(6, 14, 4, 3, 303);
    if ((int)m3.ecam.size() >= kSetupChunks) { std::fprintf(stderr, "FAILED: map 3 has %zu edges\n", m3.ecam.size()); return 1; }
    if (!check_map(m3, "map 3", 6, false, 1, 0)) return 1;
    const Out ordered = run_setup(m1, SERIAL, 1);
    {   // shuffled edges: the serial fall-back under a session; pairs, counts and lpEntries of the ordered twin (edge numbers differ)
        const Map ms = shuffled(m1, 404);
        for (Form form : {SERIAL, SESSION}) {
            const Out o = run_setup(ms, form, 5);
            if (!check_against_reference(ms, o, "map 1 shuffled")) return 1;
            if (o.countedInChunks) { std::fprintf(stderr, "FAILED: a shuffled edge list was counted in chunks\n"); return 1; }
            if (!same_arrays(ordered, o, "map 1 shuffled against its ordered twin", false)) return 1;
        }
    }
    {   // plane edges (serial form): landmarks = points then planes, edges = point edges then plane edges
        Map mp = m1;
        mp.nPl = 3;
        mp.pcam = {1, 12, 30, 2, 12, 8, 40, 41}; mp.ppl = {0, 0, 0, 1, 1, 2, 2, 2};
        const Out o = run_setup(mp, SERIAL, 1);
        if (!check_against_reference(mp, o, "map 1 with plane edges")) return 1;
        const Out s = run_setup(mp, SESSION, 5);      // (a session, but plane edges keep the count serial)
        if (s.countedInChunks) { std::fprintf(stderr, "FAILED: plane edges were counted in chunks\n"); return 1; }
        if (!same_arrays(o, s, "map 1 with plane edges, session")) return 1;
    }
    {   // the malformed lists the library refuses: the same words from the serial walk and from the chunks of a session
        const int Ept = (int)m1.ecam.size();
        if (Ept <= 1235) { std::fprintf(stderr, "FAILED: map 1 has only %d edges\n", Ept); return 1; }
        Map bad = m1; bad.ecam[1234] = m1.nC;
        if (!check_refusal(bad, "edge 1234 out of range", "camera index == nC")) return 1;
        bad = m1; bad.ept[0] = -1;
        if (!check_refusal(bad, "edge 0 out of range", "landmark -1")) return 1;
        bad = m1;
        const int e = 1000;
        bad.ecam.insert(bad.ecam.begin() + e + 1, m1.ecam[e]); bad.ept.insert(bad.ept.begin() + e + 1, m1.ept[e]);
        if (!check_refusal(bad, "two edges join camera " + std::to_string(m1.ecam[e]) + " and point " + std::to_string(m1.ept[e]), "duplicated edge")) return 1;
        bad = m1;
        const int s = (int)((long long)Ept * 17 / 48);      // chunk 17 of the session's count starts exactly here once the two entries differ
        bad.ept[s - 1] = -1000000; bad.ept[s] = -999999;
        if (!check_refusal(bad, "edge " + std::to_string(s - 1) + " out of range", "two ascending negative landmarks across a chunk boundary")) return 1;
    }
    {   // launch order, overflow: one camera holds most of the pairs -- the deal would need more slots than there are, so the plain order
        const int nz = 200, kLong = 3;
        ivec lpStart(nz + 1, 0), lpPair(2 * nz), order(2 * nz + 64, -7);
        for (int k = 0; k < nz; k++) { lpPair[2 * k] = k < 190 ? 0 : k - 189; lpPair[2 * k + 1] = k; lpStart[k + 1] = lpStart[k] + (k % 3 == 0 ? 5 : 2); }
        int nLong = 0, nSlots = 0;
        deal_launch_order(lpStart.data(), lpPair.data(), nz, kLong, order.size(), g_scratch, order.data(), nLong, nSlots);
        int at = 0;
        bool plain = nSlots == nz;
        for (int k = 0; k < nz && plain; k++) if (k % 3 == 0) plain = order[at++] == k;
        plain = plain && nLong == at;
        for (int k = 0; k < nz && plain; k++) if (k % 3 != 0) plain = order[at++] == k;
        if (!plain) { std::fprintf(stderr, "FAILED: overflow case did not give the plain launch order (%d long, %d slots)\n", nLong, nSlots); return 1; }
    }
    std::printf("ba set-up: three maps in three forms at 2, 5 and 12 threads, shuffled edges, plane edges, four refusals, launch order: all as the reference\n");
    return g_failed ? 1 : 0;
}
