// lm_host.hip -- host side of the Levenberg-Marquardt engine: per-thread contexts, BAJob (arena, pinned mirror, uploads, tile structure, host-stepped trials; its set-up
// stages that need no device -- validation, the map-scale path's covisibility structure, the active structure, the launch order -- are ba_setup.h, plain C++),
// eao_local_ba / eao_local_ba_batch (BABatch: one call's windows and groups with its stages as members -- worker, lead, finish_window, join -- over BABatchPool and the
// plan of ba_batch_plan.h, plain C++) / eao_bundle_adjustment(_planes) and the traces.  Kernels: lba.hip, gba.hip (launched through BALaunch).  Shared pieces:
// lm_internal.h.  (Round 6: split out of csrc/lm.hip.)
#include "lm_internal.h"
#include "ba_setup.h"
#include "ba_batch_plan.h"

namespace eao {
namespace lm {
thread_local LMTraceHost g_trace;
thread_local LMContext g_ctx;

eao_status ctx_init(LMContext& c, bool ownStream, eao::StreamClass cls) {
    eao_status st = eao::require_device();
    if (st) return st;
    if (ownStream) {
        hipStream_t& q = c.byClass[(int)cls];
        if (!q) EAO_HIP(eao::create_stream(&q, cls));
        c.stream = q;
        if (!c.ev0) {
            EAO_HIP(hipEventCreate(&c.ev0));
            EAO_HIP(hipEventCreate(&c.ev1));
        }
    }
    if (!c.status) {
        EAO_HIP(hipHostMalloc((void**)&c.status, sizeof(BAStatus), hipHostMallocMapped));
        std::memset(c.status, 0, sizeof(BAStatus));
    }
    return EAO_OK;
}
}  // namespace lm
}  // namespace eao

// mode 0: Optimizer::LocalBundleAdjustment (two passes with the outlier pass between them, Huber kernels in the first).
// mode 1: Optimizer::BundleAdjustment over keyframes and map points (src/Optimizer.cc:55-323): ONE optimize(its_first) call,
//         Huber kernels only when `robust`, delta_mono = sqrt(5.99) (:94), no outlier pass, no observation is erased.
//         With `pl`: the MapPlane vertices / EdgePlane edges of :203-252 ride along as landmarks nPo.. / edges Ept.. .
namespace {


// One window in flight: LocalBundleAdjustment / BundleAdjustment of one problem on one context (device arena + pinned mirrors).
// The uploads of a batch group: window y of the launch is copied from its pinned host mirror (read over PCIe by the kernel itself) into
// its device arena, 16 bytes per lane.  Both ends are 16-byte aligned (arena offsets are multiples of 256).
struct BAUploadArgs { unsigned char* dst[8]; const unsigned char* src[8]; unsigned long long n16[8]; };
__global__ __launch_bounds__(256) void k_ba_upload(BAUploadArgs A) {
    const int w = blockIdx.y;
    const uint4* __restrict__ s = reinterpret_cast<const uint4*>(A.src[w]);
    uint4* __restrict__ d = reinterpret_cast<uint4*>(A.dst[w]);
    const unsigned long long n = A.n16[w];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) d[i] = s[i];
}

struct BAJob {
    const eao_ba_problem* p = nullptr; const volatile uint8_t* stop = nullptr; eao_ba_result* r = nullptr;
    int mode = 0, robust = 1; const eao_ba_planes* pl = nullptr; float* planes_out = nullptr;
    LMContext* c = nullptr; LMTraceHost* tr = nullptr;
    int nPo = 0, nPl = 0, Ept = 0, Epl = 0, nC = 0, nP = 0, E = 0;
    bool hasPl = false, trivial = false, chained = false, pollStop = false, lazy = false;
    int nPairsLong = 0, nPairsSlots = 0;      // map-scale path: launch slots (lpOrder) of the four-wave assembly kernel / of both kernels
    BADev D; BADev* dW = nullptr;
    BALaunch L;
    int curHost = 0;
    SE3* outCams = nullptr; double* outPts = nullptr; double* outPlanes = nullptr; unsigned char* outCls = nullptr;

    void write_records(BADev* dst) const {      // the two records of this window (see BA_WIN)
        dst[0] = D; dst[0].ctl = D.ctl0; dst[0].lm = D.lm0;
        dst[1] = D; dst[1].ctl = D.ctl0 + 8; dst[1].lm = D.lm0 + 8;
    }
    bool batchable() const { return !trivial && chained && L.d.usePairs && L.d.solveTiles && !hasPl && !L.d.bigPath && D.nFree > 0 && D.nL > 0 && mode == 0; }

    // ---- prepare(): validation, arena, pinned mirror, upload (two copies on `s`), active structure.  No kernel is launched here.  The stages that need no device
    //      (counts, covisibility lists and pairs, active structure, launch order) are the free functions of ba_setup.h; the members below are the ones that need
    //      the window record, the arena, the context and the HIP runtime.
    // deferUpload (batches): NO call into the HIP runtime at all -- the pinned mirror is filled and [upSrc, upSrc + upBytes) is left
    // for the group's leader, which moves every window of its group with ONE launch of k_ba_upload (the copies' enqueue calls
    // serialise inside the runtime: 50 of them were most of a batch's 0.55 ms of set-up, and more host threads made it worse).
    const unsigned char* upSrc = nullptr; unsigned char* upDst = nullptr; size_t upBytes = 0;
    bool bigPath = false;      // the map-scale path: dense system in HBM factorised by the whole chip (k_bal_*)
    int nFreeIn = 0;           // free keyframes of the problem (with or without edges)
    bool pair_path() const { return !bigPath && nFreeIn > 0 && nFreeIn <= kTileMaxFree; }

    // The uploaded part of the window's arena, slice by slice: device addresses, and host() = the same slice in the pinned mirror (filled in place, sent with two copies).
    struct Carve {
        unsigned char* base = nullptr; unsigned char* pin = nullptr;
        size_t off0 = 0, off1 = 0;      // the uploaded part is [off0, off1)
        float* obs; float* info; int* ecam; int* ept; SE3* cams; double* pts; unsigned char* flag;
        int* camIdx; int* ptIdx; int* actCam; int* actPt; int* ptStart; int* ptEdges; int* camStart; int* camEdges;
        int* ctl;      // two control blocks: see BADecision
        int* lpStart; int* lpPair; int* lpOrder; size_t lpOrderCap;
        size_t nObs;      // (observer list entries + 1)
        int* lmOff; int* lmCam; int* lmEdge; int* cmOff; int* cmLm; int* cmU;
        int* bigTile; int4* bigWork; int* bigRow; int* bigRowCam; int4* bigSB; int* bigDiagList;
        double* pl0; double* pmeas;
        template <typename T> T* host(T* dev) const { return reinterpret_cast<T*>(pin + (reinterpret_cast<unsigned char*>(dev) - base)); }
    };

    eao_status check_arguments() {
        EAO_REQUIRE(p && r && r->cam_Tcw && r->points && (p->n_edges == 0 || r->edge_outlier || mode == 1), "null argument");
        EAO_REQUIRE(p->n_cams > 0 && p->n_points >= 0 && p->n_edges >= 0, "bad sizes");
        if (pl && pl->n_planes <= 0) pl = nullptr;
        EAO_REQUIRE(!pl || (mode == 1 && pl->plane_world && planes_out && pl->n_pedges >= 0 && (pl->n_pedges == 0 || (pl->pedge_plane && pl->pedge_cam && pl->pedge_obs))),
                    "bad plane arguments");
        nPo = p->n_points; nPl = pl ? pl->n_planes : 0; Ept = p->n_edges; Epl = pl ? pl->n_pedges : 0;
        nC = p->n_cams; nP = nPo + nPl; E = Ept + Epl;          // landmarks = points then planes, edges = point edges then plane edges
        hasPl = nPl > 0;
        return EAO_OK;
    }
    EdgeView edge_view() const {
        EdgeView v;
        v.nC = nC; v.nPo = nPo; v.nPl = nPl; v.Ept = Ept; v.Epl = Epl;
        v.edge_cam = p->edge_cam; v.edge_point = p->edge_point; v.cam_fixed = p->cam_fixed;
        v.pedge_cam = pl ? pl->pedge_cam : nullptr; v.pedge_plane = pl ? pl->pedge_plane : nullptr;
        return v;
    }
    void abort_shortcut() {  // src/Optimizer.cc:961-963: nothing is optimised; poses go through the same SE3 round trip
        r->aborted = 1;
        for (int i = 0; i < nC; i++) se3_to_Tcw_f32(se3_from_Tcw_f32(p->cam_Tcw + 16 * i), r->cam_Tcw + 16 * i);
        for (size_t i = 0; i < (size_t)nPo * 3; i++) r->points[i] = p->points[i];
        for (int i = 0; i < nPl; i++) { double c4[4]; plane_from_f32(pl->plane_world + 4 * i, c4); for (int k = 0; k < 4; k++) planes_out[4 * i + k] = (float)c4[k]; }
        if (Ept && r->edge_outlier) std::memset(r->edge_outlier, 0, Ept);
        trivial = true;
    }

    // ---- the ORDER, TILE structure and launch SCHEDULE of the map-scale system (GbaPlan, gba.hip; round 5 built the tile structure here in natural keyframe order):
    //      which 64 x 64 tiles of the lower triangle can ever be non-zero -- the tiles a covisible camera pair's 6 x 6 block touches in the elimination order, the
    //      diagonal, the tile row of the right-hand side, and the fill-in of the elimination worked out at tile level (the block form of the symbolic factorisation a
    //      sparse LDL^T starts with, solvers/linear_solver_eigen.h:95-112).  Memory and the launches' grids follow this structure.  The plan is a pure function of
    //      the pair list; the context keeps it while the list's hash stays the same (it is read by the launches of this window, long after prepare has returned).
    eao_status update_plan(const SetupScratch& S, bool hostStamps) {
        GbaPlan& plan = c->plan;
        const int nFa = S.nFa;
        const int forceP = getenv("EAO_BA_ND") ? atoi(getenv("EAO_BA_ND")) : 0;      // (read per call: A/B runs and the tests -- 1 = natural order, p > 1 = p segments)
        const uint64_t key = gba_pattern_hash(nFa, S.prA, S.prB) ^ ((uint64_t)(unsigned)forceP << 48);
        if (!plan.valid || plan.key != key || plan.nFa != nFa) {
            gba_build_plan(nFa, S.prA, S.prB, forceP, plan);
            plan.key = key; plan.valid = true;
            if (hostStamps) fprintf(stderr, "[eao map-scale plan] %d free keyframes (bandwidth %d%s): %d segment(s), %d separator keyframes, %d rows in %d tiles; %zu factorisation launches "
                                    "(natural order: %d), %zu back-substitution launches, %zu work records\n", nFa, plan.bandwidth, plan.rcm ? ", reverse Cuthill-McKee line" : "", plan.P,
                                    plan.nSep, plan.N, plan.bigTiles, plan.launches.size(), plan.chainNatural, plan.sbLaunches.size(), plan.work.size() / 2);
        }
        EAO_REQUIRE(plan.work.size() < ((size_t)1 << 28), "tile structure too large (%zu work records)", plan.work.size() / 2);
        return EAO_OK;
    }

    void start_record() {      // the window record's scalars
        std::memset(&D, 0, sizeof(D));
        D.nCams = nC; D.nPts = nP; D.nEdges = E;
        D.cam.fx = p->fx; D.cam.fy = p->fy; D.cam.cx = p->cx; D.cam.cy = p->cy; D.cam.bf = p->bf; D.cam.bf_f = p->bf;
        D.cam.deltaMono = (float)std::sqrt(mode == 1 ? refc::GBA_HUBER2_MONO : refc::LBA_HUBER2_MONO);
        D.cam.deltaStereo = (float)std::sqrt(mode == 1 ? refc::GBA_HUBER2_STEREO : refc::LBA_HUBER2_STEREO);
        D.nPtsOnly = nPo; D.nEdgesPt = Ept;
        D.deltaPlane = (float)std::sqrt(refc::PLANE_CHI2); D.infoAngle = refc::PLANE_ANGLE_INFO / (1.0 * 1.0); D.infoDist = refc::PLANE_DIST_INFO_ROOT * refc::PLANE_DIST_INFO_ROOT;   // src/Optimizer.cc:203-208
        D.status = c->status;
    }

    // Sizes the context's arena for this problem and cuts it up: the size formula and the carve it must cover, one after the other (a.off <= a.cap is checked at
    // the end).  First the uploaded part (problem, initial state, adjacency, zeroed control block, the window record itself: into `k`, mirrored in pinned host
    // memory), then the device-only part (straight into the window record D).
    eao_status carve_arena(const SetupScratch& S, Carve& k) {
        LMContext& c = *this->c;
        const GbaPlan& plan = c.plan;
        const size_t lpEntries = bigPath ? S.lpEntries : 0, lpPairsMax = bigPath ? S.prA.size() : 0;
        const int bigT = bigPath ? plan.T : 0, bigTiles = bigPath ? plan.bigTiles : 0;
        eao_status st;
        size_t need = 0;
        need += (size_t)E * (3 * 4 + 4 + 4 + 4 + 1 + 4 + 4 + 4 + 1 + 24 + 18 * 8);
        need += (size_t)nP * (3 + 3 + 9 + 3 + 3 + 1 + 1) * 8 + (size_t)nP * 16 + (bigPath ? 64 : (size_t)nP * nC * 4);
        need += (size_t)nC * (2 * sizeof(SE3) + 36 * 8 + 6 * 8 + 6 * 8 + 16);
        need += (size_t)nP * 8 * sizeof(int4) + 256;
        need += (size_t)nP * 9 * 8 + 2048 + 256;      // Tl, ul, the zero block
        need += 128 * 256 + (size_t)nPl * 4 * 8 * 2 + (size_t)Epl * 4 * 8 + 2 * sizeof(BADev) + (size_t)nP + 1024;     // (+ k_ba_backsub's workgroup sums)
        if (bigPath) {
            need += (2 * ((size_t)bigTiles << 12) + 2 * (size_t)plan.N * kBigNB) * 8;
            need += (3 * lpEntries + 5 * lpPairsMax + 72 + 4 * (S.lmCam.size() + 2) + (size_t)nP + nC + 16) * 4 + (plan.tileMap.size() + plan.rowOf.size() + plan.rowCam.size() + plan.diagList.size() + 8) * 4 + (plan.work.size() + plan.sb.size()) * sizeof(int4) + 4096;
        } else {
            need += 2 * ((size_t)(nC * 6 + 6) * (nC * 6 + 34) + 8) * 8;
            need += (size_t)nC * (nC + 1) / 2 * ((size_t)nP + 64) * (4 + 16);   // landmark lists / item records of the camera pairs
            need += (size_t)nP * 9 * 8 + 1024;
            need += (size_t)nC * (nC + 1) / 2 * 4;
        }
        if ((st = c.bytes.reserve(need))) return st;
        if (bigPath && getenv("EAO_DEBUG_STAMPS"))
            fprintf(stderr, "[eao map-scale arena] %.1f MB for this problem (%d x %d tile grid, %d live tiles = %.1f MB in the two pools, %zu work records), context arena %.1f MB\n",
                    need / 1e6, bigT, bigT, bigTiles, 2.0 * bigTiles * 32768 / 1e6, plan.work.size() / 2, c.bytes.n / 1e6);
        Arena a{c.bytes.p, c.bytes.n};
        // ---- the uploaded part
        k.base = a.base; k.off0 = a.off;
        k.obs = a.take<float>((size_t)E * 3); k.info = a.take<float>(E);
        k.ecam = a.take<int>(E); k.ept = a.take<int>(E);
        k.cams = a.take<SE3>(nC);
        k.pts = a.take<double>((size_t)nP * 3);
        k.flag = a.take<unsigned char>(E);
        k.camIdx = a.take<int>(nC); k.ptIdx = a.take<int>(nP); k.actCam = a.take<int>(nC); k.actPt = a.take<int>(nP);
        k.ptStart = a.take<int>(nP + 1); k.ptEdges = a.take<int>(E); k.camStart = a.take<int>(nC + 1); k.camEdges = a.take<int>(E);
        k.ctl = a.take<int>(16);
        k.lpOrderCap = 2 * lpPairsMax + 64;
        k.lpStart = a.take<int>(bigPath ? lpPairsMax + 1 : 1);
        k.lpPair = a.take<int>(bigPath ? 2 * lpPairsMax : 1);
        k.lpOrder = a.take<int>(bigPath ? k.lpOrderCap : 1);
        k.nObs = bigPath ? S.lmCam.size() : 1;
        k.lmOff = a.take<int>(bigPath ? (size_t)nP + 1 : 1); k.lmCam = a.take<int>(k.nObs); k.lmEdge = a.take<int>(k.nObs);
        k.cmOff = a.take<int>(bigPath ? S.cmOff.size() : 1); k.cmLm = a.take<int>(k.nObs); k.cmU = a.take<int>(k.nObs);
        k.bigTile = a.take<int>(bigPath ? plan.tileMap.size() : 1);
        k.bigWork = a.take<int4>(bigPath ? std::max<size_t>(plan.work.size(), 1) : 1);
        k.bigRow = a.take<int>(bigPath ? std::max<size_t>(plan.rowOf.size(), 1) : 1);
        k.bigRowCam = a.take<int>(bigPath ? std::max<size_t>(plan.rowCam.size(), 1) : 1);
        k.bigSB = a.take<int4>(bigPath ? std::max<size_t>(plan.sb.size(), 1) : 1);
        k.bigDiagList = a.take<int>(bigPath ? std::max<size_t>(plan.diagList.size(), 1) : 1);
        k.pl0 = a.take<double>((size_t)nPl * 4 + 1);
        k.pmeas = a.take<double>((size_t)Epl * 4 + 1);
        dW = a.take<BADev>(2);
        k.off1 = eao::align256(a.off);
        // ---- device-only part
        D.table = bigPath ? nullptr : a.take<int>((size_t)nP * nC);      // (the map-scale path finds a landmark's edges in its pair lists)
        D.lpPts = a.take<int>(bigPath ? lpEntries : 1);                  // (filled by k_bal_pair_fill)
        D.lpE1 = a.take<int>(bigPath ? lpEntries : 1);
        D.lpE2 = a.take<int>(bigPath ? lpEntries : 1);
        D.slot = a.take<int4>((size_t)std::max(nP, 1) * 8);
        D.camEdgeL = a.take<int>(E);
        const bool pairPath = pair_path();
        const int nPairsMax = nFreeIn * (nFreeIn + 1) / 2;
        D.pairCnt = a.take<int>(bigPath ? 1 : std::max(nPairsMax, 1));
        D.pairPts = a.take<int>(pairPath ? (size_t)nPairsMax * std::max(nP, 1) : 1);
        const bool wmode = pairPath && !hasPl;
        D.wmode = wmode ? 1 : 0;
        D.pairItems = a.take<int4>(wmode ? (size_t)nPairsMax * std::max(nP, 1) : 1);
        D.Tl = a.take<double>((size_t)std::max(nP, 1) * 6); D.ul = a.take<double>(((size_t)std::max(nP, 1) + 1) * 3);
        D.cls = a.take<unsigned char>(E);
        D.camsBuf[0] = k.cams; D.camsBuf[1] = a.take<SE3>(nC);
        D.ptsBuf[0] = k.pts; D.ptsBuf[1] = a.take<double>((size_t)nP * 3);
        D.plBuf[0] = k.pl0; D.plBuf[1] = a.take<double>((size_t)nPl * 4 + 1); D.pmeas = k.pmeas;
        D.err = a.take<double>((size_t)E * 3);
        D.Hpp = a.take<double>((size_t)nC * 36); D.bp = a.take<double>((size_t)nC * 6);
        D.Hll = a.take<double>((size_t)nP * 9); D.bl = a.take<double>((size_t)nP * 3);
        D.Hpl = a.take<double>(((size_t)E + 1) * 18);      // (+ the zero block of k_ba_schur_pairs_mfma)
        D.sys = a.take<double>(bigPath ? 8 : std::max((size_t)(nFreeIn * 6) * (nFreeIn * 6 + 1), (size_t)tile_geom(std::max(nFreeIn, 1)).nTiles * 256) + 8);
        D.big = a.take<double>(bigPath ? ((size_t)bigTiles << 12) : 8);
        D.bigL = a.take<double>(bigPath ? ((size_t)bigTiles << 12) : 8);
        D.bigTile = k.bigTile; D.bigT = bigT; D.bigTiles = bigTiles; D.bigWork = k.bigWork; D.bigDense = bigPath && bigTiles == bigT * (bigT + 1) / 2 ? 1 : 0;
        D.bigDiag = a.take<double>(bigPath ? (size_t)plan.N * kBigNB : 8);
        D.bigLinv = a.take<double>(bigPath ? (size_t)plan.N * kBigNB : 8);
        D.bigN = bigPath ? plan.N : 0; D.bigRow = k.bigRow; D.bigRowCam = k.bigRowCam; D.bigSB = k.bigSB; D.bigDiagList = k.bigDiagList;
        D.bigFail = a.take<int>(4);
        D.lpStart = k.lpStart; D.lpPair = k.lpPair; D.lpOrder = k.lpOrder;
        D.lmOff = k.lmOff; D.lmCam = k.lmCam; D.lmEdge = k.lmEdge; D.cmOff = k.cmOff; D.cmLm = k.cmLm; D.cmU = k.cmU;
        D.xp = a.take<double>((size_t)nC * 6); D.xl = a.take<double>((size_t)nP * 3);
        D.partChi = a.take<double>(nP); D.partScale = a.take<double>(nP);
        D.lm0 = a.take<double>(16);
        D.solveOk = a.take<int>(4);
        D.doneCnt = a.take<int>(4);
        D.wgPart = a.take<double>(2 * (size_t)eao::cdiv(std::max(nP, 1) * 8, 256) + 2);
        long long* ddbg = a.take<long long>(32);
        D.dbg = getenv("EAO_DEBUG_STAMPS") ? ddbg : nullptr;
        EAO_REQUIRE(a.off <= a.cap, "internal: arena overflow");
        D.obs = k.obs; D.info = k.info; D.ecam = k.ecam; D.ept = k.ept; D.eflag = k.flag;
        D.camIdx = k.camIdx; D.ptIdx = k.ptIdx; D.actCam = k.actCam; D.actPt = k.actPt;
        D.ptStart = k.ptStart; D.ptEdges = k.ptEdges; D.camStart = k.camStart; D.camEdges = k.camEdges;
        D.ctl0 = k.ctl; D.ctl = k.ctl; D.lm = D.lm0;
        if ((st = c.pin.reserve(k.off1))) return st;
        k.pin = c.pin.p;
        return EAO_OK;
    }
    eao_status reserve_results() {      // pinned results, written by k_ba_finish
        LMContext& c = *this->c;
        eao_status st;
        const size_t outBytes = (size_t)nC * sizeof(SE3) + (size_t)nP * 24 + (size_t)nPl * 32 + (((size_t)E + 15) & ~(size_t)15) + 64;
        if ((st = c.pinOut.reserve(outBytes))) return st;
        outCams = (SE3*)c.pinOut.p;
        outPts = (double*)(c.pinOut.p + (((size_t)nC * sizeof(SE3) + 15) & ~(size_t)15));
        outPlanes = outPts + (size_t)nP * 3;
        outCls = (unsigned char*)(outPlanes + (size_t)nPl * 4);
        D.outCams = outCams; D.outPts = outPts; D.outPlanes = outPlanes; D.outCls = outCls;
        return EAO_OK;
    }

    // the problem itself (observations, indices, initial state, flags, zeroed control block) into the pinned mirror
    void pack_problem(const EdgeView& v, const Carve& k, Workers& crew) {
        unsigned char* const hf = k.host(k.flag);      // edge flags: bit0 stereo, bit2 robust kernel present (bit1 = level 1 is only ever set on the device)
        double* const hp = k.host(k.pts);
        {
            unsigned char* const hobs = (unsigned char*)k.host(k.obs); unsigned char* const hinfo = (unsigned char*)k.host(k.info);
            unsigned char* const hecam = (unsigned char*)k.host(k.ecam); unsigned char* const hept = (unsigned char*)k.host(k.ept);
            const eao_ba_problem* const pp = p;
            const int Ept_ = Ept, nPo_ = nPo; const unsigned char rb = robust ? 4 : 0;
            const int nPack = crew.open ? 16 : 1;
            crew.pass(0, nPack, [=](int q) {
                const size_t e0 = (size_t)Ept_ * q / nPack, e1 = (size_t)Ept_ * (q + 1) / nPack;
                std::memcpy(hobs + e0 * 12, pp->edge_obs + e0 * 3, (e1 - e0) * 12);
                std::memcpy(hinfo + e0 * 4, pp->edge_inv_sigma2 + e0, (e1 - e0) * 4);
                std::memcpy(hecam + e0 * 4, pp->edge_cam + e0, (e1 - e0) * 4);
                std::memcpy(hept + e0 * 4, pp->edge_point + e0, (e1 - e0) * 4);
                for (size_t e = e0; e < e1; e++) hf[e] = (unsigned char)((!(pp->edge_obs[3 * e + 2] < 0) ? 1 : 0) | rb);
                for (size_t i = (size_t)nPo_ * 3 * q / nPack, i1 = (size_t)nPo_ * 3 * (q + 1) / nPack; i < i1; i++) hp[i] = pp->points[i];
            });
        }
        if (hasPl) {
            std::memset(k.host(k.obs) + (size_t)Ept * 3, 0, (size_t)Epl * 12);
            std::memset(k.host(k.info) + (size_t)Ept, 0, (size_t)Epl * 4);
            int* hc2 = k.host(k.ecam); int* hp2 = k.host(k.ept);
            for (int e = Ept; e < E; e++) { hc2[e] = v.cam(e); hp2[e] = v.lm(e); }
            double* hpl = k.host(k.pl0); double* hpm = k.host(k.pmeas);
            for (int i = 0; i < nPl; i++) plane_from_f32(pl->plane_world + 4 * i, hpl + 4 * i);          // Converter::toPlane3D (:217)
            for (int e = 0; e < Epl; e++) plane_from_f32(pl->pedge_obs + 4 * e, hpm + 4 * e);           // (:239)
        }
        SE3* hc = k.host(k.cams);
        for (int i = 0; i < nC; i++) hc[i] = se3_from_Tcw_f32(p->cam_Tcw + 16 * i);
        for (size_t i = (size_t)nPo * 3; i < (size_t)nP * 3; i++) hp[i] = 0;
        for (int e = Ept; e < E; e++) hf[e] = 8 | 4;      // EdgePlane: always a Huber kernel (:246-248)
        std::memset(k.host(k.ctl), 0, 16 * sizeof(int));
    }

    // map-scale path, into the pinned mirror: the plan's tables, the covisibility CSR (for every camera pair (i1 <= i2) sharing a landmark where its entries start;
    // the diagonal pairs carry each camera's own landmarks), the observer lists (they travel instead of the pairs' entries: k_bal_pair_fill writes those on the
    // device) and the launch order of the pair kernels.  All of it was worked out before the arena was sized.
    eao_status fill_map_scale_mirror(SetupScratch& S, const Carve& k, Workers& crew) {
        const GbaPlan& plan = c->plan;
        const int nF = D.nFree;
        int* lpStart = k.host(k.lpStart); int* lpPair = k.host(k.lpPair);
        EAO_REQUIRE(plan.valid && plan.nFa == nF && plan.T == D.bigT, "internal: tile structure built for another system size");
        std::memcpy(k.host(k.bigTile), plan.tileMap.data(), plan.tileMap.size() * sizeof(int));
        if (!plan.work.empty()) std::memcpy(k.host(k.bigWork), plan.work.data(), plan.work.size() * sizeof(int4));
        std::memcpy(k.host(k.bigRow), plan.rowOf.data(), plan.rowOf.size() * sizeof(int));
        std::memcpy(k.host(k.bigRowCam), plan.rowCam.data(), plan.rowCam.size() * sizeof(int));
        if (!plan.sb.empty()) std::memcpy(k.host(k.bigSB), plan.sb.data(), plan.sb.size() * sizeof(int4));
        if (!plan.diagList.empty()) std::memcpy(k.host(k.bigDiagList), plan.diagList.data(), plan.diagList.size() * sizeof(int));
        EAO_REQUIRE((int)S.cmPairStart.size() == nF + 1, "internal: covisibility structure built for another set of free keyframes");
        const int nz = (int)S.prA.size();
        for (int i = 0; i < nz; i++) { lpPair[2 * i] = S.prA[i]; lpPair[2 * i + 1] = S.prB[i]; }
        std::memcpy(lpStart, S.prStart.data(), ((size_t)nz + 1) * sizeof(int));
        EAO_REQUIRE((int)S.lmOff.size() == nP + 1 && (int)S.cmOff.size() == nF + 1 && S.lmCam.size() == k.nObs && S.cmLm.size() + 1 == k.nObs, "internal: observer lists built for another problem");
        {
            int* const hLmOff = k.host(k.lmOff); int* const hLmCam = k.host(k.lmCam); int* const hLmEdge = k.host(k.lmEdge);
            int* const hCmOff = k.host(k.cmOff); int* const hCmLm = k.host(k.cmLm); int* const hCmU = k.host(k.cmU);
            const int* const lmOffp = S.lmOff.data(); const int* const lmCamp = S.lmCam.data(); const int* const lmEdgep = S.lmEdge.data();
            const int* const cmOffp = S.cmOff.data(); const int* const cmLmp = S.cmLm.data(); const int* const cmUp = S.cmU.data();
            const size_t nO = k.nObs - 1, nPp = (size_t)nP + 1, nFp = (size_t)nF + 1;
            const int nCopy = crew.open ? 12 : 1;
            crew.pass(0, nCopy, [=](int q) {
                auto part = [&](int* dst, const int* src, size_t n) { const size_t i0 = n * q / nCopy, i1 = n * (q + 1) / nCopy; std::memcpy(dst + i0, src + i0, (i1 - i0) * sizeof(int)); };
                part(hLmOff, lmOffp, nPp); part(hLmCam, lmCamp, nO); part(hLmEdge, lmEdgep, nO);
                part(hCmOff, cmOffp, nFp); part(hCmLm, cmLmp, nO); part(hCmU, cmUp, nO);
            });
        }
        D.nPairsNZ = nz;
        const int kLong = getenv("EAO_BA_PAIR_LONG") ? atoi(getenv("EAO_BA_PAIR_LONG")) : kBigPairLong;      // (read per call; tests: the four-wave kernel on small maps)
        deal_launch_order(lpStart, lpPair, nz, kLong, k.lpOrderCap, S, k.host(k.lpOrder), nPairsLong, nPairsSlots);
        return EAO_OK;
    }

    // launch geometry and solver choice of this window; how far optimize() may run ahead of the device
    void set_launch_geometry() {
        const GbaPlan& plan = c->plan;
        const int nF = D.nFree, nL = D.nL;
        BADims& d = L.d;
        d = BADims();
        d.nF = nF; d.nL = nL; d.nP = nP; d.nC = nC; d.E = E; d.nPl = nPl; d.hasPl = hasPl; d.bigPath = bigPath;
        d.usePairs = pair_path() && nF > 0 && nL > 0;
        d.wmode = D.wmode != 0 && d.usePairs;
        if (!d.wmode) D.wmode = 0;
        // solver choice: register tiles + MFMA up to kTileMaxFree free keyframes, the map-scale path beyond
        d.solveTiles = !bigPath && nF > 0 && nF <= kTileMaxFree;
        d.tileLds = tile_solver_lds(std::max(nF, 1));
        d.tiles3 = tile_geom(std::max(nF, 1)).nTiles <= 3 * (kTileThreads / 64);
        d.gB = big_geom(std::max(nF, 1));
        if (bigPath) { d.gB.N = plan.N; d.gB.RP = plan.RP; }
        d.nPairsNZ = D.nPairsNZ; d.nPairsLong = nPairsLong; d.nPairsSlots = nPairsSlots; d.big = D.big; d.bigTiles = D.bigTiles;
        d.plan = bigPath ? &plan : nullptr;
        d.bigCtl0 = D.ctl0;
        d.bigArgs = BigStepArgs{D.big, D.bigL, D.bigDiag, D.bigFail, D.bigWork, D.ctl0, D.dbg, d.gB.N, 0, {}};
        // map-scale runs (tens of milliseconds) are NOT enqueued speculatively when the caller can abort them: optimize() then
        // submits one LM iteration at a time and reads *stop in between, like g2o's forceStopFlag
        pollStop = bigPath && stop != nullptr;
        // ... and never more than two LM iterations ahead of the device otherwise (`lazy`, see optimize()): a map-scale iteration is ~50 launches, and
        // everything enqueued behind a rejected trial drains as no-ops at the launch rate -- 1.5 of 14 ms on the 200-keyframe benchmark map when all ten
        // iterations were enqueued up front
        lazy = bigPath && !pollStop;
        chained = E > 0 && (nF + nL) > 0 && !pollStop && !lazy;
    }
    static void print_laps(const Laps& l) {      // (EAO_DEBUG_STAMPS: host phases of a map-scale set-up, in ms on stderr)
        const double* const t = l.t;
        fprintf(stderr, "[eao map-scale host set-up] observer / camera lists %.3f (counts %.3f, observer scatter %.3f, sort %.3f, camera scatter %.3f), pair counts %.3f, pair list %.3f, order + tiles + symbolic elimination + schedule (GbaPlan; cached per pattern) %.3f ms\n",
                t[5], t[8], t[9] - t[8], t[10] - t[9], t[5] - t[10], t[6] - t[5], t[7] - t[6], t[0] - t[7]);
        fprintf(stderr, "[eao map-scale host set-up] covisibility lists + pairs + plan %.3f, arena + problem pack %.3f, active structure %.3f, pair CSR + launch order %.3f, records + upload enqueue %.3f ms (cumulative %.3f)\n",
                t[0], t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[4]);
    }

    eao_status prepare(hipStream_t s, bool deferUpload = false) {
        eao::Range rg("lm: window set-up + upload");
        eao_status st;
        if ((st = check_arguments())) return st;                                                 // 1. arguments
        LMContext& c = *this->c;
        tr->clear();
        static const bool hostStamps = getenv("EAO_DEBUG_STAMPS") != nullptr;      // host phases of the set-up, in ms on stderr (once per process)
        Laps laps;
        laps.on = hostStamps;
        r->iters[0] = r->iters[1] = 0; r->aborted = 0; r->chi2[0] = r->chi2[1] = 0;
        if (stop && *stop) { abort_shortcut(); return EAO_OK; }                                  // 2. abort shortcut
        nFreeIn = 0;
        for (int i = 0; i < nC; i++) nFreeIn += p->cam_fixed[i] ? 0 : 1;
        EAO_REQUIRE(nFreeIn <= kBigMaxFree, "at most %d free keyframes in this build (got %d)", kBigMaxFree, nFreeIn);
        // more free keyframes than the single-workgroup solvers take (or EAO_BA_SOLVER=big, the harness's A/B switch): the map-scale path
        // (measured, LocalBundleAdjustment wall time, tools/dbg_ba_sizes.py: the LDS / global-scratch single-workgroup solver with
        //  the slab assembly takes 5.8 ms at 31 free keyframes and 29 ms at 64, the map-scale path 3.6 and 6.9 ms -- so everything
        //  beyond the register-tile solver goes there; that older path was removed in round 5)
        const char* const solverEnv = getenv("EAO_BA_SOLVER");      // (read per call, like the other switches: a test sets it after the process's first call)
        bigPath = nFreeIn > kTileMaxFree || (nFreeIn > 0 && solverEnv && !strcmp(solverEnv, "big"));
        static thread_local SetupScratch t_setup;
        SetupScratch& S = t_setup;           // (one look-up per call: see SetupScratch)
        Workers crew(bigPath, Ept);          // (a map-scale set-up is a session of the host crew, open until this function returns)
        const EdgeView v = edge_view();
        std::vector<int>& cnt = c.scratch;
        if (!count_edges(v, crew, S, cnt)) return EAO_ERR_INVALID;                               // 3. validation + counts
        if (bigPath) {                                                                           // 4. map-scale: covisibility lists, pairs, plan
            if (!build_observer_lists(v, crew, S, cnt.data(), laps) || !build_pairs(crew, S, laps)) return EAO_ERR_INVALID;
            if ((st = update_plan(S, hostStamps))) return st;
        }
        laps.lap(0);
        Carve k;                                                                                 // 5. arena
        start_record();
        if ((st = carve_arena(S, k)) || (st = reserve_results())) return st;
        pack_problem(v, k, crew);                                                                // 6. problem pack + first upload
        // The problem itself is on its way to the device while the host builds the active structure below; the structure follows in a second copy.
        const size_t offSplit = (size_t)((unsigned char*)k.camIdx - k.base) & ~(size_t)255;
        laps.lap(1);
        if (!deferUpload) EAO_HIP(hipMemcpyAsync(k.base + k.off0, k.pin + k.off0, offSplit - k.off0, hipMemcpyHostToDevice, s));
        ActiveStructure A{k.host(k.camIdx), k.host(k.ptIdx), k.host(k.actCam), k.host(k.actPt), k.host(k.ptStart), k.host(k.ptEdges), k.host(k.camStart), k.host(k.camEdges)};
        if (!build_active_structure(v, crew, S, bigPath, cnt, A)) return EAO_ERR_INVALID;        // 7. active structure
        D.nFree = A.nF; D.nL = A.nL;
        laps.lap(2);
        if (bigPath && A.nF > 0 && (st = fill_map_scale_mirror(S, k, crew))) return st;          // 8. map-scale: tables, observer lists, launch order
        laps.lap(3);
        set_launch_geometry();                                                                   // 9. launch geometry
        write_records(k.host(dW));                                                               // 10. records (they travel with the structure) + second upload
        if (!deferUpload) EAO_HIP(hipMemcpyAsync(k.base + offSplit, k.pin + offSplit, k.off1 - offSplit, hipMemcpyHostToDevice, s));
        else { upSrc = k.pin + k.off0; upDst = k.base + k.off0; upBytes = (k.off1 - k.off0 + 15) & ~(size_t)15; }
        L.W = dW; L.nz = 1; L.s = s; L.seq = c.status->seq;
        c.status->ph[0].touched = c.status->ph[1].touched = 0;
        laps.lap(4);
        if (hostStamps && bigPath) print_laps(laps);
        return EAO_OK;
    }

    // The set-up launches and, for a chained window, its whole run on `on`: the window's own launch, or the batched launch of its group (whose first window speaks for
    // all of them: they share its iteration counts).
    eao_status enqueue(BALaunch& on) {
        eao_status st = on.attributes();
        if (st) return st;
        on.setup();
        if (chained) on.chain(mode, p->its_first, p->its_second);
        return EAO_OK;
    }

    eao_status wait_status(int want) {
        EAO_HIP(hipStreamSynchronize(L.s));
        if (c->status->seq != want) { eao::set_error("LM status hand-off out of sequence"); return EAO_ERR_INTERNAL; }
        return EAO_OK;
    }
    eao_status set_ctl(int halt, int iters, int nBad) {
        const int v[5] = {halt, curHost, iters, kStRunning, nBad};
        EAO_HIP(hipMemcpyAsync(D.ctl0, v, sizeof(v), hipMemcpyHostToDevice, L.s));
        return EAO_OK;
    }
    // ---- SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve per iteration.
    // Iterations are enqueued in bulk (one trial each, no host round trip); the device finishes clean iterations itself
    // and halts the window on anything else, which the host then replays trial by trial like g2o's do/while.
    // resume: the first bulk segment of this call was already enqueued (and has finished) -- start from its outcome
    eao_status optimize(int phase, int iterations, int* itersDone, double* chiOut, const BAPhase* resume) {
        *itersDone = 0;
        LMContext& c = *this->c;
        eao_status st;
        if (D.nFree + D.nL == 0) return EAO_OK;   // "_ivMap.size() == 0": nothing to optimise
        bool needErrors = true, ok = true;
        double currentChi = 0;
        int nBad = 0, done = 0;
        while (done < iterations && !(stop && *stop && !resume) && ok) {
            if (!resume) {
                // ---- bulk segment: every remaining iteration, one trial each.  The control block is clean at the start of
                //      an optimize() call (zeros from the upload / reset by the outlier pass); after a takeover it is rewritten.
                if (done > 0 && (st = set_ctl(0, done, nBad))) return st;
                if (lazy) {
                    // one iteration per enqueue, the next one as soon as the decision of the one before the last has landed in the pinned status block.  The
                    // poll is a pacing hint only: a stale read enqueues later (or one no-op iteration more), never something else -- what the host acts on is
                    // read after the stream synchronisation below, as in the bulk path.
                    volatile const int* pseq = &c.status->seq;
                    volatile const int* pstat = &c.status->status;
                    static thread_local std::vector<int> seqAt;
                    seqAt.assign((size_t)iterations + 1, 0);
                    for (int enq = done; enq < iterations; enq++) {
                        if (enq - done >= 2) {
                            while (*pseq - seqAt[enq - 2] < 0) { if (hipStreamQuery(L.s) != hipErrorNotReady) break; }
                            if (*pstat != kStRunning) break;
                        }
                        L.bulk(enq, enq + 1, needErrors && enq == done);
                        seqAt[enq] = L.seq;
                    }
                } else L.bulk(done, pollStop ? std::min(iterations, done + 1) : iterations, needErrors);
                needErrors = false;
                EAO_HIP(hipStreamSynchronize(L.s));
            }
            const BAPhase S = resume ? *resume : c.status->ph[phase];
            resume = nullptr;
            for (int k = done; k < S.iters && k < 32; k++) {
                tr->lambda.push_back(c.status->trLambda[32 * phase + k]); tr->chi2.push_back(c.status->trChi[32 * phase + k]);
                tr->trials.push_back(c.status->trTrials[32 * phase + k]);
            }
            tr->linearizations += S.iters - done;
            done = S.iters; nBad = S.nBad; curHost = S.cur; currentChi = S.chi;
            if (S.status == kStEmpty) { done = -1; break; }
            if (S.status == kStTerminate) { ok = false; break; }
            if (S.status == kStRunning && done < iterations && pollStop) continue;   // next iteration (after a look at *stop)
            if (S.status != kStTakeover) break;           // all requested iterations done
            // ---- host takeover of iteration `done`: its first trial was rejected (or rho == 0 / NaN)
            tr->linearizations++;
            const double iniChi = S.chi;
            double rho = S.rho;
            int qmax = 1;
            bool accepted = S.accepted != 0;
            while (rho < 0 && qmax < refc::LM_MAX_TRIALS && !(stop && *stop)) {
                if ((st = set_ctl(0, done, nBad))) return st;
                L.relinearize();
                L.trial(0, 0, false, true);
                if ((st = wait_status(L.seq))) return st;
                rho = c.status->rho; accepted = c.status->accepted != 0; curHost = c.status->cur;
                if (accepted) currentChi = c.status->chi;
                qmax++;
            }
            needErrors = !accepted;             // pop(): residuals belong to the rejected state
            tr->lambda.push_back(c.status->lambda); tr->chi2.push_back(currentChi); tr->trials.push_back(qmax);
            done++;
            if (qmax == refc::LM_MAX_TRIALS || rho == 0) { ok = false; break; }
            if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
            if (nBad >= 3) ok = false;
        }
        *itersDone = done;
        *chiOut = currentChi;
        return EAO_OK;
    }

    // After the chained enqueue (own or as part of a batch) has finished: takeovers, results.  The abort flag is read before
    // and after: a clean window takes less time than one g2o iteration on the CPU.
    eao_status complete() {
        eao::Range rg("lm: takeovers + results");
        LMContext& c = *this->c;
        eao_status st;
        hipStream_t s = L.s;
        const BAPhase A = c.status->ph[0], B = c.status->ph[1];
        if ((st = optimize(0, p->its_first, &r->iters[0], &r->chi2[0], chained ? &A : nullptr))) return st;
        const bool firstClean = chained && A.status != kStTakeover;
        const bool doMore = mode == 0 && (firstClean || !(stop && *stop));
        bool redo = !chained || (mode == 1 && !firstClean);
        if (doMore && E) {
            // outlier pass (src/Optimizer.cc:978-1008): chi2 of the residual each edge last computed + depth test.  g2o's
            // initializeOptimization(0) would now drop the level-1 edges (and vertices left without edges) from the active
            // set; here they stay in the lists with zero weight, which leaves every sum -- and a vertex without edges --
            // unchanged, and saves the host round trip of rebuilding and re-uploading the structure.
            if (firstClean) {
                if (B.status == kStTakeover) redo = true;
                if ((st = optimize(1, p->its_second, &r->iters[1], &r->chi2[1], &B))) return st;
            } else {
                redo = true;
                if ((st = set_ctl(0, 0, 0))) return st;            // the frozen window left "takeover" in the control block
                L.classify();
                if ((st = optimize(1, p->its_second, &r->iters[1], &r->chi2[1], nullptr))) return st;
            }
        }
        if (redo) {
            L.finish();
            EAO_HIP(hipStreamSynchronize(s));
        }
        EAO_HIP(hipGetLastError());
        if (D.dbg) {
            long long stt[32];
            EAO_HIP(hipMemcpy(stt, D.dbg, sizeof(stt), hipMemcpyDeviceToHost));
            fprintf(stderr, "[eao pair stamps] workgroup 0 (a diagonal pair): loads + accumulation %lld, block sum of 42 values %lld shader-cycles; linearisation: landmark workgroup 0 %lld, camera workgroup 0 %lld\n",
                    stt[13] >> 20, stt[13] & 0xFFFFF, stt[14], stt[15]);
            if (L.d.bigPath) fprintf(stderr, "[eao bal_backsolve stamps] super-block 1, workgroup 0: loads issued %lld, the 256-column triangle (8 blocks) %lld, removal from the columns to the left %lld shader-cycles\n",
                                     stt[25] - stt[24], stt[26] - stt[25], stt[27] - stt[26]);
            if (L.d.bigPath) fprintf(stderr, "[eao bal_step stamps] look-ahead workgroup of panel 2: prologue + loads + barrier %lld, row solves %lld, update %lld, tile to LDS and rows back %lld, 32 x 32 LDL^T %lld, store %lld shader-cycles\n",
                                     stt[17] - stt[16], stt[18] - stt[17], stt[19] - stt[18], stt[20] - stt[19], stt[21] - stt[20], stt[22] - stt[21]);
            fprintf(stderr, "[eao solve stamps] assemble %lld factor %lld (panel %lld trailing %lld / %lld) backsub %lld tail %lld shader-cycles; wall(100MHz) %lld %lld %lld %lld\n",
                    stt[2] - stt[0], stt[4] - stt[2], stt[10], stt[11], stt[12], stt[6] - stt[4], stt[8] - stt[6], stt[3] - stt[1], stt[5] - stt[3], stt[7] - stt[5], stt[9] - stt[7]);
        }
        for (int i = 0; i < nC; i++) se3_to_Tcw_f32(outCams[i], r->cam_Tcw + 16 * i);
        for (size_t i = 0; i < (size_t)nPo * 3; i++) r->points[i] = (float)outPts[i];
        for (size_t i = 0; i < (size_t)nPl * 4; i++) planes_out[i] = (float)outPlanes[i];           // Converter::toCvMat(Plane3D)
        if (Ept && r->edge_outlier) {
            if (mode == 0) std::memcpy(r->edge_outlier, outCls, Ept);
            else std::memset(r->edge_outlier, 0, Ept);
        }
        return EAO_OK;
    }
};

}  // namespace

static eao_status ba_run(const eao_ba_problem* p, const volatile uint8_t* stop, eao_ba_result* r, int mode, int robust,
                         const eao_ba_planes* pl = nullptr, float* planes_out = nullptr) {
    LMContext& c = g_ctx;
    eao_status st = ctx_init(c, true, mode == 0 ? eao::StreamClass::Background : eao::StreamClass::Bulk);
    if (st) return st;
    BAJob j;
    j.p = p; j.stop = stop; j.r = r; j.mode = mode; j.robust = robust; j.pl = pl; j.planes_out = planes_out; j.c = &c; j.tr = &g_trace;
    static const bool hostStamps = getenv("EAO_DEBUG_STAMPS") != nullptr;
    const auto w0 = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count(); };
    EAO_HIP(hipEventRecord(c.ev0, c.stream));
    if ((st = j.prepare(c.stream))) return st;
    if (j.trivial) return EAO_OK;
    const double tPrep = ms();
    if ((st = j.enqueue(j.L))) return st;
    double tEnq = 0;
    if (j.chained) {
        tEnq = ms();
        EAO_HIP(hipStreamSynchronize(c.stream));
    }
    const double tSetup = ms();
    if ((st = j.complete())) return st;
    EAO_HIP(hipEventRecord(c.ev1, c.stream));
    EAO_HIP(hipStreamSynchronize(c.stream));
    EAO_HIP(hipEventElapsedTime(&g_trace.deviceMs, c.ev0, c.ev1));
    if (hostStamps && !j.L.d.bigPath) fprintf(stderr, "[eao window wall] prepare %.3f, enqueue %.3f, wait %.3f, takeovers + results %.3f ms; whole call %.3f ms\n", tPrep, tEnq - tPrep, tSetup - tEnq, ms() - tSetup, ms());
    if (hostStamps && j.L.d.bigPath) fprintf(stderr, "[eao map-scale wall] prepare %.3f, set-up launches (+ chain) %.3f, iterations + results %.3f ms; whole call %.3f ms\n", tPrep, tSetup - tPrep, ms() - tSetup, ms());
    return EAO_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// LocalBundleAdjustment of MANY independent windows (the batched-sequence configuration: 25 windows of 20 keyframes): the
// window is the z dimension of every launch.  Each window owns a context (arena, pinned mirrors, status block); the
// host-side set-up of the windows runs on a few host threads; ONE chained enqueue serves them all; a window whose LM
// rejected a trial freezes by itself (its halt flag) and is finished by the host afterwards exactly like a single call.
namespace {
struct BABatchPool {
    std::vector<std::unique_ptr<LMContext>> ctx;
    std::vector<LMTraceHost> trace;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipStream_t> side;              // streams of the window groups beyond the first
    std::vector<hipEvent_t> sideDone;
    BADev* hW = nullptr; size_t hWCap = 0;      // pinned mirror of the window array
    eao::DevBuf<BADev> dW;
    eao_status reserve(int n) {          // the main stream and its events; a context and a trace per window; the window array, pinned and on the device
        eao_status st;
        if (!stream) {
            EAO_HIP(eao::create_stream(&stream, eao::StreamClass::Background));
            EAO_HIP(hipEventCreate(&ev0));
            EAO_HIP(hipEventCreate(&ev1));
        }
        while ((int)ctx.size() < n) ctx.emplace_back(new LMContext());
        if ((int)trace.size() < n) trace.resize(n);
        for (int w = 0; w < n; w++)
            if ((st = ctx_init(*ctx[w], false, eao::StreamClass::Background))) return st;
        if (hWCap < (size_t)n * 2) {
            if (hW) (void)hipHostFree(hW);
            hW = nullptr; hWCap = 0;
            EAO_HIP(hipHostMalloc((void**)&hW, (size_t)n * 2 * sizeof(BADev), hipHostMallocDefault));
            hWCap = (size_t)n * 2;
        }
        return dW.reserve((size_t)n * 2);
    }
    eao_status reserve_groups(int G) {      // a stream and an event per group beyond the first
        while ((int)side.size() < G - 1) {
            hipStream_t q; hipEvent_t e;
            EAO_HIP(eao::create_stream(&q, eao::StreamClass::Background));
            EAO_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            side.push_back(q); sideDone.push_back(e);
        }
        return EAO_OK;
    }
    ~BABatchPool() {
        if (hW) (void)hipHostFree(hW);
        for (hipEvent_t e : sideDone) (void)hipEventDestroy(e);
        for (hipStream_t q : side) (void)hipStreamDestroy(q);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};
thread_local BABatchPool g_batch;

struct Outcome {      // a status and, if it is an error, the text that came with it (eao_last_error() belongs to the thread that failed)
    eao_status st = EAO_OK; std::string err;
    void capture(eao_status s) { st = s; if (s) err = eao_last_error(); }
};

// One eao_local_ba_batch call: its jobs, the plan that deals them to set-up threads and groups (ba_batch_plan.h), a record per window and per group, and the call's
// stages as members.  worker(t) and lead(g) are the tasks of the host crew (a batch of one runs them on the caller's thread); what they share is in here.
struct BABatch {
    struct Window { Outcome out; bool batched = false; };      // (batched: it shares its group's enqueue)
    struct Group {
        BALaunch L;                                  // the batched enqueue of its windows
        Outcome out;
        int nBatched = 0, first = -1;                // windows in the batched enqueue / the first of them
        std::atomic<int> prepared{0};                // windows the set-up workers are through with
        double msPrep = 0, msEnq = 0, msDone = 0;    // since the call's start: windows prepared, launches enqueued, stream drained
        int state = 0;                               // 0: running, 1: drained, 2: failed (nothing to take out); under doneMu
    };
    BABatchPool& B;
    const int n;
    std::vector<BAJob> jobs;
    BatchPlan plan;
    std::vector<Window> win;
    std::vector<Group> grp;
    int dev = 0;
    // results: when a group's stream has drained, the set-up workers (idle since the first tenth of the call) take its windows' results out in parallel -- the last
    // group's nine windows were ~0.1 ms of conversions on one thread at the very end of the call
    bool crewDone = false;
    std::mutex doneMu;
    std::condition_variable doneCv;
    std::chrono::steady_clock::time_point tp0;

    BABatch(BABatchPool& pool, const eao_ba_problem* problems, int n_, const volatile uint8_t* stop, eao_ba_result* results) : B(pool), n(n_), jobs(n_), win(n_) {
        for (int w = 0; w < n; w++) {
            BAJob& j = jobs[w];
            j.p = &problems[w]; j.stop = stop; j.r = &results[w]; j.mode = 0; j.robust = 1; j.c = B.ctx[w].get(); j.tr = &B.trace[w];
            j.c->status->seq = 0;        // every window of the batch sees the same hand-off sequence numbers
        }
        tp0 = std::chrono::steady_clock::now();
    }
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count(); }
    hipStream_t stream_of(int g) const { return g == 0 ? B.stream : B.side[g - 1]; }

    // The switches and the latency marker are read here; the dealing itself is plan_batch.
    void deal() {
        static const int envThreads = getenv("EAO_BA_BATCH_THREADS") ? atoi(getenv("EAO_BA_BATCH_THREADS")) : 0;
        static const int envGroups = getenv("EAO_BA_BATCH_GROUPS") ? atoi(getenv("EAO_BA_BATCH_GROUPS")) : 0;
        plan_batch(BatchPlanIn{n, envThreads, envGroups, (int)std::thread::hardware_concurrency(), getenv("EAO_BA_BATCH_EVEN") != nullptr, eao::latency_caller_alive()}, plan);
        grp = std::vector<Group>(plan.G);
        crewDone = !(plan.nThreads == 1 && plan.G == 1);
    }

    void finish_window(int w) {
        BAJob& j = jobs[w];
        if (j.trivial || win[w].out.st) return;
        if (win[w].batched) j.L.seq = grp[plan.group_of(w)].L.seq;
        win[w].out.capture(j.complete());
    }

    // set-up: nThreads workers take the windows in order (window w's uploads go to its group's stream), so the first
    // group is complete after one round; each group's leader then enqueues its chain while the workers carry on
    void worker(int t) {
        (void)hipSetDevice(dev);
        for (int w = t; w < n; w += plan.nThreads) {
            const int g = plan.group_of(w);
            win[w].out.capture(jobs[w].prepare(stream_of(g), true));
            grp[g].prepared.fetch_add(1, std::memory_order_release);
        }
        if (!crewDone) return;
        for (int w = t; w < n; w += plan.nThreads) {
            Group& gr = grp[plan.group_of(w)];
            int state;
            { std::unique_lock<std::mutex> lk(doneMu); doneCv.wait(lk, [&] { return gr.state != 0; }); state = gr.state; }
            if (state == 1) finish_window(w);
        }
    }

    // ---- the group leader's steps, in the order lead() takes them; false: the group stops here
    bool wait_for_windows(int g) {
        Group& gr = grp[g];
        const int w0 = plan.gStart[g], w1 = plan.gStart[g + 1];
        while (gr.prepared.load(std::memory_order_acquire) < w1 - w0) std::this_thread::yield();    // (the workers above)
        gr.msPrep = ms();
        for (int w = w0; w < w1; w++)
            if (win[w].out.st) return false;
        return true;
    }
    void upload_windows(int g) {      // this group's uploads: one launch per eight windows (see BAJob::prepare)
        BAUploadArgs U;
        int k = 0;
        auto flush = [&]() {
            if (k) hipLaunchKernelGGL(k_ba_upload, dim3(48, k), dim3(256), 0, stream_of(g), U);
            k = 0;
        };
        for (int w = plan.gStart[g]; w < plan.gStart[g + 1]; w++) {
            if (jobs[w].trivial || !jobs[w].upBytes) continue;
            U.dst[k] = jobs[w].upDst; U.src[k] = jobs[w].upSrc; U.n16[k] = jobs[w].upBytes / 16;
            if (++k == 8) flush();
        }
        flush();
    }
    // the windows that share the batched enqueue (tile-solver path, something to optimise); the others -- windows beyond
    // 30 free keyframes, empty ones -- follow one by one on the same stream
    void choose_batched(int g) {
        Group& gr = grp[g];
        const int w0 = plan.gStart[g], w1 = plan.gStart[g + 1];
        BALaunch& L = gr.L;
        L.s = stream_of(g); L.W = B.dW.p + 2 * w0; L.seq = 0; L.rot = w0 & 7;
        for (int w = w0; w < w1; w++) {
            BAJob& j = jobs[w];
            if (!j.batchable()) continue;
            if (gr.first >= 0 && (j.p->its_first != jobs[gr.first].p->its_first || j.p->its_second != jobs[gr.first].p->its_second)) continue;
            if (gr.first < 0) { gr.first = w; L.d = j.L.d; } else L.d.merge(j.L.d);
            j.write_records(B.hW + 2 * (w0 + gr.nBatched));
            gr.nBatched++;
            win[w].batched = true;
        }
    }
    bool enqueue_batched(int g) {
        Group& gr = grp[g];
        if (!gr.nBatched) return true;
        const int w0 = plan.gStart[g];
        gr.L.nz = gr.nBatched;
        if (hipMemcpyAsync(B.dW.p + 2 * w0, B.hW + 2 * w0, (size_t)gr.nBatched * 2 * sizeof(BADev), hipMemcpyHostToDevice, stream_of(g)) != hipSuccess) {
            eao::set_error("hipMemcpyAsync of the window records failed");
            gr.out.capture(EAO_ERR_NO_DEVICE);
            return false;
        }
        gr.out.capture(jobs[gr.first].enqueue(gr.L));
        return !gr.out.st;
    }
    bool enqueue_singles(int g) {
        for (int w = plan.gStart[g]; w < plan.gStart[g + 1]; w++) {
            if (win[w].batched || jobs[w].trivial) continue;
            grp[g].out.capture(jobs[w].enqueue(jobs[w].L));
            if (grp[g].out.st) return false;
        }
        grp[g].msEnq = ms();
        return true;
    }
    // results (and, for a window whose device-side run handed over to the host, the rest of its run) as soon as THIS
    // group's stream has drained: only the last group's ~10 us per window are not hidden behind the other groups' kernels
    bool drain(int g) {
        Group& gr = grp[g];
        hipStream_t sg = stream_of(g);
        if (g > 0 && hipEventRecord(B.sideDone[g - 1], sg) != hipSuccess) { eao::set_error("hipEventRecord failed"); gr.out.capture(EAO_ERR_NO_DEVICE); return false; }
        if (hipStreamSynchronize(sg) != hipSuccess) {
            eao::set_error("hipStreamSynchronize: %s", hipGetErrorString(hipGetLastError()));
            gr.out.capture(EAO_ERR_NO_DEVICE);
            return false;
        }
        gr.msDone = ms();
        return true;
    }
    void lead(int g) {
        (void)hipSetDevice(dev);
        struct Announce {      // whatever way this group ends, the workers waiting for it are told
            std::mutex& mu; std::condition_variable& cv; int& state; int value = 2;
            ~Announce() { { std::lock_guard<std::mutex> lk(mu); state = value; } cv.notify_all(); }
        } announce{doneMu, doneCv, grp[g].state};
        if (!wait_for_windows(g)) return;
        upload_windows(g);
        choose_batched(g);
        if (!enqueue_batched(g) || !enqueue_singles(g) || !drain(g)) return;
        announce.value = 1;
        if (!crewDone)
            for (int w = plan.gStart[g]; w < plan.gStart[g + 1]; w++) finish_window(w);
    }

    void run() {
        const int nThreads = plan.nThreads, G = plan.G;
        if (nThreads == 1 && G == 1) { worker(0); lead(0); }          // (a batch of one: no thread is involved)
        else host_crew().run(nThreads + G - 1, [&](int i) { if (i < nThreads) worker(i); else lead(i - nThreads + 1); }, [&] { lead(0); });
    }

    // The groups' streams meet again on the main one (or are drained, if anything failed), the first error is raised, the call's trace and timing are written.
    eao_status join() {
        const int G = plan.G;
        bool failed = false;
        for (const Window& x : win) failed = failed || x.out.st;
        for (const Group& x : grp) failed = failed || x.out.st;
        if (failed)
            for (int g = 1; g < G; g++) (void)hipStreamSynchronize(B.side[g - 1]);
        else
            for (int g = 1; g < G; g++) EAO_HIP(hipStreamWaitEvent(B.stream, B.sideDone[g - 1], 0));   // (device time of the call: ev0 .. ev1)
        for (int w = 0; w < n; w++)
            if (win[w].out.st) { eao::set_error("window %d: %s", w, win[w].out.err.c_str()); (void)hipStreamSynchronize(B.stream); return win[w].out.st; }
        for (const Group& x : grp)
            if (x.out.st) { eao::set_error("%s", x.out.err.c_str()); (void)hipStreamSynchronize(B.stream); return x.out.st; }
        for (int w = 0; w < n; w++)
            if (!jobs[w].trivial) g_trace.linearizations += jobs[w].tr->linearizations;
        EAO_HIP(hipEventRecord(B.ev1, B.stream));
        EAO_HIP(hipStreamSynchronize(B.stream));
        EAO_HIP(hipEventElapsedTime(&g_trace.deviceMs, B.ev0, B.ev1));
        static const bool envTiming = getenv("EAO_BA_BATCH_TIMING") != nullptr;
        if (envTiming) print_timing();
        return EAO_OK;
    }
    void print_timing() const {
        int nBatched = 0;
        double msPrepare = 0, msEnqueue = 0, msSync = 0;
        std::string sizes;
        for (int g = 0; g < plan.G; g++) {
            nBatched += grp[g].nBatched;
            msPrepare = std::max(msPrepare, grp[g].msPrep); msEnqueue = std::max(msEnqueue, grp[g].msEnq); msSync = std::max(msSync, grp[g].msDone);
            sizes += (g ? "+" : "") + std::to_string(plan.gStart[g + 1] - plan.gStart[g]);
        }
        fprintf(stderr, "[eao_local_ba_batch] %d windows (%d batched, %d host threads): set-up + uploads enqueued %.3f ms, launches enqueued %.3f, device done %.3f, results out %.3f, groups %s\n",
                n, nBatched, plan.nThreads, msPrepare, msEnqueue, msSync, ms(), sizes.c_str());
    }
};

}  // namespace

extern "C" {

eao_status eao_local_ba(const eao_ba_problem* p, const volatile uint8_t* stop, eao_ba_result* r) { return ba_run(p, stop, r, 0, 1); }

eao_status eao_local_ba_batch(const eao_ba_problem* problems, int32_t n, const volatile uint8_t* stop, eao_ba_result* results) {
    EAO_REQUIRE(n >= 0 && (n == 0 || (problems && results)), "null argument");
    if (n == 0) return EAO_OK;
    eao_status st = eao::require_device();
    if (st) return st;
    BABatchPool& B = g_batch;
    if ((st = B.reserve(n))) return st;
    g_trace.clear();
    BABatch batch(B, problems, n, stop, results);
    EAO_HIP(hipEventRecord(B.ev0, B.stream));
    batch.deal();
    if ((st = B.reserve_groups(batch.plan.G))) return st;
    EAO_HIP(hipGetDevice(&batch.dev));
    batch.run();
    return batch.join();
}

eao_status eao_bundle_adjustment(const eao_ba_problem* p, int32_t robust, const volatile uint8_t* stop, eao_ba_result* r) {
    return ba_run(p, stop, r, 1, robust != 0);
}

eao_status eao_bundle_adjustment_planes(const eao_ba_problem* p, const eao_ba_planes* planes, int32_t robust, const volatile uint8_t* stop,
                                        eao_ba_result* r, float* planes_out) {
    return ba_run(p, stop, r, 1, robust != 0, planes, planes_out);
}

eao_status eao_last_lm_trace(double* lambda, double* chi2, int32_t* trials, int32_t cap, int32_t* n) {
    EAO_REQUIRE(n, "null argument");
    const int m = std::min((int)g_trace.lambda.size(), cap);
    for (int i = 0; i < m; i++) {
        if (lambda) lambda[i] = g_trace.lambda[i];
        if (chi2) chi2[i] = g_trace.chi2[i];
        if (trials) trials[i] = g_trace.trials[i];
    }
    *n = m;
    return EAO_OK;
}

eao_status eao_last_pose_rounds(int32_t frame, double* lambda, double* chi2, int32_t* trials, int32_t cap, int32_t* n, int32_t* round_start, int32_t* n_rounds) {
    EAO_REQUIRE(n && n_rounds, "null argument");
    EAO_REQUIRE(frame >= 0 && frame < (int)g_trace.pose.size(), "frame %d: the last PoseOptimization call of this thread had %d frames", frame, (int)g_trace.pose.size());
    const PoseRoundsHost& h = g_trace.pose[frame];
    const int m = std::min(h.n, cap);
    for (int i = 0; i < m; i++) {
        if (lambda) lambda[i] = h.lambda[i];
        if (chi2) chi2[i] = h.chi2[i];
        if (trials) trials[i] = h.trials[i];
    }
    *n = m;
    if (round_start) for (int k = 0; k < 4; k++) round_start[k] = h.roundStart[k];
    *n_rounds = h.nRounds;
    return EAO_OK;
}

eao_status eao_last_lm_timing(float* device_ms, int32_t* linearizations) {
    if (device_ms) *device_ms = g_trace.deviceMs;
    if (linearizations) *linearizations = g_trace.linearizations;
    return EAO_OK;
}

}  // extern "C"
