// keyframe_db.hip -- KeyFrameDatabase on the device (include/eao_fusion.h, "KeyFrameDatabase"; reference src/KeyFrameDatabase.cc): the BoW vectors of the added
// keyframes stay in HBM, a query uploads the query vector alone and downloads 16 bytes per live keyframe.
//
// Resident: one arena of two columns, word ids (uint32) and values (double), appended to by add; one (begin, count) record per LIVE entry in storage order, which
// is what the kernel's grid runs over.  The entry table and the per-keyframe state are the host's (keyframe_db_internal.h); growth and compaction are the policy
// of resident_arena.h, carried out by dev_arena.h.
//
// k_kfdb_intersect: one wavefront per live stored vector, four per workgroup (the shape of k_bow_score_l1), the query's ids staged in LDS.  Upstream's inverted-file walk is, per stored
// keyframe, the count of the query's words it holds; its scoring is the sorted intersection of the same two vectors.  One pass of bow_l1_pair gives the count,
// the first common word (the key of the list order) and the L1 score.  No atomics; every double is a single IEEE operation in upstream's order.
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "bow_intersect.h"
#include "dev_arena.h"
#include "keyframe_db_internal.h"

namespace kfdb = eao::kfdb;
static_assert(kfdb::kMaxWordsPerVector == EAO_VOCABULARY_MAX_FEATURES, "the cap of a vector is the vocabulary's");

namespace {
constexpr size_t kInitialWords = 1 << 14;      // 192 KiB of arena; doubles from there
constexpr size_t kInitialRecs = 256;
constexpr uint64_t kMaxArenaWords = 0xffffffffull;      // a record's begin is 32 bits
}  // namespace

struct eao_keyframe_db {
    std::mutex mutex;      // upstream's mMutex, widened to the whole call
    int32_t nWords = 0;
    kfdb::Table table;
    eao::DevArena<unsigned, double> words{kInitialWords, kMaxArenaWords};      // the arena: ids (0) and values (1)
    eao::DevArena<uint2> rec{kInitialRecs};      // (begin, count) of the live entries, storage order
    bool recStale = false;                       // an erase / compaction / clear happened since rec was written
};

namespace {

// The workgroup stages the query's ids in LDS first (nq <= 8192 ids = 32 KiB of dynamic LDS) and the binary searches probe LDS: measured against probing
// global memory (profiles/keyframe_database_timing.txt: 0.132 against 0.203 ms at 20 000 keyframes), after which the plain form was dropped.
__global__ __launch_bounds__(256) void k_kfdb_intersect(int nq, const unsigned* qId, const double* qVal, int nLive, const uint2* rec, const unsigned* ids,
                                                        const double* vals, int* common, unsigned* firstWord, double* score) {
    extern __shared__ unsigned sQ[];
    for (int i = threadIdx.x; i < nq; i += 256) sQ[i] = qId[i];
    __syncthreads();
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= nLive) return;      // (a whole wavefront leaves together)
    const uint2 r = rec[j];
    const size_t b = r.x, e = b + r.y;
    int c = 0;
    unsigned f = 0;
    const double s = eao::bow_l1_pair<true>(nq, sQ, qVal, ids, vals, b, e, lane, c, f);
    if (lane == 0) {
        common[j] = c;
        firstWord[j] = f;
        score[j] = -s / 2.0;      // ScoringObject.cpp:65 (no common word: -0.0)
    }
}

struct KfdbCtx : eao::ThreadStream {
    eao::DevBuf<unsigned char> dev;
    eao::PinBuf<hipHostMallocDefault> host;
};
thread_local KfdbCtx g_kfdb;

eao_status reserve_words(eao_keyframe_db* db, uint64_t need, hipStream_t stream) {
    if (need > kMaxArenaWords) {
        eao::set_error("the arena would hold %llu words; at most %llu are supported", (unsigned long long)need, (unsigned long long)kMaxArenaWords);
        return EAO_ERR_CAPACITY;
    }
    return db->words.reserve(need, db->table.used, stream);
}

eao_status check_query(const eao_keyframe_db* db, int32_t nq, const uint32_t* qId, const double* qVal) {
    EAO_REQUIRE(nq >= 0 && (nq == 0 || (qId && qVal)), "bad query vector");
    EAO_REQUIRE(nq <= EAO_VOCABULARY_MAX_FEATURES, "the query has %d words; at most %d are supported", nq, EAO_VOCABULARY_MAX_FEATURES);
    for (int i = 0; i < nq; i++) {
        EAO_REQUIRE((int64_t)qId[i] < db->nWords, "the query's word id %u is not below n_words = %d", qId[i], db->nWords);
        EAO_REQUIRE(i == 0 || qId[i - 1] < qId[i], "the query's word ids do not ascend strictly at entry %d", i);
    }
    return EAO_OK;
}

struct Raw {      // the kernel's result in this thread's pinned block, storage order over the live entries
    int32_t n = 0;
    const int32_t* common = nullptr;
    const uint32_t* firstWord = nullptr;
    const double* score = nullptr;
    std::vector<uint64_t> id;
};

// the query is valid and the handle's mutex is held
eao_status intersect(eao_keyframe_db* db, int32_t nq, const uint32_t* qId, const double* qVal, Raw& raw) {
    const int32_t n = db->table.nLive;
    raw.n = n;
    raw.id.clear();
    raw.id.reserve((size_t)n);
    for (const kfdb::Entry& e : db->table.entries)
        if (e.live) raw.id.push_back(e.id);
    if (n == 0) return EAO_OK;
    KfdbCtx& ctx = g_kfdb;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = eao::align256(o + bytes); return at; };
    const size_t oQi = take((size_t)nq * 4), oQv = take((size_t)nq * 8), inEnd = o;
    const size_t oRec = take(db->recStale ? (size_t)n * sizeof(uint2) : 0);
    const size_t oCommon = take((size_t)n * 4), oFirst = take((size_t)n * 4), oScore = take((size_t)n * 8), end = o;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    eao::Drain drain(ctx.stream);
    if (nq > 0) {
        std::memcpy(h + oQi, qId, (size_t)nq * 4);
        std::memcpy(h + oQv, qVal, (size_t)nq * 8);
        EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    }
    if (db->recStale) {      // after an erase: the records of the live entries again (8 bytes each)
        if ((st = db->rec.reserve((size_t)n, 0, ctx.stream))) return st;
        uint2* hr = (uint2*)(h + oRec);
        size_t k = 0;
        for (const kfdb::Entry& e : db->table.entries)
            if (e.live) hr[k++] = make_uint2((unsigned)e.begin, e.count);
        EAO_HIP(hipMemcpyAsync(db->rec.at(), hr, (size_t)n * sizeof(uint2), hipMemcpyHostToDevice, ctx.stream));
    }
    hipLaunchKernelGGL(k_kfdb_intersect, dim3(eao::cdiv(n, 4)), dim3(256), (size_t)nq * 4, ctx.stream, nq, (const unsigned*)(d + oQi), (const double*)(d + oQv), n, db->rec.at(),
                       db->words.at<0>(), db->words.at<1>(), (int*)(d + oCommon), (unsigned*)(d + oFirst), (double*)(d + oScore));
    EAO_HIP(hipGetLastError());
    EAO_HIP(hipMemcpyAsync(h + oCommon, d + oCommon, end - oCommon, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    db->recStale = false;
    raw.common = (const int32_t*)(h + oCommon);
    raw.firstWord = (const uint32_t*)(h + oFirst);
    raw.score = (const double*)(h + oScore);
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_keyframe_db_create(int32_t n_words, eao_keyframe_db** out) {
    EAO_REQUIRE(out, "out is NULL");
    EAO_REQUIRE(n_words >= 0, "n_words < 0");
    const eao_status st = eao::require_device();
    if (st) return st;
    eao_keyframe_db* db = new eao_keyframe_db;
    db->nWords = n_words;
    *out = db;
    return EAO_OK;
}

void eao_keyframe_db_destroy(eao_keyframe_db* db) { delete db; }

eao_status eao_keyframe_db_clear(eao_keyframe_db* db) {
    EAO_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lock(db->mutex);
    db->table.clear();      // (the allocations stay)
    db->recStale = true;
    return EAO_OK;
}

eao_status eao_keyframe_db_info(eao_keyframe_db* db, int32_t* n_live, int64_t* n_stored_words, int64_t* arena_capacity) {
    EAO_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lock(db->mutex);
    if (n_live) *n_live = db->table.nLive;
    if (n_stored_words) *n_stored_words = (int64_t)db->table.used;
    if (arena_capacity) *arena_capacity = (int64_t)db->words.cap;
    return EAO_OK;
}

eao_status eao_keyframe_db_add(eao_keyframe_db* db, uint64_t kf_id, int32_t n, const uint32_t* word_id, const double* word_val) {
    EAO_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lock(db->mutex);
    const std::string err = db->table.check_add(kf_id, n, word_id, db->nWords);
    EAO_REQUIRE(err.empty(), "eao_keyframe_db_add: %s", err.c_str());
    EAO_REQUIRE(n == 0 || word_val, "word_val is NULL");
    KfdbCtx& ctx = g_kfdb;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const uint64_t begin = db->table.used;
    eao::Drain drain(ctx.stream);      // (the arenas' growth enqueues its copies and waits for them itself)
    if ((st = reserve_words(db, begin + (uint64_t)n, ctx.stream))) return st;
    const size_t at = (size_t)db->table.nLive;      // the new entry's record (when the records are stale the next query writes them all)
    if (!db->recStale && (st = db->rec.reserve(at + 1, at, ctx.stream))) return st;
    const size_t oId = 0, oVal = eao::align256((size_t)n * 4), oRec = oVal + eao::align256((size_t)n * 8);
    if ((st = ctx.host.reserve(oRec + sizeof(uint2)))) return st;
    unsigned char* h = ctx.host.p;
    if (n > 0) {
        std::memcpy(h + oId, word_id, (size_t)n * 4);
        std::memcpy(h + oVal, word_val, (size_t)n * 8);
        EAO_HIP(hipMemcpyAsync(db->words.at<0>() + begin, h + oId, (size_t)n * 4, hipMemcpyHostToDevice, ctx.stream));
        EAO_HIP(hipMemcpyAsync(db->words.at<1>() + begin, h + oVal, (size_t)n * 8, hipMemcpyHostToDevice, ctx.stream));
    }
    if (!db->recStale) {
        *(uint2*)(h + oRec) = make_uint2((unsigned)begin, (unsigned)n);
        EAO_HIP(hipMemcpyAsync(db->rec.at() + at, h + oRec, sizeof(uint2), hipMemcpyHostToDevice, ctx.stream));
    }
    EAO_HIP(drain.wait(eao::Drain::Block));
    db->table.append(kf_id, (uint32_t)n);      // (only now: a failed call leaves the table as it was)
    return EAO_OK;
}

eao_status eao_keyframe_db_erase(eao_keyframe_db* db, uint64_t kf_id) {
    EAO_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lock(db->mutex);
    if (!db->table.erase(kf_id)) return EAO_OK;      // unknown: a no-op, as upstream (:52-64 finds nothing to erase)
    db->recStale = true;
    return eao::compact_if_wanted(g_kfdb, db->table, db->words);
}

eao_status eao_keyframe_db_intersect(eao_keyframe_db* db, int32_t nq, const uint32_t* q_id, const double* q_val, int32_t cap, uint64_t* kf_id, int32_t* common,
                                     uint32_t* first_word, double* score, int32_t* n_live) {
    EAO_REQUIRE(db && n_live, "bad argument");
    std::lock_guard<std::mutex> lock(db->mutex);
    eao_status st = check_query(db, nq, q_id, q_val);
    if (st) return st;
    const int32_t n = db->table.nLive;
    EAO_REQUIRE(cap >= n, "cap = %d is below the %d live keyframes", cap, n);
    EAO_REQUIRE(n == 0 || (kf_id && common && first_word && score), "a result array is NULL");
    Raw raw;
    if ((st = intersect(db, nq, q_id, q_val, raw))) return st;
    *n_live = n;
    if (n > 0) {
        std::memcpy(kf_id, raw.id.data(), (size_t)n * 8);
        std::memcpy(common, raw.common, (size_t)n * 4);
        std::memcpy(first_word, raw.firstWord, (size_t)n * 4);
        std::memcpy(score, raw.score, (size_t)n * 8);
    }
    return EAO_OK;
}

eao_status eao_keyframe_db_query_scores(eao_keyframe_db* db, const eao_keyframe_db_query* query, int32_t cap, eao_keyframe_db_scored* out) {
    EAO_REQUIRE(db && query && out, "bad argument");
    std::lock_guard<std::mutex> lock(db->mutex);
    EAO_REQUIRE(query->kind == 0 || query->kind == 1, "kind is not 0 (DetectLoopCandidates) or 1 (DetectRelocalizationCandidates)");
    eao_status st = check_query(db, query->nq, query->q_id, query->q_val);
    if (st) return st;
    EAO_REQUIRE(query->n_connected >= 0 && (query->n_connected == 0 || query->connected_id), "bad connected_id");
    const int32_t n = db->table.nLive;
    EAO_REQUIRE(cap >= n, "cap = %d is below the %d live keyframes", cap, n);
    EAO_REQUIRE(n == 0 || (out->sharing_id && out->sharing_words && out->scored_id && out->scored_score), "a result array is NULL");
    Raw raw;
    if ((st = intersect(db, query->nq, query->q_id, query->q_val, raw))) return st;
    std::unordered_set<uint64_t> connected;
    if (query->kind == 0) connected.insert(query->connected_id, query->connected_id + query->n_connected);
    kfdb::Stage1 r;
    kfdb::walk(db->table, query->kind, query->query_id, n, raw.id.data(), raw.common, raw.firstWord, raw.score, connected, query->min_score, r);
    out->n_sharing = (int32_t)r.sharingId.size();
    out->max_common_words = r.maxCommonWords;
    out->min_common_words = r.minCommonWords;
    out->n_scores = r.nScores;
    out->n_scored = (int32_t)r.scoredId.size();
    if (!r.sharingId.empty()) {
        std::memcpy(out->sharing_id, r.sharingId.data(), r.sharingId.size() * 8);
        std::memcpy(out->sharing_words, r.sharingWords.data(), r.sharingWords.size() * 4);
    }
    if (!r.scoredId.empty()) {
        std::memcpy(out->scored_id, r.scoredId.data(), r.scoredId.size() * 8);
        std::memcpy(out->scored_score, r.scoredScore.data(), r.scoredScore.size() * 4);
    }
    return EAO_OK;
}

eao_status eao_keyframe_db_candidates(eao_keyframe_db* db, int32_t kind, uint64_t query_id, int32_t min_common_words, float min_score, int32_t n_scored,
                                      const uint64_t* scored_id, const float* scored_score, const int32_t* nb_start, const uint64_t* nb_id, uint64_t* cand_id,
                                      int32_t* n_cand, float* acc_score, uint64_t* best_id, int32_t* used_unset) {
    EAO_REQUIRE(db && n_cand && used_unset, "bad argument");
    EAO_REQUIRE(kind == 0 || kind == 1, "kind is not 0 (DetectLoopCandidates) or 1 (DetectRelocalizationCandidates)");
    EAO_REQUIRE(n_scored >= 0 && (n_scored == 0 || (scored_id && scored_score && nb_start && cand_id)), "bad argument");
    if (n_scored > 0) {
        EAO_REQUIRE(nb_start[0] == 0, "nb_start[0] != 0");
        for (int32_t i = 0; i < n_scored; i++) EAO_REQUIRE(nb_start[i] <= nb_start[i + 1], "nb_start does not ascend at entry %d", i);
        EAO_REQUIRE(nb_start[n_scored] == 0 || nb_id, "nb_id is NULL");
    }
    std::lock_guard<std::mutex> lock(db->mutex);
    kfdb::Stage2 r;
    kfdb::candidates(db->table, kind, query_id, min_common_words, min_score, n_scored, scored_id, scored_score, nb_start, nb_id, r);
    *n_cand = (int32_t)r.candId.size();
    *used_unset = r.usedUnset;
    if (!r.candId.empty()) std::memcpy(cand_id, r.candId.data(), r.candId.size() * 8);
    if (n_scored > 0 && acc_score) std::memcpy(acc_score, r.accScore.data(), (size_t)n_scored * 4);
    if (n_scored > 0 && best_id) std::memcpy(best_id, r.bestId.data(), (size_t)n_scored * 8);
    return EAO_OK;
}

}  // extern "C"
