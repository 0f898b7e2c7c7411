// A stand-in for libeaofusion_hip.so's KeyFrameDatabase entry points that needs no device: it prints every call it receives and answers by a made-up rule, so
// that the CPU suite can check what include/eaofusion/KeyFrameDatabase.h sends and what it does with the answer (tests/test_keyframe_database_class_cpu.py
// restates the rules).
//   add: an id that is held is EAO_ERR_INVALID, as in the library.
//   query_scores: lKFsSharingWords = the held ids in add order with 3 words each; min_common_words = 2; lScoreAndMatch = the held ids in REVERSE add order,
//                 entry i with score 0.5 + i / 8.
//   candidates: the first neighbour of the first scored entry that has one, then the scored ids in reverse.
#include <algorithm>
#include <cstdio>
#include <vector>

#include <eao_fusion.h>

struct eao_keyframe_db {
    std::vector<uint64_t> held;
};

extern "C" {

const char* eao_last_error(void) { return "stub"; }

eao_status eao_keyframe_db_create(int32_t n_words, eao_keyframe_db** out) {
    printf("create n_words %d\n", n_words);
    *out = new eao_keyframe_db;
    return EAO_OK;
}

void eao_keyframe_db_destroy(eao_keyframe_db* db) {
    printf("destroy\n");
    delete db;
}

eao_status eao_keyframe_db_clear(eao_keyframe_db* db) {
    printf("clear\n");
    db->held.clear();
    return EAO_OK;
}

eao_status eao_keyframe_db_add(eao_keyframe_db* db, uint64_t kf_id, int32_t n, const uint32_t* word_id, const double* word_val) {
    printf("add %llu n %d", (unsigned long long)kf_id, n);
    for (int i = 0; i < n; i++) printf(" %u:%.17g", word_id[i], word_val[i]);
    printf("\n");
    if (std::find(db->held.begin(), db->held.end(), kf_id) != db->held.end()) return EAO_ERR_INVALID;
    db->held.push_back(kf_id);
    return EAO_OK;
}

eao_status eao_keyframe_db_erase(eao_keyframe_db* db, uint64_t kf_id) {
    printf("erase %llu\n", (unsigned long long)kf_id);
    db->held.erase(std::remove(db->held.begin(), db->held.end(), kf_id), db->held.end());
    return EAO_OK;
}

eao_status eao_keyframe_db_query_scores(eao_keyframe_db* db, const eao_keyframe_db_query* q, int32_t cap, eao_keyframe_db_scored* out) {
    printf("query kind %d id %llu min_score %.9g cap %d q", q->kind, (unsigned long long)q->query_id, q->min_score, cap);
    for (int i = 0; i < q->nq; i++) printf(" %u:%.17g", q->q_id[i], q->q_val[i]);
    printf(" connected");
    std::vector<uint64_t> c(q->connected_id, q->connected_id + q->n_connected);
    std::sort(c.begin(), c.end());
    for (uint64_t x : c) printf(" %llu", (unsigned long long)x);
    printf("\n");
    const int n = (int)db->held.size();
    if (cap < n) return EAO_ERR_INVALID;
    out->n_sharing = out->n_scored = out->n_scores = n;
    out->max_common_words = 3;
    out->min_common_words = 2;
    for (int i = 0; i < n; i++) {
        out->sharing_id[i] = db->held[i];
        out->sharing_words[i] = 3;
        out->scored_id[i] = db->held[n - 1 - i];
        out->scored_score[i] = 0.5f + i / 8.0f;
    }
    return EAO_OK;
}

eao_status eao_keyframe_db_candidates(eao_keyframe_db*, int32_t kind, uint64_t query_id, int32_t min_common_words, float min_score, int32_t n_scored,
                                      const uint64_t* scored_id, const float* scored_score, const int32_t* nb_start, const uint64_t* nb_id, uint64_t* cand_id,
                                      int32_t* n_cand, float* acc_score, uint64_t* best_id, int32_t* used_unset) {
    printf("candidates kind %d id %llu min_common %d min_score %.9g scored", kind, (unsigned long long)query_id, min_common_words, min_score);
    for (int i = 0; i < n_scored; i++) printf(" %llu:%.9g", (unsigned long long)scored_id[i], scored_score[i]);
    printf(" start");
    for (int i = 0; i <= n_scored; i++) printf(" %d", nb_start[i]);
    printf(" nb");
    for (int k = 0; k < nb_start[n_scored]; k++) printf(" %llu", (unsigned long long)nb_id[k]);
    printf(" optional %d %d\n", acc_score ? 1 : 0, best_id ? 1 : 0);
    std::vector<uint64_t> cand;
    if (nb_start[n_scored] > 0) cand.push_back(nb_id[0]);
    for (int i = n_scored - 1; i >= 0; i--)
        if (std::find(cand.begin(), cand.end(), scored_id[i]) == cand.end() && (int)cand.size() < n_scored) cand.push_back(scored_id[i]);
    *n_cand = (int32_t)cand.size();
    for (size_t i = 0; i < cand.size(); i++) cand_id[i] = cand[i];
    *used_unset = 0;
    return EAO_OK;
}

}  // extern "C"
