// A stand-in for libeaofusion_hip.so's vocabulary entry points that needs no device: it prints every call it receives and answers by a made-up rule, so that
// the CPU suite can check what include/eaofusion/ORBVocabulary.h sends and what it does with the answer (tests/test_vocabulary_class_cpu.py restates the rules).
//   create: rejects parent[i] >= i + 1, as the library does; n_words = the number of leaf flags.
//   transform: feature i has word d[i][0] % 5 with weight 0.5 (the value of a word = 0.5 * its count) and node 10 + d[i][1] % 3.
//   score: scores[j] = 1000 nq + 10 (entries of vector j) + 0.25 j.
#include <cstdio>
#include <map>
#include <vector>

#include <eao_fusion.h>

struct eao_vocabulary {
    int32_t n_nodes, n_words;
};

extern "C" {

const char* eao_last_error(void) { return "stub"; }

eao_status eao_vocabulary_create(const eao_vocabulary_desc* d, eao_vocabulary** out) {
    printf("create n %d weighting %d norm %d parent", d->n_nodes, d->weighting, d->norm);
    for (int i = 0; i < d->n_nodes; i++) printf(" %d", d->parent[i]);
    printf(" leaf");
    for (int i = 0; i < d->n_nodes; i++) printf(" %d", d->is_leaf[i]);
    printf(" weight");
    for (int i = 0; i < d->n_nodes; i++) printf(" %.17g", d->weight[i]);
    printf(" desc");
    for (int i = 0; i < d->n_nodes * 32; i++) printf(" %d", d->descriptor[i]);
    printf("\n");
    int words = 0;
    for (int i = 0; i < d->n_nodes; i++) {
        if (d->parent[i] < 0 || d->parent[i] >= i + 1) return EAO_ERR_INVALID;
        words += d->is_leaf[i] ? 1 : 0;
    }
    *out = new eao_vocabulary{d->n_nodes, words};
    return EAO_OK;
}

void eao_vocabulary_destroy(eao_vocabulary* v) {
    printf("destroy\n");
    delete v;
}

eao_status eao_vocabulary_info(const eao_vocabulary* v, int32_t* n_nodes, int32_t* n_words, int32_t* depth, int32_t* max_children) {
    if (n_nodes) *n_nodes = v->n_nodes;
    if (n_words) *n_words = v->n_words;
    if (depth) *depth = 0;
    if (max_children) *max_children = 0;
    return EAO_OK;
}

eao_status eao_vocabulary_transform(const eao_vocabulary*, const uint8_t* desc, int32_t n, int32_t levelsup, eao_bow_result* r) {
    printf("transform n %d levelsup %d bytes", n, levelsup);
    for (int i = 0; i < n * 32; i++) printf(" %d", desc[i]);
    printf("\n");
    std::map<uint32_t, int> words;
    std::map<uint32_t, std::vector<uint32_t>> nodes;
    for (int i = 0; i < n; i++) {
        words[desc[i * 32] % 5]++;
        nodes[10 + desc[i * 32 + 1] % 3].push_back((uint32_t)i);
    }
    r->n_words = 0;
    for (const auto& w : words) {
        r->word_id[r->n_words] = w.first;
        r->word_value[r->n_words++] = 0.5 * w.second;
    }
    r->n_fv_nodes = 0;
    int at = 0;
    for (const auto& nd : nodes) {
        r->node_id[r->n_fv_nodes] = nd.first;
        r->node_start[r->n_fv_nodes++] = at;
        for (uint32_t i : nd.second) r->index[at++] = i;
    }
    r->node_start[r->n_fv_nodes] = at;
    return EAO_OK;
}

eao_status eao_bow_score_l1(int32_t nq, const uint32_t* q_id, const double* q_val, int32_t n_db, const int32_t* db_start, const uint32_t* db_id, const double* db_val,
                            double* scores) {
    printf("score nq %d q", nq);
    for (int i = 0; i < nq; i++) printf(" %u:%.17g", q_id[i], q_val[i]);
    printf(" ndb %d start", n_db);
    for (int j = 0; j <= n_db; j++) printf(" %d", db_start[j]);
    printf(" db");
    for (int c = 0; c < db_start[n_db]; c++) printf(" %u:%.17g", db_id[c], db_val[c]);
    printf("\n");
    for (int j = 0; j < n_db; j++) scores[j] = 1000.0 * nq + 10.0 * (db_start[j + 1] - db_start[j]) + 0.25 * j;
    return EAO_OK;
}

}  // extern "C"
