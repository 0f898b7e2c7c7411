// A single-threaded host walk of the flattened vocabulary table (eao_fusion_amd/csrc/vocabulary_internal.h: the layout the device kernels read), built with
// -O3 by tools/bench_vocabulary.py as the CPU yardstick of its timings.  This project's own code; it computes what k_voc_descend computes, per feature.
//   vocabulary_walk IN OUT REPS
// IN:  int32 n_nodes, n_features, levelsup; parent[n_nodes] i32; descriptor[n_nodes*32]; weight[n_nodes] f64; is_leaf[n_nodes]; features[n_features*32]
// OUT: word[n_features] u32, node[n_features] u32, stopped[n_features] u8; stdout: "first_ms <the first pass> best_ms <the fastest of REPS passes>"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../eao_fusion_amd/csrc/vocabulary_internal.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[3];
    if (!read_all(f, head, sizeof(head))) return 3;
    const int32_t n = head[0], nf = head[1], levelsup = head[2];
    std::vector<int32_t> parent(n);
    std::vector<uint8_t> desc((size_t)n * 32), leaf(n), feats((size_t)nf * 32);
    std::vector<double> weight(n);
    if (!read_all(f, parent.data(), (size_t)n * 4) || !read_all(f, desc.data(), desc.size()) || !read_all(f, weight.data(), (size_t)n * 8) ||
        !read_all(f, leaf.data(), (size_t)n) || !read_all(f, feats.data(), feats.size()))
        return 3;
    fclose(f);
    eao_vocabulary_desc d = eao_vocabulary_desc();
    d.n_nodes = n;
    d.parent = parent.data();
    d.descriptor = desc.data();
    d.weight = weight.data();
    d.is_leaf = leaf.data();
    d.weighting = 0;
    d.norm = 1;
    eao::voc::Table t;
    std::string err;
    if (!eao::voc::flatten(&d, t, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 4;
    }
    std::vector<uint32_t> word(nf), node(nf);
    std::vector<uint8_t> stopped(nf);
    const int nidLevel = t.depth - levelsup;
    double first = 0, best = 1e30;
    const int reps = atoi(argv[3]);
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < nf; i++) {
            uint32_t q[8];
            std::memcpy(q, &feats[(size_t)i * 32], 32);
            int cur = 0, level = 0;
            uint32_t nid = 0;
            bool have = nidLevel <= 0;
            while (t.meta[cur].child_count > 0) {
                level++;
                const eao::voc::NodeMeta m = t.meta[cur];
                int bestD = 1 << 30, bestC = 0;
                for (int c = 0; c < m.child_count; c++) {
                    uint32_t w[8];
                    std::memcpy(w, &t.descriptor[(size_t)(m.child_begin + c) * 32], 32);
                    int dist = 0;
                    for (int k = 0; k < 8; k++) dist += __builtin_popcount(q[k] ^ w[k]);
                    if (dist < bestD) {
                        bestD = dist;
                        bestC = c;
                    }
                }
                cur = m.child_begin + bestC;
                if (level == nidLevel) {
                    nid = t.meta[cur].file_id;
                    have = true;
                }
            }
            uint8_t st = t.weight[cur] > 0 ? 0 : 1;
            if (!have) {
                nid = t.meta[cur].file_id;
                st |= 2;
            }
            word[i] = t.meta[cur].word_id;
            node[i] = nid;
            stopped[i] = st;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (r == 0) first = ms;
        if (ms < best) best = ms;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    fwrite(word.data(), 4, nf, o);
    fwrite(node.data(), 4, nf, o);
    fwrite(stopped.data(), 1, nf, o);
    fclose(o);
    printf("first_ms %.6f best_ms %.6f nodes %d words %d depth %d max_children %d\n", first, best, t.n_nodes, t.n_words, t.depth, t.max_children);
    return 0;
}
