// vocabulary_internal.h -- the host half of eao_vocabulary_create (vocabulary.hip), free of HIP: validation of an eao_vocabulary_desc and the remap of its
// nodes into the device table, in which the children of one node are contiguous.
//
// Slot 0 is the root; the slots follow in breadth-first order, every node's children in ascending file id (the loaders' push_back order,
// Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1404, :1464: the order the descent breaks ties in).  File ids need not be contiguous among siblings, the slots are.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eao_fusion.h"

namespace eao {
namespace voc {

struct NodeMeta {            // one 16-byte load per level of the descent
    int32_t child_begin;     // slot of the first child
    int32_t child_count;     // 0 = the descent ends here
    uint32_t file_id;        // the node id upstream knows (0 = root)
    uint32_t word_id;        // of a leaf: its rank among the leaf-flagged nodes in id order
};
static_assert(sizeof(NodeMeta) == 16, "NodeMeta is loaded as one int4");

struct Table {
    int32_t n_nodes = 0, n_words = 0, depth = 0, max_children = 0, weighting = 0, norm = 0;
    std::vector<NodeMeta> meta;          // n_nodes + 1
    std::vector<uint8_t> descriptor;     // (n_nodes + 1) * 32, slot order (the root's is zero and never read)
    std::vector<double> weight;          // n_nodes + 1, slot order
};

// false + a message when the desc is not a vocabulary (include/eao_fusion.h, "The handle")
inline bool flatten(const eao_vocabulary_desc* d, Table& t, std::string& err) {
    if (!d) { err = "desc is NULL"; return false; }
    if (d->n_nodes < 0) { err = "n_nodes < 0"; return false; }
    if (d->weighting < 0 || d->weighting > 3) { err = "weighting is not one of TF_IDF, TF, IDF, BINARY (0 .. 3)"; return false; }
    if (d->norm < 0 || d->norm > 2) { err = "norm is not one of none, L1, L2 (0 .. 2)"; return false; }
    const int32_t n = d->n_nodes;
    if (n > 0 && (!d->parent || !d->descriptor || !d->weight || !d->is_leaf)) { err = "a node array is NULL"; return false; }
    t = Table();
    t.n_nodes = n;
    t.weighting = d->weighting;
    t.norm = d->norm;
    if (n == 0) return true;
    std::vector<int32_t> count((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; i++) {
        if (d->parent[i] < 0 || d->parent[i] >= i + 1) { err = "parent[" + std::to_string(i) + "] is not in 0 .. " + std::to_string(i); return false; }
        count[d->parent[i]]++;
    }
    for (int32_t i = 0; i < n; i++)
        if ((d->is_leaf[i] != 0) != (count[(size_t)i + 1] == 0)) {
            err = "is_leaf[" + std::to_string(i) + "] disagrees with the children of node " + std::to_string(i + 1);
            return false;
        }
    // children of every node in ascending id: a counting sort by parent over the ids in order
    std::vector<int32_t> first((size_t)n + 2, 0), kids(n);
    for (int32_t id = 0; id <= n; id++) first[(size_t)id + 1] = first[id] + count[id];
    {
        std::vector<int32_t> fill(first.begin(), first.end() - 1);
        for (int32_t i = 0; i < n; i++) kids[fill[d->parent[i]]++] = i + 1;
    }
    std::vector<uint32_t> word((size_t)n + 1, 0);
    for (int32_t i = 0; i < n; i++)
        if (d->is_leaf[i]) word[(size_t)i + 1] = (uint32_t)t.n_words++;
    std::vector<int32_t> ids((size_t)n + 1), level((size_t)n + 1, 0);      // slot -> file id; parent[i] < i + 1 makes the tree connected, so every id gets a slot
    ids[0] = 0;
    t.meta.resize((size_t)n + 1);
    t.descriptor.assign(((size_t)n + 1) * 32, 0);
    t.weight.assign((size_t)n + 1, 0.0);
    int32_t next = 1;
    for (int32_t s = 0; s <= n; s++) {
        const int32_t id = ids[s];
        NodeMeta& m = t.meta[s];
        m.child_begin = next;
        m.child_count = count[id];
        m.file_id = (uint32_t)id;
        m.word_id = word[id];
        if (id > 0) {
            std::memcpy(&t.descriptor[(size_t)s * 32], d->descriptor + (size_t)(id - 1) * 32, 32);
            t.weight[s] = d->weight[id - 1];
        }
        if (count[id] > t.max_children) t.max_children = count[id];
        if (count[id] == 0 && level[s] > t.depth) t.depth = level[s];
        for (int32_t c = 0; c < count[id]; c++) {
            ids[next] = kids[first[id] + c];
            level[next] = level[s] + 1;
            next++;
        }
    }
    return true;
}

}  // namespace voc
}  // namespace eao
