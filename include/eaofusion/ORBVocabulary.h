// ORBVocabulary.h -- ORBVocabulary (reference include/ORBVocabulary.h = DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB>) on top of the
// C-ABI (eao_vocabulary_*, eao_bow_score_l1).
//
// The file parse stays on the host: both loaders are this project's own code over the two file formats (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1350-1480
// describes them), flatten the nodes into the five arrays of eao_vocabulary_desc and hand them to the library once.  transform is one library call (the descent,
// both sorts and the sums run on the device); the maps are rebuilt from its arrays.  score for one pair is a merge of two short lists and runs here, op for op
// upstream's (ScoringObject.cpp:23-68); scoreBatch -- an addition -- sends one query and the stored vectors of a candidate loop (src/KeyFrameDatabase.cc:124-138,
// 243-254, src/LoopClosing.cc:125-138) through eao_bow_score_l1 in one call.
//
//   // include/ORBVocabulary.h in an EAO-Fusion checkout: the typedef becomes a using-declaration, src/System.cc:77-79 and every caller compile unchanged
//   #include <eaofusion/ORBVocabulary.h>
//   #include "Thirdparty/DBoW2/DBoW2/BowVector.h"
//   #include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"
//   namespace ORB_SLAM2 { using ORBVocabulary = eaofusion::ORBVocabularyT<DBoW2::BowVector, DBoW2::FeatureVector>; }
//
// Divergences from upstream, all on files upstream mis-reads ("ORBVocabulary"):
//  * Both upstream loaders loop on `!f.eof()` and so process one record past the end of the data.  The text loader appends a junk child of the root with
//    uninitialised descriptor bytes (:1390-1432); the binary loader appends a duplicate of the last node (:1457-1477), which strict < can never select but which,
//    when it is a leaf, makes size() one larger.  These loaders stop at the end of the data.
//  * m_L is not taken from the header but derived by the library as the largest leaf depth (include/eao_fusion.h, "The handle"); k is not used at all.
//  * A missing file, a header outside upstream's own range check (:1371), a binary header whose node size is not 41 bytes, a truncated record or a node the
//    library rejects make the loader return false; upstream reads on.
//  * score / scoreBatch offer L1 only (ORB-SLAM2 uses nothing else): on a vocabulary of another scoring type they throw.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

// BowVectorT: std::map<WordId, WordValue> (DBoW2::BowVector); FeatureVectorT: std::map<NodeId, std::vector<unsigned int>> (DBoW2::FeatureVector)
template <class BowVectorT, class FeatureVectorT>
class ORBVocabularyT {
public:
    ORBVocabularyT() {}
    ~ORBVocabularyT() { reset(); }
    ORBVocabularyT(const ORBVocabularyT&) = delete;
    ORBVocabularyT& operator=(const ORBVocabularyT&) = delete;

    // "k L scoring weighting", then one line per node: "parent isLeaf d0 .. d31 weight" (:1350-1436)
    bool loadFromTextFile(const std::string& filename) {
        std::ifstream f(filename.c_str());
        if (!f.is_open()) return false;
        std::string line;
        if (!std::getline(f, line)) return false;
        int k = -1, L = -1, n1 = -1, n2 = -1;
        {
            std::stringstream ss(line);
            ss >> k >> L >> n1 >> n2;
            if (ss.fail()) return false;
        }
        if (k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3) return false;      // upstream's check (:1371)
        std::vector<int32_t> parent;
        std::vector<uint8_t> desc, leaf;
        std::vector<double> weight;
        while (std::getline(f, line)) {
            if (line.find_first_not_of(" \t\r\n") == std::string::npos) continue;      // the end of the data: a trailing newline is no node
            std::stringstream ss(line);
            int pid = 0, isLeaf = 0;
            ss >> pid >> isLeaf;
            uint8_t d[32];
            for (int i = 0; i < 32; i++) {
                int v = 0;
                ss >> v;
                d[i] = (uint8_t)v;
            }
            double w = 0;
            ss >> w;
            if (ss.fail()) return false;
            parent.push_back(pid);
            leaf.push_back(isLeaf > 0 ? 1 : 0);
            desc.insert(desc.end(), d, d + 32);
            weight.push_back(w);
        }
        return create(parent, desc, weight, leaf, n1, n2);
    }

    // u32 nb_nodes (the root included), u32 size_node, i32 k, i32 L, i32 scoring, i32 weighting, then nb_nodes - 1 records of
    // { u32 parent, 32 descriptor bytes, f32 weight, u8 isLeaf } (:1438-1506)
    bool loadFromBinaryFile(const std::string& filename) {
        std::ifstream f(filename.c_str(), std::ios::in | std::ios::binary);
        if (!f.is_open()) return false;
        uint32_t head[2];
        int32_t mode[4];
        f.read((char*)head, sizeof(head));
        f.read((char*)mode, sizeof(mode));
        if (!f || head[1] != kRecord || head[0] < 1 || mode[2] < 0 || mode[2] > 5 || mode[3] < 0 || mode[3] > 3) return false;
        const size_t n = (size_t)head[0] - 1;
        std::vector<char> raw(n * kRecord);
        f.read(raw.data(), (std::streamsize)raw.size());
        if ((size_t)f.gcount() != raw.size()) return false;      // a truncated record
        std::vector<int32_t> parent(n);
        std::vector<uint8_t> desc(n * 32), leaf(n);
        std::vector<double> weight(n);
        for (size_t i = 0; i < n; i++) {
            const char* r = raw.data() + i * kRecord;
            uint32_t p;
            float w;
            std::memcpy(&p, r, 4);
            std::memcpy(&desc[i * 32], r + 4, 32);
            std::memcpy(&w, r + 36, 4);
            if (p > 0x7fffffffu) return false;
            parent[i] = (int32_t)p;
            weight[i] = w;      // float -> WordValue (:1467)
            leaf[i] = r[40] ? 1 : 0;
        }
        return create(parent, desc, weight, leaf, mode[2], mode[3]);
    }

    // TemplatedVocabulary::transform(features, v, fv, levelsup) (:1138-1206): features are 1 x 32 CV_8U rows (Frame::ComputeBoW's toDescriptorVector)
    void transform(const std::vector<cv::Mat>& features, BowVectorT& v, FeatureVectorT& fv, int levelsup) const {
        v.clear();
        fv.clear();
        if (!mHandle || mWords == 0 || features.empty()) return;      // empty() (:1146)
        const int n = (int)features.size();
        std::vector<uint8_t> desc((size_t)n * 32);
        for (int i = 0; i < n; i++) std::memcpy(&desc[(size_t)i * 32], features[i].data, 32);
        std::vector<uint32_t> wordId(n), nodeId(n), index(n);
        std::vector<double> wordValue(n);
        std::vector<int32_t> nodeStart((size_t)n + 1);
        eao_bow_result r = eao_bow_result();
        r.word_id = wordId.data();
        r.word_value = wordValue.data();
        r.node_id = nodeId.data();
        r.node_start = nodeStart.data();
        r.index = index.data();
        detail::check(eao_vocabulary_transform(mHandle, desc.data(), n, levelsup, &r), "eao_vocabulary_transform");
        for (int k = 0; k < r.n_words; k++) v.insert(v.end(), typename BowVectorT::value_type(wordId[k], wordValue[k]));
        for (int k = 0; k < r.n_fv_nodes; k++) {
            auto it = fv.insert(fv.end(), typename FeatureVectorT::value_type(nodeId[k], typename FeatureVectorT::mapped_type()));
            it->second.assign(index.begin() + nodeStart[k], index.begin() + nodeStart[k + 1]);
        }
    }

    // L1Scoring::score (ScoringObject.cpp:23-68) on the host, op for op
    double score(const BowVectorT& v1, const BowVectorT& v2) const {
        requireL1();
        auto a = v1.begin();
        auto b = v2.begin();
        double s = 0;
        while (a != v1.end() && b != v2.end()) {
            if (a->first == b->first) {
                const double vi = a->second, wi = b->second;
                s += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
                ++a;
                ++b;
            } else if (a->first < b->first) {
                a = v1.lower_bound(b->first);
            } else {
                b = v2.lower_bound(a->first);
            }
        }
        return -s / 2.0;
    }

    // score(query, *stored[j]) for every j, in one library call
    std::vector<double> scoreBatch(const BowVectorT& query, const std::vector<const BowVectorT*>& stored) const {
        requireL1();
        std::vector<uint32_t> qId, dId;
        std::vector<double> qVal, dVal;
        for (const auto& e : query) {
            qId.push_back(e.first);
            qVal.push_back(e.second);
        }
        std::vector<int32_t> start(stored.size() + 1, 0);
        for (size_t j = 0; j < stored.size(); j++) {
            for (const auto& e : *stored[j]) {
                dId.push_back(e.first);
                dVal.push_back(e.second);
            }
            start[j + 1] = (int32_t)dId.size();
        }
        std::vector<double> out(stored.size());
        detail::check(eao_bow_score_l1((int32_t)qId.size(), qId.data(), qVal.data(), (int32_t)stored.size(), start.data(), dId.data(), dVal.data(), out.data()), "eao_bow_score_l1");
        return out;
    }

    unsigned int size() const { return (unsigned int)mWords; }      // m_words.size()
    bool empty() const { return mWords == 0; }

private:
    static constexpr uint32_t kRecord = 4 + 32 + 4 + 1;

    // what mustNormalize() yields for upstream's ScoringType (ScoringObject.h:74-89): L1_NORM L1, L2_NORM L2, CHI_SQUARE / KL / BHATTACHARYYA L1, DOT_PRODUCT none
    static int32_t normOf(int scoring) { return scoring == 1 ? 2 : scoring == 5 ? 0 : 1; }

    void requireL1() const {
        if (mScoring != 0) throw std::logic_error("eaofusion::ORBVocabulary offers L1 scoring only");
    }

    void reset() {
        if (mHandle) eao_vocabulary_destroy(mHandle);
        mHandle = nullptr;
        mWords = 0;
    }

    bool create(const std::vector<int32_t>& parent, const std::vector<uint8_t>& desc, const std::vector<double>& weight, const std::vector<uint8_t>& leaf, int scoring,
                int weighting) {
        reset();
        eao_vocabulary_desc d = eao_vocabulary_desc();
        d.n_nodes = (int32_t)parent.size();
        d.parent = parent.data();
        d.descriptor = desc.data();
        d.weight = weight.data();
        d.is_leaf = leaf.data();
        d.weighting = weighting;
        d.norm = normOf(scoring);
        if (eao_vocabulary_create(&d, &mHandle) != EAO_OK) {
            mHandle = nullptr;
            return false;
        }
        int32_t words = 0;
        eao_vocabulary_info(mHandle, nullptr, &words, nullptr, nullptr);
        mWords = words;
        mScoring = scoring;
        return true;
    }

    eao_vocabulary* mHandle = nullptr;
    int32_t mWords = 0;
    int mScoring = 0;
};

}  // namespace eaofusion
