// KeyFrameDatabase.h -- KeyFrameDatabase (reference include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) on top of the C-ABI (eao_keyframe_db_*).
//
// The BoW vectors of the added keyframes are resident on the device; there is no inverted file.  A query is two library calls: stage 1
// (eao_keyframe_db_query_scores: the intersection kernel, then lKFsSharingWords and lScoreAndMatch in upstream's order) and stage 2
// (eao_keyframe_db_candidates: the covisibility accumulation, on the host) with GetBestCovisibilityKeyFrames(10) of the scored keyframes gathered in between.
// This class keeps the mnId -> KeyFrame* map and returns upstream's pointers in upstream's order.
//
//   // include/KeyFrameDatabase.h in an EAO-Fusion checkout: the class becomes a using-declaration; src/KeyFrameDatabase.cc leaves the build
//   #include <eaofusion/KeyFrameDatabase.h>
//   namespace ORB_SLAM2 { class KeyFrame; class Frame; using KeyFrameDatabase = eaofusion::KeyFrameDatabaseT<KeyFrame, Frame, ORBVocabulary>; }
//
// It does NOT write KeyFrame::mnLoopQuery / mnLoopWords / mLoopScore / mnRelocQuery / mnRelocWords / mRelocScore: the library keeps them per id, and nothing
// else in the reference reads them.  Other divergences are the library's (include/eao_fusion.h, "KeyFrameDatabase"): adding a keyframe that is held throws where
// upstream would list it twice; a keyframe that is erased and added again starts with fresh state.
//
// KeyFrameT: mnId, mBowVec (std::map<WordId, WordValue>), GetConnectedKeyFrames() -> std::set<KeyFrameT*>, GetBestCovisibilityKeyFrames(int) ->
// std::vector<KeyFrameT*>.  FrameT: mnId, mBowVec.  VocabularyT: size().
#pragma once

#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

template <class KeyFrameT, class FrameT, class VocabularyT>
class KeyFrameDatabaseT {
public:
    explicit KeyFrameDatabaseT(const VocabularyT& voc) : mpVoc(&voc) {      // :33-37
        detail::check(eao_keyframe_db_create((int32_t)voc.size(), &mHandle), "eao_keyframe_db_create");
    }
    ~KeyFrameDatabaseT() {
        if (mHandle) eao_keyframe_db_destroy(mHandle);
    }
    KeyFrameDatabaseT(const KeyFrameDatabaseT&) = delete;
    KeyFrameDatabaseT& operator=(const KeyFrameDatabaseT&) = delete;

    void add(KeyFrameT* pKF) {      // :39-45
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<uint32_t> id;
        std::vector<double> val;
        pack(pKF->mBowVec, id, val);
        detail::check(eao_keyframe_db_add(mHandle, (uint64_t)pKF->mnId, (int32_t)id.size(), id.data(), val.data()), "eao_keyframe_db_add");
        mKeyFrames[(uint64_t)pKF->mnId] = pKF;
    }

    void erase(KeyFrameT* pKF) {      // :47-66
        std::unique_lock<std::mutex> lock(mMutex);
        auto it = mKeyFrames.find((uint64_t)pKF->mnId);
        if (it == mKeyFrames.end() || it->second != pKF) return;
        detail::check(eao_keyframe_db_erase(mHandle, (uint64_t)pKF->mnId), "eao_keyframe_db_erase");
        mKeyFrames.erase(it);
    }

    void clear() {      // :68-72
        std::unique_lock<std::mutex> lock(mMutex);
        detail::check(eao_keyframe_db_clear(mHandle), "eao_keyframe_db_clear");
        mKeyFrames.clear();
    }

    std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT* pKF, float minScore) {      // :75-196
        std::vector<uint64_t> connected;
        for (KeyFrameT* c : pKF->GetConnectedKeyFrames()) connected.push_back((uint64_t)c->mnId);      // :77, outside the lock as upstream
        return detect(0, (uint64_t)pKF->mnId, pKF->mBowVec, connected, minScore);
    }

    std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F) {      // :198-308
        return detect(1, (uint64_t)F->mnId, F->mBowVec, std::vector<uint64_t>(), 0.0f);
    }

private:
    template <class BowVectorT>
    static void pack(const BowVectorT& v, std::vector<uint32_t>& id, std::vector<double>& val) {
        id.reserve(v.size());
        val.reserve(v.size());
        for (const auto& e : v) {
            id.push_back((uint32_t)e.first);
            val.push_back((double)e.second);
        }
    }

    template <class BowVectorT>
    std::vector<KeyFrameT*> detect(int32_t kind, uint64_t queryId, const BowVectorT& bow, const std::vector<uint64_t>& connected, float minScore) {
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<uint32_t> qId;
        std::vector<double> qVal;
        pack(bow, qId, qVal);
        const int32_t cap = (int32_t)mKeyFrames.size();
        std::vector<uint64_t> sharingId((size_t)cap), scoredId((size_t)cap);
        std::vector<int32_t> sharingWords((size_t)cap);
        std::vector<float> scoredScore((size_t)cap);
        eao_keyframe_db_query q = eao_keyframe_db_query();
        q.kind = kind;
        q.query_id = queryId;
        q.nq = (int32_t)qId.size();
        q.q_id = qId.data();
        q.q_val = qVal.data();
        q.n_connected = (int32_t)connected.size();
        q.connected_id = connected.data();
        q.min_score = minScore;
        eao_keyframe_db_scored s = eao_keyframe_db_scored();
        s.sharing_id = sharingId.data();
        s.sharing_words = sharingWords.data();
        s.scored_id = scoredId.data();
        s.scored_score = scoredScore.data();
        detail::check(eao_keyframe_db_query_scores(mHandle, &q, cap, &s), "eao_keyframe_db_query_scores");
        if (s.n_scored == 0) return std::vector<KeyFrameT*>();      // :106, :140 / :223, :254
        // GetBestCovisibilityKeyFrames(10) of every scored keyframe (:150, :264) as a CSR over ids; a neighbour need not be held by the database
        std::map<uint64_t, KeyFrameT*> seen;
        std::vector<int32_t> nbStart(1, 0);
        std::vector<uint64_t> nbId;
        for (int32_t i = 0; i < s.n_scored; i++) {
            KeyFrameT* pKFi = mKeyFrames.at(scoredId[i]);
            seen[scoredId[i]] = pKFi;
            for (KeyFrameT* pKF2 : pKFi->GetBestCovisibilityKeyFrames(10)) {
                nbId.push_back((uint64_t)pKF2->mnId);
                seen[(uint64_t)pKF2->mnId] = pKF2;
            }
            nbStart.push_back((int32_t)nbId.size());
        }
        std::vector<uint64_t> candId((size_t)s.n_scored);
        int32_t nCand = 0, usedUnset = 0;
        detail::check(eao_keyframe_db_candidates(mHandle, kind, queryId, s.min_common_words, minScore, s.n_scored, scoredId.data(), scoredScore.data(), nbStart.data(),
                                                 nbId.data(), candId.data(), &nCand, nullptr, nullptr, &usedUnset),
                      "eao_keyframe_db_candidates");
        std::vector<KeyFrameT*> out;
        out.reserve((size_t)nCand);
        for (int32_t i = 0; i < nCand; i++) out.push_back(seen.at(candId[i]));
        return out;
    }

    const VocabularyT* mpVoc;
    eao_keyframe_db* mHandle = nullptr;
    std::map<uint64_t, KeyFrameT*> mKeyFrames;      // mnId -> the keyframes held
    std::mutex mMutex;
};

}  // namespace eaofusion
