// keyframe_db_internal.h -- the host half of eao_keyframe_db_* (keyframe_db.hip), free of HIP: the entry table of the resident arena, the per-keyframe state of
// the reference's KeyFrame (include/KeyFrame.h:207-212) and everything src/KeyFrameDatabase.cc does with the result of its inverted-file walk.
//
// No inverted file is kept.  Upstream's walk (:85-103, :206-221) goes over the query's words in ascending id (std::map) and inside one word's list in push_back
// order; every add pushes to all of its words at once (:43-44) and erase removes from all of them (:52-64), so the position inside ANY list is the add order of the
// keyframes still held.  A keyframe enters lKFsSharingWords at the first of the query's words it holds, so the list order is ascending (first common word, add
// sequence) over the listed keyframes.  The device hands back, per stored vector, the number of common words, the first common word and the L1 score
// (k_kfdb_intersect); walk() below turns them into the lists, counts and scores of :75-141 / :198-255, candidates() is :143-195 / :257-307.
//
// Per-keyframe state: mnLoopQuery / mnLoopWords / mLoopScore and mnRelocQuery / mnRelocWords / mRelocScore, per id, initial state (0, 0, unset) as the
// constructor leaves them (src/KeyFrame.cc:37 sets the four integers, the two floats stay uninitialised).  A score that was never written reads as 0.0f and the
// read is counted (used_unset).  An id the table does not hold -- never added, or erased -- reads as the initial state.
//
// Deviations from upstream:
//   - adding an id that is live is refused (upstream would push it twice and list it twice);
//   - erasing an unknown id is a no-op, as upstream;
//   - a re-added id starts with fresh state (upstream's KeyFrame object would keep its members; a keyframe is erased when it is set bad and never comes back);
//   - word ids at or above n_words are refused (upstream indexes past mvInvertedFile).
// Storage: the policy of resident_arena.h over one arena of words; storage order is add order.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "resident_arena.h"

namespace eao {
namespace kfdb {

constexpr int kMaxWordsPerVector = 8192;      // EAO_VOCABULARY_MAX_FEATURES

struct KfState {      // include/KeyFrame.h:207-212
    uint64_t loopQuery = 0;
    int32_t loopWords = 0;
    float loopScore = 0.0f;
    bool loopSet = false;
    uint64_t relocQuery = 0;
    int32_t relocWords = 0;
    float relocScore = 0.0f;
    bool relocSet = false;
};

using Entry = arena::Entry<arena::NoPayload>;      // one stored vector: words begin .. begin + count - 1 of the arena

struct Table : arena::Table<arena::NoPayload> {      // entries in storage order = add order
    std::unordered_map<uint64_t, KfState> state;       // live ids

    void clear() {
        arena::Table<arena::NoPayload>::clear();
        state.clear();
    }
    // "" when (id, n, wordId) may be added
    std::string check_add(uint64_t id, int64_t n, const uint32_t* wordId, int64_t nWords) const {
        if (n < 0) return "n < 0";
        if (n > kMaxWordsPerVector) return "the vector has " + std::to_string(n) + " words; at most " + std::to_string(kMaxWordsPerVector) + " are supported";
        if (n > 0 && !wordId) return "word_id is NULL";
        if (byId.count(id)) return "keyframe " + std::to_string(id) + " is already held";
        for (int64_t i = 0; i < n; i++) {
            if ((int64_t)wordId[i] >= nWords) return "word id " + std::to_string(wordId[i]) + " is not below n_words = " + std::to_string(nWords);
            if (i > 0 && wordId[i - 1] >= wordId[i]) return "the word ids do not ascend strictly at entry " + std::to_string(i);
        }
        return "";
    }
    // appends with fresh state; returns the arena position of the vector's first word
    uint64_t append(uint64_t id, uint32_t n) {
        state[id] = KfState();
        return arena::Table<arena::NoPayload>::append(id, n);
    }
    bool erase(uint64_t id) {
        state.erase(id);
        return arena::Table<arena::NoPayload>::erase(id);
    }
    KfState read(uint64_t id) const {
        auto it = state.find(id);
        return it == state.end() ? KfState() : it->second;
    }
};

struct Stage1 {
    std::vector<uint64_t> sharingId;      // lKFsSharingWords, list order
    std::vector<int32_t> sharingWords;    // mnLoopWords / mnRelocWords of each
    int32_t maxCommonWords = 0, minCommonWords = 0, nScores = 0;
    std::vector<uint64_t> scoredId;       // lScoreAndMatch, list order
    std::vector<float> scoredScore;
};

// KeyFrameDatabase.cc:85-138 (kind 0) / :206-252 (kind 1) over the intersection of the query with the n live entries in storage order.
inline void walk(Table& t, int kind, uint64_t queryId, int32_t n, const uint64_t* id, const int32_t* common, const uint32_t* firstWord, const double* score,
                 const std::unordered_set<uint64_t>& connected, float minScore, Stage1& r) {
    r = Stage1();
    std::vector<int32_t> listed;
    for (int32_t j = 0; j < n; j++) {
        const int32_t c = common[j];
        if (c <= 0) continue;      // in none of the query's lists
        KfState& s = t.state[id[j]];
        if (kind == 0) {
            if (s.loopQuery != queryId) {      // :92
                if (connected.count(id[j])) {
                    s.loopWords = 1;      // :94, :101 at every word: reset, then one
                } else {
                    s.loopQuery = queryId;      // :97-98
                    s.loopWords = c;
                    listed.push_back(j);
                }
            } else {
                s.loopWords += c;      // :101 on top of what an earlier query with this id left
            }
        } else {
            if (s.relocQuery != queryId) {      // :213-217
                s.relocQuery = queryId;
                s.relocWords = c;
                listed.push_back(j);
            } else {
                s.relocWords += c;      // :219
            }
        }
    }
    if (listed.empty()) return;      // :106, :223
    // first-encounter order: the first common word, then the position inside that word's list = add order = storage order
    std::stable_sort(listed.begin(), listed.end(), [&](int32_t a, int32_t b) { return firstWord[a] < firstWord[b]; });
    int maxCommonWords = 0;
    for (int32_t j : listed) {      // :112-117 (a listed entry's count is c: it was reset by this query)
        r.sharingId.push_back(id[j]);
        r.sharingWords.push_back(common[j]);
        if (common[j] > maxCommonWords) maxCommonWords = common[j];
    }
    const int minCommonWords = maxCommonWords * 0.8f;      // :119, :234: int * float, truncated
    r.maxCommonWords = maxCommonWords;
    r.minCommonWords = minCommonWords;
    for (int32_t j : listed) {
        if (common[j] > minCommonWords) {      // :128, :245
            r.nScores++;
            const float si = score[j];      // :132, :248: the double narrowed once
            KfState& s = t.state[id[j]];
            if (kind == 0) {
                s.loopScore = si;
                s.loopSet = true;
                if (si >= minScore) {      // :135
                    r.scoredId.push_back(id[j]);
                    r.scoredScore.push_back(si);
                }
            } else {
                s.relocScore = si;
                s.relocSet = true;
                r.scoredId.push_back(id[j]);
                r.scoredScore.push_back(si);
            }
        }
    }
}

struct Stage2 {
    std::vector<uint64_t> candId;      // vpLoopCandidates / vpRelocCandidates
    std::vector<float> accScore;       // per scored entry
    std::vector<uint64_t> bestId;      // per scored entry
    int32_t usedUnset = 0;             // reads of a score that was never written (upstream: an uninitialised float)
};

// KeyFrameDatabase.cc:143-195 (kind 0) / :257-307 (kind 1).  nbStart / nbId: GetBestCovisibilityKeyFrames(10) of every scored entry as a CSR.
inline void candidates(const Table& t, int kind, uint64_t queryId, int32_t minCommonWords, float minScore, int32_t nScored, const uint64_t* scoredId,
                       const float* scoredScore, const int32_t* nbStart, const uint64_t* nbId, Stage2& r) {
    r = Stage2();
    if (nScored <= 0) return;      // :140, :254
    float bestAccScore = kind == 0 ? minScore : 0.0f;      // :144, :258
    for (int32_t i = 0; i < nScored; i++) {
        float bestScore = scoredScore[i];
        float accScore = scoredScore[i];
        uint64_t best = scoredId[i];
        for (int32_t k = nbStart[i]; k < nbStart[i + 1]; k++) {
            const KfState s = t.read(nbId[k]);
            float sc;
            if (kind == 0) {
                if (!(s.loopQuery == queryId && s.loopWords > minCommonWords)) continue;      // :158
                sc = s.loopScore;
                if (!s.loopSet) r.usedUnset++;
            } else {
                if (s.relocQuery != queryId) continue;      // :272
                sc = s.relocScore;
                if (!s.relocSet) r.usedUnset++;
            }
            accScore += sc;      // :160, :275
            if (sc > bestScore) {      // :161, :276
                best = nbId[k];
                bestScore = sc;
            }
        }
        r.accScore.push_back(accScore);
        r.bestId.push_back(best);
        if (accScore > bestAccScore) bestAccScore = accScore;      // :170, :284
    }
    const float minScoreToRetain = 0.75f * bestAccScore;      // :175, :289
    std::unordered_set<uint64_t> added;
    for (int32_t i = 0; i < nScored; i++)
        if (r.accScore[i] > minScoreToRetain && added.insert(r.bestId[i]).second) r.candId.push_back(r.bestId[i]);      // :183-190, :296-303
}

}  // namespace kfdb
}  // namespace eao
