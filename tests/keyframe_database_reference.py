"""The yardstick of the KeyFrameDatabase tests: a literal restatement of the reference's src/KeyFrameDatabase.cc in plain Python, quirks included.  It keeps a real
list per word (mvInvertedFile), KeyFrame objects with the six members of include/KeyFrame.h:207-212, and numpy.float32 wherever upstream has a float; the score is
vocabulary_reference.score_l1 (ScoringObject.cpp:23-68).  Cited lines are src/KeyFrameDatabase.cc's.

What is defined here where upstream is not: mLoopScore / mRelocScore are left uninitialised by the constructor (src/KeyFrame.cc:37); a read of a score that was never
written gives float32(0) and is counted in used_unset.  Neighbours are named by id; an id the database does not hold reads as a freshly constructed KeyFrame.  A
re-added id is a new KeyFrame object."""
import numpy as np

import vocabulary_reference as VY

F32 = np.float32
N_NEIGHBOURS = 10      # :150, :264 GetBestCovisibilityKeyFrames(10)
LOOP, RELOC = 0, 1


class KeyFrame:
    def __init__(self, mnId, bow=((), ())):
        self.mnId = int(mnId)
        self.mBowVec = ([int(k) for k in bow[0]], [float(x) for x in bow[1]])      # std::map order
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = 0, 0, None           # src/KeyFrame.cc:37; None = uninitialised
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, None


class Database:
    def __init__(self, n_words):
        self.n_words = int(n_words)
        self.mvInvertedFile = {}      # word id -> list of KeyFrame, push_back order (the vector of lists, held sparsely)
        self.held = {}                # mnId -> KeyFrame, insertion order = add order of the keyframes still held
        self.used_unset = 0

    def add(self, kf):      # :39-45
        assert kf.mnId not in self.held and all(0 <= k < self.n_words for k in kf.mBowVec[0])
        for w in kf.mBowVec[0]:
            self.mvInvertedFile.setdefault(w, []).append(kf)
        self.held[kf.mnId] = kf

    def erase(self, mnId):      # :47-66
        kf = self.held.pop(mnId, None)
        if kf is None:
            return
        for w in kf.mBowVec[0]:
            lKFs = self.mvInvertedFile[w]
            for i, other in enumerate(lKFs):
                if other is kf:
                    del lKFs[i]
                    break

    def clear(self):      # :68-72
        self.mvInvertedFile = {}
        self.held = {}

    def keyframe(self, mnId):
        return self.held[mnId] if mnId in self.held else KeyFrame(mnId)

    def _score(self, kf, attr):
        s = getattr(kf, attr)
        if s is None:
            self.used_unset += 1
            return F32(0)
        return s

    def intersect(self, bow):
        """per held keyframe in add order: (mnId, number of common words, smallest common word, L1 score as a double)"""
        q = set(int(k) for k in bow[0])
        out = []
        for kf in self.held.values():
            common = [w for w in kf.mBowVec[0] if w in q]
            out.append((kf.mnId, len(common), common[0] if common else 0, VY.score_l1(bow, kf.mBowVec)))
        return out

    def detect_loop_candidates(self, mnId, bow, connected_ids, minScore, neighbours_of):      # :75-196
        minScore = F32(minScore)
        self.used_unset = 0
        r = dict(sharing_id=[], sharing_words=[], max_common_words=0, min_common_words=0, n_scores=0, scored_id=[], scored_score=[], acc_score=[], best_id=[],
                 cand_id=[], used_unset=0)
        spConnectedKeyFrames = set(connected_ids)
        lKFsSharingWords = []
        for w in [int(k) for k in bow[0]]:      # :85
            for pKFi in self.mvInvertedFile.get(w, []):      # :89
                if pKFi.mnLoopQuery != mnId:      # :92
                    pKFi.mnLoopWords = 0
                    if pKFi.mnId not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1      # :101
        if not lKFsSharingWords:      # :106
            return r
        maxCommonWords = 0
        for kf in lKFsSharingWords:      # :113-117
            if kf.mnLoopWords > maxCommonWords:
                maxCommonWords = kf.mnLoopWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))      # :119 int = int * float
        r.update(sharing_id=[kf.mnId for kf in lKFsSharingWords], sharing_words=[kf.mnLoopWords for kf in lKFsSharingWords], max_common_words=maxCommonWords,
                 min_common_words=minCommonWords)
        lScoreAndMatch = []
        nscores = 0
        for pKFi in lKFsSharingWords:      # :124-138
            if pKFi.mnLoopWords > minCommonWords:
                nscores += 1
                si = F32(VY.score_l1(bow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        r.update(n_scores=nscores, scored_id=[kf.mnId for _, kf in lScoreAndMatch], scored_score=[s for s, _ in lScoreAndMatch])
        if not lScoreAndMatch:      # :140
            return r
        lAccScoreAndMatch = []
        bestAccScore = minScore      # :144
        for s, pKFi in lScoreAndMatch:      # :147-172
            vpNeighs = [self.keyframe(i) for i in list(neighbours_of(pKFi.mnId))[:N_NEIGHBOURS]]
            bestScore, accScore, pBestKF = s, s, pKFi
            for pKF2 in vpNeighs:
                if pKF2.mnLoopQuery == mnId and pKF2.mnLoopWords > minCommonWords:      # :158
                    s2 = self._score(pKF2, "mLoopScore")
                    accScore = F32(accScore + s2)
                    if s2 > bestScore:
                        pBestKF, bestScore = pKF2, s2
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(r, lAccScoreAndMatch, bestAccScore)

    def detect_relocalization_candidates(self, mnId, bow, neighbours_of):      # :198-308
        self.used_unset = 0
        r = dict(sharing_id=[], sharing_words=[], max_common_words=0, min_common_words=0, n_scores=0, scored_id=[], scored_score=[], acc_score=[], best_id=[],
                 cand_id=[], used_unset=0)
        lKFsSharingWords = []
        for w in [int(k) for k in bow[0]]:      # :206
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnRelocQuery != mnId:      # :213
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1      # :219
        if not lKFsSharingWords:      # :223
            return r
        maxCommonWords = 0
        for kf in lKFsSharingWords:      # :228-232
            if kf.mnRelocWords > maxCommonWords:
                maxCommonWords = kf.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))      # :234
        r.update(sharing_id=[kf.mnId for kf in lKFsSharingWords], sharing_words=[kf.mnRelocWords for kf in lKFsSharingWords], max_common_words=maxCommonWords,
                 min_common_words=minCommonWords)
        lScoreAndMatch = []
        nscores = 0
        for pKFi in lKFsSharingWords:      # :241-252
            if pKFi.mnRelocWords > minCommonWords:
                nscores += 1
                si = F32(VY.score_l1(bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        r.update(n_scores=nscores, scored_id=[kf.mnId for _, kf in lScoreAndMatch], scored_score=[s for s, _ in lScoreAndMatch])
        if not lScoreAndMatch:      # :254
            return r
        lAccScoreAndMatch = []
        bestAccScore = F32(0)      # :258
        for s, pKFi in lScoreAndMatch:      # :261-286
            vpNeighs = [self.keyframe(i) for i in list(neighbours_of(pKFi.mnId))[:N_NEIGHBOURS]]
            bestScore, accScore, pBestKF = s, s, pKFi
            for pKF2 in vpNeighs:
                if pKF2.mnRelocQuery != mnId:      # :272
                    continue
                s2 = self._score(pKF2, "mRelocScore")
                accScore = F32(accScore + s2)
                if s2 > bestScore:
                    pBestKF, bestScore = pKF2, s2
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(r, lAccScoreAndMatch, bestAccScore)

    def _retain(self, r, lAccScoreAndMatch, bestAccScore):      # :174-195, :288-307
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF, vpCandidates = set(), []
        for acc, kf in lAccScoreAndMatch:
            if acc > minScoreToRetain:
                if kf.mnId not in spAlreadyAddedKF:
                    vpCandidates.append(kf.mnId)
                    spAlreadyAddedKF.add(kf.mnId)
        r.update(acc_score=[a for a, _ in lAccScoreAndMatch], best_id=[kf.mnId for _, kf in lAccScoreAndMatch], cand_id=vpCandidates, used_unset=self.used_unset)
        return r
