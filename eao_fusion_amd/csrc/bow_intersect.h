// bow_intersect.h -- the per-pair loop shared by k_bow_score_l1 (vocabulary.hip) and k_kfdb_intersect (keyframe_db.hip): ONE wavefront intersects one stored
// BowVector (ascending word ids dbId[b .. e), values dbVal) with the query (ascending qId[0 .. nq), qVal).
// Every lane looks one stored word up in the query by binary search; a 64-bit ballot names the common words of the 64-word chunk, and their terms are added in
// ascending word id, the same additions in every lane: L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), the sum s before :65's -s / 2.
// kCount: also the number of common words and the smallest common word id (unspecified while the count is 0).
#pragma once
#include <hip/hip_runtime.h>

namespace eao {

template <bool kCount, typename Index>
__device__ __forceinline__ double bow_l1_pair(int nq, const unsigned* qId, const double* qVal, const unsigned* dbId, const double* dbVal, Index b, Index e, int lane,
                                              int& common, unsigned& firstWord) {
    typedef unsigned long long u64;
    double s = 0.0;
    for (Index c0 = b; c0 < e; c0 += 64) {
        const Index c = c0 + lane;
        double term = 0.0;
        bool hit = false;
        unsigned id = 0;
        if (c < e) {
            id = dbId[c];
            int lo = 0, hi = nq;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (qId[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            if (lo < nq && qId[lo] == id) {
                const double vi = qVal[lo], wi = dbVal[c];
                term = (fabs(vi - wi) - fabs(vi)) - fabs(wi);      // ScoringObject.cpp:41, left to right
                hit = true;
            }
        }
        u64 mask = __ballot(hit);
        if (kCount && mask) {
            if (common == 0) firstWord = (unsigned)__shfl((int)id, __ffsll((long long)mask) - 1);      // ids ascend: the first hit of the first chunk with one
            common += __popcll(mask);
        }
        while (mask) {      // the common words in ascending id: the same additions in every lane
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            s += __shfl(term, l);
        }
    }
    return s;
}

}  // namespace eao
