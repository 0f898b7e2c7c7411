// Stand-ins of the reference's KeyFrame / Frame (mnId, mBowVec, GetConnectedKeyFrames, GetBestCovisibilityKeyFrames) and a driver over
// include/eaofusion/KeyFrameDatabase.h.
//   keyframe_database_driver surface      a fixed call sequence (add x3, add of a held keyframe, DetectLoopCandidates, DetectRelocalizationCandidates, erase, clear);
//                                         linked with keyframe_database_stub.cpp, which prints the library calls (tests/test_keyframe_database_class_cpu.py).
//   keyframe_database_driver chain VOC.bin LEVELSUP F0.desc .. FN.desc      (built with -DKFDB_CHAIN, linked with libeaofusion_hip.so) the vocabulary file through
//                                         ORBVocabulary::transform into KeyFrameDatabase::add for F0 .. FN-1 (mnId = index, neighbours index -1 / +1) and
//                                         DetectRelocalizationCandidates for a Frame over FN (mnId 77), then DetectLoopCandidates for keyframe N-1 (connected: N-2).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include <eaofusion/KeyFrameDatabase.h>
#ifdef KFDB_CHAIN
#include <eaofusion/ORBVocabulary.h>
#endif

namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
typedef unsigned int NodeId;
class BowVector : public std::map<WordId, WordValue> {};
class FeatureVector : public std::map<NodeId, std::vector<unsigned int>> {};
}  // namespace DBoW2

struct KeyFrame {
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
    std::set<KeyFrame*> connected;
    std::vector<KeyFrame*> covisible;      // best first
    int asked = -1;
    std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
        asked = N;
        return (int)covisible.size() <= N ? covisible : std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + N);
    }
};

struct Frame {
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};

static void print(const char* what, const std::vector<KeyFrame*>& v) {
    printf("%s", what);
    for (KeyFrame* k : v) printf(" %lu", k->mnId);
    printf("\n");
}

struct FixedVocabulary {
    unsigned int size() const { return 50; }
};

static int surface() {
    FixedVocabulary voc;
    eaofusion::KeyFrameDatabaseT<KeyFrame, Frame, FixedVocabulary> db(voc);
    KeyFrame k4, k2, k9, k12, k33, twin;
    k4.mnId = 4; k2.mnId = 2; k9.mnId = 9; k12.mnId = 12; k33.mnId = 33; twin.mnId = 2;
    k4.mBowVec[7] = 0.5; k4.mBowVec[1] = 0.5;
    k2.mBowVec[7] = 1.0;
    k12.mBowVec[1] = 0.25; k12.mBowVec[7] = 0.25; k12.mBowVec[30] = 0.5;
    k12.connected = {&k2, &k33};
    k4.covisible = {&k2, &k33};      // (33 is not held by the database)
    k9.covisible = {};
    for (int i = 0; i < 12; i++) k2.covisible.push_back(i % 2 ? &k4 : &k9);      // more than ten: ten are asked for
    db.add(&k4);
    db.add(&k2);
    db.add(&k9);
    try {
        db.add(&k2);
        printf("no throw\n");
    } catch (const std::runtime_error& e) {
        printf("threw %s\n", e.what());
    }
    print("loop", db.DetectLoopCandidates(&k12, 0.25f));
    printf("asked %d %d %d\n", k4.asked, k2.asked, k9.asked);
    Frame f;
    f.mnId = 40;
    f.mBowVec[3] = 1.0;
    print("reloc", db.DetectRelocalizationCandidates(&f));
    db.erase(&twin);      // another object with a held id: not this database's keyframe
    db.erase(&k2);
    db.erase(&k33);       // never added
    print("reloc", db.DetectRelocalizationCandidates(&f));
    db.clear();
    print("reloc", db.DetectRelocalizationCandidates(&f));
    return 0;
}

#ifdef KFDB_CHAIN
using ORBVocabulary = eaofusion::ORBVocabularyT<DBoW2::BowVector, DBoW2::FeatureVector>;

static bool read_features(const char* path, std::vector<cv::Mat>& features) {
    FILE* fp = fopen(path, "rb");
    if (!fp) return false;
    unsigned char row[32];
    while (fread(row, 1, 32, fp) == 32) {
        cv::Mat m(1, 32, CV_8U);
        memcpy(m.data, row, 32);
        features.push_back(m);
    }
    fclose(fp);
    return true;
}

static int chain(int argc, char** argv) {
    ORBVocabulary voc;
    if (!voc.loadFromBinaryFile(argv[2])) return 3;
    const int levelsup = atoi(argv[3]), n = argc - 5;      // n keyframes, then the frame
    eaofusion::KeyFrameDatabaseT<KeyFrame, Frame, ORBVocabulary> db(voc);
    std::vector<std::unique_ptr<KeyFrame>> kfs;
    DBoW2::FeatureVector fv;
    for (int i = 0; i < n; i++) {
        std::vector<cv::Mat> features;
        if (!read_features(argv[4 + i], features)) return 3;
        kfs.emplace_back(new KeyFrame);
        kfs.back()->mnId = (long unsigned int)i;
        voc.transform(features, kfs.back()->mBowVec, fv, levelsup);
    }
    for (int i = 0; i < n; i++) {
        if (i > 0) kfs[i]->covisible.push_back(kfs[i - 1].get());
        if (i + 1 < n) kfs[i]->covisible.push_back(kfs[i + 1].get());
        db.add(kfs[i].get());
    }
    Frame f;
    f.mnId = 77;
    std::vector<cv::Mat> features;
    if (!read_features(argv[4 + n], features)) return 3;
    voc.transform(features, f.mBowVec, fv, levelsup);
    printf("words");
    for (int i = 0; i < n; i++) printf(" %zu", kfs[i]->mBowVec.size());
    printf(" %zu\n", f.mBowVec.size());
    print("reloc", db.DetectRelocalizationCandidates(&f));
    kfs[n - 1]->connected = {kfs[n - 2].get()};
    print("loop", db.DetectLoopCandidates(kfs[n - 1].get(), 0.01f));
    return 0;
}
#endif

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "surface") return surface();
#ifdef KFDB_CHAIN
    if (argc >= 6 && std::string(argv[1]) == "chain") return chain(argc, argv);
#endif
    return 2;
}
