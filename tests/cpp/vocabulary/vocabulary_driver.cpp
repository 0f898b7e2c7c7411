// Stand-ins of DBoW2::BowVector / DBoW2::FeatureVector (the two std::maps, Thirdparty/DBoW2/DBoW2/BowVector.h:56-57, FeatureVector.h:24-25) and a driver over
// include/eaofusion/ORBVocabulary.h.
//   vocabulary_driver text|binary FILE     loads FILE; prints "loaded 0|1 size N empty 0|1"; on success transforms six made-up features (feature i: byte 0 =
//                                          7 i + 3, byte 1 = i * i, the rest i) at levelsup 4 and prints the two maps it rebuilt, then scoreBatch of that vector
//                                          against {itself, a second vector, an empty one} and the host score of each (or that scoring was refused).
//   vocabulary_driver text|binary FILE FEATURES LEVELSUP    the same over the descriptors of the file FEATURES (n x 32 raw bytes) at LEVELSUP.
// Linked with vocabulary_stub.cpp (prints the library calls) in the CPU suite, with libeaofusion_hip.so in the device suite.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <eaofusion/ORBVocabulary.h>

namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
typedef unsigned int NodeId;
class BowVector : public std::map<WordId, WordValue> {};
class FeatureVector : public std::map<NodeId, std::vector<unsigned int>> {};
}  // namespace DBoW2

namespace ORB_SLAM2 {
using ORBVocabulary = eaofusion::ORBVocabularyT<DBoW2::BowVector, DBoW2::FeatureVector>;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string kind = argv[1];
    ORB_SLAM2::ORBVocabulary voc;
    const bool ok = kind == "text" ? voc.loadFromTextFile(argv[2]) : voc.loadFromBinaryFile(argv[2]);
    printf("loaded %d size %u empty %d\n", ok ? 1 : 0, voc.size(), voc.empty() ? 1 : 0);
    if (!ok) return 0;
    std::vector<cv::Mat> features;
    int levelsup = 4;
    if (argc >= 5) {
        levelsup = atoi(argv[4]);
        FILE* fp = fopen(argv[3], "rb");
        if (!fp) return 3;
        unsigned char row[32];
        while (fread(row, 1, 32, fp) == 32) {
            cv::Mat m(1, 32, CV_8U);
            memcpy(m.data, row, 32);
            features.push_back(m);
        }
        fclose(fp);
    } else {
        for (int i = 0; i < 6; i++) {
            cv::Mat m(1, 32, CV_8U);
            for (int b = 0; b < 32; b++) m.data[b] = (unsigned char)i;
            m.data[0] = (unsigned char)(7 * i + 3);
            m.data[1] = (unsigned char)(i * i);
            features.push_back(m);
        }
    }
    DBoW2::BowVector v;
    DBoW2::FeatureVector fv;
    v[99] = 1.0;      // (transform clears what it is given)
    fv[99].push_back(1);
    voc.transform(features, v, fv, levelsup);
    printf("bow");
    for (const auto& e : v) printf(" %u:%.17g", e.first, e.second);
    printf("\nfv");
    for (const auto& e : fv) {
        printf(" %u:", e.first);
        for (size_t k = 0; k < e.second.size(); k++) printf("%s%u", k ? "," : "", e.second[k]);
    }
    printf("\n");
    DBoW2::BowVector second, none;
    second[0] = 0.125;
    second[3] = 0.3;
    second[4] = 0.7;
    second[77] = 0.1;
    try {
        const std::vector<double> s = voc.scoreBatch(v, {&v, &second, &none});
        printf("scores");
        for (double x : s) printf(" %.17g", x);
        printf("\nhost %.17g %.17g %.17g\n", voc.score(v, v), voc.score(v, second), voc.score(v, none));
    } catch (const std::logic_error& e) {      // a vocabulary of another scoring type than L1_NORM
        printf("scores refused: %s\n", e.what());
    }
    return 0;
}
