// Drives include/eaofusion/Initializer.h through InitializerT with stand-in frames and a RandomT that replays a recorded RandomInt sequence.  Linked with
// initializer_stub.cpp (tests/test_initializer_class_cpu.py) or with libeaofusion_hip.so (tests/test_gpu_initializer.py).  Standard input:
//   fx fy cx cy sigma iterations | n1, n1 x (x y) | n2, n2 x (x y) | n1 x vMatches12 | count, count x randi
// Output: the generator's log, what Initialize returned, R21 / t21 (rows, cols, values; pre-set to 2 x 2 so that "left alone" shows), vP3D and vbTriangulated
// (pre-set to one sentinel element each).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <eaofusion/Initializer.h>

struct Frame {
    cv::Mat mK;
    std::vector<cv::KeyPoint> mvKeysUn;
};

struct ReplayRandom {
    static std::vector<int>& seq() { static std::vector<int> s; return s; }
    static size_t& pos() { static size_t p = 0; return p; }
    static int& seeds() { static int n = 0; return n; }
    static int& bad() { static int n = 0; return n; }
    static void SeedRandOnce(int seed) { seeds() += 1 + 1000 * seed; }
    static int RandomInt(int min, int max) {
        if (pos() >= seq().size()) { bad()++; return min; }
        const int v = seq()[pos()++];
        if (min != 0 || v > max) bad()++;
        return v;
    }
};

static void read_keys(std::vector<cv::KeyPoint>& keys) {
    int n = 0;
    if (scanf("%d", &n) != 1) exit(2);
    keys.resize(n);
    for (int i = 0; i < n; i++)
        if (scanf("%f %f", &keys[i].pt.x, &keys[i].pt.y) != 2) exit(2);
}

static void print_mat(const char* name, const cv::Mat& m) {
    printf("%s %d %d", name, m.rows, m.cols);
    for (int i = 0; i < m.rows; i++)
        for (int j = 0; j < m.cols; j++) printf(" %.9g", m.at<float>(i, j));
    printf("\n");
}

int main() {
    float fx, fy, cx, cy, sigma;
    int iterations;
    if (scanf("%f %f %f %f %f %d", &fx, &fy, &cx, &cy, &sigma, &iterations) != 6) return 2;
    Frame f1, f2;
    f1.mK = cv::Mat::eye(3, 3, CV_32F);
    f1.mK.at<float>(0, 0) = fx; f1.mK.at<float>(1, 1) = fy; f1.mK.at<float>(0, 2) = cx; f1.mK.at<float>(1, 2) = cy;
    f2.mK = f1.mK.clone();
    read_keys(f1.mvKeysUn);
    read_keys(f2.mvKeysUn);
    std::vector<int> vMatches12(f1.mvKeysUn.size());
    for (size_t i = 0; i < vMatches12.size(); i++)
        if (scanf("%d", &vMatches12[i]) != 1) return 2;
    int count = 0;
    if (scanf("%d", &count) != 1) return 2;
    ReplayRandom::seq().resize(count);
    for (int i = 0; i < count; i++)
        if (scanf("%d", &ReplayRandom::seq()[i]) != 1) return 2;
    eaofusion::InitializerT<Frame, ReplayRandom> init(f1, sigma, iterations);
    cv::Mat R21 = cv::Mat::zeros(2, 2, CV_32F), t21 = cv::Mat::zeros(2, 2, CV_32F);
    std::vector<cv::Point3f> vP3D(1, cv::Point3f(-1, -2, -3));
    std::vector<bool> vbTriangulated(1, true);
    const bool ok = init.Initialize(f2, vMatches12, R21, t21, vP3D, vbTriangulated);
    printf("random seeds %d draws %zu bad %d\n", ReplayRandom::seeds(), ReplayRandom::pos(), ReplayRandom::bad());
    printf("returned %d\n", ok ? 1 : 0);
    print_mat("R21", R21);
    print_mat("t21", t21);
    printf("p3d %zu", vP3D.size());
    for (const cv::Point3f& p : vP3D) printf(" %.9g %.9g %.9g", p.x, p.y, p.z);
    printf("\ntriangulated %zu", vbTriangulated.size());
    for (bool b : vbTriangulated) printf(" %d", b ? 1 : 0);
    printf("\n");
    return 0;
}
