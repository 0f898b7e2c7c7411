// adapter_detail_test.cpp -- include/eaofusion/adapter_detail.h held to literals, as a program of its own (tests/test_adapter_detail_cpu.py builds it with
// -fsanitize=address,undefined and runs it).  Nothing of the library is linked: eao_last_error is the two-function stub below.
//
// Every matrix carries asymmetric contents, m(r, c) = 10 r + c + 0.5, so that a transposition or a stride slip shows.  Every vector helper is tried on a
// 3 x 1 (4 x 1) and on a 1 x 3 (1 x 4).  The 4 x 4 read is also tried on a matrix whose step exceeds cols * sizeof(float) (the stand-in cv::Mat can be built
// over external storage with a step, and as a roi of a wider matrix).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <eaofusion/adapter_detail.h>

static const char* g_error = "";
static void set_last_error(const char* e) { g_error = e; }
extern "C" const char* eao_last_error(void) { return g_error; }

namespace D = eaofusion::detail;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static float cell(int r, int c) { return 10.f * r + c + 0.5f; }
static cv::Mat filled(int rows, int cols) {
    cv::Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) m.at<float>(r, c) = cell(r, c);
    return m;
}
static cv::Mat col(int n) { cv::Mat m(n, 1, CV_32F); for (int k = 0; k < n; k++) m.at<float>(k, 0) = 100.f + 7.f * k; return m; }
static cv::Mat row(int n) { cv::Mat m(1, n, CV_32F); for (int k = 0; k < n; k++) m.at<float>(0, k) = 100.f + 7.f * k; return m; }
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void test_check() {
    set_last_error("must not be read");
    bool threw = false;
    try { D::check(EAO_OK, "eao_plane_map_add"); } catch (...) { threw = true; }
    EXPECT(!threw);
    set_last_error("stub");
    std::string what;
    try { D::check(EAO_ERR_INVALID, "eao_plane_map_add"); } catch (const std::runtime_error& e) { what = e.what(); }
    EXPECT(what == "eao_plane_map_add: stub");
}

static void test_matrix_reads() {
    float out[16];
    const cv::Mat m4 = filled(4, 4);
    D::read44(m4, out);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) EXPECT(out[r * 4 + c] == cell(r, c));
    // step > cols * sizeof(float): (a) external storage with a row pitch of six floats, (b) the 4 x 4 block at (1, 2) of a 7 x 8 matrix
    float wide[4 * 6];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 6; c++) wide[r * 6 + c] = c < 4 ? cell(r, c) : -1.f;
    const cv::Mat pitched(4, 4, CV_32F, wide, 6 * sizeof(float));
    EXPECT(pitched.step > (size_t)pitched.cols * sizeof(float));
    std::memset(out, 0, sizeof out);
    D::read44(pitched, out);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) EXPECT(out[r * 4 + c] == cell(r, c));
    const cv::Mat big = filled(7, 8), block = big.roi(2, 1, 4, 4);
    EXPECT(!block.isContinuous());
    D::read44(block, out);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) EXPECT(out[r * 4 + c] == cell(r + 1, c + 2));

    float o9[9];
    D::read33(filled(3, 3), o9);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) EXPECT(o9[r * 3 + c] == cell(r, c));
    D::read33(big.roi(3, 2, 3, 3), o9);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) EXPECT(o9[r * 3 + c] == cell(r + 2, c + 3));

    const cv::Mat shapes3[2] = {col(3), row(3)}, shapes4[2] = {col(4), row(4)};
    for (int s = 0; s < 2; s++) {
        float v[5] = {-1, -1, -1, -1, -1};
        D::read3(shapes3[s], v);
        EXPECT(v[0] == 100.f && v[1] == 107.f && v[2] == 114.f && v[3] == -1.f);
        D::read4(shapes4[s], v);
        EXPECT(v[0] == 100.f && v[1] == 107.f && v[2] == 114.f && v[3] == 121.f && v[4] == -1.f);
        std::vector<float> p(1, 9.f);
        D::push3(shapes3[s], p);
        EXPECT(p.size() == 4 && p[0] == 9.f && p[1] == 100.f && p[2] == 107.f && p[3] == 114.f);
        D::push4(shapes4[s], p);
        EXPECT(p.size() == 8 && p[4] == 100.f && p[5] == 107.f && p[6] == 114.f && p[7] == 121.f);
    }
    // a column of a wider matrix (step = eight floats)
    cv::Mat tall = filled(5, 8);
    float v[3];
    D::read3(tall.roi(6, 1, 1, 3), v);
    EXPECT(v[0] == cell(1, 6) && v[1] == cell(2, 6) && v[2] == cell(3, 6));
}

static void test_pose_and_intrinsics() {
    const cv::Mat R = filled(3, 3);
    const cv::Mat ts[2] = {col(3), row(3)};
    for (int s = 0; s < 2; s++) {
        float T[16];
        for (int k = 0; k < 16; k++) T[k] = -5.f;
        D::read_pose(R, ts[s], T);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) EXPECT(T[r * 4 + c] == cell(r, c));
            EXPECT(T[r * 4 + 3] == 100.f + 7.f * r);
        }
        EXPECT(T[12] == 0.f && T[13] == 0.f && T[14] == 0.f && T[15] == 1.f);
    }
    float K[4];
    D::read_intrinsics(filled(3, 3), K);
    EXPECT(K[0] == cell(0, 0) && K[1] == cell(1, 1) && K[2] == cell(0, 2) && K[3] == cell(1, 2));
}

static void test_writes() {
    float src[16];
    for (int k = 0; k < 16; k++) src[k] = cell(k / 4, k % 4);
    const cv::Mat m = D::mat_of(src, 4, 4);
    EXPECT(m.rows == 4 && m.cols == 4 && m.type() == CV_32F);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) EXPECT(m.at<float>(r, c) == cell(r, c));
    const cv::Mat m23 = D::mat_of(src, 2, 3);      // rows of THREE: element (1, 0) is src[3]
    EXPECT(m23.rows == 2 && m23.cols == 3 && m23.at<float>(1, 0) == src[3] && m23.at<float>(0, 2) == src[2]);
    const cv::Mat c3 = D::mat_of(src, 3, 1);
    EXPECT(c3.rows == 3 && c3.cols == 1 && c3.at<float>(0, 0) == src[0] && c3.at<float>(1, 0) == src[1] && c3.at<float>(2, 0) == src[2]);

    cv::Mat big = cv::Mat::zeros(7, 8, CV_32F), block = big.roi(2, 1, 4, 4);      // a write through a step of eight floats
    D::write44(block, src);
    for (int r = 0; r < 7; r++)
        for (int c = 0; c < 8; c++) {
            const bool in = r >= 1 && r < 5 && c >= 2 && c < 6;
            EXPECT(big.at<float>(r, c) == (in ? cell(r - 1, c - 2) : 0.f));
        }
    cv::Mat c4(4, 1, CV_32F), r4(1, 4, CV_32F);
    D::write_vec(c4, src + 1, 4);
    D::write_vec(r4, src + 1, 4);
    for (int k = 0; k < 4; k++) EXPECT(c4.at<float>(k, 0) == src[1 + k] && r4.at<float>(0, k) == src[1 + k]);
    cv::Mat c3w = cv::Mat::zeros(4, 1, CV_32F);
    D::write_vec(c3w, src + 4, 3);
    EXPECT(c3w.at<float>(0, 0) == src[4] && c3w.at<float>(2, 0) == src[6] && c3w.at<float>(3, 0) == 0.f);
}

// The epipole against the literal expression of the header's contract: a double accumulator over k = 0, 1, 2, then + (double)t, rounded once to float; then
// invz = 1.0f / C2[2], ex = fx * C2[0] * invz + cx, ey the same.  The inputs come from a small seeded search for cases in which a FLOAT accumulator would give
// another ex or ey: only on those does the test tell the two apart.
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s; }
static float unit(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f) * 2.f - 1.f; }      // [-1, 1)
static void test_epipole() {
    uint32_t seed = 20240611u;
    int found = 0;
    for (int trial = 0; trial < 4000 && found < 8; trial++) {
        cv::Mat R(3, 3, CV_32F), Cw(3, 1, CV_32F), t(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R.at<float>(r, c) = unit(seed); Cw.at<float>(r) = 3.f * unit(seed); t.at<float>(r) = 2.f * unit(seed); }
        t.at<float>(2) += 6.f;      // the first camera in front of the second
        const float fx = 517.306408f, fy = 516.469215f, cx = 318.643040f, cy = 255.313989f;
        float Cd[3], Cf[3];
        for (int r = 0; r < 3; r++) {
            double acc = 0;
            for (int k = 0; k < 3; k++) acc += (double)R.at<float>(r, k) * (double)Cw.at<float>(k);
            Cd[r] = (float)(acc + (double)t.at<float>(r));
            float accf = 0;
            for (int k = 0; k < 3; k++) accf += R.at<float>(r, k) * Cw.at<float>(k);
            Cf[r] = accf + t.at<float>(r);
        }
        const float invz = 1.0f / Cd[2], wantx = fx * Cd[0] * invz + cx, wanty = fy * Cd[1] * invz + cy;
        const float invzf = 1.0f / Cf[2], fltx = fx * Cf[0] * invzf + cx, flty = fy * Cf[1] * invzf + cy;
        if (!std::isfinite(wantx) || !std::isfinite(wanty) || (same_bits(wantx, fltx) && same_bits(wanty, flty))) continue;
        found++;
        float ex = 0, ey = 0;
        D::epipole(Cw, R, t, fx, fy, cx, cy, ex, ey);
        EXPECT(same_bits(ex, wantx) && same_bits(ey, wanty));
        EXPECT(!(same_bits(ex, fltx) && same_bits(ey, flty)));      // the case means something: float accumulation lands elsewhere
        cv::Mat CwRow(1, 3, CV_32F), tRow(1, 3, CV_32F);            // 1 x 3 vectors give the same
        for (int k = 0; k < 3; k++) { CwRow.at<float>(0, k) = Cw.at<float>(k); tRow.at<float>(0, k) = t.at<float>(k); }
        float exr = 0, eyr = 0;
        D::epipole(CwRow, R, tRow, fx, fy, cx, cy, exr, eyr);
        EXPECT(same_bits(exr, wantx) && same_bits(eyr, wanty));
    }
    EXPECT(found == 8);
}

static void test_flatten() {
    std::map<unsigned, std::vector<unsigned> > fv;
    fv[12] = std::vector<unsigned>(1, 1u);
    fv[3] = std::vector<unsigned>{7u, 9u};
    fv[10] = std::vector<unsigned>();
    D::FeatVecArrays a;
    a.id.assign(5, 99u); a.index.assign(5, 99u); a.start.assign(5, 99);      // what an earlier call left is dropped
    const eao_feature_vector f = D::flatten(fv, a);
    EXPECT(f.n_nodes == 3 && f.node_id == a.id.data() && f.node_start == a.start.data() && f.index == a.index.data());
    EXPECT((a.id == std::vector<uint32_t>{3u, 10u, 12u}));
    EXPECT((a.start == std::vector<int32_t>{0, 2, 2, 3}));
    EXPECT((a.index == std::vector<uint32_t>{7u, 9u, 1u}));
    const eao_feature_vector e = D::flatten(std::map<unsigned, std::vector<unsigned> >(), a);
    EXPECT(e.n_nodes == 0 && a.start == std::vector<int32_t>(1, 0) && a.index.empty());
}

// A generator that answers 1, 1, 1, ... and records what it was asked.
struct Scripted {
    static std::vector<std::pair<int, int> > asked;
    static int RandomInt(int lo, int hi) { asked.push_back(std::make_pair(lo, hi)); return 1; }
};
std::vector<std::pair<int, int> > Scripted::asked;

// Initializer.h's loop as it stands (reference src/Initializer.cc:78-97): the drawn POSITION is overwritten with the back and popped
template <class RandomT> static std::vector<int> initializer_draw(int N, int k) {
    std::vector<size_t> vAvailableIndices;
    for (int i = 0; i < N; i++) vAvailableIndices.push_back(i);
    std::vector<int> set;
    for (int j = 0; j < k; j++) {
        int randi = RandomT::RandomInt(0, (int)vAvailableIndices.size() - 1);
        int idx = (int)vAvailableIndices[randi];
        set.push_back(idx);
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
    }
    return set;
}

static void test_draw() {
    // by hand, N = 5, k = 3, every draw answers position 1:
    //   the solvers' loop:  [0 1 2 3 4] -> 1, slot[1] = 4;  [0 4 2 3|4] -> 4, slot[4] = 3 (past the live part);  [0 4 2|3 3] -> 4        => (1, 4, 4)
    //   Initializer's loop: [0 1 2 3 4] -> 1, slot[1] = 4;  [0 4 2 3]   -> 4, slot[1] = 3;                        [0 3 2]     -> 3        => (1, 4, 3)
    const std::vector<std::pair<int, int> > args = {{0, 4}, {0, 3}, {0, 2}};
    int32_t sets[6] = {-1, -1, -1, -1, -1, -1};
    Scripted::asked.clear();
    D::draw_sets<Scripted>(5, 3, 1, sets);
    EXPECT(sets[0] == 1 && sets[1] == 4 && sets[2] == 4 && sets[3] == -1);
    EXPECT(Scripted::asked == args);
    Scripted::asked.clear();
    D::draw_sets<Scripted>(5, 3, 2, sets);      // every hypothesis starts from 0 .. N-1 again
    EXPECT(sets[0] == 1 && sets[1] == 4 && sets[2] == 4 && sets[3] == 1 && sets[4] == 4 && sets[5] == 4);
    EXPECT(Scripted::asked.size() == 6 && Scripted::asked[3] == args[0] && Scripted::asked[5] == args[2]);
    Scripted::asked.clear();
    D::draw_sets<Scripted>(5, 3, 0, sets);
    EXPECT(Scripted::asked.empty());
    Scripted::asked.clear();
    const std::vector<int> other = initializer_draw<Scripted>(5, 3);
    EXPECT((other == std::vector<int>{1, 4, 3}));
    EXPECT(Scripted::asked == args);
}

int main() {
    test_check();
    test_matrix_reads();
    test_pose_and_intrinsics();
    test_writes();
    test_epipole();
    test_flatten();
    test_draw();
    if (failures) { std::printf("%d expectation(s) failed\n", failures); return 1; }
    std::printf("adapter_detail: all as written\n");
    return 0;
}
