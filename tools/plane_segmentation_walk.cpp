// plane_segmentation_walk.cpp -- csrc/plane_seg_internal.h as a stand-alone host program: the whole of Frame::ComputePlanesFromPEAC (reference src/Frame.cc:381-460)
// over block records computed on the host, for the CPU tests (built there with -fsanitize=address,undefined) and as the single-thread baseline of
// tools/bench_plane_segmentation.py.
//
//   walk script <scene>            prints every intermediate as bit patterns (tests/test_plane_seg_host_cpu.py compares them with the yardstick's)
//   walk bench <scene> <calls>     the median time of the whole function in microseconds; build with -O3 -march=native -ffp-contract=off
//   walk fit <sums>                pseg::fit, the function the device runs, over lines "<N> <nine sums as hex doubles>": centre, normal, mse, curvature as bits
//   walk cluster <graph>           ahCluster over hand-built nodes: lines "node <rid> <N> <nine sums as hex doubles>", "edge <a> <b>", "min_support <n>"
// <scene>: a binary file, the 144 bytes of eao_plane_seg_cfg and then height * width floats.
//
// The voxel grid here is written as upstream's (PCL 1.8 VoxelGrid::applyFilter): one (voxel index, point index) entry per point and ONE std::sort of them; the
// point index as the second key is this build's reading of the order inside a voxel (ascending pixel index).
#include <chrono>
#include <cinttypes>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "../eao_fusion_amd/csrc/plane_seg_internal.h"

namespace pseg = eao::pseg;

static uint64_t bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }
static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static double from_bits(uint64_t b) { double d; std::memcpy(&d, &b, 8); return d; }

struct Scene {
    eao_plane_seg_cfg cfg;
    std::vector<float> depth;
};

static bool load(const char* path, Scene& s) {
    std::ifstream f(path, std::ios::binary);
    if (!f.read((char*)&s.cfg, sizeof(s.cfg))) return false;
    if (s.cfg.width < 1 || s.cfg.height < 1 || s.cfg.window < 2 || (int64_t)s.cfg.width * s.cfg.height > EAO_PLANE_SEG_MAX_PIXELS) return false;
    s.depth.resize((size_t)s.cfg.width * s.cfg.height);
    return (bool)f.read((char*)s.depth.data(), (std::streamsize)(s.depth.size() * 4));
}

struct Frame {
    std::vector<pseg::BlockRecord> rec;
    pseg::Segmenter seg;
    std::vector<int32_t> member;
    std::vector<std::vector<float>> clouds;      // xyz per final plane
    std::vector<int> nPixels;
};

// pcl::VoxelGrid<PointT>::applyFilter of PCL 1.8 for an all-finite cloud
static bool voxel_grid(const std::vector<float>& pts, float leaf, std::vector<float>& out) {
    const size_t n = pts.size() / 3;
    out.clear();
    if (n == 0) return true;
    float mn[3], mx[3];
    for (int k = 0; k < 3; k++) mn[k] = mx[k] = pts[k];
    for (size_t i = 1; i < n; i++)
        for (int k = 0; k < 3; k++) { mn[k] = std::min(mn[k], pts[3 * i + k]); mx[k] = std::max(mx[k], pts[3 * i + k]); }
    const float inv = 1.0f / leaf;
    int minb[3];
    int64_t div[3];
    for (int k = 0; k < 3; k++) {
        minb[k] = (int)std::floor(mn[k] * inv);
        div[k] = (int64_t)(int)std::floor(mx[k] * inv) - minb[k] + 1;
    }
    if (div[0] * div[1] * div[2] > INT_MAX) return false;
    std::vector<std::pair<int, int>> idx(n);
    for (size_t i = 0; i < n; i++) {
        const int i0 = (int)std::floor(pts[3 * i] * inv) - minb[0], i1 = (int)std::floor(pts[3 * i + 1] * inv) - minb[1], i2 = (int)std::floor(pts[3 * i + 2] * inv) - minb[2];
        idx[i] = {(int)(i0 + i1 * div[0] + i2 * div[0] * div[1]), (int)i};
    }
    std::sort(idx.begin(), idx.end());
    for (size_t i = 0; i < n;) {
        size_t j = i;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (; j < n && idx[j].first == idx[i].first; j++) { sx += pts[3 * idx[j].second]; sy += pts[3 * idx[j].second + 1]; sz += pts[3 * idx[j].second + 2]; }
        const float cnt = (float)(j - i);
        out.push_back(sx / cnt); out.push_back(sy / cnt); out.push_back(sz / cnt);
        i = j;
    }
    return true;
}

static bool run_frame(const Scene& s, Frame& f) {
    const eao_plane_seg_cfg& c = s.cfg;
    const int W = c.width, H = c.height, w = c.window, Nh = H / w, Nw = W / w;
    f.rec.resize((size_t)Nh * Nw);
    for (int bi = 0; bi < Nh; bi++)
        for (int bj = 0; bj < Nw; bj++) f.rec[(size_t)bi * Nw + bj] = pseg::block_record(c, s.depth.data(), W, bi, bj);
    f.seg.run(c, f.rec.data(), s.depth.data(), W);
    // the membership image: what k_ps_membership and k_ps_claims write
    f.member.assign((size_t)W * H, -1);
    for (int y = 0; y < Nh * w; y++)
        for (int x = 0; x < Nw * w; x++) {
            const int p = f.seg.blkMap[(size_t)(y / w) * Nw + x / w];
            if (p >= 0) f.member[(size_t)y * W + x] = f.seg.plidmap[p];
        }
    for (size_t k = 0; k + 1 < f.seg.claims.size(); k += 2) f.member[f.seg.claims[k]] = f.seg.plidmap[f.seg.claims[k + 1]];
    const size_t P = f.seg.planes.size();
    std::vector<std::vector<float>> pts(P);
    for (int i = 0; i < W * H; i++) {
        const int p = f.member[i];
        if (p < 0) continue;
        const int m = i / W, n = i - m * W;
        const double d = (double)s.depth[i];
        double x, y;
        pseg::pixel_point(c.fx, c.fy, c.cx, c.cy, m, n, d, x, y);
        pts[p].push_back((float)x); pts[p].push_back((float)y); pts[p].push_back((float)d);
    }
    f.clouds.resize(P);
    f.nPixels.resize(P);
    for (size_t p = 0; p < P; p++) {
        f.nPixels[p] = (int)(pts[p].size() / 3);
        if (!voxel_grid(pts[p], c.leaf, f.clouds[p])) return false;
    }
    return true;
}

static void print_planes(const pseg::Segmenter& sg) {
    printf("planes %zu\n", sg.planes.size());
    for (const pseg::FinalPlane& p : sg.planes) {
        for (int k = 0; k < 3; k++) printf("%016" PRIx64 " ", bits(p.normal[k]));
        for (int k = 0; k < 3; k++) printf("%016" PRIx64 " ", bits(p.center[k]));
        printf("%016" PRIx64 " %016" PRIx64 " %d %d", bits(p.mse), bits(p.curvature), p.N, p.rid);
        for (int k = 0; k < 4; k++) printf(" %08x", bits(p.coef[k]));
        printf(" %d\n", p.kept);
    }
}

static int script(const Scene& s) {
    Frame f;
    if (!run_frame(s, f)) { fprintf(stderr, "voxel grid too fine\n"); return 2; }
    printf("blocks %zu\n", f.rec.size());
    for (const pseg::BlockRecord& r : f.rec) {
        printf("%d %d", r.flag, r.N);
        for (int k = 0; k < 9; k++) printf(" %016" PRIx64, bits(r.sums[k]));
        for (int k = 0; k < 3; k++) printf(" %016" PRIx64, bits(r.center[k]));
        for (int k = 0; k < 3; k++) printf(" %016" PRIx64, bits(r.normal[k]));
        printf(" %016" PRIx64 " %016" PRIx64 "\n", bits(r.mse), bits(r.curvature));
    }
    const pseg::Segmenter& sg = f.seg;
    printf("graph %d %d\n", sg.nInitial, sg.nEdges);
    printf("merges %zu %d\n", sg.merges.size(), sg.nMergesFirst);
    for (const pseg::Merge& m : sg.merges) printf("%d %d %d\n", m.rid_p, m.rid_nb, m.N);
    printf("fill %d %d %d %d\n", sg.nSeeds, sg.nConnects, sg.nStopped, sg.nRetaken);
    printf("blkmap");
    for (int32_t v : sg.blkMap) printf(" %d", v);
    printf("\nplidmap");
    for (int32_t v : sg.plidmap) printf(" %d", v);
    printf("\nclaims %zu", sg.claims.size() / 2);
    for (int32_t v : sg.claims) printf(" %d", v);
    printf("\n");
    print_planes(sg);
    for (size_t p = 0; p < f.clouds.size(); p++) {
        printf("cloud %zu %d %zu", p, f.nPixels[p], f.clouds[p].size() / 3);
        for (float v : f.clouds[p]) printf(" %08x", bits(v));
        printf("\n");
    }
    return 0;
}

static int bench(const Scene& s, int calls) {
    std::vector<double> us;
    Frame f;
    for (int k = 0; k < calls + 3; k++) {
        const auto t0 = std::chrono::steady_clock::now();
        if (!run_frame(s, f)) return 2;
        const auto t1 = std::chrono::steady_clock::now();
        if (k >= 3) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    std::sort(us.begin(), us.end());
    printf("walk_bench_us median %.1f min %.1f max %.1f calls %d planes %zu\n", us[us.size() / 2], us.front(), us.back(), calls, f.seg.planes.size());
    return 0;
}

static int cluster(const char* path) {
    std::ifstream in(path);
    if (!in) return 1;
    pseg::Segmenter sg;
    eao_plane_seg_cfg c;
    std::memset(&c, 0, sizeof(c));
    c.min_support = 3000; c.max_step = 100000;
    c.depth_sigma = 1.6e-6; c.std_tol_init = 5; c.std_tol_merge = 8;
    c.similarity_merge = std::cos((60.0) * M_PI / 180.0);
    std::string line, word;
    int maxRid = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        if (!(ls >> word)) continue;
        if (word == "node") {
            pseg::Node n;
            ls >> n.rid >> n.N;
            for (int k = 0; k < 9; k++) { std::string h; ls >> h; n.sums[k] = from_bits(std::strtoull(h.c_str(), nullptr, 16)); }
            if (!ls || n.N < 4 || n.rid < 0 || n.rid > (1 << 20)) return 1;
            pseg::fit(n.sums, n.N, n.center, n.normal, n.mse, n.curvature);
            maxRid = std::max(maxRid, n.rid);
            sg.nodes.push_back(n);
        } else if (word == "edge") {
            int a = -1, b = -1;
            ls >> a >> b;
            if (!ls || a < 0 || b < 0 || a >= (int)sg.nodes.size() || b >= (int)sg.nodes.size() || a == b) return 1;
            sg.connect(a, b);
        } else if (word == "min_support") {
            ls >> c.min_support;
        }
    }
    sg.c = c;
    sg.ds.reset(maxRid + 1);
    for (size_t k = 0; k < sg.nodes.size(); k++)
        if (sg.nodes[k].mse == sg.nodes[k].mse) sg.queue.insert({sg.nodes[k].mse, (int)k});
    const int steps = sg.cluster();
    printf("steps %d\nmerges %zu\n", steps, sg.merges.size());
    for (const pseg::Merge& m : sg.merges) printf("%d %d %d\n", m.rid_p, m.rid_nb, m.N);
    printf("extracted %zu\n", sg.extracted.size());
    for (int e : sg.extracted) printf("%d %d %d %016" PRIx64 "\n", e, sg.nodes[e].rid, sg.nodes[e].N, bits(sg.nodes[e].mse));
    return 0;
}

static int fit_lines(const char* path) {
    std::ifstream in(path);
    if (!in) return 1;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        int N = 0;
        double sums[9], center[3], normal[3], mse, curvature;
        if (!(ls >> N)) continue;
        for (int k = 0; k < 9; k++) { std::string h; ls >> h; sums[k] = from_bits(std::strtoull(h.c_str(), nullptr, 16)); }
        if (!ls || N < 4) return 1;
        pseg::fit(sums, N, center, normal, mse, curvature);
        for (int k = 0; k < 3; k++) printf("%016" PRIx64 " ", bits(center[k]));
        for (int k = 0; k < 3; k++) printf("%016" PRIx64 " ", bits(normal[k]));
        printf("%016" PRIx64 " %016" PRIx64 "\n", bits(mse), bits(curvature));
    }
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "cluster" && argc == 3) return cluster(argv[2]);
    if (mode == "fit" && argc == 3) return fit_lines(argv[2]);
    Scene s;
    if ((mode != "script" && mode != "bench") || argc < 3 || !load(argv[2], s)) {
        fprintf(stderr, "usage: %s script <scene> | bench <scene> <calls> | fit <sums> | cluster <graph>\n", argv[0]);
        return 1;
    }
    if (mode == "script") return script(s);
    return bench(s, argc > 3 ? std::max(1, atoi(argv[3])) : 20);
}
