// yolox_walk.cpp -- the host header of the yolox feature (eao_fusion_amd/csrc/yolox_internal.h) as a program of its own: the sanitizer target of
// tests/test_yolox_host_cpu.py (g++ -fsanitize=address,undefined) and the -O3 single-thread host baseline of tools/bench_yolox.py.
//
//     g++ -O3 -std=c++17 -ffp-contract=off tools/yolox_walk.cpp -o yolox_walk
//
// Commands on stdin, one per line; floats travel as 8 hex digits, bytes as 2:
//     exp <kind> <n> <x ...>                    kind 0 yolox_exp_f32, 1 this machine's expf, 2 (float)exp((double)x): prints the n results
//     sample <seed> <n>                         n floats uniform in [-20, 20) from a 64-bit LCG: prints how many times yolox_exp_f32 differs from
//                                               (float)exp((double)x) and from expf
//     geometry <cols> <rows> <S>                prints ok, r, unpad_w, unpad_h
//     pre <cols> <rows> <S> <rgb> <bytes ...>   StaticResize + BlobFromImage + grey of a tight BGR frame: prints the blob and the grey image
//     decode <S> <classes> <conf> <nms> <img_w> <img_h> <stable> <kind> <floats ...>
//                                               DecodeOutputs: prints n_proposals, n_tied, the sorted proposals and the objects
//     bench <reps>                              times the pre-processing of a 640 x 480 frame and the decode of a 640 head with about 300 proposals
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../eao_fusion_amd/csrc/yolox_internal.h"

using namespace eao::yolox;

static float unhex(const std::string& s) {
    const uint32_t b = (uint32_t)std::stoul(s, nullptr, 16);
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
struct MachineExp { float operator()(float v) const { return std::exp(v); } };                 // expf, as the reference's unqualified call resolves
struct DoubleExp { float operator()(float v) const { return (float)std::exp((double)v); } };
static float exp_kind(int kind, float x) { return kind == 0 ? yolox_exp_f32(x) : (kind == 1 ? MachineExp{}(x) : DoubleExp{}(x)); }

static void print_objects(const char* tag, const std::vector<Object>& v) {
    std::printf("%s %zu\n", tag, v.size());
    for (const Object& o : v) std::printf("%08x %08x %08x %08x %08x %d\n", bits(o.x), bits(o.y), bits(o.w), bits(o.h), bits(o.prob), o.label);
}

template <typename Exp>
static void run_decode(const std::vector<float>& feat, int S, int nc, float conf, float nms, int imgW, int imgH, bool stable, Exp ex) {
    Geometry g;
    if (!geometry(imgW, imgH, S, &g)) { std::printf("refused\n"); return; }
    std::vector<Object> objects, proposals;
    decode_literal(feat.data(), S, nc, conf, nms, g.r, imgW, imgH, stable, ex, objects, &proposals);
    std::printf("n_proposals %zu\nn_tied %d\n", proposals.size(), count_tied(proposals));
    print_objects("proposals", proposals);
    print_objects("objects", objects);
}

static void bench(int reps) {
    const int cols = 640, rows = 480, S = 640;
    std::vector<uint8_t> img((size_t)cols * rows * 3), gray((size_t)cols * rows);
    uint64_t st = 12345;
    for (uint8_t& p : img) { st = st * 6364136223846793005ull + 1442695040888963407ull; p = (uint8_t)(st >> 56); }
    std::vector<float> blob((size_t)3 * S * S);
    const int A = num_anchors(S), row = 5 + kNumClasses;
    std::vector<float> feat((size_t)A * row, 0.f);
    for (int a = 0; a < A; a += 28) {      // 300 anchors, one class each above the threshold; few overlap, so nearly all are compared with all and survive
        float* f = feat.data() + (size_t)a * row;
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        f[0] = 0.5f; f[1] = 0.5f; f[2] = 1.0f + (float)((st >> 40) & 255) / 256.f; f[3] = 1.5f; f[4] = 0.9f;
        f[5 + (a % kNumClasses)] = 0.4f + (float)((st >> 20) & 1023) / 2048.f;
    }
    auto now = [] { return std::chrono::steady_clock::now(); };
    double preMs = 1e30, decMs = 1e30;
    size_t nObj = 0, nProp = 0;
    for (int r = 0; r < reps; r++) {
        auto t0 = now();
        preprocess_literal(img.data(), cols, rows, 3 * cols, S, false, blob.data(), gray.data(), cols);
        auto t1 = now();
        std::vector<Object> objects, proposals;
        decode_literal(feat.data(), S, kNumClasses, kConfThresh, kNmsThresh, 1.0f, cols, rows, false, OurExp{}, objects, &proposals);
        auto t2 = now();
        preMs = std::min(preMs, std::chrono::duration<double, std::milli>(t1 - t0).count());
        decMs = std::min(decMs, std::chrono::duration<double, std::milli>(t2 - t1).count());
        nObj = objects.size(); nProp = proposals.size();
    }
    std::printf("host_pre_ms %.4f\nhost_decode_ms %.4f\nproposals %zu\nobjects %zu\nblob0 %08x\n", preMs, decMs, nProp, nObj, bits(blob[0]));
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        if (!(in >> cmd)) continue;
        if (cmd == "exp") {
            int kind; size_t n;
            in >> kind >> n;
            for (size_t i = 0; i < n; i++) { in >> tok; std::printf("%08x%c", bits(exp_kind(kind, unhex(tok))), i + 1 == n ? '\n' : ' '); }
            if (n == 0) std::printf("\n");
        } else if (cmd == "sample") {
            uint64_t st; long n;
            in >> st >> n;
            long dDouble = 0, dMachine = 0;
            for (long i = 0; i < n; i++) {
                st = st * 6364136223846793005ull + 1442695040888963407ull;
                const float x = (float)((double)(st >> 11) / 9007199254740992.0 * 40.0 - 20.0);
                const uint32_t ours = bits(yolox_exp_f32(x));
                dDouble += ours != bits(DoubleExp{}(x));
                dMachine += ours != bits(MachineExp{}(x));
            }
            std::printf("differs_from_double %ld\ndiffers_from_expf %ld\n", dDouble, dMachine);
        } else if (cmd == "geometry") {
            int cols, rows, S;
            in >> cols >> rows >> S;
            Geometry g{};
            const bool ok = geometry(cols, rows, S, &g);
            std::printf("%d %08x %d %d\n", ok ? 1 : 0, bits(g.r), g.unpadW, g.unpadH);
        } else if (cmd == "pre") {
            int cols, rows, S, rgb;
            in >> cols >> rows >> S >> rgb;
            std::vector<uint8_t> img((size_t)cols * rows * 3), gray((size_t)cols * rows);
            for (uint8_t& p : img) { in >> tok; p = (uint8_t)std::stoul(tok, nullptr, 16); }
            std::vector<float> blob((size_t)3 * S * S);
            if (!preprocess_literal(img.data(), cols, rows, 3 * cols, S, rgb != 0, blob.data(), gray.data(), cols)) { std::printf("refused\n"); continue; }
            for (size_t i = 0; i < blob.size(); i++) std::printf("%08x%c", bits(blob[i]), i + 1 == blob.size() ? '\n' : ' ');
            for (size_t i = 0; i < gray.size(); i++) std::printf("%02x%c", gray[i], i + 1 == gray.size() ? '\n' : ' ');
        } else if (cmd == "decode") {
            int S, nc, imgW, imgH, stable, kind;
            std::string conf, nms;
            in >> S >> nc >> conf >> nms >> imgW >> imgH >> stable >> kind;
            std::vector<float> feat((size_t)num_anchors(S) * (5 + nc));
            for (float& f : feat) { in >> tok; f = unhex(tok); }
            if (kind == 0) run_decode(feat, S, nc, unhex(conf), unhex(nms), imgW, imgH, stable != 0, OurExp{});
            else if (kind == 1) run_decode(feat, S, nc, unhex(conf), unhex(nms), imgW, imgH, stable != 0, MachineExp{});
            else run_decode(feat, S, nc, unhex(conf), unhex(nms), imgW, imgH, stable != 0, DoubleExp{});
        } else if (cmd == "bench") {
            int reps;
            in >> reps;
            bench(reps);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
