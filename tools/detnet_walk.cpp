// detnet_walk.cpp -- the host header of the detector network (eao_fusion_amd/csrc/detnet_internal.h) as a program of its own: the sanitizer target of
// tests/test_detnet_host_cpu.py (g++ -fsanitize=address,undefined), the yardstick of the device tests (-O2) and the -O3 single-thread host baseline of
// tools/bench_detnet.py.
//
//     g++ -O3 -std=c++17 -ffp-contract=off tools/detnet_walk.cpp -o detnet_walk
//
//     detnet_walk fma <in> <out>                        <in>: n triples of float32 (x, w, acc); <out>: the n results of std::fmaf(x, w, acc)
//     detnet_walk check <model> <S>                     prints "ok" and the tensor table, or "refused: <why>"; exit status 0 either way
//     detnet_walk run <model> <S> <blob> <out> [<act>]  one frame: <blob> holds 3 x S x S floats ("-" for zeros), <act> the activation block to start from (the
//                                                       caller's input tensors); writes <out>.act (the activation block) and <out>.prob (the head)
//     detnet_walk bench <model> <S> <reps>              times the forward pass of one frame on one thread: prints the median in ms
//     detnet_walk forms <model> <S> <batch>             one line per op: its kind, M (the output pixels over the batch), Cout, k, stride, residual tensor, channel
//                                                       offsets and, for a convolution, the tile form conv_form() gives the device at this batch
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../eao_fusion_amd/csrc/detnet_internal.h"

using namespace eao::detnet;

static bool read_file(const char* path, std::vector<char>& out) {
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in.good()) return false;
    const std::streamoff n = in.tellg();
    out.resize((size_t)n);
    in.seekg(0);
    if (n) in.read(out.data(), n);
    return in.good();
}
static bool write_floats(const std::string& path, const std::vector<float>& v) {
    std::ofstream out(path, std::ios::binary);
    if (!v.empty()) out.write((const char*)v.data(), (std::streamsize)(v.size() * 4));
    return out.good();
}

static bool load_model(const char* path, int S, std::vector<char>& file, Net& net) {
    if (!read_file(path, file)) { std::printf("refused: cannot read %s\n", path); return false; }
    std::string why;
    // (the vector holds the file's own bytes and no more: a read past them is the sanitizer's to find)
    if (!load(file.empty() ? (const void*)"" : (const void*)file.data(), file.size(), S, true, &net, &why)) { std::printf("refused: %s\n", why.c_str()); return false; }
    return true;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "fma" && argc == 4) {
        std::vector<char> in;
        if (!read_file(argv[2], in) || in.size() % 12) return 2;
        const size_t n = in.size() / 12;
        std::vector<float> t(3 * n), r(n);
        if (n) std::memcpy(t.data(), in.data(), in.size());
        for (size_t i = 0; i < n; i++) r[i] = std::fmaf(t[3 * i], t[3 * i + 1], t[3 * i + 2]);
        return write_floats(argv[3], r) ? 0 : 2;
    }
    if ((cmd == "check" && argc == 4) || (cmd == "run" && (argc == 6 || argc == 7)) || (cmd == "bench" && argc == 5)) {
        const int S = std::atoi(argv[3]);
        std::vector<char> file;
        Net net;
        if (!load_model(argv[2], S, file, net)) return 0;
        std::printf("ok classes %d anchors %d act %zu flops %.0f\n", net.classes, net.anchors, net.actFloats, net.flops);
        for (size_t t = 0; t < net.tensors.size(); t++)
            std::printf("tensor %zu kind %u offset %zu shape %d %d %d\n", t, net.tensors[t].kind, net.tensors[t].offset, net.tensors[t].H, net.tensors[t].W, net.tensors[t].C);
        if (cmd == "check") return 0;
        std::vector<float> blob((size_t)3 * S * S, 0.f), act(net.actFloats, 0.f), prob((size_t)net.anchors * net.row, 0.f);
        if (cmd == "run") {
            std::vector<char> b;
            if (std::string(argv[4]) != "-") {
                if (!read_file(argv[4], b) || b.size() != blob.size() * 4) { std::printf("error: the blob is not 3 x %d x %d floats\n", S, S); return 2; }
                std::memcpy(blob.data(), b.data(), b.size());
            }
            if (argc == 7) {
                if (!read_file(argv[6], b) || b.size() != act.size() * 4) { std::printf("error: the activation block is not %zu floats\n", act.size()); return 2; }
                if (!b.empty()) std::memcpy(act.data(), b.data(), b.size());
            }
            forward_host(net, blob.data(), act.data(), prob.data());
            return write_floats(std::string(argv[5]) + ".act", act) && write_floats(std::string(argv[5]) + ".prob", prob) ? 0 : 2;
        }
        uint64_t lcg = 88172645463325252ull;
        for (float& v : blob) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; v = (float)((double)(lcg >> 40) / 16777216.0 * 4.0 - 2.0); }
        const int reps = std::max(1, std::atoi(argv[4]));
        std::vector<double> ms;
        for (int i = 0; i < reps; i++) {
            const auto t0 = std::chrono::steady_clock::now();
            forward_host(net, blob.data(), act.data(), prob.data());
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        std::printf("host_walk_ms %.3f\n", ms[ms.size() / 2]);
        return 0;
    }
    if (cmd == "forms" && argc == 5) {
        const int S = std::atoi(argv[3]), batch = std::atoi(argv[4]);
        std::vector<char> file;
        Net net;
        if (batch < 1) { std::printf("refused: batch = %d\n", batch); return 0; }
        if (!load_model(argv[2], S, file, net)) return 0;
        std::printf("ok ops %zu\n", net.ops.size());
        static const char* const kinds[] = {"focus", "conv", "maxpool", "upsample2"};
        for (size_t i = 0; i < net.ops.size(); i++) {
            const OpRec& r = net.ops[i].r;
            const Tensor &Ts = net.tensors[r.src], &Td = net.tensors[r.dst];
            const bool head = Td.kind == HEAD;
            const long long M = (long long)batch * (head ? Ts.H : Td.H) * (head ? Ts.W : Td.W);
            std::printf("op %zu kind %s M %lld Cout %u k %u stride %u res %d src_c0 %u dst_c0 %u head %d", i, kinds[r.kind], M, r.dst_c, r.k, r.stride, r.res, r.src_c0,
                        r.dst_c0, head ? 1 : 0);
            if (r.kind == CONV) std::printf(" form %s", conv_form_name(conv_form(M, (int)r.dst_c)));
            std::printf("\n");
        }
        return 0;
    }
    std::fprintf(stderr, "usage: detnet_walk fma|check|run|bench|forms ... (see the head of tools/detnet_walk.cpp)\n");
    return 2;
}
