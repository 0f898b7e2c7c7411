// yolox_exp_census.cpp -- yolox_exp_f32 (eao_fusion_amd/csrc/yolox_internal.h) over EVERY float32 in [-20, 20]: where it differs from (float)exp((double)x) -- the
// double-rounding cases of this machine's libm and of ours -- and how often it differs from this machine's expf, the call the reference makes (src/YOLOX.cc:183-184).
// Neither count is a pass mark: both are facts, recorded in profiles/yolox_exp_census.txt.
//
//     g++ -O2 -std=c++17 -ffp-contract=off -pthread tools/yolox_exp_census.cpp -o yolox_exp_census && ./yolox_exp_census [threads] > profiles/yolox_exp_census.txt
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../eao_fusion_amd/csrc/yolox_internal.h"

static float of_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t bits_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

struct Part { uint64_t n = 0, vsDouble = 0, vsExpf = 0; std::vector<uint32_t> where; };

int main(int argc, char** argv) {
    const int T = argc > 1 ? std::atoi(argv[1]) : 8;
    const uint32_t top = bits_of(20.0f);      // magnitudes 0 .. top, both signs
    std::vector<Part> parts((size_t)T);
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++)
        pool.emplace_back([&, t] {
            Part& P = parts[(size_t)t];
            for (uint64_t m = (uint64_t)t; m <= top; m += (uint64_t)T)
                for (uint32_t sign = 0; sign < 2; sign++) {
                    const uint32_t b = (uint32_t)m | (sign << 31);
                    const float x = of_bits(b);
                    const uint32_t ours = bits_of(eao::yolox::yolox_exp_f32(x));
                    P.n++;
                    if (ours != bits_of((float)std::exp((double)x))) { P.vsDouble++; P.where.push_back(b); }
                    if (ours != bits_of(std::exp(x))) P.vsExpf++;
                }
        });
    for (std::thread& th : pool) th.join();
    Part all;
    for (const Part& P : parts) { all.n += P.n; all.vsDouble += P.vsDouble; all.vsExpf += P.vsExpf; all.where.insert(all.where.end(), P.where.begin(), P.where.end()); }
    std::sort(all.where.begin(), all.where.end());
    std::printf("yolox_exp_f32 over every float32 in [-20, 20] (both zeros included): %llu inputs\n", (unsigned long long)all.n);
    std::printf("differs from (float)exp((double)x): %llu\n", (unsigned long long)all.vsDouble);
    std::printf("differs from this machine's expf:   %llu (%.4f %%)\n", (unsigned long long)all.vsExpf, 100.0 * (double)all.vsExpf / (double)all.n);
    std::printf("inputs of the first kind (bit pattern, value, ours, libm's double exp rounded):\n");
    for (uint32_t b : all.where) {
        const float x = of_bits(b);
        std::printf("  %08x %.9g %08x %08x\n", b, (double)x, bits_of(eao::yolox::yolox_exp_f32(x)), bits_of((float)std::exp((double)x)));
    }
    return 0;
}
