// orb_blur_tables_test.cpp -- the operand tables of the matrix-core blur (eao_fusion_amd/csrc/orb_blur_tables.h) without a GPU: the kernel's tile products are
// replayed in integer arithmetic, operand fragment by operand fragment, and held byte for byte to the direct 7 x 7 blur.  The replay models the instruction
// as the kernel uses it: D[m][n] = C[m][n] + sum over slots (half, j) of A[lane m + 32 half][j] * B[lane n + 32 half][j], result register q of lane
// (n, half) <-> m = (q & 3) + 8 (q >> 2) + 4 half.  Asserted on the way: every table entry <= 127, every table column sums to 257 or 0, every byte the
// replay loads lies inside what the level may read.  Built and run under AddressSanitizer by tests/test_orb_blur_tables_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../eao_fusion_amd/csrc/orb_blur_tables.h"

using namespace eao::orb;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static std::vector<uint8_t> direct_blur(const std::vector<uint8_t>& img, int w, int h, int pitch) {
    std::vector<uint8_t> out((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            long long acc = 0;
            for (int i = 0; i < 7; i++)
                for (int j = 0; j < 7; j++)
                    acc += (long long)kBlurTaps[i] * kBlurTaps[j] * img[(size_t)blur_reflect101(y - 3 + i, h) * pitch + blur_reflect101(x - 3 + j, w)];
            const long long v = (acc + 32768) >> 16;
            out[(size_t)y * w + x] = (uint8_t)(v > 255 ? 255 : v);
        }
    return out;
}

struct Frag { int8_t b[64][16]; };
struct Acc { int32_t r[64][16]; };
static void mfma(const Frag& A, const Frag& B, Acc& D) {
    for (int lane = 0; lane < 64; lane++)
        for (int q = 0; q < 16; q++) {
            const int n = lane & 31, m = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
            int32_t s = 0;
            for (int half = 0; half < 2; half++)
                for (int j = 0; j < 16; j++) s += (int32_t)A.b[m + 32 * half][j] * (int32_t)B.b[n + 32 * half][j];
            D.r[lane][q] += s;
        }
}
static Frag table_frag(const BlurMTables& T, int off) {
    Frag F;
    for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 16; j++) F.b[lane][j] = (int8_t)T.frag[(size_t)off + lane * 16 + j];
    return F;
}

struct Packed { Frag hi, lo; };
// stage 1 of source block blk of column strip window ws: what blur_m_load + blur_m_stage1 of the kernel do
static Packed stage1(const std::vector<uint8_t>& img, int h, int pitch, int readable, int blk, int ws, const Frag tx[2]) {
    Acc X;
    for (int lane = 0; lane < 64; lane++) for (int q = 0; q < 16; q++) X.r[lane][q] = 128;
    for (int s = 0; s < 2; s++) {
        Frag A;
        for (int lane = 0; lane < 64; lane++) {
            int y = kBlurMTile * blk + (lane & 31);
            y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
            for (int j = 0; j < 16; j++) {
                const int col = ws + 32 * s + 16 * (lane >> 5) + j;
                CHECK(col >= 0 && col < readable, "load of column %d, readable %d", col, readable);
                A.b[lane][j] = (int8_t)(img.at((size_t)y * pitch + col) ^ 0x80);
            }
        }
        mfma(A, tx[s], X);
    }
    Packed P;
    for (int lane = 0; lane < 64; lane++)
        for (int q = 0; q < 16; q++) {
            const int32_t v = X.r[lane][q];
            CHECK(v >= -32768 && v <= 32767, "stage 1 leaves int16: %d", v);
            P.hi.b[lane][q] = (int8_t)(uint8_t)((uint32_t)v >> 8);
            P.lo.b[lane][q] = (int8_t)(uint8_t)(((uint32_t)v & 255u) ^ 0x80u);
        }
    return P;
}

static void check_tables(const BlurMTables& T, const BlurMLevel& M) {
    // every column (one output: lanes n and n + 32 over all K steps) sums to 257 or 0
    for (int e = 0; e < M.tilesX + M.blocksY; e++) {
        const int off = T.idx[2 * (M.xIdx + e) + 1], steps = e < M.tilesX ? 2 : 3;
        for (int n = 0; n < 32; n++) {
            int sum = 0;
            for (int s = 0; s < steps; s++)
                for (int half = 0; half < 2; half++)
                    for (int j = 0; j < 16; j++) sum += T.frag[(size_t)off + s * kBlurMFrag + (n + 32 * half) * 16 + j];
            CHECK(sum == 257 || sum == 0, "column sum %d", sum);
        }
    }
}

static void run_level(int w, int h, int readable, int kind, unsigned seed) {
    const int pitch = readable;      // exactly what may be read: a load beyond it leaves the vector on the last row
    std::vector<uint8_t> img((size_t)pitch * h);
    unsigned st = seed * 2654435761u + 12345u;
    auto rnd = [&] { st = st * 1664525u + 1013904223u; return st >> 8; };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < pitch; x++) {
            uint8_t v;
            if (kind == 0) v = (uint8_t)rnd();
            else if (kind == 1) v = 0;
            else if (kind == 2) v = 255;
            else if (kind == 3) v = ((x + y) & 1) ? 255 : 0;
            else v = (rnd() & 1) ? 255 : 0;
            if (x >= w) v = (uint8_t)rnd();      // padding: arbitrary bytes, zero weights
            img[(size_t)y * pitch + x] = v;
        }
    const BlurMTables T = blur_m_build({{w, h, readable}});
    const BlurMLevel& M = T.level[0];
    CHECK(M.ok, "level %dx%d (readable %d) refused", w, h, readable);
    if (!M.ok) return;
    CHECK(T.maxEntry <= 127, "table entry %d", T.maxEntry);
    CHECK(T.frag.size() % kBlurMFrag == 0, "table size");
    check_tables(T, M);
    const std::vector<uint8_t> want = direct_blur(img, w, h, pitch);
    for (int cx = 0; cx < M.tilesX; cx++) {
        const int ws = T.idx[2 * (M.xIdx + cx)], xoff = T.idx[2 * (M.xIdx + cx) + 1];
        CHECK(ws == blur_m_window_start(cx, readable) && ws + kBlurMWin <= readable, "window start %d", ws);
        const Frag tx[2] = {table_frag(T, xoff), table_frag(T, xoff + kBlurMFrag)};
        std::vector<Packed> P(M.blocksY + 2);      // P[b + 1]: source block b; block -1 does not exist (zero operand), block blocksY repeats the last row
        for (int b = 0; b <= M.blocksY; b++) P[b + 1] = stage1(img, h, pitch, readable, b, ws, tx);
        for (int lane = 0; lane < 64; lane++) for (int j = 0; j < 16; j++) P[0].hi.b[lane][j] = P[0].lo.b[lane][j] = 0;
        for (int b = 0; b < M.blocksY; b++) {
            const int yoff = T.idx[2 * (M.yIdx + b) + 1];
            Acc ah, al;
            for (int lane = 0; lane < 64; lane++) for (int q = 0; q < 16; q++) { ah.r[lane][q] = 0; al.r[lane][q] = 257 * (32768 + 128) + 32768; }
            for (int s = 0; s < 3; s++) {
                const Frag ty = table_frag(T, yoff + s * kBlurMFrag);
                mfma(P[b + s].hi, ty, ah);
                mfma(P[b + s].lo, ty, al);
            }
            for (int lane = 0; lane < 64; lane++) {
                const int y = kBlurMTile * b + (lane & 31);
                if (y >= h) continue;
                for (int q = 0; q < 16; q++) {
                    const int x = kBlurMTile * cx + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                    if (x >= w) continue;
                    const uint32_t v = ((uint32_t)ah.r[lane][q] << 8) + (uint32_t)al.r[lane][q];
                    const uint32_t o = (v >> 16) > 255 ? 255 : (v >> 16);
                    CHECK(o == want[(size_t)y * w + x], "%dx%d kind %d at (%d, %d): %u, direct blur %u", w, h, kind, x, y, o, (unsigned)want[(size_t)y * w + x]);
                }
            }
        }
    }
}

int main() {
    // the eight levels of a 320 x 240 frame at scale 1.2, the smallest sizes the path accepts, a remainder of one column and of one row, a wide level
    const int sizes[][2] = {{320, 240}, {267, 200}, {222, 167}, {185, 139}, {154, 116}, {129, 96}, {107, 80}, {89, 67}, {64, 64}, {70, 70}, {65, 97}, {161, 65}, {640, 64}};
    unsigned seed = 1;
    for (const auto& s : sizes)
        for (int kind = 0; kind < 5; kind++) {
            run_level(s[0], s[1], (s[0] + 3) & ~3, kind, seed++);        // level 0: rows readable up to the next multiple of 4
            run_level(s[0], s[1], (s[0] + 63) & ~63, kind, seed++);      // pyramid level: up to the pitch
        }
    // refused: narrower or lower than the source window
    {
        const BlurMTables T = blur_m_build({{63, 100, 64}, {100, 63, 128}, {72, 60, 72}, {320, 240, 320}});
        CHECK(!T.level[0].ok && !T.level[1].ok && !T.level[2].ok && T.level[3].ok, "which levels take the matrix path");
    }
    // one table set for a whole pyramid: identical tables are stored once, the index stays per level
    {
        std::vector<BlurMLevelIn> in;
        for (const auto& s : sizes) in.push_back({s[0], s[1], (s[0] + 63) & ~63});
        const BlurMTables T = blur_m_build(in);
        size_t alone = 0;
        for (const BlurMLevelIn& L : in) alone += blur_m_build({L}).frag.size();
        CHECK(T.frag.size() < alone, "tables are not shared between levels: %zu vs %zu", T.frag.size(), alone);
        for (size_t l = 0; l < in.size(); l++) {
            CHECK(T.level[l].ok, "level %zu refused", l);
            check_tables(T, T.level[l]);
        }
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all as the direct blur\n");
    return 0;
}
