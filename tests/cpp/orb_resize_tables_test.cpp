// orb_resize_tables_test.cpp -- the operand tables of the matrix-core pyramid resize (eao_fusion_amd/csrc/orb_resize_tables.h) without a GPU: the kernel's tile
// products are replayed in integer arithmetic, operand fragment by operand fragment, and held byte for byte to the direct formula, every pixel of every level.
// The replay models the instruction as k_resize_mfma uses it: D[m][n] = C[m][n] + sum over slots (half, j) of A[lane m + 32 half][j] * B[lane n + 32 half][j],
// result register q of lane (n, half) <-> m = (q & 3) + 8 (q >> 2) + 4 half; A = weight fragments (m = output column of the strip), B = pixel fragments
// (n = output row of the tile, 16 bytes of its source row sy0 / sy1).  Asserted on the way: every non-zero weight pair lies inside its strip's window, every
// weight piece fits int8, no window ends beyond what the source may be read, the column offsets are 128 (a0 + a1), a block's source rows fit kResizeMRows.
// Built and run under AddressSanitizer by tests/test_orb_resize_tables_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../eao_fusion_amd/csrc/orb_resize_tables.h"

using namespace eao::orb;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Image { int w, h, pitch; std::vector<uint8_t> px; };      // pitch = exactly what may be read: a load beyond it leaves the vector on the last row

// the formula as the issue states it (tests/test_oracle_orb.py::_resize_numpy restates it too), coefficient by coefficient from the float / double expressions
static void coef(int d, int dn, int sn, int* o, float* f) {
    const double scale = 1.0 / ((double)dn / sn);
    float fr = (float)(((double)d + 0.5) * scale - 0.5);
    *o = (int)std::floor(fr);
    *f = fr - (float)*o;
}
static std::vector<uint8_t> direct_resize(const Image& S, int dw, int dh) {
    std::vector<uint8_t> out((size_t)dw * dh);
    for (int y = 0; y < dh; y++) {
        int iy; float fy;
        coef(y, dh, S.h, &iy, &fy);
        const long long b0 = std::lrintf((1.f - fy) * 2048.f), b1 = std::lrintf(fy * 2048.f);
        const int y0 = std::min(std::max(iy, 0), S.h - 1), y1 = std::min(std::max(iy + 1, 0), S.h - 1);
        for (int x = 0; x < dw; x++) {
            int ix; float fx;
            coef(x, dw, S.w, &ix, &fx);
            if (ix < 0) { fx = 0; ix = 0; }
            if (ix >= S.w - 1) { fx = 0; ix = S.w - 1; }
            const long long a0 = std::lrintf((1.f - fx) * 2048.f), a1 = std::lrintf(fx * 2048.f);
            CHECK(a0 >= 0 && a1 >= 0 && a0 + a1 == 2048 && b0 >= 0 && b1 >= 0 && b0 + b1 == 2048, "weights (%lld %lld) (%lld %lld)", a0, a1, b0, b1);
            const int ix1 = std::min(ix + 1, S.w - 1);
            const long long H0 = S.px[(size_t)y0 * S.pitch + ix] * a0 + S.px[(size_t)y0 * S.pitch + ix1] * a1;
            const long long H1 = S.px[(size_t)y1 * S.pitch + ix] * a0 + S.px[(size_t)y1 * S.pitch + ix1] * a1;
            const long long v = (((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2;
            out[(size_t)y * dw + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
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
static Frag table_frag(const ResizeMTables& T, size_t off) {
    Frag F;
    for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 16; j++) {
            const uint8_t v = T.strips.at(off + lane * 16 + j);
            CHECK(v <= 127, "weight piece %d", (int)v);
            F.b[lane][j] = (int8_t)v;
        }
    return F;
}

// the strip's table against the coefficients: window, pieces, offsets
static void check_strip(const ResizeMTables& T, int ws, int off, int cx, int dw, const ResizeMLevelIn& S, double invX) {
    CHECK(ws >= 0 && (ws & 3) == 0 && ws + kResizeMWin <= S.readable, "window %d .. %d, readable %d", ws, ws + kResizeMWin, S.readable);
    CHECK(off % kResizeMStrip == 0 && (size_t)off + kResizeMStrip <= T.strips.size(), "strip table offset %d", off);
    for (int c = 0; c < kResizeMTile; c++) {
        int want[kResizeMWin] = {}, sum = 0;
        const int x = kResizeMTile * cx + c;
        if (x < dw) {
            int o; unsigned wp;
            resize_coef_host(x, invX, S.w, true, &o, &wp);
            const int a[2] = {(short)(wp & 0xFFFF), (short)(wp >> 16)}, col[2] = {o, std::min(o + 1, S.w - 1)};
            for (int t = 0; t < 2; t++) {
                if (!a[t]) continue;
                CHECK(col[t] >= ws && col[t] < ws + kResizeMWin && col[t] < S.w, "strip %d column %d: source %d outside the window at %d", cx, c, col[t], ws);
                if (col[t] >= ws && col[t] < ws + kResizeMWin) want[col[t] - ws] += a[t];
                sum += a[t];
            }
        }
        int32_t coff;
        std::memcpy(&coff, &T.strips.at((size_t)off + 4 * kResizeMFrag + 4 * c), 4);
        CHECK(coff == 128 * sum, "strip %d column %d: offset %d, 128 (a0 + a1) = %d", cx, c, coff, 128 * sum);
        for (int k = 0; k < kResizeMWin; k++) {
            const size_t slot = (size_t)(c + 32 * ((k >> 4) & 1)) * 16 + (k & 15);
            const int c1 = T.strips.at((size_t)off + (k >> 5) * kResizeMFrag + slot), c0 = T.strips.at((size_t)off + (2 + (k >> 5)) * kResizeMFrag + slot);
            CHECK(c1 <= 127 && c0 <= 127 && 64 * c1 + c0 == want[k], "strip %d column %d slot %d: pieces (%d, %d), weight %d", cx, c, k, c1, c0, want[k]);
        }
    }
}

static Image make_image(int w, int h, int readable, int kind, unsigned seed) {
    Image I{w, h, readable, std::vector<uint8_t>((size_t)readable * h)};
    unsigned st = seed * 2654435761u + 12345u;
    auto rnd = [&] { st = st * 1664525u + 1013904223u; return st >> 8; };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < readable; x++) {
            uint8_t v;
            if (kind == 0) v = (uint8_t)rnd();
            else if (kind == 1) v = 0;
            else if (kind == 2) v = 255;
            else if (kind == 3) v = ((x + y) & 1) ? 255 : 0;
            else if (kind == 4) v = (rnd() & 1) ? 255 : 0;
            else v = (x & 1) ? 255 : 0;      // vertical stripes: the largest column excursions
            if (x >= w) v = (uint8_t)rnd();      // padding: arbitrary bytes, zero weights
            I.px[(size_t)y * readable + x] = v;
        }
    return I;
}

// one level from its source as k_resize_mfma computes it, held to the direct formula
static void replay_level(const ResizeMTables& T, const ResizeMLevel& M, const ResizeMLevelIn& D, const ResizeMLevelIn& Sin, const Image& S, const char* what) {
    const std::vector<uint8_t> want = direct_resize(S, D.w, D.h);
    const double invX = 1. / ((double)D.w / Sin.w);
    CHECK(M.tilesX == (D.w + 31) / 32 && M.blocksY == (D.h + 31) / 32, "tiling");
    CHECK(M.maxSpan <= kResizeMRows, "rows of a block: %d", M.maxSpan);
    for (int cx = 0; cx < M.tilesX; cx++) {
        const int ws = T.idx.at(2 * (M.xIdx + cx)), off = T.idx.at(2 * (M.xIdx + cx) + 1);
        check_strip(T, ws, off, cx, D.w, Sin, invX);
        const Frag t1[2] = {table_frag(T, off), table_frag(T, (size_t)off + kResizeMFrag)};
        const Frag t0[2] = {table_frag(T, (size_t)off + 2 * kResizeMFrag), table_frag(T, (size_t)off + 3 * kResizeMFrag)};
        for (int b = 0; b < M.blocksY; b++) {
            const ResizeMRow* rt = &T.rows.at((size_t)M.rowOff + kResizeMTile * b);
            const int base = rt[0].sy0, end = rt[31].sy1, n = (end - base + 16) >> 4;
            CHECK(n >= 1 && 16 * n <= kResizeMRows, "block %d reads %d rows", b, end - base + 1);
            // the wave's LDS image: rows base .. base + 16 n - 1 (clamped to the last row), 64 bytes of each from the window start, ^ 0x80
            std::vector<uint8_t> stage((size_t)16 * n * kResizeMWin);
            for (int r = 0; r < 16 * n; r++)
                for (int k = 0; k < kResizeMWin; k++) stage[(size_t)r * kResizeMWin + k] = S.px.at((size_t)std::min(base + r, S.h - 1) * S.pitch + ws + k) ^ 0x80;
            Acc h[2], l[2];
            for (int t = 0; t < 2; t++) {
                for (int lane = 0; lane < 64; lane++)
                    for (int q = 0; q < 16; q++) {
                        h[t].r[lane][q] = 0;
                        std::memcpy(&l[t].r[lane][q], &T.strips.at((size_t)off + 4 * kResizeMFrag + 4 * ((q & 3) + 8 * (q >> 2) + 4 * (lane >> 5))), 4);
                    }
                for (int s = 0; s < 2; s++) {
                    Frag P;
                    for (int lane = 0; lane < 64; lane++) {
                        const int sy = t ? rt[lane & 31].sy1 : rt[lane & 31].sy0;
                        CHECK(sy >= base && sy <= end && sy < S.h, "row %d outside the block's rows %d .. %d", sy, base, end);
                        for (int j = 0; j < 16; j++) P.b[lane][j] = (int8_t)stage.at((size_t)(sy - base) * kResizeMWin + 32 * s + 16 * (lane >> 5) + j);
                    }
                    mfma(t1[s], P, h[t]);
                    mfma(t0[s], P, l[t]);
                }
            }
            for (int lane = 0; lane < 64; lane++) {
                const int y = kResizeMTile * b + (lane & 31);
                const ResizeMRow& R = rt[lane & 31];
                CHECK(R.b0 >= 0 && R.b1 >= 0 && R.b0 + R.b1 == 2048, "row weights %d %d", R.b0, R.b1);
                const uint32_t B0 = (uint32_t)R.b0 << 16, B1 = (uint32_t)R.b1 << 16;
                for (int q = 0; q < 16; q++) {
                    const int x = kResizeMTile * cx + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                    const uint32_t H0 = ((uint32_t)h[0].r[lane][q] << 6) + (uint32_t)l[0].r[lane][q], H1 = ((uint32_t)h[1].r[lane][q] << 6) + (uint32_t)l[1].r[lane][q];
                    const uint32_t m0 = (uint32_t)(((uint64_t)B0 * (H0 >> 4)) >> 32), m1 = (uint32_t)(((uint64_t)B1 * (H1 >> 4)) >> 32);
                    const uint32_t v = (m0 + m1 + 2) >> 2;
                    CHECK(v <= 255, "%s: value %u leaves a byte", what, v);      // (the kernel packs without a clamp)
                    if (x >= D.w) { CHECK(v == 0, "%s: column %d beyond the width gives %u", what, x, v); continue; }
                    if (y >= D.h) continue;
                    CHECK(v == want[(size_t)y * D.w + x], "%s at (%d, %d): %u, direct formula %u", what, x, y, v, (unsigned)want[(size_t)y * D.w + x]);
                }
            }
        }
    }
}

// level sizes as the extractor computes them: cvRound(W * (float)(1 / factor^l)) in float
static std::vector<ResizeMLevelIn> pyramid(int W, int H, float factor, int nlevels) {
    std::vector<ResizeMLevelIn> in;
    float scale = 1.f;
    for (int l = 0; l < nlevels; l++) {
        if (l) scale *= factor;
        const float inv = 1.0f / scale;
        const int w = (int)std::lrint((float)W * inv), h = (int)std::lrint((float)H * inv);
        in.push_back({w, h, l == 0 ? (w + 3) & ~3 : (w + 63) & ~63});
    }
    return in;
}

static void run_geometry(int W, int H, float factor, int nlevels, unsigned* seed) {
    const std::vector<ResizeMLevelIn> in = pyramid(W, H, factor, nlevels);
    const ResizeMTables T = resize_m_build(in);
    CHECK((int)T.level.size() == nlevels && !T.level[0].ok, "levels");
    CHECK(T.maxPiece <= 127, "piece %d", T.maxPiece);
    CHECK(T.strips.size() % kResizeMStrip == 0, "table size");
    char what[128];
    for (int l = 1; l < nlevels; l++) {
        CHECK(T.level[l].ok, "%dx%d at %.2f: level %d (%dx%d) refused", W, H, factor, l, in[l].w, in[l].h);
        if (!T.level[l].ok) continue;
        for (int kind = 0; kind < 6; kind++) {
            if (W > 320 && (kind == 1 || kind == 3 || kind == 4)) continue;      // (the large frames: random, all-255 and stripes)
            std::snprintf(what, sizeof what, "%dx%d at %.2f level %d kind %d", W, H, factor, l, kind);
            replay_level(T, T.level[l], in[l], in[l - 1], make_image(in[l - 1].w, in[l - 1].h, in[l - 1].readable, kind, (*seed)++), what);
        }
    }
}

int main() {
    unsigned seed = 1;
    const int frames[][2] = {{640, 480}, {320, 240}, {752, 480}, {1241, 376}, {96, 76}};
    for (const auto& f : frames) run_geometry(f[0], f[1], 1.2f, 8, &seed);
    run_geometry(640, 480, 1.1f, 8, &seed);
    run_geometry(640, 480, 1.5f, 6, &seed);
    run_geometry(640, 480, 2.0f, 4, &seed);
    // refused: at factor 2.5 the sources of 32 output pixels span 80 bytes, more than the window; a source narrower than the window; the levels beside them stand
    {
        const ResizeMTables T = resize_m_build(pyramid(640, 480, 2.5f, 3));
        CHECK(!T.level[1].ok && !T.level[2].ok && T.idx.empty() && T.rows.empty() && T.strips.empty(), "factor 2.5 is not refused");
        const ResizeMTables U = resize_m_build({{60, 50, 60}, {50, 42, 64}, {42, 35, 64}});
        CHECK(!U.level[1].ok && U.level[2].ok, "a 60-byte source row holds no 64-byte window: %d %d", U.level[1].ok, U.level[2].ok);
    }
    // identical strip tables are stored once: at factor 2 every strip of a level has the same phase (one table per level), and a level built twice adds nothing
    {
        const std::vector<ResizeMLevelIn> in = pyramid(640, 480, 2.0f, 2);
        const ResizeMTables A = resize_m_build(in);
        CHECK(A.level[1].ok && A.level[1].tilesX == 10 && A.strips.size() == (size_t)kResizeMStrip, "640 -> 320: %zu bytes of tables", A.strips.size());
        const ResizeMTables B = resize_m_build({in[0], in[1], in[0], in[1]});      // (level 2 = 640 x 480 from 320 x 240 has tables of its own; level 3 repeats level 1)
        CHECK(B.level[3].ok && B.idx[2 * B.level[3].xIdx + 1] == B.idx[2 * B.level[1].xIdx + 1], "a repeated level has a second copy of its tables");
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("all as the direct formula\n");
    return 0;
}
