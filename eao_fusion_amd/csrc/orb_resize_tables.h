// orb_resize_tables.h -- the operand tables of the matrix-core pyramid resize (k_resize_mfma in orb_resize_mfma.hip) and its tiling, built once per geometry on
// the host.  Plain C++17, no HIP: tests/cpp/orb_resize_tables_test.cpp replays the kernel's tile products from these tables in integer arithmetic against the
// direct formula under AddressSanitizer on a machine without a GPU.
//
// Level l from level l - 1 (OpenCV's 11-bit fixed-point bilinear resize, the arithmetic of resize_coef / resize_item in orb.hip):
//   H[y][x] = S[y][sx] a0 + S[y][min(sx + 1, sw - 1)] a1                                  a banded linear map along x: an exact integer matrix product
//   out     = ((b0 (H[sy0] >> 4)) >> 16 + (b1 (H[sy1] >> 4)) >> 16 + 2) >> 2              two truncations per source row: stays on the VALU, in-lane
// A tile is 32 x 32 outputs, computed as H^T = Tx^T . S^T over a 64-byte source window (two K steps of v_mfma_i32_32x32x32_i8), once for the rows sy0(y) and
// once for the rows sy1(y): the weights are the FIRST operand (lane = output column c of the strip), the pixels the second (lane = output row y, 16 consecutive
// bytes of ITS source row per K step), so a lane ends with sixteen output columns of one output row: register r <-> c = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
// Pixels enter as P - 128 (int8), a weight c <= 2048 as c = 64 c1 + c0 with both pieces in 0 .. 127 -- two products, H = 64 acc1 + acc0 -- and the term
// 128 (a0 + a1) of every output column sits in the C input of the acc0 chain; the sum comes from the table (0 for the columns beyond the level's width).
// A strip's table is 4 operand fragments (c1 of K step 0, 1; c0 of K step 0, 1: lane (c, half), byte j <-> source column window start + 32 s + 16 half + j, 1 KiB each)
// followed by its 32 column offsets.  Identical strip tables are stored once.  Per output row the row table holds (sy0, sy1, b0, b1), rows clamped as the load
// clamps them and weights kept; it is padded to whole 32-row blocks with copies of the last row (those lanes compute, and store nothing).
// The builder refuses a level (ok = 0, the level keeps k_resize) when a strip's non-zero weights do not fit one window that may be loaded, when a block's
// source rows exceed kResizeMRows, or when a weight is negative or its pieces leave int8.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace eao {
namespace orb {

constexpr int kResizeMTile = 32;       // outputs per tile edge
constexpr int kResizeMWin = 64;        // source window of a column strip, bytes per row
constexpr int kResizeMSeg = 4;         // tiles a wave walks down its column strip, at most
constexpr int kResizeMFrag = 1024;     // bytes of one operand fragment
constexpr int kResizeMRows = 80;       // source rows of a 32-row output block, at most (scale factor 2: 65)
constexpr int kResizeMStrip = 4 * kResizeMFrag + 4 * kResizeMTile;      // bytes of a strip's table: four fragments + 32 column offsets

// the bilinear coefficients of destination index d, as OpenCV 3.3.x evaluates them on the host: (float)((d + 0.5) * inv_scale - 0.5), floor, cvRound(w * 2048)
// (lrintf rounds to nearest even like v_cvt_i32_f32; the kernels' resize_coef is the same expression on the device)
inline void resize_coef_host(int d, double inv, int slimit, bool clampHi, int* ofs, unsigned* wpair) {
    float fr = (float)(((double)d + 0.5) * inv - 0.5);
    int o = (int)std::floor(fr);
    fr -= (float)o;
    if (clampHi) {
        if (o < 0) { fr = 0; o = 0; }
        if (o >= slimit - 1) { fr = 0; o = slimit - 1; }
    }
    const int w0 = std::min(std::max((int)std::lrintf((1.f - fr) * 2048.f), -32768), 32767);
    const int w1 = std::min(std::max((int)std::lrintf(fr * 2048.f), -32768), 32767);
    *ofs = o;
    *wpair = ((unsigned)w0 & 0xFFFFu) | ((unsigned)w1 << 16);
}

struct ResizeMLevelIn { int w, h, readable; };      // readable: bytes of every row that may be loaded when the level is a SOURCE (>= w, a multiple of 4)
struct ResizeMLevel {
    int ok;                 // the level is produced on the matrix cores
    int tilesX, blocksY;    // column strips, 32-row blocks
    int xIdx;               // first (window start, strip table offset) pair of the level in ResizeMTables::idx
    int rowOff;             // first row record of the level in ResizeMTables::rows (32 * blocksY records)
    int maxSpan;            // most source rows any block reads
};
struct ResizeMRow { int sy0, sy1, b0, b1; };
struct ResizeMTables {
    std::vector<ResizeMLevel> level;      // level[0] is the input image: never produced, ok = 0
    std::vector<int> idx;                 // pairs of ints, see ResizeMLevel
    std::vector<ResizeMRow> rows;
    std::vector<uint8_t> strips;          // the strip tables, kResizeMStrip bytes each
    int maxPiece = 0;                     // largest weight piece of any table
};

// the fewest walks of at most kResizeMSeg tiles down a column strip, of equal length (the last one may be shorter): the strip's table is loaded once per walk
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int resize_m_walks(int blocksY, int* len) {
    const int n = (blocksY + kResizeMSeg - 1) / kResizeMSeg;
    *len = (blocksY + n - 1) / n;
    return n;
}

// the table of column strip cx of a level of width dw from a source of width sw; false: the strip's weights do not fit a window
inline bool resize_m_strip(int cx, int dw, int sw, int readable, double invX, int* wsOut, uint8_t* out /* kResizeMStrip */, int* maxPiece) {
    int comb[kResizeMTile][2][2];      // per column: (source column, weight) of its two taps
    int lo = 1 << 30, hi = -1;
    for (int c = 0; c < kResizeMTile; c++) {
        const int x = kResizeMTile * cx + c;
        comb[c][0][1] = comb[c][1][1] = 0; comb[c][0][0] = comb[c][1][0] = 0;
        if (x >= dw) continue;
        int o; unsigned wp;
        resize_coef_host(x, invX, sw, true, &o, &wp);
        const int w0 = (short)(wp & 0xFFFF), w1 = (short)(wp >> 16);
        if (w0 < 0 || w1 < 0) return false;
        comb[c][0][0] = o; comb[c][0][1] = w0;
        comb[c][1][0] = std::min(o + 1, sw - 1); comb[c][1][1] = w1;
        for (int t = 0; t < 2; t++)
            if (comb[c][t][1]) { lo = std::min(lo, comb[c][t][0]); hi = std::max(hi, comb[c][t][0]); }
    }
    if (hi < 0) return false;
    // a 16-byte-aligned source column at or below the first one used, pulled inside what may be loaded
    int ws = lo & ~15;
    if (ws > readable - kResizeMWin) ws = readable - kResizeMWin;
    if (ws < 0 || (ws & 3) || lo < ws || hi >= ws + kResizeMWin) return false;
    *wsOut = ws;
    std::memset(out, 0, kResizeMStrip);
    int weight[kResizeMTile][kResizeMWin] = {};
    int32_t colOff[kResizeMTile];
    for (int c = 0; c < kResizeMTile; c++) {
        int sum = 0;
        for (int t = 0; t < 2; t++)
            if (comb[c][t][1]) { weight[c][comb[c][t][0] - ws] += comb[c][t][1]; sum += comb[c][t][1]; }
        colOff[c] = 128 * sum;
        for (int k = 0; k < kResizeMWin; k++) {
            const int c1 = weight[c][k] >> 6, c0 = weight[c][k] & 63;
            if (c1 > 127) return false;
            *maxPiece = std::max(*maxPiece, std::max(c1, c0));
            const int slot = (c + 32 * ((k >> 4) & 1)) * 16 + (k & 15);
            out[(0 + (k >> 5)) * kResizeMFrag + slot] = (uint8_t)c1;
            out[(2 + (k >> 5)) * kResizeMFrag + slot] = (uint8_t)c0;
        }
    }
    std::memcpy(out + 4 * kResizeMFrag, colOff, sizeof(colOff));
    return true;
}

inline ResizeMTables resize_m_build(const std::vector<ResizeMLevelIn>& in) {
    ResizeMTables T;
    std::map<std::string, int> seen;
    std::vector<uint8_t> buf(kResizeMStrip);
    for (size_t l = 0; l < in.size(); l++) {
        ResizeMLevel M{};
        if (l == 0) { T.level.push_back(M); continue; }
        const ResizeMLevelIn &D = in[l], &S = in[l - 1];
        M.tilesX = (D.w + kResizeMTile - 1) / kResizeMTile;
        M.blocksY = (D.h + kResizeMTile - 1) / kResizeMTile;
        M.ok = D.w > 0 && D.h > 0 && S.w > 0 && S.h > 0 && S.readable >= S.w && S.readable >= kResizeMWin && (S.readable & 3) == 0;
        const double invX = 1. / ((double)D.w / S.w), invY = 1. / ((double)D.h / S.h);      // (as the launch of k_resize computes them)
        std::vector<int> idx;
        std::vector<std::string> fresh;
        std::map<std::string, int> mine;
        for (int cx = 0; M.ok && cx < M.tilesX; cx++) {
            int ws = 0;
            if (!resize_m_strip(cx, D.w, S.w, S.readable, invX, &ws, buf.data(), &T.maxPiece)) { M.ok = 0; break; }
            const std::string key((const char*)buf.data(), buf.size());
            int off;
            auto it = seen.find(key);
            if (it != seen.end()) off = it->second;
            else if ((it = mine.find(key)) != mine.end()) off = it->second;
            else {
                off = (int)(T.strips.size() + fresh.size() * kResizeMStrip);
                mine.emplace(key, off);
                fresh.push_back(key);
            }
            idx.push_back(ws); idx.push_back(off);
        }
        std::vector<ResizeMRow> rows;
        for (int y = 0; M.ok && y < kResizeMTile * M.blocksY; y++) {
            int o; unsigned wp;
            resize_coef_host(std::min(y, D.h - 1), invY, S.h, false, &o, &wp);
            ResizeMRow R;
            R.sy0 = std::min(std::max(o, 0), S.h - 1); R.sy1 = std::min(std::max(o + 1, 0), S.h - 1);
            R.b0 = (short)(wp & 0xFFFF); R.b1 = (short)(wp >> 16);
            if (R.b0 < 0 || R.b1 < 0) M.ok = 0;
            if (!rows.empty() && (R.sy0 < rows.back().sy0 || R.sy1 < rows.back().sy1)) M.ok = 0;      // (a block reads the rows sy0(first) .. sy1(last))
            rows.push_back(R);
        }
        for (int b = 0; M.ok && b < M.blocksY; b++) {
            const int span = rows[kResizeMTile * b + kResizeMTile - 1].sy1 - rows[kResizeMTile * b].sy0 + 1;
            if (span > kResizeMRows) M.ok = 0;
            M.maxSpan = std::max(M.maxSpan, span);
        }
        if (M.ok) {      // (a refused level leaves nothing behind)
            M.xIdx = (int)T.idx.size() / 2; M.rowOff = (int)T.rows.size();
            T.idx.insert(T.idx.end(), idx.begin(), idx.end());
            T.rows.insert(T.rows.end(), rows.begin(), rows.end());
            for (const std::string& k : fresh) T.strips.insert(T.strips.end(), k.begin(), k.end());
            seen.insert(mine.begin(), mine.end());
        } else M.maxSpan = 0;
        T.level.push_back(M);
    }
    return T;
}

}  // namespace orb
}  // namespace eao
