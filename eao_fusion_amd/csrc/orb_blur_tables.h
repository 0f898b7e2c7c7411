// orb_blur_tables.h -- the operand tables of the matrix-core blur (k_blur7_mfma in orb.hip) and its tiling, built once per geometry on the host.
// Plain C++17, no HIP: tests/cpp/orb_blur_tables_test.cpp replays the kernel's tile products from these tables in integer arithmetic against the direct
// 7 x 7 blur under AddressSanitizer on a machine without a GPU.
//
// The blur is out = min(255, (Ty . P . Tx + 32768) >> 16) with banded Toeplitz matrices of the taps 18 34 49 55 49 34 18.  A tile is 32 x 32 outputs:
//   stage 1   X[source row][out x] = (P - 128) . Tx over a 64-byte source window (two K steps of v_mfma_i32_32x32x32_i8)
//   stage 2   out[y][x] = Ty . X over the 32-row source blocks b - 1, b, b + 1 of output block b (three K steps)
// BORDER_REFLECT_101 is FOLDED INTO THE TABLES: a tap whose source falls outside the image is added to the entry of the in-image source it reflects to,
// outputs beyond the image get all-zero weights, and so do sources the window holds but no tap reaches -- whatever bytes sit there are harmless.
// A table is stored as the instruction's operand fragments: K step s, lane (n = lane & 31, half = lane >> 5), byte j -- 1 KiB per K step, one 16-byte
// load per lane.  The instruction multiplies slot (half, j) of one operand with slot (half, j) of the other, so only the pairing matters:
//   Tx   slot (s, half, j) <-> source column  window start + 32 s + 16 half + j            (the pixel fragment is 16 consecutive bytes of a row)
//   Ty   slot (s, half, j) <-> source row     32 (b - 1 + s) + (j & 3) + 8 (j >> 2) + 4 half   (stage 1's accumulator register j, packed to byte j)
// Identical tables are stored once (every interior tile of every level shares one Tx and one Ty).
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace eao {
namespace orb {

constexpr int kBlurMTile = 32;       // outputs per tile edge, and rows per source block
constexpr int kBlurMWin = 64;        // source window of a tile, bytes per row
constexpr int kBlurMSeg = 8;         // output blocks a wave walks down its column strip, at most
constexpr int kBlurMFrag = 1024;     // bytes of one K step of a table
constexpr int kBlurTaps[7] = {18, 34, 49, 55, 49, 34, 18};

struct BlurMLevelIn { int w, h, readable; };      // readable: bytes of every row that may be loaded (>= w)
struct BlurMLevel {
    int ok;                 // the level takes the matrix-core path (else: narrower or lower than the source window)
    int tilesX, blocksY;    // column strips, 32-row blocks
    int xIdx, yIdx;         // first entry of the level in BlurMTables::idx: tilesX pairs (window start, Tx offset), then blocksY pairs (0, Ty offset)
};
struct BlurMTables {
    std::vector<BlurMLevel> level;
    std::vector<int> idx;            // pairs of ints, see BlurMLevel
    std::vector<uint8_t> frag;       // the tables, kBlurMFrag-aligned offsets
    int maxEntry = 0;
};

inline int blur_reflect101(int p, int len) {
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}
// first source column of the window of column strip cx: 16 bytes left of the strip, pulled inside what may be loaded
inline int blur_m_window_start(int cx, int readable) {
    int ws = kBlurMTile * cx - 16;
    if (ws > readable - kBlurMWin) ws = readable - kBlurMWin;
    return ws < 0 ? 0 : ws;
}
// a column strip of blocksY blocks is cut into the fewest walks of at most kBlurMSeg blocks, of equal length (the last one may be shorter): every walk
// computes the source block above and below its outputs once more, so walks are long, and equal so that no wave is left with a stub
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int blur_m_walks(int blocksY, int* len) {
    const int n = (blocksY + kBlurMSeg - 1) / kBlurMSeg;
    *len = (blocksY + n - 1) / n;
    return n;
}
inline int blur_m_ty_slot(int rowInBlock, int* half) {     // byte j of the fragment holding this row of a source block
    *half = (rowInBlock >> 2) & 1;
    return (rowInBlock & 3) + 4 * (rowInBlock >> 3);
}

// false: some tap leaves the window (the caller keeps the VALU kernel for the level)
inline bool blur_m_tx(int cx, int w, int ws, uint8_t* out /* 2 K steps */) {
    std::memset(out, 0, 2 * kBlurMFrag);
    for (int c = 0; c < kBlurMTile; c++) {
        const int x = kBlurMTile * cx + c;
        if (x >= w) continue;
        for (int t = 0; t < 7; t++) {
            const int k = blur_reflect101(x - 3 + t, w) - ws;
            if (k < 0 || k >= kBlurMWin) return false;
            out[(k >> 5) * kBlurMFrag + (c + 32 * ((k >> 4) & 1)) * 16 + (k & 15)] += (uint8_t)kBlurTaps[t];
        }
    }
    return true;
}
inline bool blur_m_ty(int b, int h, uint8_t* out /* 3 K steps */) {
    std::memset(out, 0, 3 * kBlurMFrag);
    for (int r = 0; r < kBlurMTile; r++) {
        const int y = kBlurMTile * b + r;
        if (y >= h) continue;
        for (int t = 0; t < 7; t++) {
            const int sy = blur_reflect101(y - 3 + t, h);
            const int s = (sy >> 5) - (b - 1);
            if (s < 0 || s > 2) return false;
            int half;
            const int j = blur_m_ty_slot(sy & 31, &half);
            out[s * kBlurMFrag + (r + 32 * half) * 16 + j] += (uint8_t)kBlurTaps[t];
        }
    }
    return true;
}

inline BlurMTables blur_m_build(const std::vector<BlurMLevelIn>& in) {
    BlurMTables T;
    std::map<std::string, int> seen;
    auto intern = [&](const uint8_t* p, int bytes) {
        for (int i = 0; i < bytes; i++) T.maxEntry = T.maxEntry > p[i] ? T.maxEntry : p[i];
        const std::string key((const char*)p, (size_t)bytes);
        auto it = seen.find(key);
        if (it != seen.end()) return it->second;
        const int off = (int)T.frag.size();
        T.frag.insert(T.frag.end(), p, p + bytes);
        seen.emplace(key, off);
        return off;
    };
    std::vector<uint8_t> buf(3 * kBlurMFrag);
    for (const BlurMLevelIn& L : in) {
        BlurMLevel M{};
        M.tilesX = (L.w + kBlurMTile - 1) / kBlurMTile;
        M.blocksY = (L.h + kBlurMTile - 1) / kBlurMTile;
        M.ok = L.w >= kBlurMWin && L.h >= kBlurMWin && L.readable >= L.w;
        std::vector<int> idx;
        for (int cx = 0; M.ok && cx < M.tilesX; cx++) {
            const int ws = blur_m_window_start(cx, L.readable);
            if (!blur_m_tx(cx, L.w, ws, buf.data())) { M.ok = 0; break; }
            idx.push_back(ws); idx.push_back(intern(buf.data(), 2 * kBlurMFrag));
        }
        for (int b = 0; M.ok && b < M.blocksY; b++) {
            if (!blur_m_ty(b, L.h, buf.data())) { M.ok = 0; break; }
            idx.push_back(0); idx.push_back(intern(buf.data(), 3 * kBlurMFrag));
        }
        if (M.ok) {
            M.xIdx = (int)T.idx.size() / 2; M.yIdx = M.xIdx + M.tilesX;
            T.idx.insert(T.idx.end(), idx.begin(), idx.end());
        }
        T.level.push_back(M);
    }
    return T;
}

}  // namespace orb
}  // namespace eao
