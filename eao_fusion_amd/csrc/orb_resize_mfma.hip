// orb_resize_mfma.hip -- one level of the chained pyramid on the matrix cores: the horizontal pass of the 11-bit fixed-point bilinear resize as exact int8
// matrix products (v_mfma_i32_32x32x32_i8, i32 accumulation), the vertical pass with its two truncations on the VALU, in-lane.  Same arithmetic as k_resize
// (orb.hip), pixel by pixel; the operand tables and the tiling are those of orb_resize_tables.h, whose header states the operand formats.
//
// A wave owns a 32-pixel column strip of the level and walks up to kResizeMSeg 32 x 32 output tiles down it; the strip's weight fragments and column offsets
// stay in registers for the walk.  Per tile:
//   load     the source rows sy0(first row) .. sy1(last row) of the tile's 64-byte window, FOUR LANES TO A ROW (64 contiguous bytes, sixteen rows per load
//            instruction), ^ 0x80, parked in the wave's own LDS image (80-byte row pitch).  Loaded as the operand wants them -- lane = row -- an instruction
//            would touch 64 separate pieces of 32 cache lines (what bound the first matrix-core blur, profiles/orb_blur_mfma_ab.txt section 2).
//   operand  lane (y, half) reads 16 bytes of ITS row sy0(y), and of sy1(y), per K step from LDS: the row choice is an address, no register is indexed
//   product  H^T = Tx^T . S^T: four chains of two K steps -- weight pieces c1, c0 x rows sy0, sy1 -- 8 MFMA; the c0 chains start from the column offsets
//   tail     per lane sixteen columns of output row y: H = 64 acc1 + acc0, (b0 (H0 >> 4) >> 16) + (b1 (H1 >> 4) >> 16) + 2 >> 2 (weights >= 0, pairs sum to 2048: no
//            clamp), four pixels to a dword; two half-wave exchanges (v_permlane32_swap) make them ONE 16-byte store of row-contiguous pixels per lane.
// The next tile's rows are in flight during the products and the tail.  Stores may run into the row padding (the pitch is a multiple of 64, a strip ends at a multiple
// of 32), never beyond: columns past the width carry zero weights and zero offsets, rows past the height are computed from the last row's record and not stored.
#include "orb_internal.h"

using namespace eao::orb;

namespace {

typedef int rm_v4i __attribute__((ext_vector_type(4)));
typedef int rm_v16i __attribute__((ext_vector_type(16)));
typedef rm_v4i rm_v4i_a4 __attribute__((aligned(4)));
typedef unsigned short rm_u16x2 __attribute__((ext_vector_type(2)));

constexpr int kLdsPitch = 80;
constexpr int kLoads = 4;                      // load instructions of a block that are in flight during the tile before it: 64 source rows
static_assert(kResizeMRows == 16 * (kLoads + 1), "a block's rows beyond the prefetched ones are one more load");

struct ResizeMArgs {
    int dw, dh, dpitch, doff;        // the level produced
    int sh, spitch, soff;            // its source (level l - 1; soff / spitch of the pyramid, or the caller's image)
    int srcIsInput, pyrFrameBytes;
    int tilesX, blocksY, walkLen;
    int frameAffinity;               // frame f is served by XCD f % 8 (batches that are a multiple of 8; see k_resize)
};

__device__ __forceinline__ void rm_load(const uint8_t* __restrict__ src, int spitch, int sh, int base, int n, unsigned ws, int lane, rm_v4i raw[kLoads]) {
#pragma unroll
    for (int k = 0; k < kLoads; k++)
        if (k < n) {      // (wave-uniform)
            const int y = min(base + 16 * k + (lane >> 2), sh - 1);      // (rows below the block's last one are read and never used)
            raw[k] = *reinterpret_cast<const rm_v4i_a4*>(src + (unsigned)(__umul24(y, spitch) + ws + 16 * (lane & 3)));
        }
}

// idx: per column strip (window start, byte offset of its table in strips); rows: per output row of the padded level (sy0, sy1, b0, b1).  Parameters of their own,
// const and __restrict__: what a wave reads from them at wave-uniform addresses comes through the scalar cache.
__global__ __launch_bounds__(64, 4) void k_resize_mfma(ResizeMArgs A, ImgSrc s, int f0, const int2* __restrict__ idx, const int4* __restrict__ rows,
                                                    const uint8_t* __restrict__ strips) {
    int f = blockIdx.z, bx = blockIdx.x;
    if (A.frameAffinity) {
        const unsigned b = blockIdx.x + gridDim.x * blockIdx.z, xcd = b & 7, slot = b >> 3;
        f = (int)(xcd + 8 * (slot / gridDim.x)); bx = (int)(slot % gridDim.x);
    }
    f += f0;
    const int lane = threadIdx.x, half = lane >> 5;
    const int cx = bx % A.tilesX, b0 = (bx / A.tilesX) * A.walkLen;
    const int b1 = min(b0 + A.walkLen, A.blocksY);
    if (b0 >= b1) return;
    const int spitch = A.srcIsInput ? s.pitch0 : A.spitch;
    const uint8_t* src = A.srcIsInput ? s.img0 + (long long)f * s.fs0 : s.pyr + (long long)f * A.pyrFrameBytes + A.soff;
    uint8_t* dst = s.pyr + (long long)f * A.pyrFrameBytes + A.doff;
    const int2 xi = idx[cx];
    const unsigned ws = (unsigned)xi.x;
    const uint8_t* tab = strips + xi.y;
    const rm_v4i t10 = *reinterpret_cast<const rm_v4i*>(tab + lane * 16), t11 = *reinterpret_cast<const rm_v4i*>(tab + kResizeMFrag + lane * 16);
    const rm_v4i t00 = *reinterpret_cast<const rm_v4i*>(tab + 2 * kResizeMFrag + lane * 16), t01 = *reinterpret_cast<const rm_v4i*>(tab + 3 * kResizeMFrag + lane * 16);
    // the C input of the c0 chains: 128 (a0 + a1) of the lane's sixteen columns, in registers of their own for the whole walk (the instruction's C input need not be
    // its destination)
    rm_v16i coff;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const rm_v4i o = *reinterpret_cast<const rm_v4i*>(tab + 4 * kResizeMFrag + 4 * (8 * q + 4 * half));
#pragma unroll
        for (int e = 0; e < 4; e++) coff[4 * q + e] = o[e];
    }
    asm volatile("" : "+v"(coff));
    rm_v16i z;
#pragma unroll
    for (int q = 0; q < 16; q++) z[q] = 0;
    __shared__ __attribute__((aligned(16))) uint8_t stage[kResizeMRows * kLdsPitch];
    const rm_v4i bias = {(int)0x80808080u, (int)0x80808080u, (int)0x80808080u, (int)0x80808080u};

    rm_v4i raw[kLoads];
    // the block's first and last source row come through the scalar cache (wave-uniform addresses): the pixel loads do not wait for the lanes' row records
    int base = rows[kResizeMTile * b0].x;
    int n = (rows[kResizeMTile * b0 + kResizeMTile - 1].y - base + 16) >> 4;      // source rows of the block, in sixteens
    int4 rt = rows[kResizeMTile * b0 + (lane & 31)];
    rm_load(src, spitch, A.sh, base, n, ws, lane, raw);
    for (int b = b0; b < b1; b++) {
        // (one wave, LDS operations in order: the previous tile's fragment reads are done before these writes land)
        eao::wave_sync();
#pragma unroll
        for (int k = 0; k < kLoads; k++)
            if (k < n) *reinterpret_cast<rm_v4i*>(stage + (16 * k + (lane >> 2)) * kLdsPitch + 16 * (lane & 3)) = raw[k] ^ bias;
        if (n > kLoads) {      // rows 64 .. 79 of a block (scale factors near 2 only): loaded here, not ahead -- four more registers would cost the fourth wave of a SIMD
            const int y = min(base + 16 * kLoads + (lane >> 2), A.sh - 1);
            const rm_v4i late = *reinterpret_cast<const rm_v4i_a4*>(src + (unsigned)(__umul24(y, spitch) + ws + 16 * (lane & 3)));
            *reinterpret_cast<rm_v4i*>(stage + (16 * kLoads + (lane >> 2)) * kLdsPitch + 16 * (lane & 3)) = late ^ bias;
        }
        eao::wave_sync();
        const uint8_t* p0 = stage + (rt.x - base) * kLdsPitch + 16 * half;
        const uint8_t* p1 = stage + (rt.y - base) * kLdsPitch + 16 * half;
        const rm_v4i a00 = *reinterpret_cast<const rm_v4i*>(p0), a01 = *reinterpret_cast<const rm_v4i*>(p0 + 32);
        const rm_v4i a10 = *reinterpret_cast<const rm_v4i*>(p1), a11 = *reinterpret_cast<const rm_v4i*>(p1 + 32);
        const unsigned B0 = (unsigned)rt.z << 16, B1 = (unsigned)rt.w << 16;
        if (b + 1 < b1) {      // the next tile's rows: in flight during the products and the tail
            base = rows[kResizeMTile * (b + 1)].x;
            n = (rows[kResizeMTile * (b + 1) + kResizeMTile - 1].y - base + 16) >> 4;
            rt = rows[kResizeMTile * (b + 1) + (lane & 31)];
            rm_load(src, spitch, A.sh, base, n, ws, lane, raw);
        }
        rm_v16i h0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(t10, a00, z, 0, 0, 0);
        rm_v16i l0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(t00, a00, coff, 0, 0, 0);
        rm_v16i h1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(t10, a10, z, 0, 0, 0);
        rm_v16i l1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(t00, a10, coff, 0, 0, 0);
        h0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(t11, a01, h0, 0, 0, 0);
        l0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(t01, a01, l0, 0, 0, 0);
        h1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(t11, a11, h1, 0, 0, 0);
        l1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(t01, a11, l1, 0, 0, 0);
        unsigned o[4];      // o[q]: columns 8 q + 4 half .. + 3 of the strip, row lane & 31 of the tile
#pragma unroll
        for (int q = 0; q < 4; q++) {
            unsigned sv[4];      // the rounded sums before their >> 2: 10 bits
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const unsigned H0 = ((unsigned)h0[4 * q + e] << 6) + (unsigned)l0[4 * q + e], H1 = ((unsigned)h1[4 * q + e] << 6) + (unsigned)l1[4 * q + e];
                sv[e] = __umulhi(B0, H0 >> 4) + __umulhi(B1, H1 >> 4) + 2;
            }
            const rm_u16x2 two = {2, 2};
            const rm_u16x2 pa = __builtin_bit_cast(rm_u16x2, sv[0] | (sv[1] << 16)) >> two, pb = __builtin_bit_cast(rm_u16x2, sv[2] | (sv[3] << 16)) >> two;
            o[q] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, pb), __builtin_bit_cast(unsigned, pa), 0x06040200u);
        }
        // A row is split over the two halves of the wave in 4-byte pieces; two half exchanges (lanes 32-63 of the first register <-> lanes 0-31 of the second) give
        // the lower half columns 0 .. 15 and the upper half 16 .. 31 of the strip (as in k_blur7_mfma)
        const auto s02 = __builtin_amdgcn_permlane32_swap(o[0], o[2], false, false);
        const auto s13 = __builtin_amdgcn_permlane32_swap(o[1], o[3], false, false);
        const int y = kResizeMTile * b + (lane & 31);
        if (y < A.dh) *reinterpret_cast<uint4*>(dst + (unsigned)(__umul24(y, A.dpitch) + kResizeMTile * cx + 16 * half)) = make_uint4(s02[0], s02[1], s13[0], s13[1]);
    }
}

}  // namespace

namespace eao {
namespace orb {

void launch_resize_mfma(const eao_orb* h, hipStream_t str, const ImgSrc& s, int l, int batch, int frameAffinity) {
    const Geom& g = h->geom;
    const ResizeMLevel& M = h->resizeM[l];
    ResizeMArgs A;
    A.dw = g.L[l].w; A.dh = g.L[l].h; A.dpitch = g.L[l].pitch; A.doff = g.L[l].off;
    A.sh = g.L[l - 1].h; A.spitch = g.L[l - 1].pitch; A.soff = g.L[l - 1].off;
    A.srcIsInput = l == 1; A.pyrFrameBytes = g.pyrFrameBytes;
    A.tilesX = M.tilesX; A.blocksY = M.blocksY;
    const int walks = resize_m_walks(M.blocksY, &A.walkLen);
    A.frameAffinity = frameAffinity;
    const int2* idx = reinterpret_cast<const int2*>(h->d_resizeTab.p) + M.xIdx;
    const int4* rows = reinterpret_cast<const int4*>(h->d_resizeTab.p + h->resizeMRowsOff) + M.rowOff;
    const uint8_t* strips = h->d_resizeTab.p + h->resizeMStripsOff;
    // one-wave workgroups, as k_resize has them (see the comment at its launch)
    hipLaunchKernelGGL(k_resize_mfma, dim3(M.tilesX * walks, 1, batch), dim3(64), 0, str, A, s, 0, idx, rows, strips);
}

}  // namespace orb
}  // namespace eao
