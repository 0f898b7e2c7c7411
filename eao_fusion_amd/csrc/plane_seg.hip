// plane_seg.hip -- Frame::ComputePlanesFromPEAC on the device (include/eao_fusion.h, "Plane segmentation"; reference src/Frame.cc:381-460 and include/PEAC/):
// the two passes over all pixels run here, the small sequential middle in plane_seg_internal.h on the host.
//
// k_ps_block_init   one wavefront per window x window block: the depth tile and its one-pixel right / lower halo in LDS, the validity and discontinuity rules of
//                   the block constructor (AHCPlaneSeg.hpp:211-285) over the tile, then nine lanes accumulate one of the nine sums each, SEQUENTIALLY in row-major
//                   order (the doubles are upstream's bit for bit), and lane 0 runs pseg::fit (Stats::compute).  One BlockRecord per block.
// k_ps_membership   block map + plidmap -> the final plane id per pixel; k_ps_claims then writes the sparse list of pixels the flood fill claimed.
// The voxel stage (pcl::VoxelGrid of every final plane, src/Frame.cc:435-439) -- no float atomics, bytes that do not depend on the schedule:
//   k_ps_minmax     float min / max of each plane's points and its pixel count: integer atomics on the floats' ordered bit patterns (exact, order-free)
//   k_ps_keys       key = first cell of the pixel's plane + voxel index; the cell count of all planes for a pixel of no plane (it sorts behind everything)
//   k_rs_*          a STABLE least-significant-digit radix sort of (key, pixel), 8 bits a pass, as many passes as the cell count has bytes.  A thread owns
//                   kRunLen consecutive elements and a private column of the 256 x threads histogram, so no pass has an atomic and equal keys keep their
//                   ascending pixel order
//   k_ps_heads      one workgroup: the first element of every run of equal keys -> the voxels in ascending (plane, voxel index)
//   k_ps_centroid   one lane per voxel: the float sum of its points in ascending pixel index, divided by the float count; 16 bytes per point (x, y, z, 0),
//                   plane_map's arena format
// Compiled with -ffp-contract=off.  Every index into a buffer is bounded by a count the same launch was sized from.
#include <chrono>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "plane_seg_internal.h"
#include "plane_seg_shared.h"
#include "small_dense.h"      // ordered_key / key_value

namespace pseg = eao::pseg;
static_assert(sizeof(eao_plane_seg_block) == sizeof(pseg::BlockRecord), "the public block record is the internal one");

namespace {

constexpr int kMaxWindow = EAO_PLANE_SEG_MAX_WINDOW;
constexpr int kMaxPlanes = EAO_PLANE_SEG_MAX_PLANES;
constexpr int kRunLen = 128;        // consecutive elements one thread of the radix sort owns
constexpr int kScanThreads = 1024;

struct Intr {
    float fx, fy, cx, cy;
    double dmin, dmax, alpha, tol;
    int W, H, w, Nw, Nh;
};

struct Grid {      // one per final plane
    int minb[3], div[3];
    unsigned cell0;      // the first cell of this plane among all planes' cells
    int pad;
};

__global__ __launch_bounds__(64) void k_ps_block_init(Intr I, const float* __restrict__ depth, pseg::BlockRecord* __restrict__ out) {
    __shared__ float sTile[(kMaxWindow + 1) * (kMaxWindow + 1)];
    __shared__ double sSum[9];
    __shared__ int sFlag;
    const int b = blockIdx.x, bi = b / I.Nw, bj = b - bi * I.Nw, lane = threadIdx.x;
    const int w = I.w, tw = w + 1;
    if (lane == 0) sFlag = 0;
    for (int e = lane; e < tw * tw; e += 64) {
        const int ty = e / tw, tx = e - ty * tw;
        const int gy = bi * w + ty, gx = bj * w + tx;
        // outside the image there is no neighbour to compare with: a NaN is a neighbour that get() refuses
        sTile[e] = (gy < I.H && gx < I.W) ? depth[(size_t)gy * I.W + gx] : __uint_as_float(0x7fc00000u);
    }
    __syncthreads();
    int flag = 0;
    for (int e = lane; e < w * w; e += 64) {
        const int ty = e / w, tx = e - ty * w;
        const double d = (double)sTile[ty * tw + tx];
        if (!pseg::pixel_valid(d, I.dmin, I.dmax)) {
            flag |= pseg::kFlagMissing;
        } else {
            const double th = pseg::t_dz(I.alpha, I.tol, d);
            const double zr = (double)sTile[ty * tw + tx + 1], zl = (double)sTile[(ty + 1) * tw + tx];
            if (pseg::pixel_valid(zr, I.dmin, I.dmax) && fabs(d - zr) > th) flag |= pseg::kFlagDiscontinuity;
            if (pseg::pixel_valid(zl, I.dmin, I.dmax) && fabs(d - zl) > th) flag |= pseg::kFlagDiscontinuity;
        }
    }
    if (flag) atomicOr(&sFlag, flag);
    __syncthreads();
    flag = sFlag;
    if (flag == 0 && lane < 9) {
        // sum `lane` of sx sy sz sxx syy szz sxy syz sxz: first factor ia, second factor ib (none for the first three)
        const int ia = lane == 8 ? 0 : lane % 3, ib = lane < 6 ? lane - 3 : (lane == 6 ? 1 : 2);
        double s = 0.0;
        for (int ty = 0; ty < w; ty++)
            for (int tx = 0; tx < w; tx++) {
                const double d = (double)sTile[ty * tw + tx];
                double x, y;
                pseg::pixel_point(I.fx, I.fy, I.cx, I.cy, bi * w + ty, bj * w + tx, d, x, y);
                const double a = ia == 0 ? x : (ia == 1 ? y : d);
                const double c = ib == 0 ? x : (ib == 1 ? y : d);
                s += lane < 3 ? a : a * c;
            }
        sSum[lane] = s;
    }
    __syncthreads();
    if (lane == 0) {
        pseg::BlockRecord r;
        r.flag = flag;
        if (flag || w * w < 4) {
            r.N = 0;
            for (int k = 0; k < 9; k++) r.sums[k] = 0.0;
            for (int k = 0; k < 3; k++) r.center[k] = r.normal[k] = 0.0;
            r.mse = r.curvature = __longlong_as_double(0x7ff8000000000000ll);
        } else {
            r.N = w * w;
            for (int k = 0; k < 9; k++) r.sums[k] = sSum[k];
            pseg::fit(r.sums, r.N, r.center, r.normal, r.mse, r.curvature);
        }
        out[b] = r;
    }
}

__global__ __launch_bounds__(256) void k_ps_membership(Intr I, int nOld, const int* __restrict__ blkMap, const int* __restrict__ plidmap, int* __restrict__ member) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= I.W * I.H) return;
    const int y = i / I.W, x = i - y * I.W, by = y / I.w, bx = x / I.w;
    int m = -1;
    if (by < I.Nh && bx < I.Nw) {
        const int p = blkMap[by * I.Nw + bx];
        if (p >= 0 && p < nOld) m = plidmap[p];
    }
    member[i] = m;
}

// claims: (pixel, plane) pairs, every pixel once, none of them inside a block that the block map gives to a plane
__global__ __launch_bounds__(256) void k_ps_claims(int n, int nPixels, int nOld, const int* __restrict__ claims, const int* __restrict__ plidmap, int* __restrict__ member) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int pix = claims[2 * i], pl = claims[2 * i + 1];
    if (pix < 0 || pix >= nPixels || pl < 0 || pl >= nOld) return;
    member[pix] = plidmap[pl];
}

__device__ __forceinline__ void plane_point(const Intr& I, const float* __restrict__ depth, int pix, float& px, float& py, float& pz) {
    const int m = pix / I.W, n = pix - m * I.W;
    const double d = (double)depth[pix];
    double x, y;
    pseg::pixel_point(I.fx, I.fy, I.cx, I.cy, m, n, d, x, y);
    px = (float)x; py = (float)y; pz = (float)d;      // src/Frame.cc:419-421
}

// mm: per plane 3 minima then 3 maxima as ordered keys (set to 0xffffffff / 0 by the host); count: pixels per plane (zeroed)
__global__ __launch_bounds__(256) void k_ps_minmax(Intr I, int nPlanes, const float* __restrict__ depth, const int* __restrict__ member, unsigned* __restrict__ mm,
                                                   int* __restrict__ count) {
    __shared__ unsigned sMM[kMaxPlanes * 6];
    __shared__ int sCnt[kMaxPlanes];
    for (int e = threadIdx.x; e < nPlanes * 6; e += 256) sMM[e] = (e % 6) < 3 ? 0xffffffffu : 0u;
    for (int e = threadIdx.x; e < nPlanes; e += 256) sCnt[e] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < I.W * I.H) {
        const int p = member[i];
        if (p >= 0 && p < nPlanes) {
            float v[3];
            plane_point(I, depth, i, v[0], v[1], v[2]);
            for (int k = 0; k < 3; k++) {
                const unsigned key = eao::dense::ordered_key(v[k]);
                atomicMin(&sMM[p * 6 + k], key);
                atomicMax(&sMM[p * 6 + 3 + k], key);
            }
            atomicAdd(&sCnt[p], 1);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nPlanes * 6; e += 256) {
        if ((e % 6) < 3) { if (sMM[e] != 0xffffffffu) atomicMin(&mm[e], sMM[e]); }
        else if (sMM[e] != 0u) atomicMax(&mm[e], sMM[e]);
    }
    for (int e = threadIdx.x; e < nPlanes; e += 256)
        if (sCnt[e]) atomicAdd(&count[e], sCnt[e]);
}

// pcl::VoxelGrid (PCL 1.8 voxel_grid.hpp): idx = i0 + i1 * div0 + i2 * div0 * div1, i = (int)floor(p * inv) - min_b
__global__ __launch_bounds__(256) void k_ps_keys(Intr I, int nPlanes, unsigned nCells, float inv, const float* __restrict__ depth, const int* __restrict__ member,
                                                 const Grid* __restrict__ grid, unsigned* __restrict__ key, int* __restrict__ pixOut) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= I.W * I.H) return;
    const int p = member[i];
    unsigned k = nCells;
    if (p >= 0 && p < nPlanes) {
        float v[3];
        plane_point(I, depth, i, v[0], v[1], v[2]);
        const Grid g = grid[p];
        const int i0 = (int)floorf(v[0] * inv) - g.minb[0], i1 = (int)floorf(v[1] * inv) - g.minb[1], i2 = (int)floorf(v[2] * inv) - g.minb[2];
        k = g.cell0 + (unsigned)(i0 + i1 * g.div[0] + i2 * g.div[0] * g.div[1]);
        if (k > nCells) k = nCells;      // (cannot happen: min_b and div come from these very points)
    }
    key[i] = k;
    pixOut[i] = i;
}

// hist[digit * T + t]: thread t's count of `digit` among its kRunLen elements (the buffer is zeroed first)
__global__ __launch_bounds__(256) void k_rs_count(int n, int T, int shift, const unsigned* __restrict__ key, int* __restrict__ hist) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int b = t * kRunLen, e = min(n, b + kRunLen);
    for (int i = b; i < e; i++) hist[(size_t)((key[i] >> shift) & 255u) * T + t] += 1;
}

// one workgroup: exclusive scan of v[0 .. m) in place
__global__ __launch_bounds__(kScanThreads) void k_rs_scan(int m, int* __restrict__ v) {
    __shared__ int sPart[kScanThreads];
    const int per = (m + kScanThreads - 1) / kScanThreads;
    const int b = min(m, (int)threadIdx.x * per), e = min(m, b + per);
    int s = 0;
    for (int i = b; i < e; i++) s += v[i];
    sPart[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const int add = threadIdx.x >= off ? sPart[threadIdx.x - off] : 0;
        __syncthreads();
        sPart[threadIdx.x] += add;
        __syncthreads();
    }
    int run = sPart[threadIdx.x] - s;
    for (int i = b; i < e; i++) {
        const int c = v[i];
        v[i] = run;
        run += c;
    }
}

__global__ __launch_bounds__(256) void k_rs_scatter(int n, int T, int shift, const unsigned* __restrict__ key, const int* __restrict__ pix, int* __restrict__ hist,
                                                    unsigned* __restrict__ keyOut, int* __restrict__ pixOut) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int b = t * kRunLen, e = min(n, b + kRunLen);
    for (int i = b; i < e; i++) {
        const unsigned k = key[i];
        int* slot = hist + (size_t)((k >> shift) & 255u) * T + t;
        const int pos = *slot;
        *slot = pos + 1;
        if (pos >= 0 && pos < n) {
            keyOut[pos] = k;
            pixOut[pos] = pix[i];
        }
    }
}

// one workgroup over the sorted keys: vstart[v] = first element of voxel v, vstart[nVox] = the number of elements of any plane; counts[0] = nVox, counts[1] = that number
__global__ __launch_bounds__(kScanThreads) void k_ps_heads(int n, unsigned nCells, const unsigned* __restrict__ key, int* __restrict__ vstart, int* __restrict__ counts) {
    __shared__ int sPart[kScanThreads];
    __shared__ int sMem[kScanThreads];
    const int per = (n + kScanThreads - 1) / kScanThreads;
    const int b = min(n, (int)threadIdx.x * per), e = min(n, b + per);
    int heads = 0, mem = 0;
    for (int i = b; i < e; i++) {
        const unsigned k = key[i];
        if (k < nCells) {
            mem++;
            if (i == 0 || key[i - 1] != k) heads++;
        }
    }
    sPart[threadIdx.x] = heads;
    sMem[threadIdx.x] = mem;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const int add = threadIdx.x >= off ? sPart[threadIdx.x - off] : 0;
        const int addm = threadIdx.x >= off ? sMem[threadIdx.x - off] : 0;
        __syncthreads();
        sPart[threadIdx.x] += add;
        sMem[threadIdx.x] += addm;
        __syncthreads();
    }
    int v = sPart[threadIdx.x] - heads;
    for (int i = b; i < e; i++) {
        const unsigned k = key[i];
        if (k < nCells && (i == 0 || key[i - 1] != k)) vstart[v++] = i;
    }
    if (threadIdx.x == kScanThreads - 1) {
        const int nVox = sPart[threadIdx.x], nMem = sMem[threadIdx.x];
        vstart[nVox] = nMem;      // (members sort before every pixel of no plane: they are the first nMem elements)
        counts[0] = nVox;
        counts[1] = nMem;
    }
}

// planeStart[p] = the first voxel of plane p (every final plane has one: it owns a whole block)
__global__ __launch_bounds__(256) void k_ps_centroid(Intr I, int n, int nPlanes, const float* __restrict__ depth, const Grid* __restrict__ grid,
                                                     const unsigned* __restrict__ key, const int* __restrict__ pix, const int* __restrict__ vstart,
                                                     const int* __restrict__ counts, float4* __restrict__ cloud, int* __restrict__ planeStart) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int nVox = counts[0];
    if (v >= nVox || v >= n) return;
    const int b = vstart[v], e = vstart[v + 1];
    if (b < 0 || e > n || b >= e) return;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = b; i < e; i++) {
        const int p = pix[i];
        if (p < 0 || p >= I.W * I.H) continue;
        float x, y, z;
        plane_point(I, depth, p, x, y, z);
        sx += x; sy += y; sz += z;
    }
    const float cnt = (float)(e - b);
    cloud[v] = make_float4(sx / cnt, sy / cnt, sz / cnt, 0.f);
    const unsigned k = key[b];
    int pl = 0;
    for (int q = 1; q < nPlanes; q++)
        if (k >= grid[q].cell0) pl = q;
    bool first = v == 0;
    if (!first) {
        const unsigned kp = key[vstart[v - 1]];
        first = kp < grid[pl].cell0;
    }
    if (first) planeStart[pl] = v;
}

struct PsegCtx : eao::ThreadStream {
    eao::PinBuf<hipHostMallocDefault> host;
};
thread_local PsegCtx g_pseg;

float key_to_float(unsigned k) {
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

}  // namespace

struct eao_plane_seg {
    std::mutex mutex;
    eao_plane_seg_cfg cfg;
    Intr I;
    int nPixels = 0, nBlocks = 0, T = 0;
    pseg::Segmenter seg;
    // device, owned by the handle
    eao::DevBuf<float> depth;
    eao::DevBuf<pseg::BlockRecord> rec;
    eao::DevBuf<int> member, pixA, pixB, hist, vstart, small;      // small: counts[2], planeStart[kMaxPlanes], count[kMaxPlanes], mm[kMaxPlanes * 6]
    eao::DevBuf<unsigned> keyA, keyB;
    eao::DevBuf<Grid> grid;
    eao::DevBuf<unsigned char> upload;
    eao::DevBuf<float4> cloud;
    // the last run's results (host)
    bool have = false;
    bool profile = false;       // eao_plane_seg_set_profiling: one more wait, behind the upload, so that the stages can be told apart
    bool haveTiming = false;
    double stageUs[4] = {0, 0, 0, 0};      // upload, block init + record download, host middle, membership + voxel stage (host clock; every stage ends in a wait)
    std::vector<pseg::BlockRecord> records;
    std::vector<eao_plane_seg_plane> planes;
    int nVox = 0;
};

namespace {

constexpr int oCounts = 0, oPlaneStart = 2, oCount = 2 + kMaxPlanes, oMM = 2 + 2 * kMaxPlanes, kSmall = 2 + 8 * kMaxPlanes;

std::string check_cfg(const eao_plane_seg_cfg& c) {
    char b[200];
    auto fail = [&](const char* what) { snprintf(b, sizeof(b), "eao_plane_seg_create: %s", what); return std::string(b); };
    if (c.width < 1 || c.height < 1 || (int64_t)c.width * c.height > EAO_PLANE_SEG_MAX_PIXELS) return fail("width x height is outside 1 .. EAO_PLANE_SEG_MAX_PIXELS");
    if (c.window < 2 || c.window > kMaxWindow) return fail("window is outside 2 .. EAO_PLANE_SEG_MAX_WINDOW");
    if (c.width < c.window || c.height < c.window) return fail("the image is smaller than one window");
    if (!(c.fx > 0.f) || !(c.fy > 0.f) || !std::isfinite(c.fx) || !std::isfinite(c.fy) || !std::isfinite(c.cx) || !std::isfinite(c.cy)) return fail("bad intrinsics");
    if (c.min_support < 1 || c.max_step < 0) return fail("min_support < 1 or max_step < 0");
    if (!(c.depth_min > 0.0) || !(c.depth_max >= c.depth_min) || !std::isfinite(c.depth_max)) return fail("the depth limits must satisfy 0 < depth_min <= depth_max < inf");
    if (!(c.leaf > 0.f) || !std::isfinite(c.leaf)) return fail("leaf must be positive");
    const double ds[] = {c.depth_sigma, c.std_tol_init, c.std_tol_merge, c.z_near, c.z_far, c.angle_near, c.angle_far, c.similarity_merge, c.similarity_refine,
                         c.depth_alpha, c.depth_change_tol};
    for (double d : ds)
        if (!std::isfinite(d)) return fail("a ParamSet value is not finite");
    if (!(c.z_far > c.z_near)) return fail("z_far <= z_near");
    return std::string();
}

// everything after the host's middle: membership, then the voxel grid of every final plane.  The handle's mutex is held; the run's guard is armed, and the
// last wait here is the run's.
eao_status device_tail(eao_plane_seg* h, PsegCtx& ctx, eao::Drain& drain) {
    const Intr& I = h->I;
    const pseg::Segmenter& sg = h->seg;
    const int n = h->nPixels, nPlanes = (int)sg.planes.size(), nOld = (int)sg.old.size(), nClaims = (int)(sg.claims.size() / 2);
    hipStream_t s = ctx.stream;
    eao_status st;
    // block map | plidmap | claims in one upload
    const size_t oBlk = 0, oPlid = eao::align256((size_t)h->nBlocks * 4), oClaims = eao::align256(oPlid + (size_t)std::max(nOld, 1) * 4),
                 end = oClaims + (size_t)std::max(nClaims, 1) * 8;
    if ((st = h->upload.reserve(end))) return st;
    if ((st = ctx.host.reserve(std::max(end, (size_t)kSmall * 4)))) return st;
    std::memcpy(ctx.host.p + oBlk, sg.blkMap.data(), (size_t)h->nBlocks * 4);
    if (nOld) std::memcpy(ctx.host.p + oPlid, sg.plidmap.data(), (size_t)nOld * 4);
    if (nClaims) std::memcpy(ctx.host.p + oClaims, sg.claims.data(), (size_t)nClaims * 8);
    EAO_HIP(hipMemcpyAsync(h->upload.p, ctx.host.p, end, hipMemcpyHostToDevice, s));
    const int* dBlk = (const int*)(h->upload.p + oBlk);
    const int* dPlid = (const int*)(h->upload.p + oPlid);
    const int* dClaims = (const int*)(h->upload.p + oClaims);
    hipLaunchKernelGGL(k_ps_membership, dim3(eao::cdiv(n, 256)), dim3(256), 0, s, I, nOld, dBlk, dPlid, h->member.p);
    EAO_HIP(hipGetLastError());
    if (nClaims) {
        hipLaunchKernelGGL(k_ps_claims, dim3(eao::cdiv(nClaims, 256)), dim3(256), 0, s, nClaims, n, nOld, dClaims, dPlid, h->member.p);
        EAO_HIP(hipGetLastError());
    }
    h->nVox = 0;
    if (nPlanes == 0) {
        EAO_HIP(drain.wait(eao::Drain::Latency));      // (the upload out of this thread's staging block has ended)
        return EAO_OK;
    }
    // min / max and pixel counts
    int* dSmall = h->small.p;
    EAO_HIP(hipMemsetAsync(dSmall, 0, (size_t)kSmall * 4, s));
    {
        unsigned* init = (unsigned*)ctx.host.p;      // (the upload above is ordered before this copy on the stream, but reads the same staging block: wait first)
        EAO_HIP(drain.wait_more(eao::Drain::Block));
        for (int e = 0; e < nPlanes * 6; e++) init[e] = (e % 6) < 3 ? 0xffffffffu : 0u;
        EAO_HIP(hipMemcpyAsync(dSmall + oMM, init, (size_t)nPlanes * 24, hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(k_ps_minmax, dim3(eao::cdiv(n, 256)), dim3(256), 0, s, I, nPlanes, (const float*)h->depth.p, (const int*)h->member.p,
                       (unsigned*)(dSmall + oMM), dSmall + oCount);
    EAO_HIP(hipGetLastError());
    EAO_HIP(drain.wait_more(eao::Drain::Block));
    EAO_HIP(hipMemcpyAsync(ctx.host.p, dSmall, (size_t)kSmall * 4, hipMemcpyDeviceToHost, s));
    EAO_HIP(drain.wait_more(eao::Drain::Latency));
    std::vector<int> pixCount(nPlanes);
    std::vector<Grid> grid(nPlanes);
    const float inv = 1.0f / h->cfg.leaf;
    uint64_t cells = 0;
    {
        const int* hs = (const int*)ctx.host.p;
        for (int p = 0; p < nPlanes; p++) {
            pixCount[p] = hs[oCount + p];
            if (pixCount[p] < 1) { eao::set_error("eao_plane_seg_run: plane %d has no pixel", p); return EAO_ERR_INTERNAL; }
            int64_t d[3];
            for (int k = 0; k < 3; k++) {
                const float mn = key_to_float((unsigned)hs[oMM + p * 6 + k]), mx = key_to_float((unsigned)hs[oMM + p * 6 + 3 + k]);
                const double lo = std::floor((double)(mn * inv)), hi = std::floor((double)(mx * inv));      // floor of a float is exact in either type
                if (!(std::fabs(lo) < 1e9) || !(std::fabs(hi) < 1e9)) { eao::set_error("eao_plane_seg_run: plane %d: the voxel grid overflows an int", p); return EAO_ERR_INVALID; }
                grid[p].minb[k] = (int)lo;
                d[k] = (int64_t)hi - (int64_t)lo + 1;
                grid[p].div[k] = (int)d[k];
            }
            // PCL refuses a grid whose cell count passes INT_MAX; so does this, and the sum over the planes has the cap of the header
            if (d[0] * d[1] > 2147483647ll || d[0] * d[1] * d[2] > 2147483647ll) { eao::set_error("eao_plane_seg_run: plane %d: more than INT_MAX voxel cells", p); return EAO_ERR_INVALID; }
            grid[p].cell0 = (unsigned)cells;
            grid[p].pad = 0;
            cells += (uint64_t)(d[0] * d[1] * d[2]);
            if (cells > (uint64_t)EAO_PLANE_SEG_MAX_CELLS) { eao::set_error("eao_plane_seg_run: more than EAO_PLANE_SEG_MAX_CELLS voxel cells over all planes"); return EAO_ERR_INVALID; }
        }
    }
    const unsigned nCells = (unsigned)cells;
    std::memcpy(ctx.host.p, grid.data(), (size_t)nPlanes * sizeof(Grid));
    EAO_HIP(hipMemcpyAsync(h->grid.p, ctx.host.p, (size_t)nPlanes * sizeof(Grid), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ps_keys, dim3(eao::cdiv(n, 256)), dim3(256), 0, s, I, nPlanes, nCells, inv, (const float*)h->depth.p, (const int*)h->member.p,
                       (const Grid*)h->grid.p, h->keyA.p, h->pixA.p);
    EAO_HIP(hipGetLastError());
    int passes = 1;
    while (passes < 4 && (nCells >> (8 * passes)) != 0) passes++;
    unsigned *kIn = h->keyA.p, *kOut = h->keyB.p;
    int *pIn = h->pixA.p, *pOut = h->pixB.p;
    const int T = h->T;
    for (int pass = 0; pass < passes; pass++) {
        EAO_HIP(hipMemsetAsync(h->hist.p, 0, (size_t)256 * T * 4, s));
        hipLaunchKernelGGL(k_rs_count, dim3(eao::cdiv(T, 256)), dim3(256), 0, s, n, T, 8 * pass, (const unsigned*)kIn, h->hist.p);
        EAO_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(kScanThreads), 0, s, 256 * T, h->hist.p);
        EAO_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_rs_scatter, dim3(eao::cdiv(T, 256)), dim3(256), 0, s, n, T, 8 * pass, (const unsigned*)kIn, (const int*)pIn, h->hist.p, kOut, pOut);
        EAO_HIP(hipGetLastError());
        std::swap(kIn, kOut);
        std::swap(pIn, pOut);
    }
    hipLaunchKernelGGL(k_ps_heads, dim3(1), dim3(kScanThreads), 0, s, n, nCells, (const unsigned*)kIn, h->vstart.p, dSmall + oCounts);
    EAO_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ps_centroid, dim3(eao::cdiv(n, 256)), dim3(256), 0, s, I, n, nPlanes, (const float*)h->depth.p, (const Grid*)h->grid.p, (const unsigned*)kIn,
                       (const int*)pIn, (const int*)h->vstart.p, (const int*)(dSmall + oCounts), h->cloud.p, dSmall + oPlaneStart);
    EAO_HIP(hipGetLastError());
    EAO_HIP(drain.wait_more(eao::Drain::Block));      // (the grid's upload out of the staging block has ended before the block is written again)
    EAO_HIP(hipMemcpyAsync(ctx.host.p, dSmall, (size_t)(2 + kMaxPlanes) * 4, hipMemcpyDeviceToHost, s));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    const int* hs = (const int*)ctx.host.p;
    const int nVox = hs[oCounts];
    if (nVox < nPlanes || nVox > n) { eao::set_error("eao_plane_seg_run: %d voxels for %d planes", nVox, nPlanes); return EAO_ERR_INTERNAL; }
    for (int p = 0; p < nPlanes; p++) {
        const int b = hs[oPlaneStart + p], e = p + 1 < nPlanes ? hs[oPlaneStart + p + 1] : nVox;
        if (b < 0 || e <= b || e > nVox) { eao::set_error("eao_plane_seg_run: plane %d: voxels %d .. %d of %d", p, b, e, nVox); return EAO_ERR_INTERNAL; }
        h->planes[p].cloud_offset = b;
        h->planes[p].cloud_count = e - b;
        h->planes[p].n_pixels = pixCount[p];
    }
    h->nVox = nVox;
    return EAO_OK;
}

}  // namespace

eao_status eao::plane_seg_kept_cloud(eao_plane_seg* h, int32_t plane, std::unique_lock<std::mutex>& lock, const float** pts, int32_t* n) {
    EAO_REQUIRE(h, "seg is NULL");
    std::unique_lock<std::mutex> mine(h->mutex);
    EAO_REQUIRE(h->have, "the segmentation handle holds no frame");
    EAO_REQUIRE(plane >= 0 && plane < (int32_t)h->planes.size(), "plane = %d is outside 0 .. %d", plane, (int)h->planes.size() - 1);
    EAO_REQUIRE(h->planes[plane].kept, "plane %d was not kept (PlaneNotSeen): upstream holds no cloud for it", plane);
    *pts = (const float*)(h->cloud.p + h->planes[plane].cloud_offset);
    *n = h->planes[plane].cloud_count;
    lock = std::move(mine);
    return EAO_OK;
}

extern "C" {

void eao_plane_seg_cfg_default(eao_plane_seg_cfg* c, int32_t width, int32_t height, float fx, float fy, float cx, float cy) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->width = width; c->height = height; c->fx = fx; c->fy = fy; c->cx = cx; c->cy = cy;
    c->window = 10; c->min_support = 3000; c->max_step = 100000;      // AHCPlaneFitter.hpp:152-156
    c->depth_min = 0.2; c->depth_max = 4.0; c->leaf = 0.05f;          // src/Frame.cc:396, :436
    // AHCParamSet.hpp:68-76
    c->depth_sigma = 1.6e-6; c->std_tol_init = 5; c->std_tol_merge = 8;
    c->z_near = 500; c->z_far = 4000;
    c->angle_near = (15.0) * M_PI / 180.0; c->angle_far = (90.0) * M_PI / 180.0;
    c->similarity_merge = std::cos((60.0) * M_PI / 180.0);
    c->similarity_refine = std::cos((30.0) * M_PI / 180.0);
    c->depth_alpha = 0.04; c->depth_change_tol = 0.02;
}

eao_status eao_plane_seg_create(const eao_plane_seg_cfg* cfg, eao_plane_seg** out) {
    EAO_REQUIRE(cfg && out, "bad argument");
    const std::string err = check_cfg(*cfg);
    EAO_REQUIRE(err.empty(), "%s", err.c_str());
    eao_status st = eao::require_device();
    if (st) return st;
    eao_plane_seg* h = new eao_plane_seg;
    h->cfg = *cfg;
    Intr& I = h->I;
    I.fx = cfg->fx; I.fy = cfg->fy; I.cx = cfg->cx; I.cy = cfg->cy;
    I.dmin = cfg->depth_min; I.dmax = cfg->depth_max; I.alpha = cfg->depth_alpha; I.tol = cfg->depth_change_tol;
    I.W = cfg->width; I.H = cfg->height; I.w = cfg->window; I.Nw = cfg->width / cfg->window; I.Nh = cfg->height / cfg->window;
    h->nPixels = I.W * I.H;
    h->nBlocks = I.Nw * I.Nh;
    h->T = eao::cdiv(h->nPixels, kRunLen);
    const size_t n = (size_t)h->nPixels;
    st = h->depth.reserve(n);
    if (!st) st = h->rec.reserve((size_t)h->nBlocks);
    if (!st) st = h->member.reserve(n);
    if (!st) st = h->pixA.reserve(n);
    if (!st) st = h->pixB.reserve(n);
    if (!st) st = h->keyA.reserve(n);
    if (!st) st = h->keyB.reserve(n);
    if (!st) st = h->hist.reserve((size_t)256 * h->T);
    if (!st) st = h->vstart.reserve(n + 1);
    if (!st) st = h->small.reserve((size_t)kSmall);
    if (!st) st = h->grid.reserve((size_t)kMaxPlanes);
    if (!st) st = h->cloud.reserve(n);
    if (st) { delete h; return st; }
    *out = h;
    return EAO_OK;
}

void eao_plane_seg_destroy(eao_plane_seg* h) { delete h; }

eao_status eao_plane_seg_run(eao_plane_seg* h, const float* depth, int32_t stride) {
    EAO_REQUIRE(h && depth, "bad argument");
    EAO_REQUIRE(stride >= h->cfg.width, "stride = %d floats is below the width %d", stride, h->cfg.width);
    std::lock_guard<std::mutex> lock(h->mutex);
    PsegCtx& ctx = g_pseg;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const Intr& I = h->I;
    const size_t n = (size_t)h->nPixels, recBytes = (size_t)h->nBlocks * sizeof(pseg::BlockRecord);
    if ((st = ctx.host.reserve(std::max(n * 4, recBytes)))) return st;
    h->have = false;      // from here on the last frame's results are gone: a failed run leaves the handle without results
    h->haveTiming = false;
    const auto t0 = std::chrono::steady_clock::now();
    for (int y = 0; y < I.H; y++) std::memcpy(ctx.host.p + (size_t)y * I.W * 4, depth + (size_t)y * stride, (size_t)I.W * 4);
    eao::Drain drain(ctx.stream);      // (armed across the host's middle, to the last wait of device_tail)
    EAO_HIP(hipMemcpyAsync(h->depth.p, ctx.host.p, n * 4, hipMemcpyHostToDevice, ctx.stream));
    if (h->profile) EAO_HIP(drain.wait_more(eao::Drain::Block));
    const auto t1 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(k_ps_block_init, dim3(h->nBlocks), dim3(64), 0, ctx.stream, I, (const float*)h->depth.p, h->rec.p);
    EAO_HIP(hipGetLastError());
    EAO_HIP(drain.wait_more(eao::Drain::Block));      // (the depth left the staging block; the records come back into it)
    EAO_HIP(hipMemcpyAsync(ctx.host.p, h->rec.p, recBytes, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait_more(eao::Drain::Latency));
    h->records.resize((size_t)h->nBlocks);
    std::memcpy(h->records.data(), ctx.host.p, recBytes);
    const auto t2 = std::chrono::steady_clock::now();
    h->seg.run(h->cfg, h->records.data(), depth, stride);
    const auto t3 = std::chrono::steady_clock::now();
    const int nPlanes = (int)h->seg.planes.size();
    if (nPlanes > kMaxPlanes) {
        eao::set_error("eao_plane_seg_run: %d planes; at most %d are supported", nPlanes, kMaxPlanes);
        return EAO_ERR_INVALID;
    }
    h->planes.assign((size_t)nPlanes, eao_plane_seg_plane());
    for (int p = 0; p < nPlanes; p++) {
        const pseg::FinalPlane& f = h->seg.planes[p];
        eao_plane_seg_plane& o = h->planes[p];
        std::memcpy(o.normal, f.normal, 24);
        std::memcpy(o.center, f.center, 24);
        o.mse = f.mse; o.curvature = f.curvature; o.N = f.N; o.rid = f.rid; o.kept = f.kept;
        std::memcpy(o.coef, f.coef, 16);
    }
    if ((st = device_tail(h, ctx, drain))) return st;
    const auto t4 = std::chrono::steady_clock::now();
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    h->stageUs[0] = us(t0, t1); h->stageUs[1] = us(t1, t2); h->stageUs[2] = us(t2, t3); h->stageUs[3] = us(t3, t4);
    h->haveTiming = h->profile;
    h->have = true;
    return EAO_OK;
}

eao_status eao_plane_seg_set_profiling(eao_plane_seg* h, int32_t on) {
    EAO_REQUIRE(h, "h is NULL");
    std::lock_guard<std::mutex> lock(h->mutex);
    h->profile = on != 0;
    h->haveTiming = false;
    return EAO_OK;
}

eao_status eao_plane_seg_last_timing(eao_plane_seg* h, double* us) {
    EAO_REQUIRE(h && us, "bad argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    EAO_REQUIRE(h->haveTiming, "eao_plane_seg_last_timing: no run with profiling on");
    for (int k = 0; k < 4; k++) us[k] = h->stageUs[k];
    return EAO_OK;
}

eao_status eao_plane_seg_info(eao_plane_seg* h, int32_t* n_planes, int32_t* n_points, int32_t* n_blocks, int32_t* n_claims) {
    EAO_REQUIRE(h, "h is NULL");
    std::lock_guard<std::mutex> lock(h->mutex);
    EAO_REQUIRE(h->have, "eao_plane_seg_info: no frame has run");
    if (n_planes) *n_planes = (int32_t)h->planes.size();
    if (n_points) *n_points = h->nVox;
    if (n_blocks) *n_blocks = h->nBlocks;
    if (n_claims) *n_claims = (int32_t)(h->seg.claims.size() / 2);
    return EAO_OK;
}

eao_status eao_plane_seg_planes(eao_plane_seg* h, int32_t cap, eao_plane_seg_plane* planes, int32_t* n) {
    EAO_REQUIRE(h && n, "bad argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    EAO_REQUIRE(h->have, "eao_plane_seg_planes: no frame has run");
    const int32_t cnt = (int32_t)h->planes.size();
    EAO_REQUIRE(!planes || cap >= cnt, "cap = %d is below the %d planes", cap, cnt);
    if (planes && cnt) std::memcpy(planes, h->planes.data(), (size_t)cnt * sizeof(eao_plane_seg_plane));
    *n = cnt;
    return EAO_OK;
}

eao_status eao_plane_seg_cloud(eao_plane_seg* h, int32_t plane, int32_t cap, float* xyz, int32_t* n) {
    EAO_REQUIRE(h && n, "bad argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    EAO_REQUIRE(h->have, "eao_plane_seg_cloud: no frame has run");
    EAO_REQUIRE(plane >= 0 && plane < (int32_t)h->planes.size(), "plane = %d is outside 0 .. %d", plane, (int)h->planes.size() - 1);
    const eao_plane_seg_plane& p = h->planes[plane];
    EAO_REQUIRE(!xyz || cap >= p.cloud_count, "cap = %d is below the cloud's %d points", cap, p.cloud_count);
    if (xyz && p.cloud_count > 0) {
        PsegCtx& ctx = g_pseg;
        eao_status st = ctx.ready(eao::StreamClass::Latency);
        if (st) return st;
        const size_t bytes = (size_t)p.cloud_count * 16;
        if ((st = ctx.host.reserve(bytes))) return st;
        eao::Drain drain(ctx.stream);
        EAO_HIP(hipMemcpyAsync(ctx.host.p, h->cloud.p + p.cloud_offset, bytes, hipMemcpyDeviceToHost, ctx.stream));
        EAO_HIP(drain.wait(eao::Drain::Latency));
        const float* q = (const float*)ctx.host.p;
        for (int32_t i = 0; i < p.cloud_count; i++) { xyz[3 * i] = q[4 * i]; xyz[3 * i + 1] = q[4 * i + 1]; xyz[3 * i + 2] = q[4 * i + 2]; }
    }
    *n = p.cloud_count;
    return EAO_OK;
}

eao_status eao_plane_seg_membership(eao_plane_seg* h, int32_t* image) {
    EAO_REQUIRE(h && image, "bad argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    EAO_REQUIRE(h->have, "eao_plane_seg_membership: no frame has run");
    PsegCtx& ctx = g_pseg;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const size_t bytes = (size_t)h->nPixels * 4;
    if ((st = ctx.host.reserve(bytes))) return st;
    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(ctx.host.p, h->member.p, bytes, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    std::memcpy(image, ctx.host.p, bytes);
    return EAO_OK;
}

eao_status eao_plane_seg_blocks(eao_plane_seg* h, int32_t cap, eao_plane_seg_block* blocks, int32_t* n) {
    EAO_REQUIRE(h && n, "bad argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    EAO_REQUIRE(h->have, "eao_plane_seg_blocks: no frame has run");
    EAO_REQUIRE(!blocks || cap >= h->nBlocks, "cap = %d is below the %d blocks", cap, h->nBlocks);
    if (blocks) std::memcpy(blocks, h->records.data(), (size_t)h->nBlocks * sizeof(eao_plane_seg_block));
    *n = h->nBlocks;
    return EAO_OK;
}

eao_status eao_plane_seg_middle(eao_plane_seg* h, int32_t* blk_map, int32_t cap_old, int32_t* plidmap, int32_t* n_old, int32_t cap_claims, int32_t* claims,
                                int32_t* n_claims) {
    EAO_REQUIRE(h && n_old && n_claims, "bad argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    EAO_REQUIRE(h->have, "eao_plane_seg_middle: no frame has run");
    const int32_t nOld = (int32_t)h->seg.plidmap.size(), nClaims = (int32_t)(h->seg.claims.size() / 2);
    EAO_REQUIRE(!plidmap || cap_old >= nOld, "cap_old = %d is below %d", cap_old, nOld);
    EAO_REQUIRE(!claims || cap_claims >= nClaims, "cap_claims = %d is below %d", cap_claims, nClaims);
    if (blk_map) std::memcpy(blk_map, h->seg.blkMap.data(), (size_t)h->nBlocks * 4);
    if (plidmap && nOld) std::memcpy(plidmap, h->seg.plidmap.data(), (size_t)nOld * 4);
    if (claims && nClaims) std::memcpy(claims, h->seg.claims.data(), (size_t)nClaims * 8);
    *n_old = nOld;
    *n_claims = nClaims;
    return EAO_OK;
}

}  // extern "C"
