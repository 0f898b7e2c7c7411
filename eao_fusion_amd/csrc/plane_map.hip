// plane_map.hip -- the boundary clouds of the map's planes on the device and the plane association over them (include/eao_fusion.h, "MapPlane boundaries";
// reference src/Map.cc:155-292, src/MapPlane.cc:34-37, :150-153): Map::AssociatePlanesByBoundary and Map::SearchMatchedPlanes upload the frame's plane
// coefficients and download one index per plane.
//
// Resident: one arena of points, 16 bytes each (x, y, z, 0), appended to by add / update_boundary.  The table (id, offset, count, world position per plane) is
// the host's (plane_map_internal.h); a query uploads one 32-byte record per candidate, so nothing on the device goes stale when a plane moves or leaves.
// Growth and compaction are the policy of resident_arena.h, carried out by dev_arena.h.
//
// k_pm_transform   pcl::transformPointCloud(cloud, out, T.inverse().matrix()): one thread per point, double, rounded once per coordinate
// k_pm_min_dist    one workgroup per (candidate, chunk of 512 of its points): the query rows (world-frame coefficients) and this candidate's gate flags in LDS,
//                  two points per lane in registers (one 16-byte load each), running minima for a tile of 8 rows in registers, a shuffle minimum over the
//                  wavefront, LDS over the four wavefronts, one integer atomicMin per (row, candidate) on the float's bit pattern.  A distance is |..| and
//                  a NaN never enters a minimum (strict <, as upstream), so every value is a non-negative non-NaN float, for which unsigned order is float
//                  order; a minimum is exact and order-free, so the result does not depend on the schedule.
// k_pm_select      upstream's sequential selection (strict <, candidate order), one thread per row.
// Compiled with -ffp-contract=off: every float expression is rounded operation by operation, left to right, as the reference's.
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "dev_arena.h"
#include "lm_internal.h"      // se3_from_Tcw_f32, quat_to_matrix: Converter::toSE3Quat and the isometry it becomes
#include "plane_map_internal.h"
#include "plane_seg_shared.h"      // plane_seg_kept_cloud: the *_from_seg entry points

namespace pmap = eao::pmap;
static_assert(pmap::kMaxRows == EAO_PLANE_MAP_MAX_ROWS && pmap::kMaxPointsPerPlane == EAO_PLANE_MAP_MAX_POINTS &&
              pmap::kMaxCandidates == EAO_PLANE_MAP_MAX_CANDIDATES, "the caps of the header are the table's");

namespace {
constexpr size_t kInitialPoints = 1 << 13;      // 128 KiB of arena; doubles from there
}  // namespace

struct eao_plane_map {
    std::mutex mutex;      // upstream's mMutexMap around both loops, widened to every call
    pmap::Table table;
    eao::DevArena<float4> pts{kInitialPoints};      // the arena (check_cloud bounds the points in use, so the doubling needs no clamp)
};

namespace {

constexpr int kRowTile = 8;                     // rows whose minima a lane keeps in registers at a time
constexpr unsigned kNoDistanceBits = 0x42C80000u;      // 100.0f
static_assert(pmap::kChunk == 512, "k_pm_min_dist holds two points per lane of 256");

struct Xf {      // rows 0..2 of T.inverse().matrix(), double
    double m[12];
};

// xyz: `stride` floats per point (3: the caller's packed points; 4: a segmentation handle's cloud)
__global__ __launch_bounds__(256) void k_pm_transform(int n, const float* __restrict__ xyz, int stride, Xf X, int identity, float4* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[stride * (size_t)i], y = xyz[stride * (size_t)i + 1], z = xyz[stride * (size_t)i + 2];
    float4 o;
    if (identity) {
        o = make_float4(x, y, z, 0.0f);
    } else {
        const double dx = x, dy = y, dz = z;
        o.x = (float)(X.m[0] * dx + X.m[1] * dy + X.m[2] * dz + X.m[3]);
        o.y = (float)(X.m[4] * dx + X.m[5] * dy + X.m[6] * dz + X.m[7]);
        o.z = (float)(X.m[8] * dx + X.m[9] * dy + X.m[10] * dz + X.m[11]);
        o.w = 0.0f;
    }
    out[i] = o;
}

__global__ __launch_bounds__(256) void k_pm_read(int n, const float4* __restrict__ in, float* __restrict__ xyz) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    xyz[3 * (size_t)i] = p.x; xyz[3 * (size_t)i + 1] = p.y; xyz[3 * (size_t)i + 2] = p.z;
}

__device__ __forceinline__ float wave_min(float v) {      // values are never NaN here
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// dynamic LDS: nRows float4 (the rows), then nRows bytes (this candidate's gate flags), then cdiv(nRows, 8) bytes (a tile has a gated row)
__global__ __launch_bounds__(256) void k_pm_min_dist(int nRows, int nCand, const float4* __restrict__ rows, const pmap::Cand* __restrict__ cands,
                                                     const pmap::Work* __restrict__ work, const float4* __restrict__ pts, float angleTh,
                                                     unsigned* __restrict__ disBits, unsigned char* __restrict__ gatedOut) {
    extern __shared__ float4 sRow[];
    unsigned char* sGate = (unsigned char*)(sRow + nRows);
    unsigned char* sTile = sGate + nRows;
    __shared__ float sMin[4][kRowTile];
    const pmap::Work w = work[blockIdx.x];
    const pmap::Cand c = cands[w.cand];
    const int nTiles = (nRows + kRowTile - 1) / kRowTile;
    for (int r = threadIdx.x; r < nRows; r += 256) {
        const float4 pM = rows[r];
        sRow[r] = pM;
        const float angle = pM.x * c.world[0] + pM.y * c.world[1] + pM.z * c.world[2];      // src/Map.cc:179-181
        const bool g = angle > angleTh || angle < -angleTh;                                 // :187; a NaN passes neither
        sGate[r] = g;
        if (w.chunk == 0) gatedOut[(size_t)r * nCand + w.cand] = g;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nTiles; t += 256) {
        unsigned char any = 0;
        for (int k = 0; k < kRowTile && t * kRowTile + k < nRows; k++) any |= sGate[t * kRowTile + k];
        sTile[t] = any;
    }
    __syncthreads();
    if (c.count == 0) return;      // PointDistanceFromPlane over no points: 100, which the matrix holds already
    // two points per lane, each one 16-byte load; a lane past the cloud's end holds nothing
    const unsigned i0 = w.chunk * (unsigned)pmap::kChunk + threadIdx.x, i1 = i0 + 256;
    const bool h0 = i0 < c.count, h1 = i1 < c.count;
    float4 p0 = make_float4(0, 0, 0, 0), p1 = p0;
    if (h0) p0 = pts[(size_t)c.begin + i0];
    if (h1) p1 = pts[(size_t)c.begin + i1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = 0; t < nTiles; t++) {
        if (!sTile[t]) continue;      // (uniform over the workgroup)
        float m[kRowTile];
#pragma unroll
        for (int k = 0; k < kRowTile; k++) {
            m[k] = pmap::kNoDistance;
            const int r = t * kRowTile + k;
            if (r < nRows && sGate[r]) {      // (uniform)
                const float4 pM = sRow[r];
                // src/Map.cc:225-230: abs(float expression), left to right; strict <, so a NaN never wins
                const float d0 = fabsf(pM.x * p0.x + pM.y * p0.y + pM.z * p0.z + pM.w);
                const float d1 = fabsf(pM.x * p1.x + pM.y * p1.y + pM.z * p1.z + pM.w);
                if (h0 && d0 < m[k]) m[k] = d0;
                if (h1 && d1 < m[k]) m[k] = d1;
            }
        }
#pragma unroll
        for (int k = 0; k < kRowTile; k++) m[k] = wave_min(m[k]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kRowTile; k++) sMin[wave][k] = m[k];
        }
        __syncthreads();
        if (threadIdx.x < kRowTile) {
            const int r = t * kRowTile + threadIdx.x;
            if (r < nRows && sGate[r]) {
                float v = sMin[0][threadIdx.x];
                for (int q = 1; q < 4; q++) v = sMin[q][threadIdx.x] < v ? sMin[q][threadIdx.x] : v;
                // non-negative and not NaN: the unsigned order of the bit patterns is the float order
                if (v < pmap::kNoDistance) atomicMin(disBits + (size_t)r * nCand + w.cand, __float_as_uint(v));
            }
        }
        __syncthreads();
    }
}

// src/Map.cc:173-203 / :264-290 for one row per thread
__global__ __launch_bounds__(256) void k_pm_select(int nRows, int nCand, const float* __restrict__ dis, const unsigned char* __restrict__ gated, float disTh,
                                                   int* __restrict__ match, float* __restrict__ matchDis) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nRows) return;
    float ldTh = disTh;
    int best = -1;
    for (int j = 0; j < nCand; j++) {
        const float d = dis[(size_t)r * nCand + j];
        if (gated[(size_t)r * nCand + j] && d < ldTh) {
            ldTh = d;
            best = j;
        }
    }
    match[r] = best;
    matchDis[r] = ldTh;
}

struct PmapCtx : eao::ThreadStream {
    eao::DevBuf<unsigned char> dev;
    eao::PinBuf<hipHostMallocDefault> host;
};
thread_local PmapCtx g_pmap;

// T.inverse().matrix() of Eigen::Isometry3d T = Converter::toSE3Quat(Tcw) (src/MapPlane.cc:34-36): the unit quaternion of the rotation block and the
// translation, as a rotation matrix again, inverted as R^T, -(R^T t)
Xf inverse_isometry(const float* Tcw) {
    const SE3 s = se3_from_Tcw_f32(Tcw);
    double R[9];
    quat_to_matrix(s.r, R);
    Xf X;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) X.m[i * 4 + j] = R[j * 3 + i];
        X.m[i * 4 + 3] = -(R[0 * 3 + i] * s.t[0] + R[1 * 3 + i] * s.t[1] + R[2 * 3 + i] * s.t[2]);
    }
    return X;
}

// n points in device memory, `stride` floats apart, through the transform into the arena at `begin` (reserved by the caller); the handle's mutex is held.
// Enqueues only: the caller waits.
eao_status transform_into(eao_plane_map* pm, PmapCtx& ctx, uint64_t begin, int32_t n, const float* devXyz, int stride, const float* Tcw) {
    Xf X = Xf();
    if (Tcw) X = inverse_isometry(Tcw);
    hipLaunchKernelGGL(k_pm_transform, dim3(eao::cdiv(n, 256)), dim3(256), 0, ctx.stream, n, devXyz, stride, X, Tcw ? 0 : 1, pm->pts.at() + begin);
    EAO_HIP(hipGetLastError());
    return EAO_OK;
}

// n points of the caller's through this thread's staging block into device memory
eao_status upload_cloud(PmapCtx& ctx, int32_t n, const float* xyz) {
    const size_t bytes = (size_t)n * 12;
    eao_status st;
    if ((st = ctx.dev.reserve(bytes))) return st;
    if ((st = ctx.host.reserve(bytes))) return st;
    std::memcpy(ctx.host.p, xyz, bytes);
    EAO_HIP(hipMemcpyAsync(ctx.dev.p, ctx.host.p, bytes, hipMemcpyHostToDevice, ctx.stream));
    return EAO_OK;
}

// where a cloud comes from: the caller's n packed points at xyz, or (seg != NULL) the voxel cloud of a segmentation handle's kept plane, device to device
struct CloudSource {
    int32_t n;
    const float* xyz;
    eao_plane_seg* seg;
    int32_t plane;
};

// The one body of add (isAdd) and update_boundary and of their *_from_seg forms.  `name` is the entry point's, in front of what check_cloud objects to.
eao_status store(eao_plane_map* pm, const char* name, bool isAdd, uint64_t id, const float* world_pos, const CloudSource& src, const float* Tcw) {
    std::lock_guard<std::mutex> lock(pm->mutex);
    std::unique_lock<std::mutex> segLock;      // (always taken after the map's: nothing in plane_seg.hip takes a map's mutex)
    eao_plane_seg* const seg = src.seg;
    const float *xyz = src.xyz, *devXyz = nullptr;
    int32_t n = src.n;
    eao_status st;
    if (seg && (st = eao::plane_seg_kept_cloud(seg, src.plane, segLock, &devXyz, &n))) return st;
    const std::string err = pm->table.check_cloud(id, n, isAdd);
    EAO_REQUIRE(err.empty(), "%s: %s", name, err.c_str());
    EAO_REQUIRE(seg || n == 0 || xyz, "xyz is NULL");
    PmapCtx& ctx = g_pmap;
    if ((st = ctx.ready(eao::StreamClass::Latency))) return st;
    const uint64_t begin = pm->table.used;
    if ((st = pm->pts.reserve(begin + (uint64_t)n, begin, ctx.stream))) return st;
    if (n > 0) {
        eao::Drain drain(ctx.stream);
        if (!seg) {
            if ((st = upload_cloud(ctx, n, xyz))) return st;
            devXyz = (const float*)ctx.dev.p;
        }
        if ((st = transform_into(pm, ctx, begin, n, devXyz, seg ? 4 : 3, Tcw))) return st;
        EAO_HIP(drain.wait(eao::Drain::Block));
    }
    // (only now: a failed call leaves the table as it was)
    if (isAdd) {
        pm->table.append(id, (uint32_t)n, world_pos);
        return EAO_OK;
    }
    pm->table.replace(id, (uint32_t)n);
    return eao::compact_if_wanted(ctx, pm->table, pm->pts);
}

}  // namespace

extern "C" {

eao_status eao_plane_map_create(eao_plane_map** out) {
    EAO_REQUIRE(out, "out is NULL");
    const eao_status st = eao::require_device();
    if (st) return st;
    *out = new eao_plane_map;
    return EAO_OK;
}

void eao_plane_map_destroy(eao_plane_map* pm) { delete pm; }

eao_status eao_plane_map_clear(eao_plane_map* pm) {
    EAO_REQUIRE(pm, "pm is NULL");
    std::lock_guard<std::mutex> lock(pm->mutex);
    pm->table.clear();      // (the allocation stays)
    return EAO_OK;
}

eao_status eao_plane_map_info(eao_plane_map* pm, int32_t* n_live, int64_t* n_points_in_use, int64_t* arena_capacity) {
    EAO_REQUIRE(pm, "pm is NULL");
    std::lock_guard<std::mutex> lock(pm->mutex);
    if (n_live) *n_live = pm->table.nLive;
    if (n_points_in_use) *n_points_in_use = (int64_t)pm->table.used;
    if (arena_capacity) *arena_capacity = (int64_t)pm->pts.cap;
    return EAO_OK;
}

eao_status eao_plane_map_add(eao_plane_map* pm, uint64_t id, const float* world_pos, int32_t n, const float* xyz, const float* Tcw) {
    EAO_REQUIRE(pm && world_pos, "bad argument");
    return store(pm, "eao_plane_map_add", true, id, world_pos, CloudSource{n, xyz, nullptr, 0}, Tcw);
}

eao_status eao_plane_map_update_boundary(eao_plane_map* pm, uint64_t id, int32_t n, const float* xyz, const float* Tcw) {
    EAO_REQUIRE(pm, "pm is NULL");
    return store(pm, "eao_plane_map_update_boundary", false, id, nullptr, CloudSource{n, xyz, nullptr, 0}, Tcw);
}

eao_status eao_plane_map_add_from_seg(eao_plane_map* pm, uint64_t id, const float* world_pos, eao_plane_seg* seg, int32_t plane, const float* Tcw) {
    EAO_REQUIRE(pm && world_pos && seg, "bad argument");
    return store(pm, "eao_plane_map_add_from_seg", true, id, world_pos, CloudSource{0, nullptr, seg, plane}, Tcw);
}

eao_status eao_plane_map_update_boundary_from_seg(eao_plane_map* pm, uint64_t id, eao_plane_seg* seg, int32_t plane, const float* Tcw) {
    EAO_REQUIRE(pm && seg, "bad argument");
    return store(pm, "eao_plane_map_update_boundary_from_seg", false, id, nullptr, CloudSource{0, nullptr, seg, plane}, Tcw);
}

eao_status eao_plane_map_set_world_pos(eao_plane_map* pm, uint64_t id, const float* world_pos) {
    EAO_REQUIRE(pm && world_pos, "bad argument");
    std::lock_guard<std::mutex> lock(pm->mutex);
    EAO_REQUIRE(pm->table.find(id), "eao_plane_map_set_world_pos: plane %llu is not held", (unsigned long long)id);
    pm->table.set_world(id, world_pos);
    return EAO_OK;
}

eao_status eao_plane_map_erase(eao_plane_map* pm, uint64_t id) {
    EAO_REQUIRE(pm, "pm is NULL");
    std::lock_guard<std::mutex> lock(pm->mutex);
    if (!pm->table.erase(id)) return EAO_OK;      // unknown: a no-op, as std::set::erase (src/Map.cc:150)
    return eao::compact_if_wanted(g_pmap, pm->table, pm->pts);
}

eao_status eao_plane_map_boundary(eao_plane_map* pm, uint64_t id, int32_t cap, float* xyz, int32_t* n, float* world_pos) {
    EAO_REQUIRE(pm && n, "bad argument");
    std::lock_guard<std::mutex> lock(pm->mutex);
    const pmap::Entry* e = pm->table.find(id);
    EAO_REQUIRE(e, "eao_plane_map_boundary: plane %llu is not held", (unsigned long long)id);
    const int32_t cnt = (int32_t)e->count;
    EAO_REQUIRE(!xyz || cap >= cnt, "cap = %d is below the cloud's %d points", cap, cnt);
    if (xyz && cnt > 0) {
        PmapCtx& ctx = g_pmap;
        eao_status st = ctx.ready(eao::StreamClass::Latency);
        if (st) return st;
        const size_t bytes = (size_t)cnt * 12;
        if ((st = ctx.dev.reserve(bytes))) return st;
        if ((st = ctx.host.reserve(bytes))) return st;
        eao::Drain drain(ctx.stream);
        hipLaunchKernelGGL(k_pm_read, dim3(eao::cdiv(cnt, 256)), dim3(256), 0, ctx.stream, cnt, (const float4*)(pm->pts.at() + e->begin), (float*)ctx.dev.p);
        EAO_HIP(hipGetLastError());
        EAO_HIP(hipMemcpyAsync(ctx.host.p, ctx.dev.p, bytes, hipMemcpyDeviceToHost, ctx.stream));
        EAO_HIP(drain.wait(eao::Drain::Block));
        std::memcpy(xyz, ctx.host.p, bytes);
    }
    *n = cnt;
    if (world_pos) std::memcpy(world_pos, e->world, 16);
    return EAO_OK;
}

eao_status eao_plane_map_associate(eao_plane_map* pm, int32_t n_sets, const float* M, const int32_t* set_start, const float* coef, int32_t n_cand,
                                   const uint64_t* cand_id, float dis_th, float angle_th, int32_t* match, float* match_dis, float* world_coef, float* dis,
                                   uint8_t* gated) {
    EAO_REQUIRE(pm, "pm is NULL");
    EAO_REQUIRE(n_sets >= 0 && (n_sets == 0 || (M && set_start)), "bad sets");
    int32_t nRows = 0;
    if (n_sets > 0) {
        EAO_REQUIRE(set_start[0] == 0, "set_start[0] != 0");
        for (int32_t s = 0; s < n_sets; s++) EAO_REQUIRE(set_start[s] <= set_start[s + 1], "set_start does not ascend at entry %d", s);
        nRows = set_start[n_sets];
    }
    EAO_REQUIRE(nRows <= EAO_PLANE_MAP_MAX_ROWS, "%d rows; at most %d per call are supported", nRows, EAO_PLANE_MAP_MAX_ROWS);
    EAO_REQUIRE(nRows == 0 || (coef && match && match_dis), "coef, match or match_dis is NULL");
    EAO_REQUIRE(n_cand >= 0 && n_cand <= EAO_PLANE_MAP_MAX_CANDIDATES, "n_cand = %d is outside 0 .. %d", n_cand, EAO_PLANE_MAP_MAX_CANDIDATES);
    std::lock_guard<std::mutex> lock(pm->mutex);
    EAO_REQUIRE(cand_id || n_cand == 0 || n_cand == pm->table.nLive, "cand_id is NULL (every live plane) and n_cand = %d is not the %d live planes", n_cand, pm->table.nLive);
    std::vector<pmap::Cand> cands;
    std::vector<uint64_t> ids;
    const std::string err = pmap::resolve_candidates(pm->table, n_cand, cand_id, cands, ids);
    EAO_REQUIRE(err.empty(), "eao_plane_map_associate: %s", err.c_str());
    const int64_t nPairs = (int64_t)nRows * n_cand;
    EAO_REQUIRE(nPairs <= pmap::kMaxPairs, "%lld pairs; at most %lld per call are supported", (long long)nPairs, (long long)pmap::kMaxPairs);
    if (nRows == 0) return EAO_OK;

    PmapCtx& ctx = g_pmap;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    std::vector<pmap::Work> work;
    pmap::plan_work(cands, work);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = eao::align256(o + bytes); return at; };
    const size_t oRows = take((size_t)nRows * 16), oCand = take(cands.size() * sizeof(pmap::Cand)), oWork = take(work.size() * sizeof(pmap::Work)), inEnd = o;
    const size_t oMatch = take((size_t)nRows * 4), oMatchDis = take((size_t)nRows * 4), oDis = take((size_t)nPairs * 4), oGated = take((size_t)nPairs), end = o;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    float* hRows = (float*)(h + oRows);
    for (int32_t s = 0; s < n_sets; s++)
        for (int32_t r = set_start[s]; r < set_start[s + 1]; r++) pmap::world_coefficients(M + 16 * (size_t)s, coef + 4 * (size_t)r, hRows + 4 * (size_t)r);
    if (n_cand > 0) {
        std::memcpy(h + oCand, cands.data(), cands.size() * sizeof(pmap::Cand));
        std::memcpy(h + oWork, work.data(), work.size() * sizeof(pmap::Work));
    }
    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    if (n_cand > 0) {
        EAO_HIP(hipMemsetD32Async((hipDeviceptr_t)(d + oDis), (int)kNoDistanceBits, (size_t)nPairs, ctx.stream));
        const size_t lds = (size_t)nRows * 17 + (size_t)eao::cdiv(nRows, kRowTile);
        hipLaunchKernelGGL(k_pm_min_dist, dim3((unsigned)work.size()), dim3(256), lds, ctx.stream, nRows, n_cand, (const float4*)(d + oRows),
                           (const pmap::Cand*)(d + oCand), (const pmap::Work*)(d + oWork), (const float4*)pm->pts.at(), angle_th, (unsigned*)(d + oDis), d + oGated);
        EAO_HIP(hipGetLastError());      // (no selection over distances that were not computed)
    }
    hipLaunchKernelGGL(k_pm_select, dim3(eao::cdiv(nRows, 256)), dim3(256), 0, ctx.stream, nRows, n_cand, (const float*)(d + oDis), d + oGated, dis_th,
                       (int*)(d + oMatch), (float*)(d + oMatchDis));
    EAO_HIP(hipGetLastError());
    const bool full = n_cand > 0 && (dis || gated);
    EAO_HIP(hipMemcpyAsync(h + oMatch, d + oMatch, (full ? end : oDis) - oMatch, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    std::memcpy(match, h + oMatch, (size_t)nRows * 4);
    std::memcpy(match_dis, h + oMatchDis, (size_t)nRows * 4);
    if (world_coef) std::memcpy(world_coef, hRows, (size_t)nRows * 16);
    if (dis && n_cand > 0) std::memcpy(dis, h + oDis, (size_t)nPairs * 4);
    if (gated && n_cand > 0) std::memcpy(gated, h + oGated, (size_t)nPairs);
    return EAO_OK;
}

}  // extern "C"
