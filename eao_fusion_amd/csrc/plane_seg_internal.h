// plane_seg_internal.h -- the host's share of eao_plane_seg_run (plane_seg.hip), free of HIP so that tools/plane_segmentation_walk.cpp and the CPU tests compile
// it with g++: what Frame::ComputePlanesFromPEAC does between the two passes over all pixels.  Reference: include/PEAC/AHCPlaneFitter.hpp (initGraph :784-953,
// ahCluster :981-1187, refineDetails :297-377, findBlockMembership :483-585, floodFill :426-474), AHCPlaneSeg.hpp (Stats::compute :125-156, the merge constructor
// :293-316, mergeNbsFrom :379-409), AHCParamSet.hpp (T_mse :87-99, T_ang :112-132, T_dz :144-146), DisjointSet.hpp, src/Frame.cc:349-371 and :425-456.
//
// In: one BlockRecord per window x window block (the device's k_ps_block_init, or block_record() below on the host) and the caller's depth image, from which the
// flood fill recomputes a point with pixel_point().  Out: the block map, the SPARSE list of pixels the flood fill claimed as (pixel, plane) pairs in ascending
// pixel order, plidmap, and the final planes.  No image leaves this header.
//
// The functions marked EAO_PSEG_HD are the ones the device runs too: pixel_valid, pixel_point, eig3_sym and fit are the same text for both compilers, built with
// -ffp-contract=off, and use + - * / sqrt in double only, so host and device agree bit for bit.
//
// Readings: an invalid pixel has z = 0 (get() false); std::pow(v, 2) is v * v; a neighbour set iterates in creation sequence (the node
// index), the queue orders by (mse, creation sequence), the size sort is stable, a NaN never enters the queue.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <set>
#include <utility>
#include <vector>

#include "../../include/eao_fusion.h"

#if defined(__HIPCC__)
#define EAO_PSEG_HD __host__ __device__ inline
#else
#define EAO_PSEG_HD inline
#endif

namespace eao {
namespace pseg {

constexpr int kJacobiSweeps = 8;
constexpr int kFlagMissing = 1, kFlagDiscontinuity = 2;      // bits of BlockRecord::flag; 0: the block holds window * window points
constexpr int kTrailStop = -6;                               // floodFill :443
constexpr double kDistFactor = 9, kDistEps = 1e-5;           // :453
constexpr double kSeenDist = 0.2, kSeenAngle = 0.9397;       // src/Frame.cc:362-365

// eao_plane_seg_block in the public header, field for field
struct BlockRecord {
    int32_t flag, N;
    double sums[9];      // sx sy sz sxx syy szz sxy syz sxz
    double center[3], normal[3], mse, curvature;
};
static_assert(sizeof(BlockRecord) == 144, "18 doubles");

// src/Frame.cc:396
EAO_PSEG_HD bool pixel_valid(double d, double dmin, double dmax) { return !(d != d || d > dmax || d < dmin); }
// src/Frame.cc:401-402: the Frame's float intrinsics promoted, left to right
EAO_PSEG_HD void pixel_point(float fx, float fy, float cx, float cy, int m, int n, double d, double& x, double& y) {
    x = ((double)n - (double)cx) * d / (double)fx;
    y = ((double)m - (double)cy) * d / (double)fy;
}

// Eigenvalues (ascending) and eigenvectors (columns of V) of the symmetric S: cyclic Jacobi over the pairs (0,1) (0,2) (1,2), kJacobiSweeps sweeps whatever the
// input (a NaN ends like any other), then three compare-exchanges.  S is destroyed.  Every index is a compile-time constant after unrolling.
EAO_PSEG_HD void eig3_sym(double (&S)[3][3], double (&l)[3], double (&V)[3][3]) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = S[p][q];
            double c = 1.0, s = 0.0;
            if (apq != 0.0) {
                const double theta = (S[q][q] - S[p][p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                c = 1.0 / sqrt(t * t + 1.0);
                s = t * c;
            }
            for (int k = 0; k < 3; k++) { const double a = S[k][p], b = S[k][q]; S[k][p] = c * a - s * b; S[k][q] = s * a + c * b; }
            for (int k = 0; k < 3; k++) { const double a = S[p][k], b = S[q][k]; S[p][k] = c * a - s * b; S[q][k] = s * a + c * b; }
            for (int k = 0; k < 3; k++) { const double a = V[k][p], b = V[k][q]; V[k][p] = c * a - s * b; V[k][q] = s * a + c * b; }
        }
    }
    l[0] = S[0][0]; l[1] = S[1][1]; l[2] = S[2][2];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < 3; e++) {
        const int a = e == 1 ? 1 : 0, b = a + 1;
        const bool sw = l[b] < l[a];
        const double t = l[a]; l[a] = sw ? l[b] : l[a]; l[b] = sw ? t : l[b];
        for (int k = 0; k < 3; k++) { const double u = V[k][a]; V[k][a] = sw ? V[k][b] : V[k][a]; V[k][b] = sw ? u : V[k][b]; }
    }
}

// Stats::compute, AHCPlaneSeg.hpp:125-156
EAO_PSEG_HD void fit(const double* sums, int N, double* center, double* normal, double& mse, double& curvature) {
    const double sx = sums[0], sy = sums[1], sz = sums[2], sxx = sums[3], syy = sums[4], szz = sums[5], sxy = sums[6], syz = sums[7], sxz = sums[8];
    const double sc = 1.0 / (double)N;
    center[0] = sx * sc; center[1] = sy * sc; center[2] = sz * sc;
    double K[3][3];
    K[0][0] = sxx - sx * sx * sc; K[0][1] = sxy - sx * sy * sc; K[0][2] = sxz - sx * sz * sc;
    K[1][1] = syy - sy * sy * sc; K[1][2] = syz - sy * sz * sc; K[2][2] = szz - sz * sz * sc;
    K[1][0] = K[0][1]; K[2][0] = K[0][2]; K[2][1] = K[1][2];
    double sv[3], V[3][3];
    eig3_sym(K, sv, V);
    if (V[0][0] * center[0] + V[1][0] * center[1] + V[2][0] * center[2] <= 0) {
        normal[0] = V[0][0]; normal[1] = V[1][0]; normal[2] = V[2][0];
    } else {
        normal[0] = -V[0][0]; normal[1] = -V[1][0]; normal[2] = -V[2][0];
    }
    mse = sv[0] * sc;
    curvature = sv[0] / (sv[0] + sv[1] + sv[2]);
}

inline double quiet_nan() {
    const uint64_t b = 0x7ff8000000000000ull;
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}

// AHCParamSet.hpp
inline double t_mse_init(const eao_plane_seg_cfg& c, double z) { const double v = c.depth_sigma * z * z + c.std_tol_init; return v * v; }
inline double t_mse_merge(const eao_plane_seg_cfg& c, double z) { const double v = c.depth_sigma * z * z + c.std_tol_merge; return v * v; }
inline double t_ang_init(const eao_plane_seg_cfg& c, double z) {
    double cz = z;
    cz = std::max(cz, c.z_near);
    cz = std::min(cz, c.z_far);
    const double factor = (c.angle_far - c.angle_near) / (c.z_far - c.z_near);
    return std::cos(factor * cz + c.angle_near - factor * c.z_near);
}
EAO_PSEG_HD double t_dz(double alpha, double tol, double z) { return alpha * fabs(z) + tol; }

// the block constructor, AHCPlaneSeg.hpp:211-285, on the host (the walk program; the device's k_ps_block_init computes the same record)
inline BlockRecord block_record(const eao_plane_seg_cfg& c, const float* depth, int stride, int bi, int bj) {
    BlockRecord r;
    std::memset(&r, 0, sizeof(r));
    const int w = c.window;
    int N = 0;
    for (int i = bi * w; i < bi * w + w; i++)
        for (int j = bj * w; j < bj * w + w; j++) {
            const double d = (double)depth[(size_t)i * stride + j];
            if (!pixel_valid(d, c.depth_min, c.depth_max)) { r.flag |= kFlagMissing; continue; }
            double x, y;
            pixel_point(c.fx, c.fy, c.cx, c.cy, i, j, d, x, y);
            if (j + 1 < c.width) {
                const double zn = (double)depth[(size_t)i * stride + j + 1];
                if (pixel_valid(zn, c.depth_min, c.depth_max) && fabs(d - zn) > t_dz(c.depth_alpha, c.depth_change_tol, d)) r.flag |= kFlagDiscontinuity;
            }
            if (i + 1 < c.height) {
                const double zn = (double)depth[(size_t)(i + 1) * stride + j];
                if (pixel_valid(zn, c.depth_min, c.depth_max) && fabs(d - zn) > t_dz(c.depth_alpha, c.depth_change_tol, d)) r.flag |= kFlagDiscontinuity;
            }
            r.sums[0] += x; r.sums[1] += y; r.sums[2] += d;
            r.sums[3] += x * x; r.sums[4] += y * y; r.sums[5] += d * d;
            r.sums[6] += x * y; r.sums[7] += y * d; r.sums[8] += x * d;
            N++;
        }
    if (r.flag || N < 4) {
        const int32_t flag = r.flag;
        std::memset(&r, 0, sizeof(r));
        r.flag = flag;
        r.mse = r.curvature = quiet_nan();
    } else {
        r.N = N;
        fit(r.sums, N, r.center, r.normal, r.mse, r.curvature);
    }
    return r;
}

struct DisjointSet {
    std::vector<int> parent, size;
    void reset(int n) {
        parent.resize(n); size.assign(n, 1);
        for (int i = 0; i < n; i++) parent[i] = i;
    }
    int find(int x) {
        int r = x;
        while (parent[r] != r) r = parent[r];
        while (parent[x] != r) { const int nx = parent[x]; parent[x] = r; x = nx; }
        return r;
    }
    int set_size(int x) { return size[find(x)]; }
    int unite(int x, int y) {
        const int xr = find(x), yr = find(y);
        if (xr == yr) return xr;
        if (size[xr] < size[yr]) { parent[xr] = yr; size[yr] += size[xr]; return yr; }
        parent[yr] = xr; size[xr] += size[yr];
        return xr;
    }
};

struct Node {
    int rid = 0, N = 0;
    double sums[9], center[3], normal[3], mse = 0, curvature = 0;
    bool nouse = false;
    std::set<int> nbs;      // node indices: the creation sequence
};

struct Merge { int rid_p, rid_nb, N; };

struct FinalPlane {
    double normal[3], center[3], mse, curvature;
    int32_t N, rid;
    float coef[4];
    int32_t kept;
};

inline double similarity(const Node& a, const Node& b) {
    return std::abs(a.normal[0] * b.normal[0] + a.normal[1] * b.normal[1] + a.normal[2] * b.normal[2]);
}

// src/Frame.cc:349-371 against the coefficients accepted so far, in order
inline bool plane_not_seen(const std::vector<const float*>& accepted, const float* coef) {
    for (const float* pM : accepted) {
        const float d = pM[3] - coef[3];
        const float angle = pM[0] * coef[0] + pM[1] * coef[1] + pM[2] * coef[2];
        if (d > kSeenDist || d < -kSeenDist) continue;
        if (angle < kSeenAngle && angle > -kSeenAngle) continue;
        return false;
    }
    return true;
}

// One frame's middle.  The vectors are kept between frames (a handle owns one Segmenter); run() starts every one of them over.
struct Segmenter {
    eao_plane_seg_cfg c;
    int Nh = 0, Nw = 0;
    DisjointSet ds;
    std::vector<Node> nodes;
    std::set<std::pair<double, int>> queue;      // (mse, node): begin() is upstream's top(), equal mse in creation sequence
    std::vector<int> extracted, old;             // node indices
    std::vector<Merge> merges;
    std::vector<int32_t> blkMap, plidmap, claims;      // claims: pixel, plane (an index into old), pixel, plane, ...
    std::vector<char> validPlane;
    std::vector<std::pair<int, int>> rf;
    std::vector<int32_t> trail;
    std::vector<float> dist;
    std::vector<FinalPlane> planes;
    int nInitial = 0, nEdges = 0, nSeeds = 0, nConnects = 0, nStopped = 0, nRetaken = 0, nMergesFirst = 0;

    void connect(int a, int b) { nodes[a].nbs.insert(b); nodes[b].nbs.insert(a); }
    void disconnect_all(int a) {
        for (int k : nodes[a].nbs) nodes[k].nbs.erase(a);
        nodes[a].nbs.clear();
    }

    // initGraph :784-953
    void init_graph(const BlockRecord* rec) {
        std::vector<int> G((size_t)Nh * Nw, -1);
        for (int b = 0; b < Nh * Nw; b++) {
            const BlockRecord& r = rec[b];
            if (r.flag == 0 && r.mse < t_mse_init(c, r.center[2])) {
                Node n;
                n.rid = b; n.N = r.N; n.mse = r.mse; n.curvature = r.curvature;
                std::memcpy(n.sums, r.sums, sizeof(n.sums));
                std::memcpy(n.center, r.center, sizeof(n.center));
                std::memcpy(n.normal, r.normal, sizeof(n.normal));
                G[b] = (int)nodes.size();
                queue.insert({n.mse, G[b]});
                nodes.push_back(n);
            }
        }
        nInitial = (int)nodes.size();
        for (int i = 0; i < Nh; i++)
            for (int j = 1; j < Nw; j += 2) {
                const int cidx = i * Nw + j;
                if (G[cidx - 1] < 0) { --j; continue; }
                if (G[cidx] < 0) continue;
                if (j < Nw - 1 && G[cidx + 1] < 0) { ++j; continue; }
                const double th = t_ang_init(c, nodes[G[cidx]].center[2]);
                if ((j < Nw - 1 && similarity(nodes[G[cidx - 1]], nodes[G[cidx + 1]]) >= th) || (j == Nw - 1 && similarity(nodes[G[cidx]], nodes[G[cidx - 1]]) >= th)) {
                    connect(G[cidx], G[cidx - 1]);
                    if (j < Nw - 1) connect(G[cidx], G[cidx + 1]);
                } else {
                    --j;
                }
            }
        for (int j = 0; j < Nw; j++)
            for (int i = 1; i < Nh; i += 2) {
                const int cidx = i * Nw + j;
                if (G[cidx - Nw] < 0) { --i; continue; }
                if (G[cidx] < 0) continue;
                if (i < Nh - 1 && G[cidx + Nw] < 0) { ++i; continue; }
                const double th = t_ang_init(c, nodes[G[cidx]].center[2]);
                if ((i < Nh - 1 && similarity(nodes[G[cidx - Nw]], nodes[G[cidx + Nw]]) >= th) || (i == Nh - 1 && similarity(nodes[G[cidx]], nodes[G[cidx - Nw]]) >= th)) {
                    connect(G[cidx], G[cidx - Nw]);
                    if (i < Nh - 1) connect(G[cidx], G[cidx + Nw]);
                } else {
                    --i;
                }
            }
        size_t e = 0;
        for (const Node& n : nodes) e += n.nbs.size();
        nEdges = (int)(e / 2);
    }

    // the merge constructor, AHCPlaneSeg.hpp:293-316
    static void merged(const Node& pa, const Node& pb, Node& m) {
        for (int k = 0; k < 9; k++) m.sums[k] = pa.sums[k] + pb.sums[k];
        m.N = pa.N + pb.N;
        m.nouse = false;
        m.rid = pa.N >= pb.N ? pa.rid : pb.rid;
        fit(m.sums, m.N, m.center, m.normal, m.mse, m.curvature);
    }

    // ahCluster :981-1187
    int cluster() {
        int step = 0;
        Node cand, m;
        while (!queue.empty() && step <= c.max_step) {
            const int pi = queue.begin()->second;
            queue.erase(queue.begin());
            if (nodes[pi].nouse) continue;
            bool have = false;
            int candNb = -1;
            for (int k : nodes[pi].nbs) {
                if (similarity(nodes[pi], nodes[k]) < c.similarity_merge) continue;
                merged(nodes[pi], nodes[k], m);
                if (!have || cand.mse > m.mse || (cand.mse == m.mse && cand.N < m.mse)) {      // (N against mse: upstream's comparison, :1043)
                    cand = m;
                    candNb = k;
                    have = true;
                }
            }
            if (have && cand.mse < t_mse_merge(c, cand.center[2])) {
                const int ni = (int)nodes.size();
                cand.nbs.clear();
                nodes.push_back(cand);
                queue.insert({cand.mse, ni});
                merges.push_back({nodes[pi].rid, nodes[candNb].rid, cand.N});
                ds.unite(nodes[pi].rid, nodes[candNb].rid);
                std::set<int> nb = nodes[pi].nbs;
                nb.insert(nodes[candNb].nbs.begin(), nodes[candNb].nbs.end());
                nb.erase(pi);
                nb.erase(candNb);
                disconnect_all(pi);
                disconnect_all(candNb);
                for (int k : nb) nodes[k].nbs.insert(ni);
                nodes[ni].nbs.swap(nb);
                nodes[pi].nouse = nodes[candNb].nouse = true;
            } else {
                if (nodes[pi].N >= c.min_support) extracted.push_back(pi);
                disconnect_all(pi);
            }
            ++step;
        }
        while (!queue.empty()) {
            const int pi = queue.begin()->second;
            queue.erase(queue.begin());
            if (nodes[pi].N >= c.min_support) extracted.push_back(pi);
            disconnect_all(pi);
        }
        std::stable_sort(extracted.begin(), extracted.end(), [&](int a, int b) { return nodes[b].N < nodes[a].N; });
        return step;
    }

    // findBlockMembership :483-585
    void block_membership() {
        const int w = c.window, W = c.width;
        std::vector<std::pair<int, int>> rid2plid;      // a handful of planes: a list searched in order stands for the std::map (first insertion wins)
        auto lookup = [&](int rid) {
            for (auto& e : rid2plid)
                if (e.first == rid) return e.second;
            rid2plid.push_back({rid, 0});      // operator[] on a missing key
            return 0;
        };
        for (int plid = 0; plid < (int)extracted.size(); plid++) {
            bool seen = false;
            for (auto& e : rid2plid) seen |= e.first == nodes[extracted[plid]].rid;
            if (!seen) rid2plid.push_back({nodes[extracted[plid]].rid, plid});
        }
        trail.assign((size_t)c.width * c.height, -1);
        blkMap.assign((size_t)Nh * Nw, 0);
        validPlane.assign(extracted.size(), 0);
        rf.clear();
        for (int i = 0, blkid = 0; i < Nh; i++)
            for (int j = 0; j < Nw; j++, blkid++) {
                const int setid = ds.find(blkid);
                if (ds.set_size(setid) * w * w >= c.min_support) {
                    int nbs[4], n = 0;
                    if (j > 0) nbs[n++] = blkid - 1;
                    if (j < Nw - 1) nbs[n++] = blkid + 1;
                    if (i > 0) nbs[n++] = blkid - Nw;
                    if (i < Nh - 1) nbs[n++] = blkid + Nw;
                    bool same = true;
                    for (int k = 0; k < n; k++)
                        if (ds.find(nbs[k]) != setid) { same = false; break; }      // ERODE_ALL_BORDER
                    const int plid = lookup(setid);
                    if (same) {
                        blkMap[blkid] = plid;
                        for (int y = i * w; y < (i + 1) * w; y++)
                            for (int x = j * w; x < (j + 1) * w; x++) trail[(size_t)y * W + x] = plid;
                        if (plid < (int)validPlane.size()) validPlane[plid] = 1;
                    } else {
                        blkMap[blkid] = -1;
                    }
                } else {
                    blkMap[blkid] = -1;
                }
                if (blkMap[blkid] < 0) {
                    if (i > 0 && blkMap[blkid - Nw] >= 0) {
                        const int s = (i * w - 1) * W + j * w;
                        for (int k = 1; k < w; k++) rf.push_back({s + k, blkMap[blkid - Nw]});
                    }
                    if (j > 0 && blkMap[blkid - 1] >= 0) {
                        const int s = (i * w) * W + j * w - 1;
                        for (int k = 0; k < w - 1; k++) rf.push_back({s + k * W, blkMap[blkid - 1]});
                    }
                } else {
                    const int plid = blkMap[blkid];
                    if (i > 0 && blkMap[blkid - Nw] != plid) {
                        const int s = (i * w) * W + j * w;
                        for (int k = 0; k < w - 1; k++) rf.push_back({s + k, plid});
                    }
                    if (j > 0 && blkMap[blkid - 1] != plid) {
                        const int s = (i * w) * W + j * w;
                        for (int k = 1; k < w; k++) rf.push_back({s + k * W, plid});
                    }
                }
            }
        nSeeds = (int)rf.size();
    }

    // floodFill :426-474
    void flood_fill(const float* depth, int stride) {
        const int W = c.width, H = c.height, w = c.window;
        dist.assign((size_t)W * H, std::numeric_limits<float>::max());
        for (size_t k = 0; k < rf.size(); k++) {
            const int s = rf[k].first, plid = rf[k].second;
            const int sy = s / W, sx = s - sy * W;
            const int pn = extracted[plid];
            int nbs[4], n = 0;
            if (sx > 0) nbs[n++] = s - 1;
            if (sx < W - 1) nbs[n++] = s + 1;
            if (sy > 0) nbs[n++] = s - W;
            if (sy < H - 1) nbs[n++] = s + W;
            for (int it = 0; it < n; it++) {
                const int ci = nbs[it];
                int32_t& t = trail[ci];
                if (t <= kTrailStop) { nStopped++; continue; }
                if (t >= 0 && t == plid) continue;
                const int cy = ci / W, cx = ci - cy * W;
                const int by = cy / w, bx = cx / w;
                if (by < Nh && bx < Nw && blkMap[by * Nw + bx] >= 0) continue;
                const double d = (double)depth[(size_t)cy * stride + cx];
                bool near = false;
                float cdist = -1;
                if (pixel_valid(d, c.depth_min, c.depth_max)) {
                    double x, y;
                    pixel_point(c.fx, c.fy, c.cx, c.cy, cy, cx, d, x, y);
                    const Node& pl = nodes[pn];
                    const double sd = pl.normal[0] * (x - pl.center[0]) + pl.normal[1] * (y - pl.center[1]) + pl.normal[2] * (d - pl.center[2]);
                    cdist = (float)std::abs(sd);
                    const double cd = (double)cdist;
                    near = cd * cd < kDistFactor * pl.mse + kDistEps;
                }
                if (near) {
                    if (t >= 0 && similarity(nodes[pn], nodes[extracted[t]]) >= c.similarity_refine) {
                        connect(extracted[t], pn);
                        nConnects++;
                    }
                    float& od = dist[ci];
                    if (cdist < od) {
                        if (t >= 0) nRetaken++;
                        t = plid;
                        od = cdist;
                        rf.push_back({ci, plid});
                    } else if (t < 0) {
                        t -= 1;
                    }
                } else if (t < 0) {
                    t -= 1;
                }
            }
        }
    }

    // eao_plane_seg_run's middle: run :209-258, refineDetails :297-377 and the per-plane coefficients of src/Frame.cc:425-456
    void run(const eao_plane_seg_cfg& cfg, const BlockRecord* rec, const float* depth, int stride) {
        c = cfg;
        Nh = c.height / c.window; Nw = c.width / c.window;
        ds.reset(Nh * Nw);
        nodes.clear(); queue.clear(); extracted.clear(); old.clear(); merges.clear(); planes.clear();
        nConnects = nStopped = nRetaken = 0;
        init_graph(rec);
        cluster();
        block_membership();
        flood_fill(depth, stride);
        old.swap(extracted);
        extracted.clear();
        for (size_t i = 0; i < old.size(); i++)
            if (validPlane[i]) queue.insert({nodes[old[i]].mse, old[i]});
        nMergesFirst = (int)merges.size();
        cluster();
        plidmap.assign(old.size(), -1);
        for (size_t i = 0; i < old.size(); i++) {
            if (!validPlane[i]) continue;
            const int rid = ds.find(nodes[old[i]].rid);
            for (size_t j = 0; j < extracted.size(); j++)
                if (rid == nodes[extracted[j]].rid) { plidmap[i] = (int32_t)j; break; }
        }
        // the pixels the fill claimed, once each, ascending, with their last owner
        std::vector<int32_t> px;
        px.reserve(rf.size() - nSeeds);
        for (size_t k = nSeeds; k < rf.size(); k++) px.push_back(rf[k].first);
        std::sort(px.begin(), px.end());
        px.erase(std::unique(px.begin(), px.end()), px.end());
        claims.clear();
        claims.reserve(px.size() * 2);
        for (int32_t p : px) { claims.push_back(p); claims.push_back(trail[p]); }
        std::vector<const float*> accepted;
        planes.resize(extracted.size());
        for (size_t j = 0; j < extracted.size(); j++) {
            const Node& n = nodes[extracted[j]];
            FinalPlane& f = planes[j];
            std::memcpy(f.normal, n.normal, 24);
            std::memcpy(f.center, n.center, 24);
            f.mse = n.mse; f.curvature = n.curvature; f.N = n.N; f.rid = n.rid;
            const float d = (float)-(n.normal[0] * n.center[0] + n.normal[1] * n.center[1] + n.normal[2] * n.center[2]);
            f.coef[0] = (float)n.normal[0]; f.coef[1] = (float)n.normal[1]; f.coef[2] = (float)n.normal[2]; f.coef[3] = d;
            if (f.coef[3] < 0)
                for (int k = 0; k < 4; k++) f.coef[k] = -f.coef[k];
            f.kept = plane_not_seen(accepted, f.coef) ? 1 : 0;
            if (f.kept) accepted.push_back(f.coef);
        }
    }
};

}  // namespace pseg

}  // namespace eao
