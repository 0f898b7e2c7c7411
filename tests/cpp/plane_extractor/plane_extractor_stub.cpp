// A stand-in for libeaofusion_hip.so's plane-segmentation entry points that needs no device: it prints every call it receives and answers by a made-up rule, so
// that the CPU suite can check what include/eaofusion/PlaneExtractor.h sends and what it does with the answer (tests/test_plane_extractor_class_cpu.py restates
// the rule).  A run "extracts" three planes: plane i has coef (i, 10 + i, 20 + i, 30 + i), a cloud of i + 1 points (100 i + k, 100 i + k + 0.25, 100 i + k + 0.5)
// and is kept unless i == 1.  A depth image whose first pixel is negative is refused.
#include <cstdio>
#include <cstring>

#include <eao_fusion.h>

struct eao_plane_seg { eao_plane_seg_cfg cfg; int runs = 0; };
struct eao_plane_map { int dummy; };

extern "C" {

const char* eao_last_error(void) { return "stub"; }

void eao_plane_seg_cfg_default(eao_plane_seg_cfg* c, int32_t w, int32_t h, float fx, float fy, float cx, float cy) {
    std::memset(c, 0, sizeof(*c));
    c->width = w; c->height = h; c->fx = fx; c->fy = fy; c->cx = cx; c->cy = cy;
    c->window = 10; c->min_support = 3000;
    printf("cfg_default %d %d %.9g %.9g %.9g %.9g\n", w, h, fx, fy, cx, cy);
}
eao_status eao_plane_seg_create(const eao_plane_seg_cfg* c, eao_plane_seg** out) {
    printf("create %d %d window %d min_support %d\n", c->width, c->height, c->window, c->min_support);
    *out = new eao_plane_seg;
    (*out)->cfg = *c;
    return EAO_OK;
}
void eao_plane_seg_destroy(eao_plane_seg* h) {
    printf("destroy %d\n", h->cfg.width);
    delete h;
}
eao_status eao_plane_seg_run(eao_plane_seg* h, const float* depth, int32_t stride) {
    printf("run stride %d first %.9g last %.9g\n", stride, depth[0], depth[(size_t)(h->cfg.height - 1) * stride + h->cfg.width - 1]);
    if (depth[0] < 0) return EAO_ERR_INVALID;
    h->runs++;
    return EAO_OK;
}
eao_status eao_plane_seg_planes(eao_plane_seg*, int32_t cap, eao_plane_seg_plane* planes, int32_t* n) {
    printf("planes cap %d %s\n", cap, planes ? "table" : "count");
    if (planes) {
        for (int i = 0; i < 3; i++) {
            std::memset(&planes[i], 0, sizeof(planes[i]));
            for (int k = 0; k < 4; k++) planes[i].coef[k] = (float)(10 * k + i);
            planes[i].kept = i != 1;
            planes[i].cloud_count = i + 1;
        }
    }
    *n = 3;
    return EAO_OK;
}
eao_status eao_plane_seg_cloud(eao_plane_seg*, int32_t plane, int32_t cap, float* xyz, int32_t* n) {
    printf("cloud %d cap %d\n", plane, cap);
    for (int k = 0; k <= plane; k++) { xyz[3 * k] = 100.f * plane + k; xyz[3 * k + 1] = 100.f * plane + k + 0.25f; xyz[3 * k + 2] = 100.f * plane + k + 0.5f; }
    *n = plane + 1;
    return EAO_OK;
}
static void floats(const char* tag, const float* p, int n) {
    printf(" %s", tag);
    for (int i = 0; i < n; i++) printf(" %.9g", p[i]);
}
eao_status eao_plane_map_add_from_seg(eao_plane_map*, uint64_t id, const float* w, eao_plane_seg* seg, int32_t plane, const float* Tcw) {
    printf("add_from_seg %llu plane %d seg %d", (unsigned long long)id, plane, seg->cfg.width);
    floats("w", w, 4);
    floats("T", Tcw, 16);
    printf("\n");
    return id == 666 ? EAO_ERR_INVALID : EAO_OK;
}
eao_status eao_plane_map_update_boundary_from_seg(eao_plane_map*, uint64_t id, eao_plane_seg* seg, int32_t plane, const float* Tcw) {
    printf("update_from_seg %llu plane %d seg %d", (unsigned long long)id, plane, seg->cfg.width);
    floats("T", Tcw, 16);
    printf("\n");
    return EAO_OK;
}

}  // extern "C"
