// A stand-in for libeaofusion_hip.so's plane-map entry points that needs no device: it prints every call it receives and answers by a made-up rule, so that the
// CPU suite can check what include/eaofusion/MapPlanes.h sends and what it does with the answer (tests/test_map_planes_class_cpu.py restates the rule).
//   associate: row i of the call matches candidate n_cand - 1 - (i / 2) % n_cand when i is even and nothing (-1) when i is odd or there are no candidates.
//   add: an id that is held is EAO_ERR_INVALID, as in the library.
#include <algorithm>
#include <cstdio>
#include <vector>

#include <eao_fusion.h>

struct eao_plane_map {
    std::vector<uint64_t> held;
};

static void floats(const char* tag, const float* p, int n) {
    printf(" %s", tag);
    for (int i = 0; i < n; i++) printf(" %.9g", p[i]);
}

extern "C" {

const char* eao_last_error(void) { return "stub"; }

eao_status eao_plane_map_create(eao_plane_map** out) {
    printf("create\n");
    *out = new eao_plane_map;
    return EAO_OK;
}
void eao_plane_map_destroy(eao_plane_map* pm) {
    printf("destroy\n");
    delete pm;
}
eao_status eao_plane_map_clear(eao_plane_map* pm) {
    printf("clear\n");
    pm->held.clear();
    return EAO_OK;
}
eao_status eao_plane_map_add(eao_plane_map* pm, uint64_t id, const float* w, int32_t n, const float* xyz, const float* Tcw) {
    printf("add %llu", (unsigned long long)id);
    floats("w", w, 4);
    printf(" n %d", n);
    floats("xyz", xyz, 3 * n);
    floats("T", Tcw, 16);
    printf("\n");
    if (std::find(pm->held.begin(), pm->held.end(), id) != pm->held.end()) return EAO_ERR_INVALID;
    pm->held.push_back(id);
    return EAO_OK;
}
eao_status eao_plane_map_update_boundary(eao_plane_map*, uint64_t id, int32_t n, const float* xyz, const float* Tcw) {
    printf("update %llu n %d", (unsigned long long)id, n);
    floats("xyz", xyz, 3 * n);
    floats("T", Tcw, 16);
    printf("\n");
    return EAO_OK;
}
eao_status eao_plane_map_set_world_pos(eao_plane_map*, uint64_t id, const float* w) {
    printf("setw %llu", (unsigned long long)id);
    floats("w", w, 4);
    printf("\n");
    return EAO_OK;
}
eao_status eao_plane_map_erase(eao_plane_map* pm, uint64_t id) {
    printf("erase %llu\n", (unsigned long long)id);
    pm->held.erase(std::remove(pm->held.begin(), pm->held.end(), id), pm->held.end());
    return EAO_OK;
}
eao_status eao_plane_map_associate(eao_plane_map*, int32_t n_sets, const float* M, const int32_t* set_start, const float* coef, int32_t n_cand,
                                   const uint64_t* cand_id, float dis_th, float angle_th, int32_t* match, float* match_dis, float* world_coef, float* dis,
                                   uint8_t* gated) {
    printf("associate sets %d start", n_sets);
    for (int s = 0; s <= n_sets; s++) printf(" %d", set_start[s]);
    floats("M", M, 16 * n_sets);
    floats("coef", coef, 4 * set_start[n_sets]);
    printf(" cand");
    for (int j = 0; j < n_cand; j++) printf(" %llu", (unsigned long long)cand_id[j]);
    printf(" th %.9g %.9g optional %d %d %d\n", dis_th, angle_th, world_coef ? 1 : 0, dis ? 1 : 0, gated ? 1 : 0);
    for (int i = 0; i < set_start[n_sets]; i++) {
        match[i] = (n_cand > 0 && i % 2 == 0) ? n_cand - 1 - (i / 2) % n_cand : -1;
        match_dis[i] = 0.0f;
    }
    return EAO_OK;
}

}  // extern "C"
