// A stand-in for libeaofusion_hip.so's eao_object_np_association_batch and eao_object_project_rects_batch that needs no device: it prints the call it receives
// and answers by a made-up rule, so that the CPU suite can check what include/eaofusion/ObjectAssociation.h sends and what it does with the answer
// (tests/test_object_association_class_cpu.py restates the rules).
//   rank-sum: the verdict of a pair is 1, 2 or 3 (EAO_OBJECT_NP_UNDEFINED) for a map object of nGood % 3 == 0, 1 or 2 good points; a detection of exactly 99 points
//             refuses the call with EAO_ERR_INVALID and writes nothing;
//   rects:    object j of n points gets rect {j, n, cols, rows}; status 0 for n == 0, 2 for n % 5 == 4, else 1; cols == 999 refuses the call.
#include <cstdio>
#include <cstring>

#include <eao_fusion.h>

static void print_floats(const float* v, int n) {
    for (int i = 0; i < n; i++) {
        uint32_t bits;
        std::memcpy(&bits, &v[i], 4);
        std::printf(" %08x", bits);
    }
}

extern "C" {

const char* eao_last_error(void) { return "stub"; }

eao_status eao_object_np_association_batch(int32_t n_det, const int32_t* det_start, const float* det_xyz, int32_t n_map, const int32_t* map_start,
                                           const float* map_xyz, const int32_t* map_total, int32_t n_pair, const int32_t* pair_det, const int32_t* pair_map,
                                           int32_t* verdict, float* w, float* r) {
    std::printf("call np n_det %d det_start", n_det);
    for (int d = 0; d <= n_det; d++) std::printf(" %d", det_start[d]);
    std::printf(" n_map %d map_start", n_map);
    for (int j = 0; j <= n_map; j++) std::printf(" %d", map_start[j]);
    std::printf(" map_total");
    for (int j = 0; j < n_map; j++) std::printf(" %d", map_total[j]);
    std::printf(" pairs");
    for (int p = 0; p < n_pair; p++) std::printf(" %d:%d", pair_det[p], pair_map[p]);
    std::printf(" w %d r %d det", w ? 1 : 0, r ? 1 : 0);
    print_floats(det_xyz + 3 * det_start[0], 3 * (det_start[n_det] - det_start[0]));
    std::printf(" map");
    print_floats(map_xyz + 3 * map_start[0], 3 * (map_start[n_map] - map_start[0]));
    std::printf("\n");
    for (int d = 0; d < n_det; d++)
        if (det_start[d + 1] - det_start[d] == 99) return EAO_ERR_INVALID;
    for (int p = 0; p < n_pair; p++) {
        const int j = pair_map[p];
        verdict[p] = 1 + (map_start[j + 1] - map_start[j]) % 3;
    }
    return EAO_OK;
}

eao_status eao_object_project_rects_batch(int32_t n_map, const int32_t* map_start, const float* map_xyz, const float* Tcw, float fx, float fy, float cx, float cy,
                                          int32_t cols, int32_t rows, int32_t* rect, uint8_t* status, float* uv) {
    std::printf("call rects n_map %d map_start", n_map);
    for (int j = 0; j <= n_map; j++) std::printf(" %d", map_start[j]);
    std::printf(" cols %d rows %d uv %d cam", cols, rows, uv ? 1 : 0);
    const float cam[4] = {fx, fy, cx, cy};
    print_floats(cam, 4);
    std::printf(" Tcw");
    print_floats(Tcw, 16);
    std::printf(" xyz");
    print_floats(map_xyz + 3 * map_start[0], 3 * (map_start[n_map] - map_start[0]));
    std::printf("\n");
    if (cols == 999) return EAO_ERR_INVALID;
    for (int j = 0; j < n_map; j++) {
        const int n = map_start[j + 1] - map_start[j];
        status[j] = n == 0 ? 0 : (n % 5 == 4 ? 2 : 1);
        if (status[j] == 1) {
            rect[4 * j] = j; rect[4 * j + 1] = n; rect[4 * j + 2] = cols; rect[4 * j + 3] = rows;
        }
    }
    return EAO_OK;
}

}  // extern "C"
