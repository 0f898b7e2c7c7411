// A stand-in for the library entries the point-list half of include/eaofusion/ObjectMap.h calls, which needs no device: it prints each call it receives and
// answers by made-up rules, so that the CPU suite can check what the adapter sends and what it does with the answer (tests/test_object_points_class_cpu.py
// restates the rules).
//   eao_object_points_update            refused when the first list point has x == 999; REJECTED when change_gate is set and project_rect1.x == -1; otherwise
//                                       gate[j] = gate != NONE && j % 3 != 2; of the gated-in candidates those with j % 3 == 0 are appended, those with
//                                       j % 3 == 1 target entry 0 (the first appended slot when the list is empty); erased[k] = erase != NONE && k % 2 == 1;
//                                       sum_pos_appended = (0.5, 1.5, 2.5), sum_pos = (10.5, 11.5, 12.5)
//   eao_object_cuboids_batch            status DONE, sum_pos = (20.5, 21.5, 22.5), everything else zero
//   eao_object_iforest_outliers_batch   flags nothing
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include <eao_fusion.h>

static void hex32(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    std::printf(" %08x", bits);
}
static void hex64(double v) {
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    std::printf(" %016llx", (unsigned long long)bits);
}

extern "C" {

const char* eao_last_error(void) { return "stub"; }

eao_status eao_object_points_update(const eao_object_points_desc* desc, const eao_object_points_out* out) {
    const eao_object_points_desc& d = *desc;
    std::printf("call points cg %d gate %d erase %d edge %d n_map %d n_cand %d nf %d cols %d rows %d rect1 %d %d %d %d box %d %d %d %d", d.change_gate, d.gate, d.erase,
                d.box_off_edge, d.n_map, d.n_cand, d.n_frames_after_push, d.cols, d.rows, d.project_rect1[0], d.project_rect1[1], d.project_rect1[2], d.project_rect1[3],
                d.box_rect[0], d.box_rect[1], d.box_rect[2], d.box_rect[3]);
    std::printf(" tcw");
    for (float v : d.Tcw) hex32(v);
    std::printf(" k");
    hex32(d.fx); hex32(d.fy); hex32(d.cx); hex32(d.cy);
    std::printf(" center");
    for (float v : d.center) hex32(v);
    hex32(d.rmax);
    std::printf(" extent");
    hex32(d.lenth); hex32(d.width); hex32(d.height);
    std::printf(" pose");
    for (double v : d.pose_q) hex64(v);
    for (double v : d.pose_t) hex64(v);
    std::printf(" cc");
    for (double v : d.cuboid_center) hex64(v);
    std::printf(" bounds");
    for (float v : d.bounds) hex32(v);
    std::printf(" overlap");
    for (float v : d.overlap) hex32(v);
    std::printf(" sum");
    for (float v : d.sum_pos) hex32(v);
    std::printf(" map");
    for (int i = 0; i < d.n_map; i++) { hex32(d.map_points[3 * i]); hex32(d.map_points[3 * i + 1]); hex32(d.map_points[3 * i + 2]); std::printf(" %d", d.map_count[i]); }
    std::printf(" cand");
    for (int i = 0; i < d.n_cand; i++) { hex32(d.cand_points[3 * i]); hex32(d.cand_points[3 * i + 1]); hex32(d.cand_points[3 * i + 2]); std::printf(" %d", d.cand_count[i]); }
    std::printf("\n");
    if (d.n_map > 0 && d.map_points[0] == 999.0f) return EAO_ERR_INVALID;
    eao_object_points_rec r;
    std::memset(&r, 0, sizeof(r));
    r.status = (d.change_gate && d.project_rect1[0] == -1) ? EAO_OBJECT_POINTS_REJECTED : EAO_OBJECT_POINTS_DONE;
    if (r.status == EAO_OBJECT_POINTS_DONE) {
        std::vector<int> app;
        for (int j = 0; j < d.n_cand; j++) {
            const int g = (d.gate != EAO_OBJECT_POINTS_GATE_NONE && j % 3 != 2) ? 1 : 0;
            out->gate[j] = (uint8_t)g;
            out->count[j] = d.cand_count[j] + g;
            out->target[j] = (g && j % 3 == 1) ? (d.n_map > 0 ? 0 : d.n_map) : -1;
            r.n_gated += g;
            if (g && j % 3 == 0) app.push_back(j);
        }
        r.n_appended = (int32_t)app.size();
        r.n_list = d.n_map + r.n_appended;
        for (int k = 0; k < r.n_list; k++) {
            out->list[2 * k] = k < d.n_map ? 0 : 1;
            out->list[2 * k + 1] = k < d.n_map ? k : app[k - d.n_map];
            const int e = (d.erase != EAO_OBJECT_POINTS_ERASE_NONE && k % 2 == 1) ? 1 : 0;
            out->erased[k] = (uint8_t)e;
            r.n_erased += e;
            if (!e) {
                const float* x = k < d.n_map ? d.map_points + 3 * k : d.cand_points + 3 * app[k - d.n_map];
                out->survivors[2 * r.n_survivors] = out->list[2 * k];
                out->survivors[2 * r.n_survivors + 1] = out->list[2 * k + 1];
                if (d.survivors) std::memcpy(d.survivors + 3 * r.n_survivors, x, 12);
                r.n_survivors++;
            }
        }
        for (int a = 0; a < 3; a++) { r.sum_pos_appended[a] = 0.5f + a; r.sum_pos[a] = 10.5f + a; }
    }
    *out->rec = r;
    return EAO_OK;
}

eao_status eao_object_cuboids_batch(int32_t n_obj, const eao_object_cuboid_desc* objs, eao_object_cuboid_rec* recs) {
    std::printf("call cuboids n_obj %d points", n_obj);
    for (int j = 0; j < n_obj; j++) std::printf(" %d", objs[j].n_points);
    std::printf("\n");
    for (int j = 0; j < n_obj; j++) {
        std::memset(&recs[j], 0, sizeof(recs[j]));
        recs[j].status = EAO_OBJECT_CUBOID_DONE;
        for (int a = 0; a < 3; a++) recs[j].sum_pos[a] = 20.5f + a;
    }
    return EAO_OK;
}

eao_status eao_object_iforest_outliers_batch(int32_t n_obj, const int32_t* start, const float* xyz, const int32_t* class_id, int32_t bi_forest, uint8_t* flags,
                                             int32_t* removed, double* scores) {
    (void)xyz; (void)class_id; (void)scores;
    std::printf("call iforest n_obj %d bi %d points %d\n", n_obj, bi_forest, start[n_obj]);
    for (int j = 0; j < n_obj; j++) removed[j] = 0;
    for (int i = 0; i < start[n_obj]; i++) flags[i] = 0;
    return EAO_OK;
}

}  // extern "C"
