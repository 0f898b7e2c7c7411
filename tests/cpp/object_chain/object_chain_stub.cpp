// A stand-in for the library entries DataAssociateUpdate and DataAssociateUpdateChained of include/eaofusion/ObjectMap.h call, which needs no device: it prints
// each call it receives and answers by made-up rules, so that the CPU suite can check that the chained form makes ONE library call, what it sends, and that both
// forms, fed the same answers, leave the same members (tests/test_object_chain_class_cpu.py).  The three single entries answer as
// tests/cpp/object_points/object_points_stub.cpp does:
//   eao_object_points_update            refused when the first list point has x == 999; REJECTED when change_gate is set and project_rect1.x == -1; otherwise
//                                       gate[j] = gate != NONE && j % 3 != 2; of the gated-in candidates those with j % 3 == 0 are appended, those with
//                                       j % 3 == 1 target entry 0 (the first appended slot when the list is empty); erased[k] = erase != NONE && k % 2 == 1;
//                                       sum_pos_appended = (0.5, 1.5, 2.5), sum_pos = (10.5, 11.5, 12.5)
//   eao_object_cuboids_batch            status DONE, sum_pos = (20.5, 21.5, 22.5), everything else zero
//   eao_object_iforest_outliers_batch   flags nothing
//   eao_object_update_chain             the three rules chained, with the erase of the bad points in between
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include <eao_fusion.h>

#include <cstdarg>

static bool g_quiet = false;      // the chain entry answers through the three rules below without their lines

static void say(const char* fmt, ...) {
    if (g_quiet) return;
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
}

static void hex32(float v) {
    if (g_quiet) return;
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    say(" %08x", bits);
}
static void hex64(double v) {
    if (g_quiet) return;
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    say(" %016llx", (unsigned long long)bits);
}

extern "C" {

const char* eao_last_error(void) { return "stub"; }

eao_status eao_object_points_update(const eao_object_points_desc* desc, const eao_object_points_out* out) {
    const eao_object_points_desc& d = *desc;
    say("call points cg %d gate %d erase %d edge %d n_map %d n_cand %d nf %d cols %d rows %d rect1 %d %d %d %d box %d %d %d %d", d.change_gate, d.gate, d.erase,
                d.box_off_edge, d.n_map, d.n_cand, d.n_frames_after_push, d.cols, d.rows, d.project_rect1[0], d.project_rect1[1], d.project_rect1[2], d.project_rect1[3],
                d.box_rect[0], d.box_rect[1], d.box_rect[2], d.box_rect[3]);
    say(" tcw");
    for (float v : d.Tcw) hex32(v);
    say(" k");
    hex32(d.fx); hex32(d.fy); hex32(d.cx); hex32(d.cy);
    say(" center");
    for (float v : d.center) hex32(v);
    hex32(d.rmax);
    say(" extent");
    hex32(d.lenth); hex32(d.width); hex32(d.height);
    say(" pose");
    for (double v : d.pose_q) hex64(v);
    for (double v : d.pose_t) hex64(v);
    say(" cc");
    for (double v : d.cuboid_center) hex64(v);
    say(" bounds");
    for (float v : d.bounds) hex32(v);
    say(" overlap");
    for (float v : d.overlap) hex32(v);
    say(" sum");
    for (float v : d.sum_pos) hex32(v);
    say(" map");
    for (int i = 0; i < d.n_map; i++) { hex32(d.map_points[3 * i]); hex32(d.map_points[3 * i + 1]); hex32(d.map_points[3 * i + 2]); say(" %d", d.map_count[i]); }
    say(" cand");
    for (int i = 0; i < d.n_cand; i++) { hex32(d.cand_points[3 * i]); hex32(d.cand_points[3 * i + 1]); hex32(d.cand_points[3 * i + 2]); say(" %d", d.cand_count[i]); }
    say("\n");
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
    say("call cuboids n_obj %d points", n_obj);
    for (int j = 0; j < n_obj; j++) say(" %d", objs[j].n_points);
    say("\n");
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
    say("call iforest n_obj %d bi %d points %d\n", n_obj, bi_forest, start[n_obj]);
    for (int j = 0; j < n_obj; j++) removed[j] = 0;
    for (int i = 0; i < start[n_obj]; i++) flags[i] = 0;
    return EAO_OK;
}

// the three rules above, chained: the points rule, then the survivors whose bad flag is set leave, then the cuboid rule over the final list and the forest rule
eao_status eao_object_update_chain(const eao_object_chain_desc* desc, const eao_object_chain_out* out) {
    const eao_object_chain_desc& d = *desc;
    say("call chain n_map %d n_cand %d class %d bi %d centroids %d last", d.points.n_map, d.points.n_cand, d.class_id, d.bi_forest, d.n_centroids);
    for (int a = 0; a < 3 && d.n_centroids > 0; a++) hex32(d.centroids[3 * (d.n_centroids - 1) + a]);
    say(" bad");
    for (int i = 0; i < d.points.n_map; i++) say(" %d", d.map_bad[i]);
    say(" |");
    for (int j = 0; j < d.points.n_cand; j++) say(" %d", d.cand_bad[j]);
    say(" alias");
    for (int j = 0; j < d.points.n_cand; j++) say(" %d", d.cand_alias ? d.cand_alias[j] : -9);
    say("\n");
    g_quiet = true;
    eao_status st = eao_object_points_update(&d.points, &out->points);
    if (st == EAO_OK && out->points.rec->status == EAO_OBJECT_POINTS_DONE) {
        // the alias rule (:1550-1559): an entry the erase rule took whose count, raised by the gated-in candidates that are this very MapPoint, exceeds the bound stays
        eao_object_points_rec& r = *out->points.rec;
        for (int k = 0; k < d.points.n_map && d.cand_alias && d.points.erase == EAO_OBJECT_POINTS_ERASE_PROJECTION; k++) {
            int raised = 0;
            for (int j = 0; j < d.points.n_cand; j++) raised += (out->points.gate[j] && d.cand_alias[j] == k) ? 1 : 0;
            if (out->points.erased[k] && raised > 0 && d.points.map_count[k] + raised > EAO_OBJECT_POINTS_KEEP_COUNT) out->points.erased[k] = 0;
        }
        r.n_survivors = r.n_erased = 0;
        for (int k = 0; k < r.n_list; k++) {
            if (out->points.erased[k]) { r.n_erased++; continue; }
            out->points.survivors[2 * r.n_survivors] = out->points.list[2 * k];
            out->points.survivors[2 * r.n_survivors + 1] = out->points.list[2 * k + 1];
            r.n_survivors++;
        }
        int nf = 0;
        for (int k = 0; k < out->points.rec->n_survivors; k++) {
            const int src = out->points.survivors[2 * k], idx = out->points.survivors[2 * k + 1];
            if (src ? d.cand_bad[idx] : d.map_bad[idx]) continue;
            out->final[2 * nf] = src;
            out->final[2 * nf + 1] = idx;
            out->forest_flags[nf] = 0;
            nf++;
        }
        eao_object_cuboid_desc c;
        std::memset(&c, 0, sizeof(c));
        c.n_points = nf;
        eao_object_cuboids_batch(1, &c, out->cuboid);
        std::memset(out->rec, 0, sizeof(*out->rec));
        out->rec->n_final = nf;
    }
    g_quiet = false;
    return st;
}

}  // extern "C"
