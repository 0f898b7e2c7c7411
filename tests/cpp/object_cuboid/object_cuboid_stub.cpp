// A stand-in for the three library entries the cuboid half of include/eaofusion/ObjectMap.h calls, which needs no device: it prints each call it receives and
// answers by made-up rules, so that the CPU suite can check what the adapter sends and what it does with the answer (tests/test_object_cuboid_class_cpu.py
// restates the rules).
//   eao_object_cuboids_batch            object j: status EMPTY when it has no points, bounds_written when it has fewer than 5 centroids; the k-th 4-byte float of the
//                                       record (in field order) is 1000 j + k + 0.5, the k-th double 1000 j + k + 0.25; a first point with x == 999 refuses the call
//   eao_object_iforest_outliers_batch   point i of an object of n points is flagged when i % 4 == 1 or i == n - 1
//   eao_object_overlaps                 verdict(i, j) = eligible[i] && eligible[j] && i < j; extents 100 i + j + {0, 0.25, 0.5}
#include <cstddef>
#include <cstdio>
#include <cstring>

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

eao_status eao_object_cuboids_batch(int32_t n_obj, const eao_object_cuboid_desc* objs, eao_object_cuboid_rec* recs) {
    std::printf("call cuboids n_obj %d\n", n_obj);
    for (int j = 0; j < n_obj; j++) {
        const eao_object_cuboid_desc& d = objs[j];
        std::printf("desc n %d m %d null %d %d ryaw", d.n_points, d.n_centroids, d.points ? 0 : 1, d.centroids ? 0 : 1);
        for (float v : d.Ryaw) hex32(v);
        std::printf(" prev");
        for (double v : d.prev_cuboid_center) hex64(v);
        std::printf(" points");
        for (int i = 0; i < 3 * d.n_points; i++) hex32(d.points[i]);
        std::printf(" centroids");
        for (int i = 0; i < 3 * d.n_centroids; i++) hex32(d.centroids[i]);
        std::printf("\n");
    }
    for (int j = 0; j < n_obj; j++)
        if (objs[j].n_points > 0 && objs[j].points[0] == 999.0f) return EAO_ERR_INVALID;
    for (int j = 0; j < n_obj; j++) {
        eao_object_cuboid_rec r;
        unsigned char* base = (unsigned char*)&r;      // the 4-byte fields from sum_pos to Twobj_without_yaw are contiguous (include/eao_fusion.h): 23 floats, `reserved`, 32 floats
        for (int k = 0; k < 56; k++) {
            const float v = 1000.0f * j + k + 0.5f;
            std::memcpy(base + offsetof(eao_object_cuboid_rec, sum_pos) + 4 * k, &v, 4);
        }
        for (int k = 0; k < 65; k++) {
            const double v = 1000.0 * j + k + 0.25;
            std::memcpy(base + offsetof(eao_object_cuboid_rec, cuboid_center) + 8 * k, &v, 8);
        }
        r.reserved = 0;
        r.status = objs[j].n_points == 0 ? EAO_OBJECT_CUBOID_EMPTY : EAO_OBJECT_CUBOID_DONE;
        r.bounds_written = (r.status == EAO_OBJECT_CUBOID_DONE && objs[j].n_centroids < 5) ? 1 : 0;
        recs[j] = r;
    }
    return EAO_OK;
}

eao_status eao_object_iforest_outliers_batch(int32_t n_obj, const int32_t* start, const float* xyz, const int32_t* class_id, int32_t bi_forest, uint8_t* flags,
                                             int32_t* removed, double* scores) {
    (void)xyz; (void)class_id; (void)scores;
    std::printf("call iforest n_obj %d bi %d start", n_obj, bi_forest);
    for (int j = 0; j <= n_obj; j++) std::printf(" %d", start[j]);
    std::printf("\n");
    for (int j = 0; j < n_obj; j++) {
        const int n = start[j + 1] - start[j];
        removed[j] = 0;
        for (int i = 0; i < n; i++) {
            flags[start[j] + i] = (i % 4 == 1 || i == n - 1) ? 1 : 0;
            removed[j] += flags[start[j] + i];
        }
    }
    return EAO_OK;
}

eao_status eao_object_overlaps(int32_t m, const eao_object_overlap_row* rows, const uint8_t* eligible, uint8_t* verdict, float* extents) {
    std::printf("call overlaps m %d extents %d", m, extents ? 1 : 0);
    for (int i = 0; i < m; i++) {
        std::printf(" row");
        for (double v : rows[i].cuboid_center) hex64(v);
        hex32(rows[i].lenth); hex32(rows[i].width); hex32(rows[i].height);
        std::printf(" %d", eligible[i]);
    }
    std::printf("\n");
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) {
            const size_t p = (size_t)i * m + j;
            verdict[p] = (eligible[i] && eligible[j] && i < j) ? 1 : 0;
            if (verdict[p] && extents)
                for (int k = 0; k < 3; k++) extents[3 * p + k] = 100.0f * i + j + 0.25f * k;
        }
    return EAO_OK;
}

}  // extern "C"
