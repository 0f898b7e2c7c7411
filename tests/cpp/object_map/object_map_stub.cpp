// A stand-in for libeaofusion_hip.so's eao_object_iforest_outliers_batch that needs no device: it prints the call it receives and answers by a made-up rule, so
// that the CPU suite can check what include/eaofusion/ObjectMap.h sends and what it does with the answer (tests/test_object_map_class_cpu.py restates the rule).
//   point i of an object of n points is flagged when i % 4 == 1 or i == n - 1 (so the last point is always the last outlier);
//   class 999 refuses the call with EAO_ERR_INVALID and writes nothing.
#include <cstdio>
#include <cstring>

#include <eao_fusion.h>

extern "C" {

const char* eao_last_error(void) { return "stub"; }

eao_status eao_object_iforest_outliers_batch(int32_t n_obj, const int32_t* start, const float* xyz, const int32_t* class_id, int32_t bi_forest, uint8_t* flags,
                                             int32_t* removed, double* scores) {
    std::printf("call n_obj %d bi %d scores %d start", n_obj, bi_forest, scores ? 1 : 0);
    for (int j = 0; j <= n_obj; j++) std::printf(" %d", start[j]);
    std::printf(" class");
    for (int j = 0; j < n_obj; j++) std::printf(" %d", class_id[j]);
    std::printf(" xyz");
    for (int i = 3 * start[0]; i < 3 * start[n_obj]; i++) {
        uint32_t bits;
        std::memcpy(&bits, &xyz[i], 4);
        std::printf(" %08x", bits);
    }
    std::printf("\n");
    for (int j = 0; j < n_obj; j++)
        if (class_id[j] == 999) return EAO_ERR_INVALID;
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

}  // extern "C"
