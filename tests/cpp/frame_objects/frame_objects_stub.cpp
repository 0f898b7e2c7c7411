// A stand-in for libeaofusion_hip.so's eao_frame_objects_batch that needs no device: it prints the call it receives and answers by a made-up rule, so that the CPU
// suite can check what include/eaofusion/FrameObjects.h sends and what it does with the answer (tests/test_frame_objects_class_cpu.py restates the rule).
//   box k of a frame: assigned = the keypoints i with a map point and i % (k + 2) == 0, kept = assigned without its first entry;
//   sum_pos = {k + 0.5, n_assigned, 2}, pos = {1.5, k, 3}, std = {0.25, 0.5, k}, center_2d = {10 + k, 20 + k}; has_feature_rect for even k with
//   feature_rect = {k, k + 1, k + 2, k + 3}; bad for k % 3 == 1; on_edge for odd k.  A frame with cols == 999 refuses the call and writes nothing.
#include <cstdio>
#include <cstring>
#include <vector>

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

eao_status eao_frame_objects_batch(int32_t n_frames, const eao_frame_objects_desc* frames, const eao_frame_objects_out* out) {
    std::printf("call frames %d caps %lld %lld\n", n_frames, (long long)out->assigned_cap, (long long)out->kept_cap);
    for (int32_t f = 0; f < n_frames; f++) {
        const eao_frame_objects_desc& F = frames[f];
        std::printf("sent %d n_kp %d n_box %d cols %d rows %d cam", f, F.n_kp, F.n_box, F.cols, F.rows);
        const float cam[4] = {F.fx, F.fy, F.cx, F.cy};
        print_floats(cam, 4);
        std::printf(" Tcw");
        print_floats(F.Tcw, 16);
        std::printf(" ids");
        for (int32_t i = 0; i < F.n_kp; i++) std::printf(" %d", F.mp_id[i]);
        std::printf(" kp");
        for (int32_t i = 0; i < F.n_kp; i++) { print_floats(F.kp_x + i, 1); print_floats(F.kp_y + i, 1); }
        std::printf(" xyz");
        for (int32_t i = 0; i < F.n_kp; i++)
            if (F.mp_id[i] >= 0) print_floats(F.mp_xyz + 3 * i, 3);
        std::printf(" boxes");
        for (int32_t k = 0; k < 4 * F.n_box; k++) std::printf(" %d", F.boxes[k]);
        std::printf(" score");
        print_floats(F.score, F.n_box);
        std::printf("\n");
    }
    for (int32_t f = 0; f < n_frames; f++)
        if (frames[f].cols == 999) return EAO_ERR_INVALID;
    int32_t b = 0, a = 0, kk = 0;
    out->assigned_start[0] = out->kept_start[0] = 0;
    for (int32_t f = 0; f < n_frames; f++) {
        const eao_frame_objects_desc& F = frames[f];
        for (int32_t k = 0; k < F.n_box; k++, b++) {
            eao_frame_object_record r;
            std::memset(&r, 0, sizeof(r));
            for (int32_t i = 0; i < F.n_kp; i++)
                if (F.mp_id[i] >= 0 && i % (k + 2) == 0) {
                    if (r.n_assigned > 0) out->kept[kk++] = i;
                    out->assigned[a++] = i;
                    r.n_assigned++;
                }
            r.n = r.n_assigned > 0 ? r.n_assigned - 1 : 0;
            r.sum_pos[0] = (float)k + 0.5f; r.sum_pos[1] = (float)r.n_assigned; r.sum_pos[2] = 2.0f;
            r.pos[0] = 1.5f; r.pos[1] = (float)k; r.pos[2] = 3.0f;
            r.std[0] = 0.25f; r.std[1] = 0.5f; r.std[2] = (float)k;
            r.center_2d[0] = 10.0f + (float)k; r.center_2d[1] = 20.0f + (float)k;
            r.has_feature_rect = k % 2 == 0;
            for (int j = 0; j < 4; j++) r.feature_rect[j] = r.has_feature_rect ? k + j : 0;
            r.bad = k % 3 == 1;
            r.on_edge = k % 2 == 1;
            out->records[b] = r;
            out->assigned_start[b + 1] = a;
            out->kept_start[b + 1] = kk;
        }
    }
    return EAO_OK;
}

}  // extern "C"
