// yolox_stub.cpp -- a recording stand-in of the eao_yolox_* entry points for tests/test_yolox_class_cpu.py: prints the call it receives and answers by script.
// "Device" buffers are host memory.  The decode answers two made-up objects and the scripted n_tied, or the scripted status with the scripted proposal count.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <eao_fusion.h>

struct eao_yolox {
    eao_yolox_cfg cfg;
    std::vector<float> blob, prob;
};

static int g_tied = 0, g_status = 0, g_proposals = 2;
static int anchors(int S) { return (S / 8) * (S / 8) + (S / 16) * (S / 16) + (S / 32) * (S / 32); }

extern "C" {

void yolox_stub_script(int nTied, int status, int nProposals) { g_tied = nTied; g_status = status; g_proposals = nProposals; }
int yolox_driver_upload(void* dst, const void* src, size_t bytes) { std::memcpy(dst, src, bytes); return 0; }

const char* eao_last_error(void) { return "stub"; }

void eao_yolox_cfg_default(eao_yolox_cfg* c) { *c = eao_yolox_cfg{640, 80, (float)0.3, (float)0.65, 4096, 1}; }

eao_status eao_yolox_create(const eao_yolox_cfg* cfg, eao_yolox** out) {
    std::printf("call create S %d classes %d max_proposals %d max_batch %d\n", cfg->input_size, cfg->num_classes, cfg->max_proposals, cfg->max_batch);
    eao_yolox* h = new eao_yolox;
    h->cfg = *cfg;
    h->blob.assign((size_t)3 * cfg->input_size * cfg->input_size, 0.f);
    h->prob.assign((size_t)anchors(cfg->input_size) * (5 + cfg->num_classes), 0.f);
    *out = h;
    return EAO_OK;
}
void eao_yolox_destroy(eao_yolox* h) { std::printf("call destroy\n"); delete h; }

eao_status eao_yolox_buffers(eao_yolox* h, float** d_blob, float** d_prob, void** stream) {
    *d_blob = h->blob.data(); *d_prob = h->prob.data(); *stream = (void*)0x5;
    return EAO_OK;
}

eao_status eao_yolox_preprocess(eao_yolox*, const uint8_t* frames, int32_t width, int32_t height, int32_t stride, int64_t, int32_t batch, int32_t rgb, uint8_t* gray,
                                int32_t) {
    std::printf("call preprocess %d x %d stride %d batch %d rgb %d gray %d first %d\n", width, height, stride, batch, rgb, gray ? 1 : 0, frames[0]);
    return width >= 1000 ? EAO_ERR_INVALID : EAO_OK;
}

eao_status eao_yolox_decode_device(eao_yolox* h, const float* d_prob, int32_t batch, const int32_t* img_w, const int32_t* img_h, eao_yolox_object* objects, int32_t cap,
                                   int32_t* n, int32_t* n_proposals, int32_t* n_tied, void* stream) {
    std::printf("call decode_device own_buffer %d batch %d img %d x %d cap %d stream %d\n", d_prob == h->prob.data() ? 1 : 0, batch, img_w[0], img_h[0], cap,
                stream == (void*)0x5 ? 1 : 0);
    if (g_status == EAO_ERR_CAPACITY) { n_proposals[0] = g_proposals; return EAO_ERR_CAPACITY; }
    if (g_status != EAO_OK) return (eao_status)g_status;
    objects[0] = eao_yolox_object{1.f, 2.f, 3.f, 4.f, 0.9f, 7};
    objects[1] = eao_yolox_object{5.f, 6.f, 7.f, 8.f, 0.8f, 9};
    n[0] = 2; n_proposals[0] = g_proposals; n_tied[0] = g_tied;
    return EAO_OK;
}

eao_status eao_yolox_head(eao_yolox* h, const float* d_prob, int32_t batch, float* prob, void*) {
    std::printf("call head batch %d\n", batch);
    std::memcpy(prob, d_prob, h->prob.size() * 4);
    return EAO_OK;
}

}  // extern "C"
