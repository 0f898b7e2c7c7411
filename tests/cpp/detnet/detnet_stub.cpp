// detnet_stub.cpp -- a recording stand-in of the eao_detnet_* entry points include/eaofusion/YOLOXNet.h uses, for tests/test_detnet_class_cpu.py: prints the call it
// receives.  DETNET_STUB_CLASSES sets the class count the "model" reports (80), DETNET_STUB_REFUSE makes the file a bad one.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <eao_fusion.h>

struct eao_detnet { int S, maxBatch; };

static int env(const char* name, int dflt) { const char* v = std::getenv(name); return v ? std::atoi(v) : dflt; }

extern "C" {

eao_status eao_detnet_create_from_file(const char* path, int32_t input_size, int32_t max_batch, eao_detnet** out) {
    const char* base = std::strrchr(path, '/');
    std::printf("call detnet_create_from_file %s S %d max_batch %d\n", base ? base + 1 : path, input_size, max_batch);
    if (env("DETNET_STUB_REFUSE", 0)) return EAO_ERR_INVALID;
    *out = new eao_detnet{input_size, max_batch};
    return EAO_OK;
}
void eao_detnet_destroy(eao_detnet* h) { std::printf("call detnet_destroy\n"); delete h; }
eao_status eao_detnet_info(const eao_detnet* h, eao_detnet_desc* d) {
    std::memset(d, 0, sizeof *d);
    d->classes = env("DETNET_STUB_CLASSES", 80);
    d->anchors = (h->S / 8) * (h->S / 8) + (h->S / 16) * (h->S / 16) + (h->S / 32) * (h->S / 32);
    d->input_size = h->S; d->max_batch = h->maxBatch;
    return EAO_OK;
}
eao_status eao_detnet_forward(eao_detnet*, const float* d_blob, float* d_prob, int32_t batch, void* stream) {
    std::printf("call detnet_forward blob %d prob %d batch %d stream %d\n", d_blob ? 1 : 0, d_prob ? 1 : 0, batch, stream == (void*)0x5 ? 1 : 0);
    return env("DETNET_STUB_FORWARD", 0) ? EAO_ERR_INVALID : EAO_OK;
}

}  // extern "C"
