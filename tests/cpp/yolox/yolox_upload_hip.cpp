// yolox_upload_hip.cpp -- the stand-in network's copy of tests/cpp/yolox/yolox_driver.cpp when it runs against the real library: host to device, through the HIP
// runtime the library itself is linked with (declared here, so that the driver builds with g++ alone).
#include <cstddef>

extern "C" int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);

extern "C" int yolox_driver_upload(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, 1 /* hipMemcpyHostToDevice */); }
