// YOLOXNet.h -- the reference's detector with its engine (include/YOLOX.h:55-129; the TensorRT runtime, engine and context of src/YOLOX.cc:7-48 and DoInference,
// :331-367) on top of the C-ABI: eaofusion::YOLOX of YOLOX.h takes the network as a callable, and this header supplies the callable from a model file through
// eao_detnet_* (csrc/detnet.hip), so that
//
//   #include <eaofusion/YOLOXNet.h>
//   eaofusion::YOLOXEngine<cv::Mat> detector(engineFile);      // was: new YOLOX(engineFile), src/System.cc:112
//
// needs no TensorRT in the build.  The file is what tools/export_detnet.py writes (csrc/detnet_internal.h states the format).
//
//   DetNet        an RAII handle of eao_detnet; infer() is the yolox::Infer that runs it on the stream it is given
//   YOLOXEngine   YOLOX<MatT> whose constructor takes the engine file path, as the reference's does (include/YOLOX.h:90); the model's class count must be the
//                 configuration's (80 by default)
#pragma once

#include <stdexcept>
#include <string>

#include "YOLOX.h"
#include "adapter_detail.h"

namespace eaofusion {

class DetNet {
public:
    DetNet(const std::string& path, int input_size, int max_batch = 1) {
        detail::check(eao_detnet_create_from_file(path.c_str(), input_size, max_batch, &h_), "eao_detnet_create_from_file");
        const eao_status st = eao_detnet_info(h_, &desc_);
        if (st != EAO_OK) eao_detnet_destroy(h_);      // (no destructor runs when a constructor throws)
        detail::check(st, "eao_detnet_info");
    }
    ~DetNet() { eao_detnet_destroy(h_); }
    DetNet(const DetNet&) = delete;
    DetNet& operator=(const DetNet&) = delete;

    // DoInference (:331-367) without its copies: one frame from d_blob to d_prob on `stream`.  A refused call throws: the detector would otherwise decode a stale head.
    yolox::Infer infer() {
        return [this](const float* d_blob, float* d_prob, void* stream) {
            detail::check(eao_detnet_forward(h_, d_blob, d_prob, 1, stream), "eao_detnet_forward");
        };
    }
    const eao_detnet_desc& info() const { return desc_; }
    eao_detnet* handle() const { return h_; }

private:
    eao_detnet* h_ = nullptr;
    eao_detnet_desc desc_{};
};

namespace detail {
struct DetNetMember {      // (a base, so that the network exists before YOLOX<MatT> is given its callable)
    DetNet net;
    DetNetMember(const std::string& path, const eao_yolox_cfg* cfg) : net(path, input_size(cfg)) {
        eao_yolox_cfg c;
        if (cfg) c = *cfg; else eao_yolox_cfg_default(&c);
        if (net.info().classes != c.num_classes)
            throw std::runtime_error("the model has " + std::to_string(net.info().classes) + " classes, the detector is configured for " + std::to_string(c.num_classes));
    }
    static int input_size(const eao_yolox_cfg* cfg) {
        if (cfg) return cfg->input_size;
        eao_yolox_cfg c;
        eao_yolox_cfg_default(&c);
        return c.input_size;
    }
};
}  // namespace detail

template <class MatT>
class YOLOXEngine : private detail::DetNetMember, public YOLOX<MatT> {
public:
    explicit YOLOXEngine(const std::string& engine_file_path, const eao_yolox_cfg* cfg = nullptr, bool rgb = false)
        : detail::DetNetMember(engine_file_path, cfg), YOLOX<MatT>(detail::DetNetMember::net.infer(), cfg, rgb) {}
    const DetNet& network() const { return detail::DetNetMember::net; }
};

}  // namespace eaofusion
