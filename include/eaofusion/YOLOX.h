// YOLOX.h -- the reference's detector thread class (include/YOLOX.h:55-129, src/YOLOX.cc) on top of the C-ABI, without TensorRT: everything YOLOX::Detect does
// around the network runs on the device through eao_yolox_*, and the network is a callable the integrator supplies,
//
//     void infer(const float* d_blob, float* d_prob, void* stream)      // device pointers; enqueue on `stream` (a hipStream_t)
//
// which is where an engine goes: it reads 3 x S x S floats and writes anchors x (5 + classes) floats, both in HBM (DoInference, :331-367, without its two copies,
// its two allocations and its stream).
//
//   #include <eaofusion/YOLOX.h>
//   eaofusion::YOLOX<cv::Mat> detector([&](const float* in, float* out, void* s) { engine.enqueue(in, out, s); });
//   detector.InsertImage(imRGB); ... detector.Run() on its thread ... if (detector.CheckResult()) detector.GetResult(objs);
//   std::vector<BoxSE> boxes = eaofusion::TrackingBoxes<BoxSE>(objs);      // src/Tracking.cc:431-452
//
// The class keeps the reference's surface: StaticResize, BlobFromImage, DecodeOutputs, Detect, InsertImage / CheckFrames / CheckResult / GetResult / Run,
// RequestFinish / CheckFinish / SetFinish / isFinished, struct Object.  StaticResize and BlobFromImage are ONE kernel here: StaticResize uploads the frame and runs
// it, BlobFromImage returns the device blob it left.
//
// Two cases go through the host's literal decode (csrc/yolox_internal.h) instead of the device's result, so that what comes back is the reference's own:
//   - the library reports n_tied > 0: the reference's quicksort orders equal probs by its own swaps, the device by proposal index;
//   - the library returns EAO_ERR_CAPACITY: the reference has no cap on proposals.
// Both copy the head output to the host (eao_yolox_head) first.  exp() is the library's on both paths: the double-precision exponential rounded once to float (the
// reference's own call is glibc's expf, which is not pinned).  Compile the including file with -ffp-contract=off on a target with fused
// multiply-add, as the library is.
//
// MatT: cols, rows, data (const unsigned char*, interleaved 8-bit colour), step (bytes between rows), empty().  Run() sleeps 5 ms between polls, as upstream does.
#pragma once

#include <chrono>
#include <cstdint>
#include <functional>
#include <list>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "adapter_detail.h"
#include "../../eao_fusion_amd/csrc/yolox_internal.h"

namespace eaofusion {

namespace yolox {
struct Rect { float x = 0, y = 0, width = 0, height = 0; };      // cv::Rect_<float>
struct Object {                                                  // include/YOLOX.h:36-46
    Rect rect;
    int label = 0;
    float prob = 0;
    int nFrames = 0;
    int lostFrames = 0;
    int idx = 0;
    int similarity = -1;
};
using Infer = std::function<void(const float* d_blob, float* d_prob, void* stream)>;
}  // namespace yolox

template <class MatT>
class YOLOX {
public:
    using Object = yolox::Object;
    enum Path { kNone = 0, kDevice = 1, kLiteral = 2 };

    explicit YOLOX(yolox::Infer infer, const eao_yolox_cfg* cfg = nullptr, bool rgb = false) : infer_(std::move(infer)), rgb_(rgb) {
        if (cfg) cfg_ = *cfg; else eao_yolox_cfg_default(&cfg_);
        detail::check(eao_yolox_create(&cfg_, &h_), "eao_yolox_create");
        eao_yolox_buffers(h_, &dBlob_, &dProb_, &stream_);
        raw_.resize((size_t)cfg_.max_proposals);
    }
    ~YOLOX() { eao_yolox_destroy(h_); }
    YOLOX(const YOLOX&) = delete;
    YOLOX& operator=(const YOLOX&) = delete;

    // :51-62 and :211-233 in one kernel; false where cv::resize would assert (an empty letterbox) or the library refuses the frame
    bool StaticResize(const MatT& img) {
        return eao_yolox_preprocess(h_, img.data, img.cols, img.rows, (int32_t)img.step, 0, 1, rgb_ ? 1 : 0, nullptr, 0) == EAO_OK;
    }
    const float* BlobFromImage() const { return dBlob_; }

    // :235-274 over a head output in HBM.  `scale` is recomputed from img_w, img_h by the library (the same float, :390).
    bool DecodeOutputs(const float* d_prob, std::vector<Object>& objects, const int img_w, const int img_h) {
        int32_t n = 0, nProposals = 0, nTied = 0;
        const eao_status st = eao_yolox_decode_device(h_, d_prob, 1, &img_w, &img_h, raw_.data(), (int32_t)raw_.size(), &n, &nProposals, &nTied, stream_);
        path_ = kNone;
        if (st == EAO_OK && nTied == 0) {
            fill(objects, raw_.data(), (size_t)n);
            path_ = kDevice;
            return true;
        }
        if (st != EAO_OK && st != EAO_ERR_CAPACITY) return false;
        // the reference's own order and its unbounded proposal list, on the host
        namespace Y = eao::yolox;
        Y::Geometry g;
        if (!Y::geometry(img_w, img_h, cfg_.input_size, &g)) return false;
        head_.resize((size_t)Y::num_anchors(cfg_.input_size) * (size_t)(5 + cfg_.num_classes));
        if (eao_yolox_head(h_, d_prob, 1, head_.data(), stream_) != EAO_OK) return false;
        std::vector<Y::Object> lit;
        Y::decode_literal(head_.data(), cfg_.input_size, cfg_.num_classes, cfg_.conf_thresh, cfg_.nms_thresh, g.r, img_w, img_h, false, Y::OurExp{}, lit);
        static_assert(sizeof(Y::Object) == sizeof(eao_yolox_object), "one record");
        fill(objects, reinterpret_cast<const eao_yolox_object*>(lit.data()), lit.size());
        path_ = kLiteral;
        return true;
    }

    // :369-410
    void Detect() {
        {
            std::unique_lock<std::mutex> lock(mMutexYOLOXQueue);
            frame = IMGQueue.front();
            IMGQueue.clear();
        }
        std::vector<Object> objects;
        if (frame.empty()) return;
        if (!StaticResize(frame)) return;
        infer_(dBlob_, dProb_, stream_);
        if (!DecodeOutputs(dProb_, objects, frame.cols, frame.rows)) return;
        {
            std::unique_lock<std::mutex> lock(mMutexResQueue);
            ResQueue.push_back(objects);
        }
    }

    void GetResult(std::vector<Object>& output) {
        std::unique_lock<std::mutex> lock(mMutexResQueue);
        output = ResQueue.front();
        ResQueue.clear();
    }
    void Run() {
        mbFinished = false;
        while (1) {
            if (CheckFrames()) Detect();
            else std::this_thread::sleep_for(std::chrono::microseconds(5000));
            if (CheckFinish()) break;
        }
        SetFinish();
    }
    bool CheckFrames() { std::unique_lock<std::mutex> lock(mMutexYOLOXQueue); return !IMGQueue.empty(); }
    bool CheckResult() { std::unique_lock<std::mutex> lock(mMutexResQueue); return !ResQueue.empty(); }
    void InsertImage(MatT rgb) { std::unique_lock<std::mutex> lock(mMutexYOLOXQueue); IMGQueue.push_back(rgb); }
    void RequestFinish() { std::unique_lock<std::mutex> lock(mMutexFinish); mbFinishRequested = true; }
    bool CheckFinish() { std::unique_lock<std::mutex> lock(mMutexFinish); return mbFinishRequested; }
    void SetFinish() { std::unique_lock<std::mutex> lock(mMutexFinish); mbFinished = true; }
    bool isFinished() { std::unique_lock<std::mutex> lock(mMutexFinish); return mbFinished; }

    Path lastPath() const { return path_; }      // which decode the last DecodeOutputs returned
    eao_yolox* handle() const { return h_; }

private:
    static void fill(std::vector<Object>& out, const eao_yolox_object* r, size_t n) {
        out.assign(n, Object{});
        for (size_t i = 0; i < n; i++) {
            out[i].rect.x = r[i].x; out[i].rect.y = r[i].y; out[i].rect.width = r[i].w; out[i].rect.height = r[i].h;
            out[i].label = r[i].label; out[i].prob = r[i].prob;
        }
    }

    yolox::Infer infer_;
    bool rgb_;
    eao_yolox_cfg cfg_{};
    eao_yolox* h_ = nullptr;
    float *dBlob_ = nullptr, *dProb_ = nullptr;
    void* stream_ = nullptr;
    std::vector<eao_yolox_object> raw_;
    std::vector<float> head_;
    Path path_ = kNone;
    MatT frame;
    bool mbFinishRequested = false, mbFinished = false;
    std::list<MatT> IMGQueue;
    std::list<std::vector<Object>> ResQueue;
    std::mutex mMutexFinish, mMutexYOLOXQueue, mMutexResQueue;
};

// src/Tracking.cc:431-452: the detections Tracking keeps (prob >= 0.5, the class list), as BoxSE rows sorted by score.  BoxT: m_class, m_score, x, y, width, height.
template <class BoxT>
std::vector<BoxT> TrackingBoxes(const std::vector<yolox::Object>& objs) {
    std::vector<BoxT> boxes;
    for (const yolox::Object& o : objs) {
        if (!eao::yolox::tracking_keeps(eao::yolox::Object{0, 0, 0, 0, o.prob, o.label})) continue;
        BoxT box{};
        box.m_class = o.label;
        box.m_score = o.prob;
        box.x = o.rect.x;
        box.y = o.rect.y;
        box.width = o.rect.width;
        box.height = o.rect.height;
        boxes.push_back(box);
    }
    std::sort(boxes.begin(), boxes.end(), [](BoxT a, BoxT b) -> bool { return a.m_score > b.m_score; });
    return boxes;
}

}  // namespace eaofusion
