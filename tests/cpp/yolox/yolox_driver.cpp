// yolox_driver.cpp -- drives include/eaofusion/YOLOX.h the way System / Tracking drive the reference's detector, over a stand-in cv::Mat.  Linked with
// yolox_stub.cpp (tests/test_yolox_class_cpu.py: a recording library, -DYOLOX_STUB) or with the real library and yolox_upload_hip.cpp (tests/test_gpu_yolox.py).
// The "network" copies a recorded head output into the device buffer it is handed.
//
//   script <n_tied> <status> <n_proposals>                     (stub only) what the next decode calls answer
//   detect <S> <max_proposals> <img_w> <img_h> <floats ...>    one frame through InsertImage / Detect / GetResult: the path taken and the objects
//   queue <S> <img_w> <img_h> <floats ...>                     two frames inserted, Run() on a thread until a result is there, then RequestFinish
//   boxes <n> <prob label x y w h> ...                         TrackingBoxes
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <thread>
#include <vector>

#include <eaofusion/YOLOX.h>

extern "C" int yolox_driver_upload(void* dst, const void* src, size_t bytes);
#ifdef YOLOX_STUB
extern "C" void yolox_stub_script(int nTied, int status, int nProposals);
#endif

struct Mat {      // the members of cv::Mat the adapter reads
    int cols = 0, rows = 0;
    size_t step = 0;
    const unsigned char* data = nullptr;
    std::shared_ptr<std::vector<unsigned char>> store;
    bool empty() const { return data == nullptr; }
};
struct BoxSE { int m_class; float m_score; int x, y, width, height; };

static float unhex(const std::string& s) {
    const uint32_t b = (uint32_t)std::stoul(s, nullptr, 16);
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
static Mat frame_of(int w, int h) {
    Mat m;
    m.cols = w; m.rows = h; m.step = (size_t)3 * w;
    m.store = std::make_shared<std::vector<unsigned char>>((size_t)3 * w * h);
    uint64_t st = 99;
    for (unsigned char& p : *m.store) { st = st * 6364136223846793005ull + 1442695040888963407ull; p = (unsigned char)(st >> 56); }
    m.data = m.store->data();
    return m;
}
static std::vector<float> floats(std::istringstream& in) {
    std::vector<float> v;
    std::string tok;
    while (in >> tok) v.push_back(unhex(tok));
    return v;
}
static void print_objects(const std::vector<eaofusion::yolox::Object>& objs) {
    std::printf("objects %zu\n", objs.size());
    for (const auto& o : objs) std::printf("%08x %08x %08x %08x %08x %d\n", bits(o.rect.x), bits(o.rect.y), bits(o.rect.width), bits(o.rect.height), bits(o.prob), o.label);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "script") {
#ifdef YOLOX_STUB
            int a, b, c;
            in >> a >> b >> c;
            yolox_stub_script(a, b, c);
#endif
        } else if (cmd == "detect" || cmd == "queue") {
            int S, cap = 0, w, h;
            in >> S;
            if (cmd == "detect") in >> cap;
            in >> w >> h;
            const std::vector<float> head = floats(in);
            eao_yolox_cfg cfg;
            eao_yolox_cfg_default(&cfg);
            cfg.input_size = S;
            if (cap) cfg.max_proposals = cap;
            int inferCalls = 0;
            eaofusion::YOLOX<Mat> det([&](const float* blob, float* prob, void*) {
                inferCalls++;
                if (!blob || yolox_driver_upload(prob, head.data(), head.size() * 4) != 0) std::printf("upload failed\n");
            }, &cfg);
            if (cmd == "detect") {
                det.InsertImage(frame_of(w, h));
                std::printf("frames %d result %d\n", det.CheckFrames() ? 1 : 0, det.CheckResult() ? 1 : 0);
                det.Detect();
                std::printf("frames %d result %d infer %d\n", det.CheckFrames() ? 1 : 0, det.CheckResult() ? 1 : 0, inferCalls);
                if (!det.CheckResult()) { std::printf("no result\n"); continue; }
                std::vector<eaofusion::yolox::Object> objs;
                det.GetResult(objs);
                std::printf("path %s\n", det.lastPath() == eaofusion::YOLOX<Mat>::kDevice ? "device" : "literal");
                print_objects(objs);
                std::printf("result %d\n", det.CheckResult() ? 1 : 0);
            } else {
                det.InsertImage(frame_of(w, h));
                det.InsertImage(frame_of(w, h));      // Detect takes the front and clears the queue (:371-375)
                std::thread t([&] { det.Run(); });
                while (!det.CheckResult()) std::this_thread::yield();
                det.RequestFinish();
                t.join();
                std::vector<eaofusion::yolox::Object> objs;
                det.GetResult(objs);
                std::printf("finished %d infer %d frames %d objects %zu\n", det.isFinished() ? 1 : 0, inferCalls, det.CheckFrames() ? 1 : 0, objs.size());
            }
        } else if (cmd == "boxes") {
            size_t n;
            in >> n;
            std::vector<eaofusion::yolox::Object> objs(n);
            for (auto& o : objs) {
                std::string p, x, y, bw, bh;
                in >> p >> o.label >> x >> y >> bw >> bh;
                o.prob = unhex(p); o.rect.x = unhex(x); o.rect.y = unhex(y); o.rect.width = unhex(bw); o.rect.height = unhex(bh);
            }
            for (const BoxSE& b : eaofusion::TrackingBoxes<BoxSE>(objs)) std::printf("box %d %08x %d %d %d %d\n", b.m_class, bits(b.m_score), b.x, b.y, b.width, b.height);
            std::printf("end\n");
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
