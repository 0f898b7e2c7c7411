// detnet_driver.cpp -- include/eaofusion/YOLOXNet.h over a stand-in cv::Mat: constructs the detector from an engine file path, as the reference does
// (src/System.cc:112), runs one frame through Detect and prints the objects.  Linked with yolox_stub.cpp and detnet_stub.cpp (tests/test_detnet_class_cpu.py) or
// with the library (tests/test_gpu_detnet_adapter.py).
//
//     detnet_driver <model> <S> <max_proposals> <width> <height> <frame file: height x width x 3 bytes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include <eaofusion/YOLOXNet.h>

struct Mat {
    int cols = 0, rows = 0;
    const unsigned char* data = nullptr;
    size_t step = 0;
    bool empty() const { return !data; }
};

static unsigned bits(float f) { unsigned b; std::memcpy(&b, &f, 4); return b; }

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    eao_yolox_cfg cfg;
    eao_yolox_cfg_default(&cfg);
    cfg.input_size = std::atoi(argv[2]);
    cfg.max_proposals = std::atoi(argv[3]);
    const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
    std::vector<unsigned char> px((size_t)w * h * 3);
    std::ifstream in(argv[6], std::ios::binary);
    in.read((char*)px.data(), (std::streamsize)px.size());
    if (!in.good()) { std::printf("error: the frame file is short\n"); return 2; }
    try {
        eaofusion::YOLOXEngine<Mat> det{std::string(argv[1]), &cfg};
        std::printf("engine classes %d anchors %d\n", det.network().info().classes, det.network().info().anchors);
        Mat m;
        m.cols = w; m.rows = h; m.data = px.data(); m.step = (size_t)w * 3;
        det.InsertImage(m);
        det.Detect();
        std::printf("result %d path %d\n", det.CheckResult() ? 1 : 0, (int)det.lastPath());
        if (det.CheckResult()) {
            std::vector<eaofusion::yolox::Object> objs;
            det.GetResult(objs);
            std::printf("objects %zu\n", objs.size());
            for (const auto& o : objs) std::printf("%08x %08x %08x %08x %08x %d\n", bits(o.rect.x), bits(o.rect.y), bits(o.rect.width), bits(o.rect.height), bits(o.prob), o.label);
        }
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
