"""include/eaofusion/adapter_detail.h -- the status check, the cv::Mat reads and writes, the epipole, the FeatureVector flattening and the RANSAC draw the
class-surface headers share -- held to literals by tests/cpp/adapter_detail_test.cpp, a program of its own built with -fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adapter_detail_helpers_against_literals(tmp_path):
    exe = str(tmp_path / "adapter_detail_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DEAOFUSION_FORCE_CV_COMPAT",
                         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "adapter_detail_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "adapter_detail: all as written" in run.stdout and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr
