"""An exception inside the threaded map walk of eaofusion::BundleAdjustment (include/eaofusion/OptimizerImpl.h) reaches the caller instead of ending the
process: tests/cpp/map_walk_throw_test.cpp, a program of its own over stand-in keyframes and 3 x 4096 map points with the library call stubbed, built plain and
with -fsanitize=thread.  One map point's observation accessor throws std::runtime_error("boom") -- in range 0, which the calling thread walks, or in the last
range, which a helper thread walks; with one in each, the message of the lower range arrives."""
import os
import platform
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["plain", "tsan"])
def program(request, tmp_path_factory):
    if request.param == "tsan" and os.environ.get("EAO_HOST_SAN"):
        pytest.skip("the suite runs under tools/run_sanitizers.sh's AddressSanitizer runtime, which a ThreadSanitizer program cannot start beside")
    exe = str(tmp_path_factory.mktemp("map_walk_throw") / ("map_walk_throw_" + request.param))
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT"] + (["-fsanitize=thread"] if request.param == "tsan" else []) +
                        ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "map_walk_throw_test.cpp"), "-o", exe, "-pthread"],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    return exe


def _run(exe, mode):
    # ThreadSanitizer's shadow layout does not fit a kernel with more than 28 bits of mmap randomisation ("unexpected memory mapping" at start-up): its
    # program runs with a fixed layout, which is the program's own personality and nothing of the machine's
    fixed = [shutil.which("setarch"), platform.machine(), "-R"] if exe.endswith("_tsan") and shutil.which("setarch") else []
    if fixed and subprocess.run(fixed + ["true"], capture_output=True).returncode != 0:      # (a sandbox may refuse the personality call)
        fixed = []
    run = subprocess.run(fixed + [exe, mode], capture_output=True, text=True, timeout=300, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0 and "Sanitizer" not in run.stderr, run.stdout[-1000:] + run.stderr[-3000:]      # (an escaped exception is std::terminate: -6)
    threads = re.search(r"^walk_threads (\d+)$", run.stdout, re.M)
    assert threads, run.stdout[-1000:]
    return run.stdout, int(threads.group(1))


def test_the_walk_without_an_exception_is_unchanged(program):
    out, _ = _run(program, "none")
    assert "returned: %d edges" % (3 * 4096) in out and "caught" not in out


def test_an_exception_in_the_callers_own_range_arrives(program):
    out, _ = _run(program, "caller")
    assert "caught: boom\n" in out and "returned" not in out


def test_an_exception_in_a_helpers_range_arrives(program):
    out, threads = _run(program, "helper")
    assert "caught: boom\n" in out and "returned" not in out      # (with one walk thread the last range is the caller's too: still caught)
    if threads < 2:
        pytest.skip("hardware_concurrency() gave this run one walk thread: no helper thread to throw in")
    assert threads <= 3


def test_the_exception_of_the_lower_range_arrives_first(program):
    out, _ = _run(program, "both")
    assert "caught: boom in range 0\n" in out and "last range" not in out
