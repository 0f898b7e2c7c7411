"""The host set-up of a bundle adjustment (eao_fusion_amd/csrc/ba_setup.h: edge validation and counts, the map-scale path's observer / camera lists and pairs, the active
structure, the launch order of the pair kernels) as plain C++ without a GPU.  tests/cpp/ba_setup_test.cpp holds every stage to a naive reference of its own on three small
maps, compares the serial, crew-run and crew-session forms array by array at 2, 5 and 12 threads, and feeds it the malformed edge lists the library refuses -- once under
AddressSanitizer + UBSan (no stage writes outside its arrays, whatever the caller's indices) and once under ThreadSanitizer (the passes of a session do not race)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags, options", [
    (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], dict(ASAN_OPTIONS="halt_on_error=1 detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")),
    (["-fsanitize=thread"], dict(TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1")),
], ids=["asan_ubsan", "tsan"])
def test_ba_setup_stages_under_sanitizers(tmp_path, flags, options):
    exe = str(tmp_path / "ba_setup_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + ["-pthread", os.path.join(ROOT, "tests", "cpp", "ba_setup_test.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}      # (tools/run_sanitizers.sh runs the suite under a preloaded ASan runtime: not in this process)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(env, **options))
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-4000:]
    assert "all as the reference" in run.stdout and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr
