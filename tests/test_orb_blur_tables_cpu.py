"""The operand tables of the matrix-core blur (eao_fusion_amd/csrc/orb_blur_tables.h) as plain C++ without a GPU.  tests/cpp/orb_blur_tables_test.cpp replays
the kernel's tile products from the tables in integer arithmetic -- operand fragments, accumulator layout, byte split and recombination as k_blur7_mfma has them --
against the direct 7 x 7 blur on the eight level sizes of a 320 x 240 frame and the smallest sizes the path accepts, with random, all-0, all-255, checkerboard and
0 / 255 noise images, and asserts that every table entry fits int8 and every table column sums to 257 or 0.  Built and run under AddressSanitizer + UBSan as a
program of its own: no table write and no replayed pixel load leaves its array."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blur_tables_replay_under_asan(tmp_path):
    exe = str(tmp_path / "orb_blur_tables_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "cpp", "orb_blur_tables_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(env, ASAN_OPTIONS="halt_on_error=1 detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all as the direct blur" in run.stdout and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr
