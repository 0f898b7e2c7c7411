"""The operand tables of the matrix-core pyramid resize (eao_fusion_amd/csrc/orb_resize_tables.h) as plain C++ without a GPU.
tests/cpp/orb_resize_tables_test.cpp replays the kernel's tile products from the tables in integer arithmetic -- operand fragments, accumulator layout, weight
split and recombination, the in-lane vertical tail as k_resize_mfma has them -- against the direct formula, every pixel of every level: 640 x 480, 320 x 240,
752 x 480, 1241 x 376 and 96 x 76 at 1.2 / 8 levels, 640 x 480 at 1.1 / 8, 1.5 / 6 and 2.0 / 4, with random, all-0, all-255, checkerboard, 0 / 255 noise and
vertical-stripe images (frames wider than 320: random, all-255 and stripes); a factor of 2.5 and a 60-byte source row are refused.  Asserted on the way: every non-zero weight pair lies inside its window, every piece
fits int8, no window ends beyond what may be read, the column offsets are 128 (a0 + a1).  Built and run under AddressSanitizer + UBSan as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resize_tables_replay_under_asan(tmp_path):
    exe = str(tmp_path / "orb_resize_tables_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "cpp", "orb_resize_tables_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(env, ASAN_OPTIONS="halt_on_error=1 detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all as the direct formula" in run.stdout and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr
