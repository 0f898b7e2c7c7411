"""How eao_local_ba_batch deals its windows to set-up threads and window groups (eao_fusion_amd/csrc/ba_batch_plan.h) as plain C++ without a GPU.
tests/cpp/ba_batch_plan_test.cpp enumerates every batch size up to 96 with every value of the switches, seven core counts and the latency marker (564 480 plans: thread and
group counts in range, no empty group, whole rows of eight, group_of consistent with the group starts) and holds 27 plans to literal values, under AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ba_batch_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ba_batch_plan_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "cpp", "ba_batch_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    assert "warning" not in cc.stderr, cc.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}      # (tools/run_sanitizers.sh runs the suite under a preloaded ASan runtime: not in this process)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(env, ASAN_OPTIONS="halt_on_error=1 detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-4000:]
    assert "564480 plans enumerated, 0 break an invariant" in run.stdout and "27 pinned plans, 0 differ" in run.stdout and "all plans as required" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr
