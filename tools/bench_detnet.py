"""Timing record of the detector network (profiles/detnet_timing.txt): YOLOX-s (depth 0.33, width 0.5, 80 classes) at S = 640 through eao_detnet_forward, batch 1
and batch 8, against PyTorch-ROCm's eager float32 forward of tests/detnet_torch.py on the same weights and the -O3 host walk (tools/detnet_walk.cpp) on one thread.

    python tools/bench_detnet.py [--reps 100] [--size 640] [--no-host] > profiles/detnet_timing.txt

Device time is taken with events on the stream of the calls, wall time around call + wait; both are medians.  Per op: the median of 20 profiled forwards
(eao_detnet_set_profiling), the FLOPs (2 per multiply-add) and the fraction of the f32 matrix peak (157.3 TFLOP/s: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PEAK = 157.3e12
KINDS = ("FOCUS", "CONV", "MAXPOOL", "UPSAMPLE2")


def timed(fn, reps, warmup, torch):
    """(median device ms, median wall ms) of fn(), which enqueues on the current torch stream"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return float(np.median(dev)), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    import detnet_models as M
    import detnet_torch as T
    import export_detnet as X
    from eao_fusion_amd import detnet as D
    S = a.size
    tnet = T.randomised(0.33, 0.5, 80, seed=640)
    model = X.export(tnet)
    data = model.tobytes()
    net = D.Detnet(data, S, max_batch=8)
    info = net.info()
    print("# detector network: yolox(0.33, 0.5, 80) at S = %d on %s" % (S, torch.cuda.get_device_name(0)))
    print("# %d tensors, %d ops, weights %.1f MiB, activations (max_batch 8) %.1f MiB, %.2f GFLOP per frame" % (info["tensors"], info["ops"], info["weight_bytes"] / 2 ** 20,
                                                                                                               info["activation_bytes"] / 2 ** 20, info["flops"] / 1e9))
    blobs = torch.from_numpy(M.blob(S, 1, batch=8)).cuda()
    prob = torch.zeros((8, net.A, net.row), dtype=torch.float32, device="cuda")
    tnet = tnet.cuda()
    stream = torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        ref = tnet(blobs[:1])
    net.forward(blobs.data_ptr(), prob.data_ptr(), 1, stream)
    torch.cuda.synchronize()
    print("# largest difference between the two heads (ours is the fmaf chain, torch's sums are blocked): %.3e" % float((ref[0] - prob[0]).abs().max()))
    print("%-28s %6s %12s %12s %10s %8s" % ("forward", "batch", "device ms", "wall ms", "TFLOP/s", "of peak"))
    for batch in (1, 8):
        d, w = timed(lambda: net.forward(blobs.data_ptr(), prob.data_ptr(), batch, stream), a.reps, 10, torch)
        tf = info["flops"] * batch / (d * 1e-3)
        print("%-28s %6d %12.3f %12.3f %10.2f %7.1f%%" % ("eao_detnet_forward", batch, d, w, tf / 1e12, 100 * tf / PEAK))
        with torch.no_grad():
            d, w = timed(lambda: tnet(blobs[:batch]), a.reps, 10, torch)
        tf = info["flops"] * batch / (d * 1e-3)
        print("%-28s %6d %12.3f %12.3f %10.2f %7.1f%%" % ("torch eager float32", batch, d, w, tf / 1e12, 100 * tf / PEAK))
    # per op
    net.set_profiling(True)
    for batch in (1, 8):
        runs = []
        for _ in range(20):
            net.forward(blobs.data_ptr(), prob.data_ptr(), batch, stream)
            runs.append(net.last_op_ms())
        ms = np.median(np.stack(runs), axis=0)
        print("\n# per op, batch %d (profiled: an event around every op; sum %.3f ms)" % (batch, float(ms.sum())))
        print("%4s %-10s %-22s %5s %6s %6s %2s %2s %10s %9s %8s" % ("op", "kind", "map", "M", "Cin", "Cout", "k", "s", "MFLOP", "ms", "of peak"))
        by_kind = {}
        for i, o in enumerate(model.ops):
            hw = model.shape(o["src"], S)[:2] if o["src"] else (S, S)
            fl = 0.0
            if o["kind"] == D.CONV:
                ho = hw[0] // o["stride"]
                fl = 2.0 * o["dst_c"] * o["k"] * o["k"] * o["src_c"] * ho * ho * batch
            by_kind.setdefault(KINDS[o["kind"]], [0.0, 0.0])
            by_kind[KINDS[o["kind"]]][0] += float(ms[i])
            by_kind[KINDS[o["kind"]]][1] += fl
            print("%4d %-10s %-22s %5d %6d %6d %2d %2d %10.1f %9.4f %7.1f%%" % (i, KINDS[o["kind"]], "%d x %d" % hw, batch * (hw[0] // max(o["stride"], 1)) ** 2 if o["kind"] == D.CONV else 0,
                                                                             o["src_c"], o["dst_c"], o["k"], o["stride"], fl / 1e6, ms[i], 100 * fl / (ms[i] * 1e-3) / PEAK if ms[i] > 0 else 0))
        for k, (t, fl) in sorted(by_kind.items()):
            print("# %-10s %9.3f ms %12.1f MFLOP" % (k, t, fl / 1e6))
    net.set_profiling(False)
    if not a.no_host:
        exe = M.walk_binary(("-O3",))
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "m.bin")
            open(p, "wb").write(data)
            out = subprocess.run([exe, "bench", p, str(S), "1"], capture_output=True, text=True, check=True).stdout
        print("\n# -O3 host walk, one thread, one frame: %s ms" % out.split("host_walk_ms")[1].split()[0])


if __name__ == "__main__":
    main()
