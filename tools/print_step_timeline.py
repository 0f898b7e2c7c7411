"""Kernel timeline of the last full ORB steps in a rocprofv3 kernel trace (tools/trace_step.sh):  python3 tools/print_step_timeline.py DIR [STEPS]

A step ends with the k_orient_describe launch that is followed by the next step's pyramid (a step may hold two description launches: the
lower levels' on the side stream, the upper levels' on the caller's).  Per step: every kernel with its queue, then per queue the time of
the first start and of the last end, the chain that ends last, and the span from the first description launch's end (the join) to the end."""
import csv, glob, re, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
nsteps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
name = lambda r: (re.search(r"(k_\w+)", r["Kernel_Name"]) or [None, "?"])[1]
marks = [(i, name(r)) for i, r in enumerate(rows) if name(r) in ("k_orient_describe", "k_resize", "k_resize_mfma", "k_pyramid_fused")]
ends = [i for (i, n), (_, n2) in zip(marks, marks[1:]) if n == "k_orient_describe" and n2 != "k_orient_describe"]   # last description launch of each complete step
S, E = lambda r: int(r["Start_Timestamp"]), lambda r: int(r["End_Timestamp"])
for k in range(len(ends) - 1 - nsteps, len(ends) - 1):      # (the trace's last step is left out: its successor is what delimits a step)
    a, b = ends[k] + 1, ends[k + 1] + 1
    t0 = S(rows[a])
    print("step span %.1f us (previous step's last kernel end -> this step's last kernel end)" % ((E(rows[b - 1]) - E(rows[a - 1])) / 1e3))
    for r in rows[a:b]:
        g = r.get("Grid_Size_X", "") or r.get("Grid_Size", "")
        print("  %-20s q%-3s grid %-8s %8.1f -> %8.1f  (%.1f)" % (name(r), r.get("Queue_Id", "?"), g, (S(r) - t0) / 1e3, (E(r) - t0) / 1e3, (E(r) - S(r)) / 1e3))
    queues = {}
    for r in rows[a:b]:
        queues.setdefault(r.get("Queue_Id", "?"), []).append(r)
    for q, rs in sorted(queues.items()):
        print("  queue %-3s %2d kernels, first start %7.1f, last end %7.1f (%s)" % (q, len(rs), (min(map(S, rs)) - t0) / 1e3, (max(map(E, rs)) - t0) / 1e3,
                                                                                   name(max(rs, key=E))))
    desc = [r for r in rows[a:b] if name(r) == "k_orient_describe"]
    before = [r for r in rows[a:b] if S(r) < S(desc[-1]) and r is not desc[-1]]
    last = max(before, key=E)
    print("  the last description launch starts %.1f us after the end of %s on queue %s, the chain that ends last in front of it; join -> end of step %.1f us"
          % ((S(desc[-1]) - E(last)) / 1e3, name(last), last.get("Queue_Id", "?"), (E(rows[b - 1]) - E(last)) / 1e3))
