#!/usr/bin/env python3
"""The conditioning gate of the irregular bundle-adjustment shapes (tests/ba_shapes.py), measured on the CPU oracle alone.

For every shape and every entry point it is used with (LocalBundleAdjustment; BundleAdjustment robust and not, 5 iterations on the windows and 8 on the maps): the oracle on the problem as built, then six
runs with every float32 entry of points / observations / poses moved ONE ulp up or down at random (monocular markers and the bottom row of the poses kept; no value moves
across zero).  Reported: does the LM schedule (iterations, and the outlier table of LocalBundleAdjustment) survive all six, and the largest displacement of poses and points
relative to the largest update.  tests/test_ba_shapes_cpu.py holds every line to "same" and to 0.7 * UPDATE_REL = 7e-5: a shape that is to be compared with another
implementation at UPDATE_REL must not sit right under that bar by itself.  Needs no GPU:
    python3 tools/ba_shape_bands.py > profiles/ba_shapes_oracle_bands.txt"""
import os
import sys
sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import ba_shapes as S
from oracle import oracle as O

O.build()
print(__doc__)
print("%-24s %-10s | %5s %6s %7s | %-9s %-10s %-10s" % ("shape", "entry", "free", "cams", "edges", "schedule", "poses", "points"))
worst = 0.0
for name in S.SHAPES:
    p, _ = S.shape(name)
    for entry in S.ENTRY_POINTS:
        b = S.oracle_band(O, entry, p)
        worst = max(worst, b["poses"], b["points"])
        print("%-24s %-10s | %5d %6d %7d | %-9s %-10.2e %-10.2e" % (name, entry, int((p["fixed"] == 0).sum()), len(p["poses"]), len(p["edge_cam"]),
                                                                    "same" if b["schedule_stable"] else "DIFFERENT", b["poses"], b["points"]))
        sys.stdout.flush()
print()
print("largest band: %.2e of the largest update" % worst)
