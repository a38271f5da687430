#!/usr/bin/env python3
"""Each launch alone (GPU box): the small-map k_conv3x3_mfma launches of the training step, in the shapes and forms of
tools/trace_conv_prologue.py -- 20 launches between two events per timing, five timings per row, median and spread (max - min).
  [PHX_LIB=other/libphx.so] bench_conv_prologue.py [--label NAME]        one arm; rows go to stdout
  bench_conv_prologue.py --compare FILE A B                             rows of labels A and B in FILE side by side: B counts as faster
                                                                        (slower) only when the medians differ by more than the larger spread
The plan-first arm is the same tree built with tools/build_variant.sh NAME -DPHX_CONV_LOADS_FIRST=0."""
import os
import re
import sys

if sys.argv[1:2] == ["--compare"]:
    path, a, b = sys.argv[2:5]
    rows = {}
    for ln in open(path):
        m = re.match(r"(\S+)\s+(\S+)\s+(.+?)\s+us:.*median\s+([\d.]+)\s+spread\s+([\d.]+)", ln)
        if m:
            rows.setdefault((m.group(2), m.group(3).strip()), {})[m.group(1)] = (float(m.group(4)), float(m.group(5)))
    print("%-22s %-17s %20s %20s %8s  %s" % ("(B,H,W,K,N)", "form", a + " median (spread)", b + " median (spread)", "delta", "verdict"))
    for (shape, form), arms in rows.items():
        if a in arms and b in arms:
            (ma, sa), (mb, sb) = arms[a], arms[b]
            verdict = "same within spread" if abs(ma - mb) <= max(sa, sb) else ("faster" if mb < ma else "SLOWER")
            print("%-22s %-17s %12.2f (%5.2f) %12.2f (%5.2f) %+7.2f  %s" % (shape, form, ma, sa, mb, sb, mb - ma, verdict))
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trace_conv_prologue import SHAPES, forms  # noqa: E402

label = os.path.basename(os.environ.get("PHX_LIB", "libphx.so"))
if sys.argv[1:2] == ["--label"]:
    label = sys.argv[2]
N_LAUNCH, REPEATS = 20, 5
for shape in SHAPES:
    fl, keep, pl = forms(*shape)
    for name, ksplit, run in fl:
        t = []
        for _ in range(REPEATS):
            run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(N_LAUNCH):
                run()
            e1.record()
            torch.cuda.synchronize()
            t.append(1e3 * e0.elapsed_time(e1) / N_LAUNCH)
        print("%-10s %-22s %-17s us: %s   median %6.2f  spread %5.2f" % (label, ",".join(str(v) for v in shape), name,
                                                                         " ".join("%6.2f" % v for v in t), sorted(t)[len(t) // 2], max(t) - min(t)), flush=True)
