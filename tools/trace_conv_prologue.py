#!/usr/bin/env python3
"""dev (GPU box): where block 0 of a small-map k_conv3x3_mfma launch spends its cycles, from the kernel's own stamps (phx_debug_set_trace;
the block's end from phx_debug_set_blocklog).  One launch per shape and form, intervals in shader-clock cycles:
  entry -> plan   slot 10 -> 0   (loads-first builds: entry -> filter-slab loads issued; plan-first builds: entry -> staging plan done)
  plan -> issued  slot 0 -> 1    (-> every load of the first chunk issued)
  issued -> LDS   slot 1 -> 2    (-> the staging stores of the stamped chunk begin: loads-first builds stamp the block's FIRST chunk,
  LDS -> MFMA     slot 2 -> 4       plan-first builds -- the order before, -DPHX_CONV_LOADS_FIRST=0 -- its SECOND, '-' where it has none)
  MFMA -> end     slot 4 -> the block's end
and the share of entry -> issued in the block's duration.
usage: [PHX_LIB=other/libphx.so] trace_conv_prologue.py [--label NAME]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phiseg_code_amd import runtime as rt  # noqa: E402

SHAPES = [(64, 2, 2, 192, 192), (64, 4, 4, 192, 192), (64, 8, 8, 192, 192), (64, 8, 8, 128, 128), (64, 16, 16, 192, 192), (64, 32, 32, 128, 128)]
label = os.path.basename(os.environ.get("PHX_LIB", "libphx.so"))
if sys.argv[1:2] == ["--label"]:
    label = sys.argv[2]
L = rt.lib()
S = torch.cuda.current_stream().cuda_stream


def forms(B, H, W, K, N):
    """(name, split-K factor of the launch, launch) of every form the plan allows for the shape"""
    pl = L.conv3x3_plan(B, H, W, K, N)
    x = torch.randn(B, H, W, K, device="cuda").to(torch.bfloat16)
    wf = (torch.randn(9 * K * N, device="cuda") / (9 * K) ** 0.5).to(torch.bfloat16)
    y = torch.empty(B, H, W, N, device="cuda", dtype=torch.bfloat16)
    yf = torch.empty(B, H, W, N, device="cuda")
    ws = torch.empty(max(int(pl.ws_bytes) // 4, 1), device="cuda")
    wsp, wsb = (ws.data_ptr(), int(pl.ws_bytes)) if pl.ws_bytes else (None, 0)
    part = torch.zeros(max(pl.tiles, 1), 2, N, device="cuda")
    sums = torch.zeros(N, 2, device="cuda")
    keep = (x, wf, y, yf, ws, part, sums)
    out = []
    if pl.f32out_ok and pl.ksplit > 1:
        out.append(("f32 slices kept", pl.ksplit, lambda: L.conv3x3_mfma_bf16_f32out(x.data_ptr(), None, 0, wf.data_ptr(), yf.data_ptr(), 0, wsp, wsb, B, H, W, K, N, S)))
    if pl.ksplit > 1:
        out.append(("split-K + finish", pl.ksplit, lambda: L.conv3x3_mfma_bf16_ws(x.data_ptr(), wf.data_ptr(), y.data_ptr(), None, 0, None, wsp, wsb, B, H, W, K, N, S)))
    if pl.stats_atomic_ok:
        out.append(("atomic stats", 1, lambda: L.conv3x3_mfma_bf16_stats_atomic(x.data_ptr(), wf.data_ptr(), y.data_ptr(), None, 0, sums.data_ptr(), B, H, W, K, N, S)))
    out.append(("per-tile stats", 1, lambda: L.conv3x3_mfma_bf16(x.data_ptr(), wf.data_ptr(), y.data_ptr(), None, 0, part.data_ptr(), B, H, W, K, N, S)))
    return out, keep, pl


if __name__ == "__main__":
    tr = torch.zeros(16, dtype=torch.int64, device="cuda")
    log = torch.zeros(1 << 16, 4, dtype=torch.int64, device="cuda")
    print("# %s: block 0, cycles; share = (entry -> issued) / (entry -> end)" % label)
    print("%-22s %-17s %6s %11s %11s %11s %11s %11s %8s %6s" % ("(B,H,W,K,N)", "form", "ksplit", "entry->plan", "plan->iss.", "iss.->LDS", "LDS->MFMA",
                                                              "MFMA->end", "total", "share"))
    for shape in SHAPES:
        fl, keep, pl = forms(*shape)
        for name, ksplit, run in fl:
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            tr.zero_()
            log[:1].zero_()
            L.debug_set_trace(tr.data_ptr())
            L.debug_set_blocklog(log.data_ptr())
            try:
                run()
                torch.cuda.synchronize()
            finally:
                L.debug_set_trace(None)
                L.debug_set_blocklog(None)
            t = [int(v) for v in tr.cpu()]
            end = int(log[0, 1])
            d = lambda a, b: "%11d" % (b - a) if a and b else "%11s" % "-"      # noqa: E731
            tot = end - t[10] if t[10] and end else 0
            share = "%5.1f%%" % (100.0 * (t[1] - t[10]) / tot) if tot and t[1] else "-"
            print("%-22s %-17s %6d %s %s %s %s %s %8d %6s" % (",".join(str(v) for v in shape), name, ksplit, d(t[10], t[0]), d(t[0], t[1]),
                                                             d(t[1], t[2]), d(t[2], t[4]), d(t[4], end), tot, share), flush=True)
