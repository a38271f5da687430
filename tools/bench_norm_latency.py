#!/usr/bin/env python3
"""Each launch alone, several timings per row (GPU box): the bf16 batch-norm kernels of the training step -- phx_norm_apply_fused,
phx_norm_apply_pool, phx_norm_bwd_reduce, phx_norm_bwd_apply_fused, phx_bn_bwd_onepass -- as tools/bench_norm.py and
tools/bench_onepass.py time them (20 launches between two events), over the shapes given on the command line.
usage: [PHX_LIB=other/libphx.so] bench_norm_latency.py [--repeats 5] [--label NAME] B,H,W,C [B,H,W,C ...]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phiseg_code_amd import runtime as rt  # noqa: E402

args = sys.argv[1:]
repeats, label = 5, os.path.basename(os.environ.get("PHX_LIB", "libphx.so"))
while args and args[0].startswith("--"):
    if args[0] == "--repeats":
        repeats = int(args[1])
    elif args[0] == "--label":
        label = args[1]
    args = args[2:]
shapes = [tuple(int(v) for v in a.split(",")) for a in args] or [(64, 16, 16, 192)]
L = rt.lib()
S = torch.cuda.current_stream().cuda_stream
BF, NREP, N = rt.BF16, 4, 20
nbar = int(L.bn_bwd_onepass_barrier_words())


def timings(fn, before=None):
    out = []
    for _ in range(repeats):
        if before:
            before()
        fn(0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(N):
            fn(i + 1)
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / N)
    return out


for B, H, W, C in shapes:
    P = B * H * W
    x = torch.randn(P, C, device="cuda").to(torch.bfloat16)
    dA = torch.randn(P, C, device="cuda").to(torch.bfloat16)
    y, dx, yp = torch.empty_like(x), torch.empty_like(x), torch.empty(P // 4, C, dtype=torch.bfloat16, device="cuda")
    z = lambda n: torch.zeros(n, device="cuda")
    sums = torch.stack([x.float().sum(0), (x.float() ** 2).sum(0)], 1).contiguous()
    gamma, beta = torch.ones(C, device="cuda"), z(C)
    mean, rstd, scale, shift = z(C), z(C), z(C), z(C)
    sums2, dg, db = z(NREP * 2 * C), z(C), z(C)
    bars = torch.zeros(N + 1, nbar, dtype=torch.int32, device="cuda")
    rows = [
        ("apply", lambda i: L.norm_apply_fused(x.data_ptr(), BF, sums.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), 1e-3, y.data_ptr(), BF,
                                               mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, None, 0.0, 1, P, C, C,
                                               1, S), None),
        ("apply_pool", lambda i: L.norm_apply_pool(x.data_ptr(), sums.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), 1e-3, y.data_ptr(),
                                                   yp.data_ptr(), mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, None,
                                                   0.0, 1, P, C, C, H, W, 1, S), None),
        ("bwd_reduce", lambda i: L.norm_bwd_reduce(dA.data_ptr(), BF, x.data_ptr(), BF, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                                                   rstd.data_ptr(), sums2.data_ptr(), 1, P, C, C, 1, NREP, S), None),
        ("bwd_apply", lambda i: L.norm_bwd_apply_fused(dA.data_ptr(), BF, x.data_ptr(), BF, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                                                       rstd.data_ptr(), gamma.data_ptr(), sums2.data_ptr(), dx.data_ptr(), BF, dg.data_ptr(),
                                                       db.data_ptr(), 1, P, C, C, 1, NREP, S), None),
    ]
    if L.bn_bwd_onepass_supported(P, C, 1):
        rows.append(("onepass", lambda i: L.bn_bwd_onepass(dA.data_ptr(), x.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                                                           rstd.data_ptr(), gamma.data_ptr(), sums2.data_ptr(), bars[i].data_ptr(), dx.data_ptr(),
                                                           dg.data_ptr(), db.data_ptr(), P, C, 1, NREP, S), lambda: bars.zero_()))
    for name, fn, before in rows:
        t = timings(fn, before)
        print("%-12s %-10s (%d,%d,%d,%d) %5.1f MB  us: %s   median %6.2f  spread %5.2f" % (
            label, name, B, H, W, C, P * C * 2 / 1e6, " ".join("%6.2f" % v for v in t), sorted(t)[len(t) // 2], max(t) - min(t)), flush=True)
    assert int(bars[:, 288].sum()) == 0, "grid barrier timed out"
