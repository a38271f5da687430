#!/usr/bin/env python3
"""What the many-class path costs on one MI355X (LABBOOK.md): one process, device events, alternating rounds.

    python tools/bench_many_class.py [--calls 50] [--rounds 7] [--steps 20] [--skip-step]

1. phx_residual_ce_wide at B = 64, 128 x 128, five levels (shifts 0 .. 4), every ds handed over, C in {9, 16, 19, 32}, beside
   phx_residual_ce at C = 8 on maps of the same geometry.  A round times every kernel once (`calls` back-to-back launches between two
   events); the figure is the median over `rounds` rounds, so a drift of the box meets all kernels alike.  Bytes are ALGORITHMIC: every
   level read once and its gradient written once (4 C bytes per level pixel each), labels read, s_out written.  ns_per_class_mb = time
   over those bytes; hbm_share = bytes / time over the 6.3 TB/s a float4 copy reaches on this part (the achievable HBM rate).
2. The phiseg_7_5 bf16 batch-64 training step at 19 classes against 2: time per replayed step (host clock between two waits over
   `steps` replays, as bench.py takes it), and from the plan's own
   wall-clock stamps (PHX_STAMPS=1, set here) the time inside the five 1x1 logit heads y_lvl0 .. y_lvl4 -- conv2d_direct above eight
   classes, phx_head1x1_* at two -- forward and backward, as a share of the step.  Operators of different lanes overlap, so the share
   is of operator time, and both sums are printed.
One JSON line per part."""
import argparse
import json
import os
import sys
import time

os.environ["PHX_STAMPS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12
B, H, W, SHIFTS = 64, 128, 128, (0, 1, 2, 3, 4)


def residual_ce_rows(calls, rounds):
    import numpy as np
    import torch
    from phiseg_code_amd import runtime as rt
    L = rt.lib()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    jobs = {}
    for C in (8, 9, 16, 19, 32):
        g = torch.Generator(device=dev).manual_seed(C)
        s = [torch.randn(B, H >> sh, W >> sh, C, device=dev, generator=g) for sh in SHIFTS]
        ds = [torch.empty_like(v) for v in s]
        lab = torch.randint(0, C, (B, H, W), device=dev, generator=g, dtype=torch.uint8)
        s_out = torch.empty(B, H, W, C, device=dev)
        sp, dsp, shp = rt.ptr_array([v.data_ptr() for v in s]), rt.ptr_array([v.data_ptr() for v in ds]), rt.int_array(list(SHIFTS))
        nbytes = sum(2 * 4 * v.numel() for v in s) + B * H * W + 4 * s_out.numel()
        if C <= 8:
            losses = torch.zeros(8 + 512, device=dev)
            fn = (lambda sp=sp, dsp=dsp, shp=shp, lab=lab, losses=losses, s_out=s_out, C=C:
                  L.residual_ce(sp, dsp, shp, len(SHIFTS), lab.data_ptr(), B, H, W, C, 1.0, 1.0 / B, losses.data_ptr(), s_out.data_ptr(), None, st))
        else:
            losses = torch.zeros(8, device=dev)
            wsb = int(L.residual_ce_wide_ws_bytes(B, H, W))
            work = torch.empty(wsb, dtype=torch.uint8, device=dev)
            fn = (lambda sp=sp, dsp=dsp, shp=shp, lab=lab, losses=losses, s_out=s_out, C=C, work=work, wsb=wsb:
                  L.residual_ce_wide(sp, dsp, shp, len(SHIFTS), lab.data_ptr(), B, H, W, C, 1.0, 1.0 / B, losses.data_ptr(), s_out.data_ptr(),
                                     None, work.data_ptr(), wsb, st))
        jobs[C] = (fn, nbytes, (s, ds, lab, s_out, losses))
    times = {C: [] for C in jobs}
    for C in jobs:                                   # warm-up
        for _ in range(10):
            jobs[C][0]()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for C in jobs:
            e0.record()
            for _ in range(calls):
                jobs[C][0]()
            e1.record()
            e1.synchronize()
            times[C].append(e0.elapsed_time(e1) * 1e3 / calls)      # us
    rows = []
    for C in jobs:
        us, nbytes = float(np.median(times[C])), jobs[C][1]
        rows.append(dict(C=C, entry="residual_ce" if C <= 8 else "residual_ce_wide", us=round(us, 2), min_us=round(min(times[C]), 2),
                         max_us=round(max(times[C]), 2), mbytes=round(nbytes / 1e6, 2), ns_per_class_mb=round(us * 1e3 / (nbytes / 1e6), 3),
                         hbm_share=round(nbytes / (us * 1e-6) / HBM_ACHIEVABLE, 4)))
    return rows


def step_row(nlabels, steps):
    import numpy as np
    import bench
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = bench.make_config(64, "bf16", nlabels=nlabels)
    model = phiseg_model.phiseg(cfg)
    sess = model.sess
    plan = sess.plan_for([model.loss_tot], True, 64, True)
    x, s = synthetic.make_batch(64, 128, nlabels, np.random.default_rng(0))
    plan.set_input("x_input", x)
    plan.set_input("s_input", s)
    sess.store.set_lr(1e-3)
    for _ in range(6):
        plan.run()
    plan.sync()
    t0 = time.perf_counter()                       # as bench.py times the step: host clock between two waits, `steps` replays
    for _ in range(steps):
        plan.run()
    plan.sync()
    step_ms = (time.perf_counter() - t0) * 1e3 / steps
    t = plan._stamp_buf.cpu().numpy().astype(np.int64)
    ops = [(ph, name, (t[i + 1] - t[i]) / 100.0, t[i] / 100.0, t[i + 1] / 100.0) for ph, name, lane, i in plan.stamps]      # us
    span = max(o[4] for o in ops) - min(o[3] for o in ops)
    total = sum(o[2] for o in ops)
    heads = [o for o in ops if "/y_lvl" in o[1] or o[1].startswith("y_lvl")]
    head_us = sum(o[2] for o in heads)
    del model, plan
    return dict(nlabels=nlabels, step_ms=round(step_ms, 3), stamped_span_us=round(span, 1), operator_time_us=round(total, 1),
                head_operators=len(heads), head_time_us=round(head_us, 1), head_share_of_operator_time=round(head_us / total, 4),
                head_share_of_span=round(head_us / span, 4))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    print(json.dumps(dict(part="residual_ce", shape=[B, H, W], shifts=list(SHIFTS), rows=residual_ce_rows(a.calls, a.rounds))), flush=True)
    if not a.skip_step:
        print(json.dumps(dict(part="train_step", rows=[step_row(2, a.steps), step_row(19, a.steps)])), flush=True)
