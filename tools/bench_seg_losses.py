#!/usr/bin/env python3
"""HIP-event time of every entry point of csrc/seg_losses.hip on one MI355X, next to phx_residual_ce (one level, loss + gradient) at
the same shape from the same run, for scale (LABBOOK.md):

    python tools/bench_seg_losses.py [--calls 200]

Shapes (B, H, W, C): 64 x 128 x 128 x 2 and 12 x 192 x 192 x 4.  Each figure is the time of `calls` back-to-back calls between two
events, divided by `calls` (after a warm-up of 20 calls), so launch gaps are part of it -- these calls are launch- and memory-bound.
GB/s is the ALGORITHMIC traffic over that time: B P (4 C + 1) bytes read by a pass over the pixels (logits + labels), plus 4 C B P
written by a pass that produces a gradient (8 C B P more where it is added to an existing one).  One JSON line per shape."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(64, 128, 128, 2), (12, 192, 192, 4)]


def main(calls, warm=20):
    import torch
    from phiseg_code_amd import runtime as rt
    L = rt.lib()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    for B, H, W, C in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B * 1000 + C)
        P = H * W
        logits = (torch.randn(B, H, W, C, device=dev, generator=g) * 3.0).contiguous()
        labels = torch.randint(0, C, (B, H, W), device=dev, generator=g, dtype=torch.uint8)
        dlog = torch.zeros_like(logits)
        cw = torch.linspace(0.5, 2.0, C, device=dev)
        wsb, xsb = int(L.dice_ws_bytes(B, H, W, C)), int(L.seg_xent_ws_bytes(B, H, W, C))
        ws, xws = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.empty(xsb, dtype=torch.uint8, device=dev)
        table, loss = torch.zeros(B * C, device=dev), torch.zeros(8 + 512, device=dev)
        coef = torch.zeros(B * C * 2, device=dev)
        lp, bp, dp = logits.data_ptr(), labels.data_ptr(), dlog.data_ptr()
        read, grad = B * P * (4 * C + 1), 4 * C * B * P
        from phiseg_code_amd.runtime import ptr_array, int_array
        sp, dsp, shp = ptr_array([lp]), ptr_array([dp]), int_array([0])
        rows = [
            ("dice_sums", read, lambda: L.dice_sums(lp, bp, ws.data_ptr(), wsb, B, H, W, C, st)),
            ("dice_finish", 0, lambda: L.dice_finish(ws.data_ptr(), wsb, B, H, W, C, 0, 0, 0, 0, 1e-10, 1.0 / B, table.data_ptr(),
                                                     loss.data_ptr(), coef.data_ptr(), st)),
            ("dice_grad", read + grad, lambda: L.dice_grad(lp, bp, coef.data_ptr(), 1.0, 0, dp, B, H, W, C, st)),
            ("dice_grad_add", read + 2 * grad, lambda: L.dice_grad(lp, bp, coef.data_ptr(), 1.0, 1, dp, B, H, W, C, st)),
            ("seg_xent_weighted_loss_and_grad", read + grad, lambda: L.seg_xent(lp, bp, cw.data_ptr(), 0, 1.0 / B, 1.0, 0, loss.data_ptr(), dp,
                                                                                 xws.data_ptr(), xsb, B, H, W, C, st)),
            ("seg_xent_sigmoid_loss_and_grad", read + grad, lambda: L.seg_xent(lp, bp, None, 1, 1.0 / B, 1.0, 0, loss.data_ptr(), dp,
                                                                                xws.data_ptr(), xsb, B, H, W, C, st)),
            ("seg_xent_loss_only", read, lambda: L.seg_xent(lp, bp, None, 0, 1.0 / B, 1.0, 0, loss.data_ptr(), None, xws.data_ptr(), xsb,
                                                            B, H, W, C, st)),
            ("nn_resize_adjoint_shift2_add", 4 * C * B * P + 3 * 4 * C * B * P // 16,
             lambda: L.nn_resize_adjoint(lp, dp, B, H // 4, W // 4, C, 2, 1, st)),
            ("residual_ce_one_level_loss_and_grad", read + grad, lambda: L.residual_ce(sp, dsp, shp, 1, bp, B, H, W, C, 1.0, 1.0 / B,
                                                                                       loss.data_ptr(), None, None, st)),
        ]
        out = {}
        for name, nbytes, fn in rows:
            ms = timed(fn)
            out[name] = dict(ms=round(ms, 5), GBps=round(nbytes / ms / 1e6, 1) if nbytes else None)
        print(json.dumps(dict(bench="seg_losses", shape=dict(B=B, H=H, W=W, C=C), calls=calls, algorithmic_read_MB=round(read / 1e6, 2), **out)),
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    main(max(ap.parse_args().calls, 200))
