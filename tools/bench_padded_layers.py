"""Benchmark (GPU box) of the explicit-geometry 2-D convolution kernels (csrc/conv2d_pad.hip), a measurement and no gate.
    python tools/bench_padded_layers.py [--batch 8] [--size 128] [--channels 32] [--iters 10] [--rounds 5]
3x3, `channels` -> `channels`, size x size, bf16 and fp32 storage.  Arms, all in ONE process and alternating (`rounds` passes over the
whole list, device events around `iters` back-to-back calls each, every arm warmed first):
  pad   forward, data gradient and filter gradient of phx_conv2d_pad_* at VALID padding -- the new kernels
  gconv the same three of phx_gconv2d_* at SAME padding on the same input: the only route such a layer had before, and the yardstick
        (its FLOPs are within 3 % of the VALID layer's at the default size)
  mfma  information only (bf16 forward): the stride-1 SAME MFMA convolution followed by a phx_spatial_window crop, which is
        arithmetically the VALID result; nothing is routed through it
One JSON line per (storage type, arm, kernel): us per call of every round (the range is the spread), the best round's GFLOP/s over the
algorithmic 2 * output pixels * 9 * Cin * Cout operations, and, on the `pad` lines, best(gconv) / best(pad)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    from phiseg_code_amd import runtime as rt
    if not torch.cuda.is_available():
        raise SystemExit("bench_padded_layers: no GPU visible (times are taken on the device only)")
    L = rt.lib()
    S = torch.cuda.current_stream().cuda_stream
    B, H, C = args.batch, args.size, args.channels
    Ho = H - 2
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    variants = []

    def add(dtype, arm, kernel, flop, call, keep):
        variants.append(dict(dtype=dtype, arm=arm, kernel=kernel, flop=flop, call=call, keep=keep, us=[]))
    for dt, tdt in ((rt.BF16, torch.bfloat16), (rt.F32, torch.float32)):
        name = "bf16" if dt == rt.BF16 else "f32"
        x = torch.randn(B, H, H, C, device="cuda").to(tdt)
        w = torch.randn(3, 3, C, C, device="cuda") / (9 * C) ** 0.5
        dw = torch.zeros_like(w)
        dx = torch.empty_like(x)
        # the new kernels, VALID
        yv = torch.empty(B, Ho, Ho, C, device="cuda", dtype=tdt)
        dyv = torch.randn(B, Ho, Ho, C, device="cuda").to(tdt)
        geo = (B, H, H, C, C, 3, 3, 1, 1, 1, 1, Ho, Ho, 0, 0)
        n = int(L.conv2d_pad_wgrad_ws_floats(B, Ho, Ho, C, C, 3, 3))
        ws = torch.empty(max(n, 1), device="cuda")
        flop_v = 2.0 * B * Ho * Ho * 9 * C * C
        keep = (x, w, dw, dx, yv, dyv, ws)
        add(name, "pad", "fwd", flop_v, lambda x=x, w=w, y=yv, dt=dt, geo=geo:
            L.conv2d_pad_fwd(x.data_ptr(), dt, w.data_ptr(), None, y.data_ptr(), dt, *geo, 1, S), keep)
        add(name, "pad", "dgrad", flop_v, lambda dy=dyv, w=w, dx=dx, dt=dt, geo=geo:
            L.conv2d_pad_dgrad(dy.data_ptr(), dt, w.data_ptr(), dx.data_ptr(), dt, *geo, S), keep)
        add(name, "pad", "wgrad", flop_v, lambda x=x, dy=dyv, dw=dw, ws=ws, dt=dt, geo=geo, n=n:
            L.conv2d_pad_wgrad(x.data_ptr(), dt, dy.data_ptr(), dt, dw.data_ptr(), ws.data_ptr() if n else None, *geo, S), keep)
        # the general kernels, SAME, on the same input
        ys = torch.empty_like(x)
        dys = torch.randn(B, H, H, C, device="cuda").to(tdt)
        old = (B, H, H, C, C, 3, 3, 1, 1, 1, 1)
        flop_s = 2.0 * B * H * H * 9 * C * C
        keep = (x, w, dw, dx, ys, dys)
        add(name, "gconv", "fwd", flop_s, lambda x=x, w=w, y=ys, dt=dt, old=old:
            L.gconv2d_fwd(x.data_ptr(), dt, w.data_ptr(), None, y.data_ptr(), dt, *old, 1, S), keep)
        add(name, "gconv", "dgrad", flop_s, lambda dy=dys, w=w, dx=dx, dt=dt, old=old:
            L.gconv2d_dgrad(dy.data_ptr(), dt, w.data_ptr(), dx.data_ptr(), dt, *old, S), keep)
        add(name, "gconv", "wgrad", flop_s, lambda x=x, dy=dys, dw=dw, dt=dt, old=old:
            L.gconv2d_wgrad(x.data_ptr(), dt, dy.data_ptr(), dt, dw.data_ptr(), *old, S), keep)
        if dt == rt.BF16 and C % 32 == 0:
            # information only: the MFMA SAME convolution + a crop of one pixel per side
            wf, wg = (torch.empty(9 * C * C, dtype=torch.bfloat16, device="cuda") for _ in range(2))
            desc = np.zeros(1, dtype=[("w", "<u8"), ("wf", "<u8"), ("wd", "<u8"), ("cin", "<i4"), ("cpad", "<i4"), ("cout", "<i4"), ("k1", "<i4")])
            desc[0] = (w.data_ptr(), wf.data_ptr(), wg.data_ptr(), C, C, C, 0)
            dd = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
            L.pack_conv3x3_bf16_multi(dd.data_ptr(), 1, S)

            def mfma_crop(x=x, wf=wf, ys=ys, yv=yv):
                L.conv3x3_mfma_bf16(x.data_ptr(), wf.data_ptr(), ys.data_ptr(), None, 0, None, B, H, H, C, C, S)
                L.spatial_window(ys.data_ptr(), yv.data_ptr(), rt.BF16, B, H, H, Ho, Ho, C, 1, 1, S)
            add(name, "mfma", "fwd+crop", flop_s, mfma_crop, (x, w, wf, wg, dd, ys, yv))
    for v in variants:                       # warm every arm
        v["call"]()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for v in variants:
            ev0.record()
            for _ in range(args.iters):
                v["call"]()
            ev1.record()
            torch.cuda.synchronize()
            v["us"].append(ev0.elapsed_time(ev1) * 1e3 / args.iters)
    best = {(v["dtype"], v["arm"], v["kernel"]): min(v["us"]) for v in variants}
    for v in variants:
        row = dict(dtype=v["dtype"], arm=v["arm"], kernel=v["kernel"], shape=[B, H, H, C], us=[round(t, 1) for t in v["us"]],
                   gflops=round(v["flop"] / min(v["us"]) * 1e-3, 1))
        if v["arm"] == "pad":
            row["gconv_over_pad"] = round(best[(v["dtype"], "gconv", v["kernel"])] / min(v["us"]), 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
