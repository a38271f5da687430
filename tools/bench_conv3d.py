"""Benchmark (GPU box) of the 3-D convolution kernels (csrc/conv3d.hip), a measurement and no gate.
    python tools/bench_conv3d.py [--batch 2] [--size 64] [--channels 32] [--iters 10] [--rounds 3]
3x3x3, stride 1: forward, data gradient and filter gradient of a `channels` -> `channels` layer on a size^3 volume, bf16 and fp32
storage, on the vector path and -- forced by a channel count of channels + 1 -- on the scalar fallback.  All variants run in ONE
process, alternating (`rounds` passes over the whole list, device events around `iters` back-to-back calls each, every shape warmed
first).  One JSON line per (storage type, path, kernel): us per call of every round, GFLOP/s of the best round over the algorithmic
2 * voxels * 27 * Cin * Cout operations (border taps included, so a little above what the kernels execute), and its share of the fp32
vector peak (157.3 TFLOP/s, the bound of an fp32-accumulating FMA kernel off the matrix cores; every case here is compute-bound by a
wide margin: 0.2 GB of tensors against 29 GFLOP at the default sizes)."""
import argparse
import json
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_VECTOR = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    from phiseg_code_amd import runtime as rt
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv3d: no GPU visible (times are taken on the device only)")
    L = rt.lib()
    S = torch.cuda.current_stream().cuda_stream
    B, D = args.batch, args.size
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    variants = []
    for dt, tdt in ((rt.BF16, torch.bfloat16), (rt.F32, torch.float32)):
        for path, C in (("vector", args.channels), ("scalar", args.channels + 1)):
            geo = (B, D, D, D, C, C, 3, 3, 3, 1, 1, 1)
            x = torch.randn(B, D, D, D, C, device="cuda").to(tdt)
            dy = torch.randn(B, D, D, D, C, device="cuda").to(tdt)
            w = torch.randn(3, 3, 3, C, C, device="cuda") / (27 * C) ** 0.5
            y, dx, dw = torch.empty_like(x), torch.empty_like(x), torch.zeros_like(w)
            calls = dict(fwd=lambda x=x, w=w, y=y, dt=dt, geo=geo: L.gconv3d_fwd(x.data_ptr(), dt, w.data_ptr(), None, y.data_ptr(), dt, *geo, 1, S),
                         dgrad=lambda dy=dy, w=w, dx=dx, dt=dt, geo=geo: L.gconv3d_dgrad(dy.data_ptr(), dt, w.data_ptr(), dx.data_ptr(), dt, *geo, S),
                         wgrad=lambda x=x, dy=dy, dw=dw, dt=dt, geo=geo: L.gconv3d_wgrad(x.data_ptr(), dt, dy.data_ptr(), dt, dw.data_ptr(), *geo, S))
            for k, call in calls.items():
                variants.append(dict(dtype="bf16" if dt == rt.BF16 else "f32", path=path if k != "wgrad" else "block-reduction", kernel=k,
                                     channels=C, flop=2.0 * B * D ** 3 * 27 * C * C, call=call, keep=(x, dy, w, y, dx, dw), us=[]))
    for v in variants:                       # warm every shape
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
    for v in variants:
        best = min(v["us"])
        print(json.dumps(dict(dtype=v["dtype"], kernel=v["kernel"], path=v["path"], channels=v["channels"], volume=[B, D, D, D],
                              us=[round(t, 1) for t in v["us"]], gflops=round(v["flop"] / best * 1e-3, 1),
                              share_of_f32_vector_peak=round(v["flop"] / (best * 1e-6) / PEAK_F32_VECTOR, 4))), flush=True)


if __name__ == "__main__":
    main()
