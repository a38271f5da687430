"""Micro-benchmark (GPU box): phx_leaky_relu_fwd / _bwd alone at n = 64 * 128 * 128 * 32 (one 32-channel activation tensor of the
128 x 128 level at batch 64), bf16 and fp32, as achieved bytes/s beside the 6.3 TB/s streaming ceiling and beside a plain device copy
of the same tensor.
    python tools/bench_leaky_relu.py [--rounds 7] [--calls 200] [--sets 6]
A call's tensors (134 MB forward in bf16) would sit in the 256 MiB last-level cache if the same buffers were used over and over: the
calls rotate over `sets` buffer sets, so every call streams from and to HBM.  Per case: `rounds` timed windows of `calls` calls
between two device events after a warm-up window; the range over the windows is printed, and one JSON line at the end."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from phiseg_code_amd import runtime as rt  # noqa: E402

CEILING = 6.3e12
N = 64 * 128 * 128 * 32


def windows(fns, rounds, calls):
    """-> seconds per call of each timed window; fns: one callable per buffer set, taken round-robin"""
    k = len(fns)
    for i in range(max(calls // 4, 2 * k)):
        fns[i % k]()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fns[i % k]()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sets", type=int, default=6)
    a = ap.parse_args()
    L = rt.lib()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for name, dt, tdt, es in (("bf16", rt.BF16, torch.bfloat16, 2), ("fp32", rt.F32, torch.float32, 4)):
        bufs = [[torch.randn(N, device="cuda").to(tdt) for _ in range(3)] for _ in range(a.sets)]
        cases = {
            "fwd": (2, [lambda b=b: L.leaky_relu_fwd(b[0].data_ptr(), dt, b[1].data_ptr(), dt, N, 0.01, st) for b in bufs]),
            "bwd": (3, [lambda b=b: L.leaky_relu_bwd(b[0].data_ptr(), dt, b[1].data_ptr(), dt, b[2].data_ptr(), dt, N, 0.01, st) for b in bufs]),
            "copy": (2, [lambda b=b: b[1].copy_(b[0]) for b in bufs]),
        }
        for what, (streams, fns) in cases.items():
            t = sorted(windows(fns, a.rounds, a.calls))
            nbytes = streams * N * es
            lo, med, hi = (nbytes / t[-1], nbytes / t[len(t) // 2], nbytes / t[0])
            rows.append(dict(case="%s %s" % (name, what), bytes=nbytes, us_min=t[0] * 1e6, us_median=t[len(t) // 2] * 1e6, us_max=t[-1] * 1e6,
                             tbps_min=lo / 1e12, tbps_median=med / 1e12, tbps_max=hi / 1e12, of_ceiling=med / CEILING))
            print("%-9s %6.1f MB  %7.1f .. %7.1f us (median %7.1f)  %.2f .. %.2f TB/s (median %.2f = %.0f %% of %.1f TB/s)"
                  % (rows[-1]["case"], nbytes / 1e6, t[0] * 1e6, t[-1] * 1e6, t[len(t) // 2] * 1e6, lo / 1e12, hi / 1e12, med / 1e12,
                     100 * med / CEILING, CEILING / 1e12), flush=True)
        del bufs
        torch.cuda.empty_cache()
    print(json.dumps(dict(n=N, rounds=a.rounds, calls=a.calls, sets=a.sets, rows=rows)))


if __name__ == "__main__":
    main()
