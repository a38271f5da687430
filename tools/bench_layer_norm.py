"""Benchmark (GPU box) of layer normalisation (csrc/layer_norm.hip).
    python tools/bench_layer_norm.py [--batch 64] [--steps 100] [--warmup 20] [--rounds 3]
        the full training step of phiseg_7_5 (128 x 128, bf16) with batch_norm, group_norm2D and layer_norm in ONE process, alternating;
        host clock around replays that end in a device synchronise.  One JSON line: ms per step, images/s, launch calls, routes.
    python tools/bench_layer_norm.py --kernels [--batch 64] [--iters 40]
        the kernels alone through the test build of the library (libphx_dbg.so: phx_debug_layer_norm_policy sets the one-launch
        maximum and the chunk length): for N = H W C of the network's levels, bf16, the one-launch form and the split form at several
        chunk lengths, forward and backward, device events around `iters` calls that rotate over enough buffer sets to exceed the
        256 MiB last-level cache.  One JSON line per (N, form); GB/s counts the algorithmic bytes (forward y + a, backward dA + y + dy)
        for both forms.  The last line times phx_norm_apply_fused (group norm, 128 x 128 x 32) on the same bytes as N = 524 288."""
import argparse
import collections
import importlib
import json
import os
import sys
import time
import types

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NS = (768, 3072, 12288, 24576, 32768, 49152, 65536, 98304, 131072, 262144, 524288, 1179648)
CHUNKS = (2048, 4096, 8192, 16384, 32768, 65536)
ONE_LAUNCH_UP_TO = 262144            # a block per sample beyond this is far off: not timed


def build(norm, batch, dtype):
    import torch  # noqa: F401
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    from phiseg_code_amd.tfwrapper import normalisation as tfnorm
    base = importlib.import_module("phiseg_code_amd.phiseg.experiments.phiseg_7_5")
    cfg = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if not k.startswith("_")})
    cfg.batch_size, cfg.compute_dtype, cfg.image_size = batch, dtype, (128, 128, 1)
    cfg.layer_norm = getattr(tfnorm, norm)
    model = phiseg_model.phiseg(cfg)
    plan = model.sess.plan_for([model.loss_tot], True, batch, True)
    x, s = synthetic.philox_batch(batch, 128, cfg.nlabels, seed=1234)
    plan.set_input("x_input", x)
    plan.set_input("s_input", s)
    model.sess.store.set_lr(1e-3)
    return model, plan


def timed(plan, steps):
    import torch
    plan.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.run()
    plan.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def routes(plan):
    c = collections.Counter()
    for sv in plan.saved.values():
        if getattr(sv, "norm", None) is not None and getattr(sv, "route", None) is not None:
            c[sv.route.name] += 1
    return dict(sorted(c.items()))


def step_benchmark(args):
    norms = ("batch_norm", "group_norm2D", "layer_norm")
    plans = {}
    for norm in norms:
        model, plan = build(norm, args.batch, args.dtype)
        for _ in range(args.warmup):
            plan.run()
        plan.sync()
        plans[norm] = (model, plan)
    ms = {n: [] for n in norms}
    order = list(norms) * args.rounds + [norms[0]]
    for norm in order:
        ms[norm].append(1e3 * timed(plans[norm][1], args.steps))
    out = {"workload": "phiseg_7_5 128x128 %s batch %d, full training step" % (args.dtype, args.batch), "steps": args.steps, "order": order}
    for norm, (model, plan) in plans.items():
        out[norm] = {"ms_per_step": [round(v, 4) for v in ms[norm]], "images_per_s": [round(args.batch / v * 1e3, 1) for v in ms[norm]],
                     "abi_launch_calls_per_step": plan.kernel_launch_count(), "forward_routes": routes(plan),
                     "barrier_timeouts": plan.barrier_timeouts()}
    print(json.dumps(out), flush=True)


def kernel_benchmark(args):
    import torch
    from phiseg_code_amd import runtime as rt
    L = rt.debug_lib()
    B, BF16 = args.batch, rt.BF16
    S = torch.cuda.current_stream().cuda_stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def time_calls(call, nsets):
        for k in range(min(nsets, 3)):
            call(k)
        torch.cuda.synchronize()
        ev0.record()
        for i in range(args.iters):
            call(i % nsets)
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) * 1e3 / args.iters          # us

    for N in NS:
        nsets = max(2, min(64, -(-(768 << 20) // (3 * B * N * 2))))
        rnd = lambda: [torch.randn(B * N, device="cuda").to(torch.bfloat16) for _ in range(nsets)]
        y, dA = rnd(), rnd()
        a = [torch.empty(B * N, dtype=torch.bfloat16, device="cuda") for _ in range(nsets)]
        mean, rstd = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        forms = ([("one_launch", 1 << 30, 8192)] if N <= ONE_LAUNCH_UP_TO else []) + [("split", 0, c) for c in CHUNKS if c < N]
        for form, one_max, chunk in forms:
            L.debug_layer_norm_policy(one_max, chunk)
            nws = int(L.layer_norm_ws_floats(B, N))
            ws = torch.empty(max(nws, 1), device="cuda")
            wsp = ws.data_ptr() if nws else None
            fwd = lambda k: L.layer_norm_fwd(y[k].data_ptr(), BF16, 1e-3, a[k].data_ptr(), BF16, mean.data_ptr(), rstd.data_ptr(), wsp, B, N, 1, 0, S)
            bwd = lambda k: L.layer_norm_bwd(dA[k].data_ptr(), BF16, y[k].data_ptr(), BF16, mean.data_ptr(), rstd.data_ptr(), a[k].data_ptr(), BF16,
                                             wsp, B, N, 1, 0, S)
            tf, tb = time_calls(fwd, nsets), time_calls(bwd, nsets)
            print(json.dumps({"N": N, "B": B, "form": form, "chunk": chunk if form == "split" else None, "fwd_us": round(tf, 2),
                              "bwd_us": round(tb, 2), "fwd_GBps": round(2 * B * N * 2 / tf * 1e-3, 1), "bwd_GBps": round(3 * B * N * 2 / tb * 1e-3, 1),
                              "buffer_sets": nsets}), flush=True)
        del y, dA, a
    # the per-channel apply pass on the bytes of N = 524 288: group norm of a 128 x 128 x 32 layer
    P, C, G = 128 * 128, 32, 2
    nsets = 4
    x = [torch.randn(B * P * C, device="cuda").to(torch.bfloat16) for _ in range(nsets)]
    o = [torch.empty(B * P * C, dtype=torch.bfloat16, device="cuda") for _ in range(nsets)]
    sums, pivot = torch.zeros(B * C * 2, device="cuda"), torch.zeros(B * C, device="cuda")
    sums.view(B * C, 2)[:, 1] = float(P)
    gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    v = [torch.empty(B * C, device="cuda") for _ in range(4)]
    ref = lambda k: L.norm_apply_fused(x[k].data_ptr(), BF16, sums.data_ptr(), pivot.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, o[k].data_ptr(),
                                       BF16, v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), v[3].data_ptr(), None, None, 0.0, B, P, C, G, 1, S)
    t = time_calls(ref, nsets)
    print(json.dumps({"reference": "phx_norm_apply_fused group norm B %d 128x128x32 bf16" % B, "us": round(t, 2),
                      "GBps": round(2 * B * P * C * 2 / t * 1e-3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    args = ap.parse_args()
    (kernel_benchmark if args.kernels else step_benchmark)(args)


if __name__ == "__main__":
    main()
