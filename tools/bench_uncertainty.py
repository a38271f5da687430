#!/usr/bin/env python3
"""Measurements of the uncertainty-map feature on one MI355X (LABBOOK.md):

    python tools/bench_uncertainty.py e2e      [--calls 50]   predict_mean_variance_and_error_maps(s, x, 100), phiseg_7_5, 128 x 128, bf16,
                                                              against the host route of the parent commit (same sampling pass, Plan.fetch
                                                              of logits + soft-max, numpy restatement), alternated in one process
    python tools/bench_uncertainty.py kernel   [--images 1]   phx_mc_stats alone on random samples (run it under
                                                              `rocprofv3 --kernel-trace --stats -- python tools/bench_uncertainty.py kernel`)
    python tools/bench_uncertainty.py feed                    launches / time of the fully fed decode plan against the unfed inference plan, batch 16
"""
import argparse
import importlib
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _model(dtype="bf16"):
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    base = importlib.import_module("phiseg_code_amd.phiseg.experiments.phiseg_7_5")
    cfg = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if not k.startswith("_")})
    cfg.compute_dtype = dtype
    data = synthetic.SyntheticLIDC(cfg, seed=5, n_validation=2)
    return phiseg_model.phiseg(cfg, rng_seed=3), cfg, data


def _host_route(model, s, x, n):
    """What a user of the parent commit does: one sampling pass, both tensors to the host, the reference's numpy arithmetic."""
    lg_t, sm_t = model.sampling_graph(n)
    lg, sm = model.sess.run([lg_t, sm_t], {model.training_pl: False, model.x_inp: x})
    model._advance_noise()
    var = np.mean(np.std(sm, axis=0), axis=-1)
    means = np.argmax(np.mean(sm, 0), axis=-1)
    mx = lg.max(axis=-1, keepdims=True)
    xe = mx[..., 0] + np.log(np.exp(lg - mx).sum(axis=-1)) - np.take_along_axis(lg, np.broadcast_to(s.astype(np.int64)[..., None], lg.shape[:3] + (1,)), axis=-1)[..., 0]
    return means, var, np.mean(xe, axis=0)


def _stats(ms):
    a = np.asarray(ms)
    return dict(median_ms=float(np.median(a)), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)), n=int(a.size))


def bench_e2e(calls, n=100):
    import torch
    model, cfg, data = _model("bf16")
    x = data.validation.images[0].reshape((1,) + tuple(cfg.image_size)).astype(np.float32)
    s = data.validation.labels[0][:, :, 0][None].astype(np.uint8)
    for _ in range(5):                                     # warm: eager run, graph capture, replays
        model.predict_mean_variance_and_error_maps(s, x, n)
        _host_route(model, s, x, n)
    t_dev, t_host = [], []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.predict_mean_variance_and_error_maps(s, x, n)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        _host_route(model, s, x, n)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_dev.append((t1 - t0) * 1e3)
        t_host.append((t2 - t1) * 1e3)
    out = dict(bench="e2e", workload="predict_mean_variance_and_error_maps(s, x, %d) phiseg_7_5 128x128 bf16" % n, device_maps=_stats(t_dev),
               host_route=_stats(t_host), ratio_host_over_device=float(np.median(t_host) / np.median(t_dev)))
    print(json.dumps(out))


def bench_kernel(images, n=100, reps=20):
    import torch
    from phiseg_code_amd import uncertainty as unc
    P, C = 128 * 128, 2
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    lg = torch.randn(images * n, P, C, device=dev, generator=g)
    sm = torch.softmax(lg, dim=-1).contiguous()
    sref = torch.zeros(images, P, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    maps = ("std_mean", "xent_mean")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        unc.mc_stats_device(lg.data_ptr(), sm.data_ptr(), None, sref.data_ptr(), images, n, 0, P, C, maps, st, amax=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        ev0.record()
        unc.mc_stats_device(lg.data_ptr(), sm.data_ptr(), None, sref.data_ptr(), images, n, 0, P, C, maps, st, amax=True)
        ev1.record()
        torch.cuda.synchronize()
        ms.append(ev0.elapsed_time(ev1))
    nbytes = 2 * images * n * P * C * 4 + images * P * (2 * 4 + 1)
    out = dict(bench="kernel", I=images, N=n, P=P, C=C, bytes=nbytes, event_timed=_stats(ms),
               note="event time includes the output fill and the launch; take the kernel's own time from the rocprofv3 kernel trace")
    out["GBps_event_median"] = nbytes / (out["event_timed"]["median_ms"] * 1e-3) / 1e9
    print(json.dumps(out))


def bench_feed(batch=16, reps=30):
    import torch
    model, cfg, data = _model("bf16")
    x, s = data.train.next_batch(batch)
    fd = {model.x_inp: x, model.s_inp: s, model.training_pl: False}
    z = model.sess.run(model.z_list, fd)
    fed = dict(fd)
    fed.update({t: v for t, v in zip(model.z_list, z)})
    res = {}
    for name, feeds in (("unfed", fd), ("fully_fed", fed)):
        plan = model.sess._launch(list(model.s_out_list), feeds)
        for _ in range(3):
            plan.run(sync=True)
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plan.run(sync=True)
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = dict(launches=plan.kernel_launch_count(), **_stats(ms))
    print(json.dumps(dict(bench="feed", batch=batch, **res)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("e2e", "kernel", "feed"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--images", type=int, default=1)
    a = ap.parse_args()
    if a.what == "e2e":
        bench_e2e(a.calls)
    elif a.what == "kernel":
        bench_kernel(a.images)
    else:
        bench_feed()
