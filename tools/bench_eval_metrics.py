#!/usr/bin/env python3
"""Measurements of the test-set evaluation on one MI355X (LABBOOK.md):

    python tools/bench_eval_metrics.py kernel [--calls 20]   phx_eval_metrics against the unchanged phx_validation_metrics on the same
                                                             inputs, alternated call by call, HIP-event time per call (all launches of
                                                             a call), at (I, N, M, P, C) = (1, 100, 4, 16384, 2), (4, 100, 4, 16384, 2),
                                                             (1, 50, 4, 36864, 4)
    python tools/bench_eval_metrics.py e2e [--rounds 3]      images/s of evaluate_split (images_per_pass 1, 2, 4) against the per-image loop
                                                             of _do_validation (sess.run of the soft-max, utils.validation_metrics):
                                                             phiseg_7_5 bf16, 100 samples, 32 synthetic images, sweeps alternated

One JSON line per measurement."""
import argparse
import importlib
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNEL_SHAPES = [(1, 100, 4, 16384, 2), (4, 100, 4, 16384, 2), (1, 50, 4, 36864, 4)]


def _stats(ms):
    a = np.asarray(ms)
    return dict(median_ms=float(np.median(a)), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)), n=int(a.size))


def bench_kernel(calls, warm=3):
    import torch
    from phiseg_code_amd import runtime as rt
    L = rt.lib()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    for I, N, M, P, C in KERNEL_SHAPES:
        g = torch.Generator(device=dev).manual_seed(1000 * I + N)
        # smooth-ish random samples: per-image base logits + per-sample noise, so that masks overlap as segmentations do
        base = torch.randn(I, 1, P, C, device=dev, generator=g) * 2.0
        sm = torch.softmax(base + torch.randn(I, N, P, C, device=dev, generator=g), dim=-1).reshape(I * N, P, C).contiguous()
        labels = torch.softmax(base + torch.randn(I, M, P, C, device=dev, generator=g), dim=-1).argmax(dim=-1).to(torch.uint8)   # [I, M, P]
        gt = labels.contiguous()                                    # phx_validation_metrics: [I, M, P] and the reference map itself
        sref_map = gt[:, 0].contiguous()
        lab_pm = labels.permute(0, 2, 1).contiguous()               # phx_eval_metrics: [I, P, M] and the annotator's index
        sref_annot = torch.zeros(I, dtype=torch.uint8, device=dev)
        wsb_new, wsb_old = int(L.eval_metrics_ws_bytes(I, N, M, P, C)), int(L.validation_metrics_ws_bytes(I, N, M, P, C))
        ws_new, ws_old = (torch.empty(b, dtype=torch.uint8, device=dev) for b in (wsb_new, wsb_old))
        out_new, out_old = (torch.zeros(I, 10, dtype=torch.float32, device=dev) for _ in range(2))
        torch.cuda.synchronize()

        def new():
            L.eval_metrics(sm.data_ptr(), lab_pm.data_ptr(), sref_annot.data_ptr(), ws_new.data_ptr(), wsb_new, I, N, M, P, C, 1,
                           out_new.data_ptr(), st)

        def old():
            L.validation_metrics(sm.data_ptr(), gt.data_ptr(), sref_map.data_ptr(), ws_old.data_ptr(), wsb_old, I, N, M, P, C, 1,
                                 out_old.data_ptr(), st)
        t = {"new": [], "old": []}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for k in range(warm + calls):
            for name, fn in (("new", new), ("old", old)):
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if k >= warm:
                    t[name].append(e0.elapsed_time(e1))
        a, b = out_new.cpu().numpy(), out_old.cpu().numpy()
        print(json.dumps(dict(bench="kernel", shape=dict(I=I, N=N, M=M, P=P, C=C), eval_metrics=_stats(t["new"]),
                              validation_metrics=_stats(t["old"]),
                              ratio_old_over_new=float(np.median(t["old"]) / np.median(t["new"])),
                              max_abs_diff=dict(ged=float(np.abs(a[:, 0] - b[:, 0]).max()), ncc=float(np.abs(a[:, 1] - b[:, 1]).max()),
                                                dice=float(np.abs(a[:, 2:2 + C] - b[:, 2:2 + C]).max())),
                              ws_bytes=dict(eval_metrics=wsb_new, validation_metrics=wsb_old))), flush=True)


def _validation_loop(model, split, n, sref):
    """What _do_validation does per image for the three scores: the soft-max of n samples to the host, utils.validation_metrics."""
    from phiseg_code_amd import utils
    cfg = model.exp_config
    rows = []
    for ii in range(split.images.shape[0]):
        x_b = np.tile(split.images[ii][None], [n, 1, 1, 1])
        s_gt = split.labels[ii]
        sm = model.sess.run(model.s_out_eval_sm, feed_dict={model.training_pl: False, model.x_inp: x_b})
        model._advance_noise()
        gts = np.ascontiguousarray(s_gt.transpose((2, 0, 1)))
        rows.append(utils.validation_metrics(sm[None], gts[None], s_gt[None, :, :, sref[ii]], cfg.nlabels))
    return rows


def bench_e2e(rounds, n=100, n_images=32):
    import torch
    from phiseg_code_amd import evaluate
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    base = importlib.import_module("phiseg_code_amd.phiseg.experiments.phiseg_7_5")
    cfg = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if not k.startswith("_")})
    cfg.compute_dtype = "bf16"
    split = synthetic.SyntheticLIDC(cfg, seed=5, n_validation=n_images).validation
    model = phiseg_model.phiseg(cfg, rng_seed=3)
    sref = np.zeros(n_images, dtype=np.int64)
    routes = [("evaluate_split_ipp%d" % k, lambda k=k: evaluate.evaluate_split(model, split, n, images_per_pass=k)) for k in (1, 2, 4)]
    routes.append(("validation_loop", lambda: _validation_loop(model, split, n, sref)))
    times = {name: [] for name, _ in routes}
    for r in range(rounds + 1):                                # round 0 warms: plans compiled, eager run, graph capture
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r > 0:
                times[name].append(time.perf_counter() - t0)
    res = {name: dict(images_per_s=float(n_images / np.median(v)), median_s=float(np.median(v)), min_s=float(min(v)), max_s=float(max(v)))
           for name, v in times.items()}
    print(json.dumps(dict(bench="e2e", workload="phiseg_7_5 128x128 bf16, %d samples, %d images" % (n, n_images), rounds=rounds, **res)),
          flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("kernel", "e2e"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.what == "kernel":
        bench_kernel(max(a.calls, 20))
    else:
        bench_e2e(a.rounds)
