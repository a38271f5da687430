#!/usr/bin/env python3
"""Multi-channel images on one MI355X (LABBOOK.md, "Multi-channel images"): one process, arms alternated window by window.

    python tools/bench_multichannel.py [--windows 20] [--launches 30] [--steps 30]

1. Producer launch, Cx = 3, 128 x 128, batch 64, 4 annotators, rotation + crop-scale on every second sample, plain and elastic:
   phx_augment_batch_mc against THREE launches of the single-channel entry on the same records (what the planes would cost).
2. Training step, phiseg_7_5 bf16 128 x 128 batch 64 at Cx = 1 and Cx = 3 (captured plan, replayed), with launch counts.
One JSON line per measurement: per-launch / per-step median, p10, p90."""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPTS = {'do_rotations': True, 'do_scaleaug': True, 'nlabels': 2}


def _stats(v):
    a = np.asarray(v)
    return dict(median=float(np.median(a)), p10=float(np.percentile(a, 10)), p90=float(np.percentile(a, 90)), n=int(a.size))


def _windows(arms, windows, per_window, warm=3):
    import torch
    t = {name: [] for name, _ in arms}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(warm + windows):
        for name, fn in arms:
            e0.record()
            for _ in range(per_window):
                fn()
            e1.record()
            e1.synchronize()
            if k >= warm:
                t[name].append(e0.elapsed_time(e1) * 1e3 / per_window)
    return t


def producer(elastic, windows, launches, B=64, X=128, A=4, Cx=3, n=256):
    import torch
    from phiseg_code_amd import runtime as rt
    from phiseg_code_amd.data import augment as pa
    L = rt.lib()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(X)
    img = torch.rand(n, X, X, Cx, device=dev, generator=g) - 0.5
    planes = [img[..., c].contiguous() for c in range(Cx)]
    lab = (torch.rand(n, X, X, A, device=dev, generator=g) > 0.7).to(torch.uint8)
    rng = np.random.default_rng(X)
    dec = [pa.draw_decisions(1234, 0, j, X, X, dict(OPTS, do_elasticaug=elastic), A) for j in range(B)]
    ctrl = np.zeros((B, 2, 3, 3)) if elastic else None
    rec = pa.pack_params(dec, np.sort(rng.choice(n, B, replace=False)), [d["annot"] for d in dec], X, X, ctrl)
    par = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    cd = torch.from_numpy(ctrl).to(dev) if elastic else None
    xo, so = torch.empty(B, X, X, Cx, device=dev), torch.empty(B, X, X, dtype=torch.uint8, device=dev)
    xs, ss = torch.empty(Cx, B, X, X, device=dev), torch.empty(Cx, B, X, X, dtype=torch.uint8, device=dev)
    assert L.augment_batch_mc_ws_bytes(B, X, X, Cx, 2, 1) == 0 and L.augment_batch_elastic_ws_bytes(B, X, X) == 0

    def mc():
        L.augment_batch_mc(img.data_ptr(), lab.data_ptr(), par.data_ptr(), cd.data_ptr() if elastic else None, xo.data_ptr(), so.data_ptr(),
                           None, 0, B, X, X, A, Cx, 2, st)

    def three():
        for c in range(Cx):
            if elastic:
                L.augment_batch_elastic(planes[c].data_ptr(), lab.data_ptr(), par.data_ptr(), cd.data_ptr(), xs[c].data_ptr(), ss[c].data_ptr(),
                                        None, 0, B, X, X, A, 2, st)
            else:
                L.augment_batch(planes[c].data_ptr(), lab.data_ptr(), par.data_ptr(), xs[c].data_ptr(), ss[c].data_ptr(), B, X, X, A, 2, st)
    t = _windows([("augment_batch_mc", mc), ("three_single_channel_launches", three)], windows, launches)
    same = all(bool(torch.equal(xo[..., c], xs[c])) and bool(torch.equal(so, ss[c])) for c in range(Cx))
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps(dict(bench="multichannel_producer", elastic=elastic, shape=dict(B=B, X=X, Y=X, A=A, Cx=Cx), unit="us per batch",
                          **{k: _stats(v) for k, v in t.items()}, ratio_mc_over_three=med["augment_batch_mc"] / med["three_single_channel_launches"],
                          outputs_bit_identical=same)), flush=True)


def training_step(windows, steps, B=64):
    import torch
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    base = importlib.import_module("phiseg_code_amd.phiseg.experiments.phiseg_7_5")
    arms, info = [], {}
    for Cx in (1, 3):
        cfg = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if not k.startswith("_")})
        cfg.compute_dtype, cfg.batch_size, cfg.image_size = "bf16", B, (128, 128, Cx)
        model = phiseg_model.phiseg(cfg)
        x, s = synthetic.philox_batch(B, 128, cfg.nlabels, channels=Cx)
        fd = {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: 1e-4}
        for _ in range(3):
            model.sess.run([model.train_step, model.loss_tot], fd)
        plan = model.sess.plan_for([model.loss_tot], True, B, True)
        info[Cx] = dict(launches=len(plan.launches), opt_launches=len(plan.opt_launches))

        arms.append(("Cx=%d" % Cx, plan))
    import time
    t = {name: [] for name, _ in arms}
    for k in range(2 + windows):                  # the plan runs on its own stream: wall clock around `steps` replays and one sync
        for name, plan in arms:
            plan.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                plan.run()
            plan.sync()
            if k >= 2:
                t[name].append((time.perf_counter() - t0) * 1e6 / steps)
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps(dict(bench="multichannel_training_step", model="phiseg_7_5 bf16 128x128", batch=B, unit="us per step",
                          **{k: dict(_stats(v), images_per_s=B / (float(np.median(v)) * 1e-6), **info[int(k[3:])]) for k, v in t.items()},
                          ratio_cx3_over_cx1=med["Cx=3"] / med["Cx=1"])), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip-training", action="store_true")
    a = ap.parse_args()
    producer(False, a.windows, a.launches)
    producer(True, a.windows, a.launches)
    if not a.skip_training:
        training_step(max(a.windows // 2, 5), a.steps)
