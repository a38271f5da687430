#!/usr/bin/env python3
"""Sampling throughput of the Probabilistic U-Net on one MI355X (LABBOOK.md): the `probunet` config, bf16, ONE 128 x 128 image,
n = 16 and n = 100 segmentation samples per call, three routes to the same [n, 128, 128, 2] soft-max:

    tiled     s_out_eval_sm on x tiled to batch n: U-Net and prior encoder n times (predict / the Monte-Carlo methods without
              exp_config.one_pass_sampling; the only route before sampling_graph served this prior)
    generic   sampling_graph(n) with PHX_RECOMB=0: U-Net and prior encoder once, the recombination layers unit by unit at batch n
    fused     sampling_graph(n): the recombination chain as one phx_recomb_samples launch

    python tools/bench_probunet_sampling.py [--rounds 15] [--replays 10]

The three plans live in one process and are timed in turn, round after round (A/B/C alternation: drift of the shared box hits all
arms alike); a timing is a host clock around `replays` hipGraph replays that end in a stream synchronise.  One JSON line."""
import argparse
import importlib
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _model():
    from phiseg_code_amd.phiseg import phiseg_model
    base = importlib.import_module("phiseg_code_amd.phiseg.experiments.probunet")
    cfg = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if not k.startswith("_")})
    cfg.compute_dtype = "bf16"
    return phiseg_model.phiseg(cfg, rng_seed=3), cfg


def _plan(model, route, n, x):
    """The compiled plan of one arm, input set.  PHX_RECOMB is read when a plan is built."""
    os.environ["PHX_RECOMB"] = "0" if route == "generic" else "1"
    if route == "tiled":
        plan = model.sess.plan_for([model.s_out_eval_sm], False, n, False)
        plan.set_input("x_input", np.repeat(x, n, axis=0))
    else:
        plan = model.sess.plan_for([model.sampling_graph(n)[1]], False, 1, False)
        plan.set_input("x_input", x)
    names = [getattr(fn, "__name__", "") for fn, _ in plan.launches]
    assert ("phx_recomb_samples" in names) == (route == "fused"), (route, "phx_recomb_samples" in names)
    return plan


def main(rounds, replays):
    from phiseg_code_amd.data import synthetic
    out = dict(bench="probunet_sampling", config="probunet bf16 B=1 128x128", rounds=rounds, replays=replays, results={})
    routes = ("tiled", "generic", "fused")
    for n in (16, 100):
        # one model per arm: a session caches its plans by (fetches, batch), and generic / fused share that key
        models = {r: _model() for r in routes}
        cfg = models["tiled"][1]
        data = synthetic.SyntheticLIDC(cfg, seed=5, n_validation=2)
        x = data.validation.images[0].reshape((1,) + tuple(cfg.image_size)).astype(np.float32)
        plans = {r: _plan(models[r][0], r, n, x) for r in routes}
        for p in plans.values():                              # warm: eager run, graph capture, replays
            for _ in range(4):
                p.run(sync=True)
        sm = {r: plans[r].fetch(plans[r].fetches[0]) for r in routes}
        ms = {r: [] for r in routes}
        for _ in range(rounds):
            for r in routes:
                p = plans[r]
                p.sync()
                t0 = time.perf_counter()
                for _ in range(replays):
                    p.run()
                p.sync()
                ms[r].append((time.perf_counter() - t0) * 1e3 / replays)
        res = {}
        for r in routes:
            a = np.asarray(ms[r])
            res[r] = dict(median_ms=float(np.median(a)), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)),
                          samples_per_s=float(n / (np.median(a) * 1e-3)), launches=plans[r].kernel_launch_count())
        # same noise step, same weights: the three routes draw the same samples (bf16 storage differs in where z is rounded)
        res["max_abs_softmax_diff_vs_tiled"] = {r: float(np.abs(sm[r] - sm["tiled"]).max()) for r in ("generic", "fused")}
        res["mean_abs_softmax_diff_vs_tiled"] = {r: float(np.abs(sm[r] - sm["tiled"]).mean()) for r in ("generic", "fused")}
        out["results"]["n=%d" % n] = res
        del plans, models
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--replays", type=int, default=10)
    a = ap.parse_args()
    main(a.rounds, a.replays)
