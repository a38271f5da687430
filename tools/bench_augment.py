#!/usr/bin/env python3
"""Launch time of the device mini-batch producer on one MI355X (LABBOOK.md): batch 64, 4 annotators, the decisions of the shipped
LIDC experiment (rotation + crop-scale on every second sample), synthetic data set of 256 images.

    python tools/bench_augment.py [--windows 30] [--launches 50] [--baseline-lib OTHER/libphx.so]

Arms, alternated window by window (a window = `launches` back-to-back launches between two HIP events, so that a window is
milliseconds of device work, not one launch's enqueue):

    augment_batch              phx_augment_batch                                   (the path without do_elasticaug)
    elastic_unflagged          phx_augment_batch_elastic, no record carries bit 16 (must cost what augment_batch costs)
    elastic_flagged            phx_augment_batch_elastic, every record carries it  (third pass on all 64 samples)

    augment_batch_baseline     phx_augment_batch of another build of the library    (--baseline-lib: e.g. the parent commit's)

at 128 x 128 (intermediates in LDS) and at 192 x 192 (second image and label map in the global workspace).  One JSON line per
size: per-launch median / p10 / p90 in microseconds per arm, the ratios, and whether the unflagged arm's output (and the baseline
build's) is bit-identical to phx_augment_batch's."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHIPPED = {'do_flip_lr': True, 'do_flip_ud': True, 'do_rotations': True, 'do_scaleaug': True, 'nlabels': 2}


def _stats(us):
    a = np.asarray(us)
    return dict(median_us=float(np.median(a)), p10_us=float(np.percentile(a, 10)), p90_us=float(np.percentile(a, 90)), n=int(a.size))


def bench(X, B, A, windows, launches, baseline=None, warm=3):
    import torch
    from phiseg_code_amd import runtime as rt
    from phiseg_code_amd.data import augment as pa
    L = rt.lib()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    n = 256
    g = torch.Generator(device=dev).manual_seed(X)
    img = torch.rand(n, X, X, device=dev, generator=g) - 0.5
    lab = (torch.rand(n, X, X, A, device=dev, generator=g) > 0.7).to(torch.uint8)
    rng = np.random.default_rng(X)
    dec = [pa.draw_decisions(1234, 0, j, X, X, SHIPPED, A) for j in range(B)]
    src = np.sort(rng.choice(n, B, replace=False))
    annots = [d["annot"] for d in dec]
    rec_plain = pa.pack_params(dec, src, annots, X, X)
    ctrl = pa.ELASTIC_SIGMA * rng.standard_normal((B, 2, 3, 3))
    rec_flag = rec_plain.copy()
    rec_flag["flags"] |= pa.ELASTIC

    def up(rec):
        return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    par_plain, par_flag, ctrl_d = up(rec_plain), up(rec_flag), torch.from_numpy(ctrl).to(dev)
    nb = int(L.augment_batch_elastic_ws_bytes(B, X, X))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    outs = {k: (torch.empty(B, X, X, device=dev), torch.empty(B, X, X, dtype=torch.uint8, device=dev))
            for k in ("augment_batch", "elastic_unflagged", "elastic_flagged", "augment_batch_baseline")}

    def plain():
        xo, so = outs["augment_batch"]
        L.augment_batch(img.data_ptr(), lab.data_ptr(), par_plain.data_ptr(), xo.data_ptr(), so.data_ptr(), B, X, X, A, 2, st)

    def elastic(name, par):
        xo, so = outs[name]
        L.augment_batch_elastic(img.data_ptr(), lab.data_ptr(), par.data_ptr(), ctrl_d.data_ptr(), xo.data_ptr(), so.data_ptr(),
                                ws.data_ptr() if nb else None, nb, B, X, X, A, 2, st)
    arms = [("augment_batch", plain), ("elastic_unflagged", lambda: elastic("elastic_unflagged", par_plain)),
            ("elastic_flagged", lambda: elastic("elastic_flagged", par_flag))]
    if baseline is not None:
        def base():
            xo, so = outs["augment_batch_baseline"]
            rc = baseline(img.data_ptr(), lab.data_ptr(), par_plain.data_ptr(), xo.data_ptr(), so.data_ptr(), B, X, X, A, 2, st)
            assert rc == 0, rc
        arms.append(("augment_batch_baseline", base))
    t = {name: [] for name, _ in arms}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(warm + windows):
        for name, fn in arms:
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            if k >= warm:
                t[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    same = all(bool(torch.equal(a, b)) for a, b in zip(outs["augment_batch"], outs["elastic_unflagged"]))
    if baseline is not None:
        same = same and all(bool(torch.equal(a, b)) for a, b in zip(outs["augment_batch"], outs["augment_batch_baseline"]))
    changed = float((outs["elastic_flagged"][0] != outs["augment_batch"][0]).float().mean())
    med = {name: float(np.median(v)) for name, v in t.items()}
    print(json.dumps(dict(bench="augment", shape=dict(B=B, X=X, Y=X, A=A), workspace_bytes=nb, launches_per_window=launches,
                          **{name: _stats(v) for name, v in t.items()},
                          ratio_unflagged_over_augment_batch=med["elastic_unflagged"] / med["augment_batch"],
                          ratio_flagged_over_unflagged=med["elastic_flagged"] / med["elastic_unflagged"],
                          images_per_s_flagged=B / (med["elastic_flagged"] * 1e-6),
                          outputs_bit_identical_to_augment_batch=same, flagged_pixels_changed=changed)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--baseline-lib", default=None)
    a = ap.parse_args()
    baseline = None
    if a.baseline_lib:
        baseline = ctypes.CDLL(os.path.abspath(a.baseline_lib)).phx_augment_batch
        baseline.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        baseline.restype = ctypes.c_int
    for X in (128, 192):
        bench(X, a.batch, 4, a.windows, a.launches, baseline)
