"""Time one TensorBoard summary write of train(summaries=True) at the benchmark shape (phiseg_7_5, 128 x 128, bf16, batch 64), and
the two phx_summary_histograms calls alone (activations + parameter arena).  Needs the GPU.  Prints one JSON line:

  summary_write_ms   host clock around _write_training_summary (inference-mode replay, histograms, grids, copies back, encoding,
                     file write + flush; ends in a device synchronise), median of --repeats after two warm-up writes
  histograms_ms      device events around the two histogram calls on the plan's stream, mean of 10 after 2 warm-ups
  histogram_bytes    bytes the two calls read (every segment once); hbm_floor_ms = those bytes at --hbm-tbs (LABBOOK.md's streaming rate)
  train_step_ms      the training plan's replay on the same batch (mean of --steps), unless --step-ms gives bench.py's figure
  share_of_training  summary_write_ms / (tensorboard_update_frequency * step ms): what summaries cost at the reference's frequency

    python tools/bench_summary.py [--batch 64] [--dtype bf16] [--repeats 5] [--steps 30] [--step-ms MS]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--step-ms", type=float, default=0.0, help="training step time to compare with (default: measured here)")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="streaming rate the floor is computed at, TB/s")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_summary.py needs the GPU"
    import bench
    from phiseg_code_amd import summary
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = bench.make_config(args.batch, args.dtype)
    model = phiseg_model.phiseg(cfg)
    data = synthetic.SyntheticLIDC(cfg, seed=1234)
    x, s = data.train.next_batch(cfg.batch_size)
    fd = {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: 1e-3}
    for _ in range(5):
        model.sess.run([model.train_step, model.loss_tot], fd)
    train_plan = model.sess._launch([model.loss_tot], fd, train=True)
    train_plan.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        train_plan.run()
    train_plan.sync()
    step_ms = 1e3 * (time.perf_counter() - t0) / args.steps

    model._summary_writer = summary.EventFileWriter(tempfile.mkdtemp(prefix="bench_summary_"))
    times = []
    for i in range(2 + args.repeats):
        t0 = time.perf_counter()
        model._write_training_summary(i, x, s, 1e-3)
        times.append(1e3 * (time.perf_counter() - t0))
    model._summary_writer.close()
    size = os.path.getsize(model._summary_writer.path)

    spec = model._summary_spec()
    plan = [p for p in model.sess.plans.values() if id(p) in spec["hist"]][0]
    act, _, _, par, _ = spec["hist"][id(plan)]
    L, st = plan.L, plan.stream
    import ctypes
    e0, e1, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float()
    L.event_create(ctypes.byref(e0))
    L.event_create(ctypes.byref(e1))
    for k in range(12):
        if k == 2:
            L.event_record(e0, st)
        act.run(st)
        par.run(st)
    L.event_record(e1, st)
    L.event_sync(e1)
    L.event_elapsed_ms(e0, e1, ctypes.byref(ms))
    hist_ms = ms.value / 10
    nbytes = act.bytes_read + par.bytes_read
    ref_step = args.step_ms or step_ms
    freq = cfg.tensorboard_update_frequency
    write_ms = float(np.median(times[2:]))
    print(json.dumps(dict(
        shape="phiseg_7_5 128x128 %s batch %d" % (args.dtype, args.batch), summary_write_ms=round(write_ms, 2),
        summary_write_ms_all=[round(t, 2) for t in times], histograms_ms=round(hist_ms, 3), histogram_segments=act.nseg + par.nseg,
        histogram_bytes=nbytes, hbm_floor_ms=round(nbytes / (args.hbm_tbs * 1e12) * 1e3, 3), hbm_tbs=args.hbm_tbs,
        histogram_read_tbs=round(nbytes / (hist_ms * 1e-3) / 1e12, 3), event_bytes_per_write=size // (2 + args.repeats),
        train_step_ms=round(step_ms, 3), step_ms_used=round(ref_step, 3), tensorboard_update_frequency=freq,
        share_of_training=round(write_ms / (freq * ref_step), 5))))


if __name__ == "__main__":
    main()
