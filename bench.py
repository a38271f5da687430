#!/usr/bin/env python3
"""bench.py -- training images/s of the PHiSeg ELBO step (phiseg_7_5, 128x128 LIDC-shaped, bf16, B=64/GPU).

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one full training step of the reference's hot loop (phiseg_model.py:194): forward of posterior,
teacher-forced prior and likelihood, 5 residual cross-entropy + 5 KL terms, backward, TF1 Adam -- for N > 1 plus
ONE flat gradient all-reduce over RCCL (weak scaling: 64 images per GPU).  Inputs are resident in HBM before the
timed region.  Rank 0 prints one JSON line.

A plain run sets up, warms up, times --steps steps and prints the line (metric, value, unit, higher_is_better, dtype,
ms_per_step = milliseconds per timed step).  --dump-outputs DIR then writes, as DIR/<name>.npy, what the timed plan computes
in the mode it was timed in: for training, one more step of that plan from the model's seeded initial state (the loss and
the updated weights and moving statistics); for sampling, the last timed pass's output.  Inputs, weights and noise are
seeded; the default mode's atomics sum in arbitrary order, so two runs agree up to rounding (PHX_DETERMINISTIC=1: bit
for bit).
--full adds the measurements that take runs of their own: `roofline` times the dominant kernel family (the bf16 MFMA 3x3
convolutions) with HIP events on the plan's own stream; `cpu_baseline` times the CPU oracle (port of the reference's TF1
graph -- TensorFlow 1.12 itself is not installable) on a bounded sample on the host cores; the other BASELINE.json
workloads and the reference's own loop; for N > 1 the gradient exchange's duration.
"""
import argparse
import importlib
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F_TRAIN_GFLOP_PER_IMAGE = 75.08       # fwd 25.026 + dgrad + wgrad, live graph, 128x128, 2 classes
PEAK_BF16_TFLOPS = 2500.0             # MI355X dense bf16 MFMA peak (/opt/skills/guides/MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3               # fp32 matrix peak (v_mfma_f32_32x32x2_f32, 64 FLOP/clk/SIMD): the fp32 parity path's roofline
DUMP_MAX_BYTES = 64 << 20             # --dump-outputs: all files together
DUMP_SAMPLE = 6 << 20                 # --dump-outputs: an output with more elements is written as a seeded sample of this many


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy, float64 kept, anything else as float32.  An array of more than DUMP_SAMPLE
    elements is written flattened as the elements at DUMP_SAMPLE fixed indices (seed 0, ascending): the same for every run and build
    of the same arguments, so two builds compare output for output.  More than DUMP_MAX_BYTES in all: ValueError, nothing written."""
    import numpy as np
    out = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
        if a.size > DUMP_SAMPLE:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, DUMP_SAMPLE, replace=False))]
        out[name] = a
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_MAX_BYTES:
        raise ValueError("--dump-outputs: %d bytes, more than %d" % (total, DUMP_MAX_BYTES))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def make_config(batch, compute_dtype, exp="phiseg_7_5", image_size=128, nlabels=None, norm="batch"):
    base = importlib.import_module("phiseg_code_amd.phiseg.experiments." + exp)
    cfg = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if not k.startswith("_")})
    cfg.batch_size = batch
    cfg.compute_dtype = compute_dtype
    cfg.image_size = (image_size, image_size, 1)
    if nlabels:
        cfg.nlabels = nlabels
    if norm != "batch":            # north_star names group / instance norm; every shipped experiment selects batch_norm
        from phiseg_code_amd.tfwrapper import normalisation as tfnorm
        cfg.layer_norm = {"group": tfnorm.group_norm2D, "instance": tfnorm.instance_norm2D}[norm]
    return cfg


def cpu_baseline(batch=12, steps=5):
    """The oracle (oracle/: port of the reference's TF 1.12 graph to torch-CPU, fp32) running the SAME training step on the
    host cores, from the SAME initial weights (seed 0, Philox stream contract) and the SAME synthetic images (seed 1234) as
    the GPU leg: `steps` timed steps at batch 12 -- the reference's own batch size (phiseg_7_5.py:40) -- after one warm-up.
    Five steps (round-3 review): a step takes ~14.5 s on the 128 host threads, a ~75 s sample; the per-step time varies by < 2 %
    between steps (round 1: 0.82 / 0.89 images/s on two boxes).
    Smaller batches are NOT a cheaper stand-in: at batch 2 the same port reaches only 0.32 images/s (the host threads
    starve), which would understate the CPU path."""
    import numpy as np
    import torch
    from oracle import init as oinit
    from oracle import train as otrain
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = dict(arch="phiseg", norm="batch_norm", n0=32, zdim0=2, latent_levels=5, resolution_levels=7, nlabels=2,
               image_size=(128, 128, 1), KL_weight=1.0, CE_weight=1.0, exponential_weighting=True)
    model = phiseg_model.phiseg(make_config(batch, "f32"))
    var_specs = [(n, v.shape) for n, v in model.graph.variables.items()]
    params = otrain.make_params(var_specs, 0, torch.float32, perturbed=False)
    x, s = oinit.synthetic_batch(batch, 128, 2, 1234)
    first = otrain.train_steps(params, [(x, s)], cfg, 42, lr=1e-3, n_steps=1, dtype=torch.float32)      # warm-up (= step 0)

    def timed(n):
        t0 = time.time()
        otrain.train_steps(params, [(x, s)], cfg, 42, lr=1e-3, n_steps=n, dtype=torch.float32)
        return time.time() - t0
    # The CPU leg gets its best thread count: one timed step on every hardware thread torch took and one on 32 threads (on a
    # multi-tenant 128-thread host the latter can be the faster one: an 8-core container runs this step in 4.4 s where 128 oversubscribed
    # threads took 13 - 30 s) -- the sample continues on the faster setting and `cores` reports it.
    nt_all = torch.get_num_threads()
    dt = timed(1)
    nthr = nt_all
    if nt_all > 32:
        torch.set_num_threads(32)
        dt32 = timed(1)
        if dt32 < dt:
            nthr, dt = 32, dt32
        else:
            torch.set_num_threads(nt_all)
    # ... then as many more steps as fit: a box whose host cores are busy with other tenants takes 30 s per step, and the default
    # run has to stay within minutes (~100 s of CPU sample).  (The warm-up call is no yardstick: its one-time costs made it 20+ s
    # on boxes whose timed steps then took 13 s, and the sample shrank to 2 steps.)
    more = max(1, min(steps - 1, int((100.0 - dt) / max(dt, 1e-3))))
    dt += timed(more)
    steps = 1 + more
    torch.set_num_threads(nt_all)
    return {"value": batch * steps / dt, "unit": "images/s", "cores": nthr, "kind": "port",
            "first_step_loss": first[0]["total_loss"],
            "sample": "%d training steps (fwd+ELBO+autograd+Adam) of phiseg_7_5 128x128 at batch %d, torch-CPU fp32 "
                      "oracle, %.1f s; same initial weights and images as the GPU leg" % (steps, batch, dt)}


def gpu_first_step_loss(args, batch=12):
    """The GPU engine's ELBO of training step 0 on the CPU baseline's twelve images, initial weights and Philox noise (bf16):
    the number to put next to cpu_baseline.first_step_loss."""
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = make_config(batch, args.dtype)
    model = phiseg_model.phiseg(cfg)
    x, s = synthetic.philox_batch(batch, 128, cfg.nlabels, seed=1234)
    _, loss = model.sess.run([model.train_step, model.loss_tot],
                             {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: 1e-3})
    return float(loss)


def conv_family(plan):
    """-> (rows, roofline dict) for the bf16 MFMA 3x3 forward + data-gradient launches of one step of `plan`, each timed alone with
    HIP events on the plan's stream."""
    rows_all = plan.time_tagged_kernels(repeats=3)
    rows = [r for r in rows_all if r[0].startswith("conv")]
    fam = {}
    for tag, fl, ms, shp in rows:
        a = fam.setdefault(tag, [0.0, 0.0, 0])
        a[0] += fl
        a[1] += ms
        a[2] += 1
    fl = sum(v[0] for k, v in fam.items() if k != "conv3x3_mfma_wgrad")
    ms = sum(v[1] for k, v in fam.items() if k != "conv3x3_mfma_wgrad")
    nl = sum(v[2] for k, v in fam.items() if k != "conv3x3_mfma_wgrad")
    return rows_all, rows, fam, fl, ms, nl


def side_workload(args, ctx, exp, norm, generate, steps=10, warmup=3, dtype=None):
    """One of the other BASELINE.json configurations inside the same bench invocation (10 timed steps): images/s and the
    convolution family's fraction of the MFMA peak, measured exactly as for the headline workload."""
    import torch
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    size = 192 if generate else 128
    batch = 1 if generate else args.batch
    spi = 16 if generate else 0
    cfg = make_config(batch, dtype or args.dtype, exp, size, 4 if generate else 0, norm)
    model = phiseg_model.phiseg(cfg)
    sess = model.sess
    if generate:
        plan = sess.plan_for([model.sampling_graph(spi)[1]], False, batch, False)
    else:
        plan = sess.plan_for([model.loss_tot], True, batch, True)
    x, s = synthetic.philox_batch(batch, size, cfg.nlabels, seed=1234)
    plan.set_input("x_input", x)
    if not generate:
        plan.set_input("s_input", s)
    sess.store.set_lr(1e-3)

    def step():
        plan.run()
        if generate:
            plan.L.step_increment(sess.store.noise_step.data_ptr(), plan.stream_handle())
    for _ in range(warmup):
        step()
    plan.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    plan.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"images_per_s": batch * max(spi, 1) * steps / dt, "ms_per_step": 1e3 * dt / steps, "steps": steps,
           "launches_per_step": len(plan.launches) + len(plan.opt_launches), "abi_launch_calls_per_step": plan.kernel_launch_count()}
    if (dtype or args.dtype) == "bf16":
        _, _, _, fl, ms, nl = conv_family(plan)
        if ms > 0:
            out["conv_frac_of_mfma_peak"] = fl / ms / 1e9 / PEAK_BF16_TFLOPS
    else:
        out["roofline"] = f32_roofline(plan)
    return out


def f32_roofline(plan):
    """The fp32 parity path's own roofline block: its 3x3 convolutions run on v_mfma_f32_32x32x2_f32 (csrc/conv_f32_mfma.hip), peak
    157.3 TFLOP/s.  Every tagged launch of one step timed alone with HIP events on the plan's stream, as for the bf16 family."""
    rows = [r for r in plan.time_tagged_kernels(repeats=2) if r[0].startswith("conv3x3_f32_mfma")]
    fam = {}
    for tag, fl, ms, shp in rows:
        a = fam.setdefault(tag, [0.0, 0.0, 0])
        a[0] += fl; a[1] += ms; a[2] += 1
    fl = sum(v[0] for v in fam.values())
    ms = sum(v[1] for v in fam.values())
    if ms <= 0:
        return None
    return {"bound": "mfma", "kernel": "k_conv3x3_f32_mfma<BN> / k_conv3x3_f32_mfma_small (forward + data gradient) + k_conv3x3_f32_wgrad<CIW,COW> "
                                       "(all three launches of every 3x3 layer of one step, each launch alone)",
            "achieved": fl / ms / 1e9, "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s", "frac": fl / ms / 1e9 / PEAK_F32_TFLOPS,
            "launches": sum(v[2] for v in fam.values()), "conv_ms_per_step": ms, "traffic": None,
            "families": {k: {"tflops": v[0] / v[1] / 1e9, "frac": v[0] / v[1] / 1e9 / PEAK_F32_TFLOPS, "ms_per_step": v[1], "launches": v[2]}
                         for k, v in fam.items()}}


def conv_in_situ(model, args, x, s, steps=6):
    """The bf16 convolution family's time INSIDE the running step, measured by this run: a second plan of the same graph on the same
    parameter store whose forward / data-gradient / filter-gradient convolution launches sit between wall-clock stamps on their lanes
    (engine.Plan(stamp_tagged=True)); `steps` replays, the last one read.  A launch's figure is stamp-to-stamp time minus the
    back-to-back stamp gap = its duration plus one launch boundary, beside whatever the other lane runs."""
    import torch
    sess = model.sess
    plan = sess.plan_for([model.loss_tot], True, args.batch, True, stamp_tagged=True)
    plan.set_input("x_input", x)
    plan.set_input("s_input", s)
    for _ in range(3):
        plan.run()
    plan.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.run()
    plan.sync()
    dt = time.perf_counter() - t0
    rows, gap = plan.tagged_in_situ()
    fam = {}
    for tag, fl, us, shp in rows:
        if tag.startswith("conv"):
            a = fam.setdefault(tag, [0.0, 0.0, 0])
            a[0] += fl; a[1] += us * 1e-3; a[2] += 1
    fl = sum(v[0] for k, v in fam.items() if k != "conv3x3_mfma_wgrad")
    ms = sum(v[1] for k, v in fam.items() if k != "conv3x3_mfma_wgrad")
    nl = sum(v[2] for k, v in fam.items() if k != "conv3x3_mfma_wgrad")
    return {"conv_fwd_dgrad_ms_per_step": ms, "conv_fwd_dgrad_launches_per_step": nl, "flops": fl, "stamp_gap_us": gap,
            "ms_per_step_with_stamps": 1e3 * dt / steps,
            "families": {k: {"tflops": v[0] / v[1] / 1e9, "ms_per_step": v[1], "launches": v[2]} for k, v in fam.items() if v[1] > 0},
            "source": "measured by this run: wall-clock stamps around every convolution launch of a replayed step (second plan, same "
                      "store; launch duration + one launch boundary each, two lanes running)"}


def train_api_rate(args, model, steps=10):
    """The reference's actual hot loop (phiseg_model.py:186-207): sess.run([train_step, loss_tot], feed_dict) with host batches and the
    loss fetched EVERY step -- H2D copy of the batch, graph replay, D2H of the scalar, one synchronisation per step."""
    from phiseg_code_amd.data import synthetic
    x, s = synthetic.philox_batch(args.batch, args.image_size, model.exp_config.nlabels, seed=4321)
    fd = {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: 1e-3}
    for _ in range(2):
        model.sess.run([model.train_step, model.loss_tot], fd)
    t0 = time.perf_counter()
    for _ in range(steps):
        _, loss = model.sess.run([model.train_step, model.loss_tot], fd)
        float(loss)
    return args.batch * steps / (time.perf_counter() - t0)


def self_launch(n):
    """`python bench.py --gpus N` from a plain shell (no WORLD_SIZE in the environment): run
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py <argv>`
    as a child process, one rank per GPU, and exit with its status; rank 0 prints the one JSON line.  (A child, not exec: the
    device count below initialises the GPU runtime, and a process holding the GPU must not replace its program.)  (RCCL refuses
    two ranks on one device: with fewer GPUs than ranks only PHX_DIST_BACKEND=gloo -- the protocol-test transport -- is accepted.)"""
    import socket
    import subprocess
    import torch
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < n and os.environ.get("PHX_DIST_BACKEND") != "gloo":
        sys.exit("bench.py: --gpus %d but %d GPU(s) visible (RCCL needs one device per rank; PHX_DIST_BACKEND=gloo runs "
                 "the ranks on the GPUs there are, host-staged: protocol check only)" % (n, have))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    rc = subprocess.call(cmd)
    sys.exit(rc if rc >= 0 else 128 - rc)            # (killed by signal k: the shell's 128 + k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)      # (>= 100 timed steps; ~1.1 s at batch 64)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the timed plan computes as DIR/<name>.npy (training: one more step "
                         "from the seeded initial state; sampling: the last timed pass)")
    ap.add_argument("--full", action="store_true",
                    help="also roofline, cpu_baseline, config.other_workloads / train_api_images_per_s and, for N > 1, the "
                         "gradient exchange's duration (each measured after the timed steps)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without cpu_baseline")
    ap.add_argument("--no-roofline", action="store_true", help="--full without roofline")
    ap.add_argument("--no-other-workloads", action="store_true", help="--full without config.other_workloads / train_api_images_per_s")
    ap.add_argument("--profile-table", action="store_true", help="--full: print the per-layer kernel timing table")
    # the other BASELINE.json configurations (the default run is config 2, the headline metric):
    ap.add_argument("--exp", default="phiseg_7_5", help="experiment config (phiseg/experiments/*.py), e.g. probunet")
    ap.add_argument("--workload", default="train", choices=["train", "generate"],
                    help="generate: Monte-Carlo sampling passes (prior sample + likelihood decode + softmax), config 5")
    ap.add_argument("--image-size", type=int, default=128)
    ap.add_argument("--nlabels", type=int, default=0, help="0: the experiment's own")
    ap.add_argument("--norm", default="batch", choices=["batch", "group", "instance"],
                    help="layer_norm of the experiment (every shipped experiment: batch; north_star also names group / instance)")
    ap.add_argument("--samples-per-image", type=int, default=16,
                    help="generate: Monte-Carlo samples drawn per image in one pass (the prior's x-only encoder is shared); "
                         "0: one sample per image and pass, the reference's call pattern")
    args = ap.parse_args()
    if args.profile_table and not args.full:
        ap.error("--profile-table prints the roofline measurement's tables: add --full")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)            # does not return: exits with the status of its torch.distributed.run child

    import numpy as np
    import torch
    from phiseg_code_amd import distributed
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model

    ctx = distributed.DistContext(force=os.environ.get("PHX_FORCE_DIST") == "1")   # dev: exercise the split path on one GPU
    assert ctx.world == args.gpus, "launch with torch.distributed.run --nproc-per-node %d" % args.gpus
    generate = args.workload == "generate"
    spi = args.samples_per_image if generate else 0
    if generate and spi and args.exp.startswith("phiseg") and args.batch == 64:
        args.batch = 1                    # BASELINE config 5: one image, 16 Monte-Carlo samples per pass
    cfg = make_config(args.batch, args.dtype, args.exp, args.image_size, args.nlabels, args.norm)
    model = phiseg_model.phiseg(cfg, dist=ctx if ctx.active else None)
    sess = model.sess
    if generate and spi and args.exp.startswith("phiseg"):
        plan = sess.plan_for([model.sampling_graph(spi)[1]], False, args.batch, False)
    elif generate:
        spi = 0
        plan = sess.plan_for([model.s_out_eval_sm], False, args.batch, False)
    else:
        plan = sess.plan_for([model.loss_tot], True, args.batch, True)
    # seeded Philox inputs: rank r draws samples [r * batch, (r + 1) * batch) of the global batch (seed 1234)
    x, s = synthetic.philox_batch(args.batch, args.image_size, cfg.nlabels, seed=1234, sample_offset=ctx.rank * args.batch)
    plan.set_input("x_input", x)          # resident in HBM for the whole run
    if not generate:
        plan.set_input("s_input", s)
    sess.store.set_lr(1e-3)
    if ctx.active:                        # identical replicas
        ctx.broadcast_(sess.store.params)
        ctx.broadcast_(sess.store.state)
        torch.cuda.synchronize()          # the plan replays on its own HIP streams: finish the broadcasts first

    def step():
        if generate:                      # one sampling pass over the batch; fresh noise for the next one (on the plan's stream)
            plan.run()
            plan.L.step_increment(sess.store.noise_step.data_ptr(), plan.stream_handle())
        elif ctx.active:
            plan.run_main()
            ctx.allreduce_sum(sess.store.grads[:sess.store.n_live], plan)
            plan.run_opt()
        else:
            plan.run()

    for _ in range(max(args.warmup, 2)):  # >= 2: eager pass, then hipGraph capture
        step()
    plan.sync()
    torch.cuda.synchronize()
    ctx.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    plan.sync()
    torch.cuda.synchronize()
    ctx.barrier()
    dt_own = time.perf_counter() - t0
    dt = ctx.max_float(dt_own)
    loss = None if generate else float(plan.fetch(model.loss_tot))
    assert plan.barrier_timeouts() == 0, "an in-kernel grid barrier timed out during the timed steps: the result is invalid"
    if args.dump_outputs:
        st = sess.store
        if not generate:
            # The state after the timed training steps is not reproducible: the default mode's atomics sum in arbitrary order, and
            # Adam and the training dynamics amplify the last-bit differences over the steps.  So the store goes back to its seeded
            # initial state (weights, moving statistics, Adam moments, step and noise counter) and the timed plan runs one more step,
            # in the mode it was timed in (every rank: the step includes the gradient exchange).
            st.initialize(model.init_seed)
            torch.cuda.synchronize()              # (torch work; the plan replays on its own streams)
            step()
            plan.sync()
            torch.cuda.synchronize()
            assert plan.barrier_timeouts() == 0, "an in-kernel grid barrier timed out in the step of --dump-outputs"
        if ctx.rank == 0:
            if generate:                          # the last timed pass's soft-max output (sampling never changes the weights)
                outs = {"output": plan.fetch(plan.fetches[0])}
            else:                                 # what a caller of the step holds after it: the loss and the updated model
                outs = {"loss_tot": plan.fetch(model.loss_tot), "params": st.params[:st.n_live]}
                if st.n_state:
                    outs["state"] = st.state[:st.n_state]
            dump_outputs(args.dump_outputs, outs)
    ranks_seen = int(round(ctx.sum_float(1.0)))          # every rank that really took part in the timed collectives
    dp_diag = None
    if args.full and ctx.active and not generate:
        try:
            # after the timed region: what a first multi-GPU run needs to diagnose itself -- every rank's own time for the timed steps and
            # the duration of the gradient exchange (HIP events on the plan's stream around phx_comm_allreduce_sum_f32, ten more steps)
            import ctypes
            from phiseg_code_amd import runtime as rt
            Lb = rt.lib()
            evs = []
            for _ in range(10):
                e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
                Lb.event_create(ctypes.byref(e0)); Lb.event_create(ctypes.byref(e1))
                plan.run_main()
                Lb.event_record(e0, ctypes.c_void_p(plan.stream_handle()))
                ctx.allreduce_sum(sess.store.grads[:sess.store.n_live], plan)
                Lb.event_record(e1, ctypes.c_void_p(plan.stream_handle()))
                plan.run_opt()
                evs.append((e0, e1))
            plan.sync()
            torch.cuda.synchronize()
            ar = []
            for e0, e1 in evs:
                ms_ = ctypes.c_float()
                Lb.event_elapsed_ms(e0, e1, ctypes.byref(ms_))
                ar.append(ms_.value)
                Lb.event_destroy(e0); Lb.event_destroy(e1)
            ar_ms = float(np.median(ar))
            dp_diag = {"allreduce_ms_median_rank0": ar_ms, "allreduce_ms_max_over_ranks": ctx.max_float(ar_ms),
                       "allreduce_mbytes": sess.store.n_live * 4 / 1e6,
                       "ms_per_step_per_rank": [1e3 * v / args.steps for v in ctx.gather_floats(dt_own)],
                       "note": "measured after the timed region (ten extra steps); allreduce_ms includes the wait for the slowest rank's backward"}
        except Exception as e:      # (the diagnostic must never cost the line; every rank runs the same code, so a failure is symmetric)
            dp_diag = {"error": repr(e)}
        ctx.barrier()
    images = args.batch * max(spi, 1) * ctx.world * args.steps
    out = {
        "metric": ("segmentation samples/sec (prior sample + likelihood decode) %s %dx%d" % (args.exp, args.image_size, args.image_size))
                  if generate else "training images/sec (ELBO step) %s %dx%d LIDC" % (args.exp, args.image_size, args.image_size),
        "value": images / dt,
        "unit": "images/s", "n_gpus": ctx.world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": ("%s %dx%dx1, %d classes, %s, %d image(s) per GPU and pass, %s (prior sample + likelihood decode + "
                                "softmax)" % (args.exp, args.image_size, args.image_size, cfg.nlabels, args.dtype, args.batch,
                                              ("%d Monte-Carlo samples per image in one pass, the prior's x-only encoder shared" % spi)
                                              if spi else "one sample per image")) if generate else
                               "%s LIDC %dx%dx1, %d classes, %s, %s norm, batch %d per GPU, full ELBO training step "
                               "(fwd + CE + KL + bwd + Adam%s)" % (args.exp, args.image_size, args.image_size, cfg.nlabels,
                                                                   args.dtype, args.norm, args.batch,
                                                                   " + RCCL grad all-reduce" if ctx.world > 1 else ""),
                   "global_batch": args.batch * ctx.world, "parallelism": "dp%d" % ctx.world,
                   # plan entries (launch calls + the event records / waits between the two lanes) and the launch calls into the C ABI
                   # alone (a split-K convolution's finishing kernel rides inside its call: a kernel trace counts ~50 more)
                   "launches_per_step": len(plan.launches) + len(plan.opt_launches),
                   "abi_launch_calls_per_step": plan.kernel_launch_count(), "final_loss": loss,
                   # which transport carried the timed gradient exchange (a fallback cannot be timed unnoticed)
                   "comm": {"path": ctx.comm_path(), "ranks_seen": ranks_seen}},
    }
    if dp_diag is not None:
        out["config"]["comm"].update(dp_diag)
    if not generate and args.exp == "phiseg_7_5" and args.image_size == 128:
        out["step_tflops"] = images / dt * F_TRAIN_GFLOP_PER_IMAGE / 1e3
    if args.full and ctx.rank == 0 and not args.no_roofline and args.dtype == "bf16":
        rows_all, rows, fam, fl, ms, nl = conv_family(plan)
        if args.profile_table:
            hb = {}
            for tag, by, ms_, shp in rows_all:
                if tag.startswith("bytes_"):
                    cls = sum(by >= lim for lim in (1e6, 4e6, 16e6, 64e6))
                    a = hb.setdefault((tag, cls), [0.0, 0.0, 0])
                    a[0] += by; a[1] += ms_; a[2] += 1
            for key in sorted(hb):
                a = hb[key]
                print("### %-24s %-8s launches=%3d %8.3f ms  %8.1f GB/s  %6.1f us/launch" % (
                    key[0], ("<1MB", "1-4MB", "4-16MB", "16-64MB", ">=64MB")[key[1]], a[2], a[1], a[0] / a[1] / 1e6, 1e3 * a[1] / a[2]),
                      file=sys.stderr)
        if args.profile_table:
            for tag, fl_, ms_, shp in sorted(rows, key=lambda r: -r[2]):
                print("# %-20s %8.3f ms %8.1f TFLOP/s  %s" % (tag, ms_, fl_ / ms_ / 1e9, shp[-5:]), file=sys.stderr)
            byh = {}
            for tag, fl_, ms_, shp in rows:
                key = (tag, shp[-4])                      # launch arguments end (..., B, H, W, Cin|K, Cout|N)
                a = byh.setdefault(key, [0.0, 0.0, 0])
                a[0] += fl_; a[1] += ms_; a[2] += 1
            for key in sorted(byh):
                a = byh[key]
                print("## %-20s H=%-4d launches=%3d  %8.3f ms  %8.1f TFLOP/s" % (key[0], key[1], a[2], a[1], a[0] / a[1] / 1e9),
                      file=sys.stderr)
        # the dominant instantiation on its own: the launches of the shape class that takes the most time (forward + data gradient)
        bysh = {}
        for tag, fl_, ms_, shp in rows:
            if tag != "conv3x3_mfma_wgrad":
                a = bysh.setdefault(tuple(shp[-5:]), [0.0, 0.0, 0])
                a[0] += fl_; a[1] += ms_; a[2] += 1
        dom = max(bysh.items(), key=lambda kv: kv[1][1]) if bysh else None
        # HBM traffic of the same kernel family and its time inside the running step: NOT measured by this run -- read from the
        # committed profile set of the headline configuration (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, corrected as
        # MI355X_MICROARCH.md prescribes, and the kernel trace of the timed steps: tools/collect_profiles.sh), so they are attached
        # to the headline configuration only and carry their source
        traffic = in_situ = traffic_src = None
        headline_cfg = (not generate and args.exp == "phiseg_7_5" and args.image_size == 128 and args.norm == "batch" and args.batch == 64)
        if headline_cfg:
            try:
                tf_ = next(f for f in ("r06_pmc_hbm_traffic.json", "r05_pmc_hbm_traffic.json") if os.path.exists(os.path.join(ROOT, "profiles", f)))
                pj = json.load(open(os.path.join(ROOT, "profiles", tf_)))
                ks = [v for k, v in pj.items() if isinstance(v, dict) and any(t in k for t in ("k_conv3x3_pp", "k_conv3x3_c32", "k_conv3x3_mfma"))]
                calls = sum(v["calls_per_step"] for v in ks)
                traffic = 1e6 * sum(v["fetch_x2_MB_per_step"] + v["write_MB_per_step"] for v in ks) / calls
                meta = pj.get("_meta") or {}
                traffic_src = ("PMC counters cannot be read by the timed process: committed profile profiles/" + tf_ +
                               (" collected at commit " + meta["commit"] if meta.get("commit") else "") + " by tools/collect_profiles.sh")
            except Exception:
                pass
            try:
                # (single process only: a data-parallel rank 0 would step its replica alone)
                in_situ = conv_in_situ(model, args, x, s) if ctx.world == 1 else None
            except Exception as e:        # the headline line must not depend on the diagnostic
                in_situ = None
                print("bench.py: in-situ measurement failed: %r" % (e,), file=sys.stderr)
        alg_bytes = 0.0
        for tag, flp, ms_, shp in rows:
            if tag != "conv3x3_mfma_wgrad":
                Bq, Hq, Wq, Kq, Nq = shp[-5:]
                alg_bytes += 2.0 * Bq * Hq * Wq * (Kq + Nq) + 18.0 * Kq * Nq
        out["roofline"] = {
            "bound": "mfma", "kernel": "k_conv3x3_pp / k_conv3x3_c32 (large maps) + k_conv3x3_mfma<BN> (forward + data-gradient launches of one step)",
            "achieved": fl / ms / 1e9, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": fl / ms / 1e9 / PEAK_BF16_TFLOPS,
            "frac_isolated": fl / ms / 1e9 / PEAK_BF16_TFLOPS,
            "traffic": traffic, "traffic_unit": "HBM bytes per launch (PMC FETCH_SIZE x 2 + WRITE_SIZE, separate rocprofv3 passes)",
            "traffic_source": traffic_src,
            "algorithmic_bytes_per_launch_avg": alg_bytes / max(nl, 1),
            "launches": nl, "avg_launch_ms": ms / max(nl, 1),
            "algorithmic_gflop_per_launch_avg": fl / max(nl, 1) / 1e9,
            "families": {k: {"tflops": v[0] / v[1] / 1e9, "ms_per_step": v[1], "launches": v[2]} for k, v in fam.items()},
            "conv_ms_per_step": sum(v[1] for v in fam.values()),
        }
        if in_situ and in_situ["conv_fwd_dgrad_ms_per_step"] > 0:
            # the family's time inside the running step, measured by this run, against the same FLOPs: THE roofline fraction;
            # `frac_isolated` (each launch alone, HIP events) stays beside it
            fi = fl / in_situ["conv_fwd_dgrad_ms_per_step"] / 1e9
            out["roofline"].update(achieved=fi, frac=fi / PEAK_BF16_TFLOPS, frac_in_situ=fi / PEAK_BF16_TFLOPS,
                                   achieved_isolated=fl / ms / 1e9, in_situ=in_situ)
            # cross-reference, NOT measured by this run: the same family's kernel durations in the committed rocprofv3 kernel trace
            # (no launch boundaries in it: the figure earlier rounds quoted as "in situ")
            try:
                kt = json.load(open(os.path.join(ROOT, "profiles", "r06_conv_in_situ.json")))
                out["roofline"]["frac_kernel_trace_committed"] = {
                    "frac": fl / kt["conv_fwd_dgrad_ms_per_step"] / 1e9 / PEAK_BF16_TFLOPS, "ms_per_step": kt["conv_fwd_dgrad_ms_per_step"],
                    "source": "profiles/r06_conv_in_situ.json (rocprofv3 --kernel-trace of bench.py, tools/collect_profiles.sh; another box, another run)"}
            except Exception:
                pass
        # launches of the family that also carry the layer's group norm (phx_conv3x3_mfma_bf16_fgn: statistics, second pass):
        # counted in `achieved` with their whole duration, listed here so that the convolution-only part can be read off
        fb = [(fl_, ms_) for tag, fl_, ms_, shp in rows if shp and shp[0] == "fgn"]
        if fb:
            out["roofline"]["fused_conv_gn_launches"] = {"launches": len(fb), "ms_per_step": sum(m for _, m in fb),
                                                         "gflop_per_step": sum(f for f, _ in fb) / 1e9}
        if dom is not None:
            out["roofline"]["dominant_shape"] = {"B_H_W_K_N": list(dom[0]), "launches": dom[1][2], "ms_per_step": dom[1][1],
                                                 "tflops": dom[1][0] / dom[1][1] / 1e9,
                                                 "frac": dom[1][0] / dom[1][1] / 1e9 / PEAK_BF16_TFLOPS}
    headline = (not generate and args.exp == "phiseg_7_5" and args.image_size == 128 and args.norm == "batch" and args.dtype == "bf16"
                and args.batch == 64)
    if args.full and ctx.rank == 0 and ctx.world == 1 and headline and not args.no_other_workloads:
        # the other BASELINE.json configurations and the reference's own loop, inside the same invocation (the headline line above is
        # unchanged by them: they run after its timed region)
        # the reference's own loop (sess.run with a host batch and the loss fetched every step, phiseg_model.py:193-194): the like-for-like figure
        out["train_api_images_per_s"] = out["config"]["train_api_images_per_s"] = train_api_rate(args, model)
        ow = {}
        ow["phiseg_7_5 group norm (config 2 as named), training step"] = side_workload(args, ctx, "phiseg_7_5", "group", False)
        ow["probunet (config 4), training step"] = side_workload(args, ctx, "probunet", "batch", False)
        ow["phiseg_7_5 192x192 4 classes, 16 Monte-Carlo samples per pass (config 5), generate"] = side_workload(args, ctx, "phiseg_7_5", "batch", True)
        # what north_star's 1e-4 parity costs: the fp32 path (conv_direct.hip, VALU), the one pinned to the oracle's per-level logits / ELBO
        ow["phiseg_7_5 fp32 parity path, training step"] = side_workload(args, ctx, "phiseg_7_5", "batch", False, steps=10, warmup=2, dtype="f32")
        out["config"]["other_workloads"] = ow
    if args.full and ctx.rank == 0 and ctx.world == 1 and not args.no_cpu_baseline and not generate and args.exp == "phiseg_7_5" \
            and args.image_size == 128 and args.norm == "batch":
        out["cpu_baseline"] = cpu_baseline()
        out["cpu_baseline"]["gpu_first_step_loss_same_inputs"] = gpu_first_step_loss(args)
    if ctx.rank == 0:
        out["config"]["hbm_peak_allocated_gb"] = torch.cuda.max_memory_allocated() / 2 ** 30
    ctx.barrier()              # the other ranks wait for rank 0's extra measurements before tearing RCCL down
    ctx.shutdown()
    if ctx.rank == 0:
        # RCCL writes its version banner through C stdio; when stdout is a pipe it sits in libc's buffer until exit and would
        # land AFTER the result.  Flush it first so that the JSON line is the last line of rank 0's stdout.
        import ctypes
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
