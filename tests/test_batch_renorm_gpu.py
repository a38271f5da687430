"""Batch renormalisation on the GPU (csrc/norm_renorm.hip and its lowering): both forward routes and the tail launch through the C ABI
against the float64 restatement tests/renorm_ref.py, a two-layer graph's gradients against torch float64 convolutions around it, and
the tiny PHiSeg configuration with layer_norm=batch_renorm: step 0 against batch norm, the clipping schedule under graph replay,
inference, checkpoints, determinism, summaries, bf16."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import renorm_ref as R
from tests.helpers import load_golden
from tests.test_graph_cpu import make_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
FP32_TOL = 1e-4                     # the project's fp32 parity bound, relative to the tensor's largest magnitude
ULP8 = 8 * 2.0 ** -23               # state after the tail launch (the bound style of tests/test_momentum_gpu.py)
SENT = 7.25
TAIL_DT = [(n, "<u8") for n in ("mean", "rstd", "r", "d", "dgs", "dbs", "dgamma", "dbeta", "rmean", "rmean_w", "rstddev", "rstddev_w", "mmean",
                                "mvar")] + [("C", "<i4"), ("eps", "<f4"), ("renorm_momentum", "<f4"), ("moving_momentum", "<f4")]


@pytest.fixture(scope="module")
def L():
    from phiseg_code_amd import runtime as rt
    return rt.lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def tdt(dt):
    return torch.float32 if dt == F32 else torch.bfloat16


def f32(a):
    return np.asarray(a, dtype=np.float32)


def padded(n, dt=F32):
    """n elements + 16 sentinels behind them"""
    t = torch.full((n + 16,), SENT, dtype=tdt(dt), device="cuda")
    return t


def body(t, n):
    assert bool((t[n:].float() == SENT).all()), "written past the end"
    return t[:n].float().cpu().numpy().astype(np.float64)


def within(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, mag = np.abs(got - want).max(), max(np.abs(want).max(), 1e-30)
    print("%-40s err %.2e of max %.2e (bound %.1e)" % (what, err, mag, tol))
    assert err <= tol * mag, (what, err, mag)


def _inputs(P, C, dt, seed):
    rng = np.random.default_rng(seed)
    x = 1.5 * rng.standard_normal((P, C)) * (0.5 + rng.random(C)) + rng.standard_normal(C)
    x = torch.as_tensor(f32(x)).to(tdt(dt)).float().numpy()              # representable in the storage dtype
    gamma, beta = f32(1.0 + 0.3 * rng.standard_normal(C)), f32(0.2 * rng.standard_normal(C))
    return rng, x, gamma, beta


def _state_for(rng, x, regime):
    """-> (t, state dict of fp32-representable float64 arrays).  The warm states are built from the batch's own moments so that every
    channel class the contract names is present; the stored mean sits about 2 sigma (or further, where d has to clip) from the batch's."""
    C = x.shape[1]
    x64 = x.astype(np.float64)
    mu, sigma = x64.mean(0), np.sqrt(x64.var(0) + 1e-3)
    if regime == "fresh":
        return 0, R.fresh_state(C)
    w = 0.95
    cls = np.arange(C) % 6
    if regime == "t100":                                   # rmax = 1, dmax = 0: r < 1 kept, r > 1 cut to 1, d = 0
        t, r_t, d_t = 100, np.where(cls % 2 == 0, 0.6, 1.7), np.where(cls < 3, 2.0, -2.0)
    elif regime == "t1500":                                # bounds 1.5714..., 2.5
        t, r_t, d_t = 1500, 0.5 + 2.0 * rng.random(C), rng.uniform(-4.0, 4.0, C)
    else:                                                  # t = 4500: r hits 3, r ~ 0.2 unclipped, d hits +-5, interior d ~ 2
        t = 4500
        r_t = np.choose(cls, [5.0, 0.2, 1.3, 0.8, 1.0, 2.0])
        d_t = np.choose(cls, [2.0, -1.0, 8.0, -8.0, 2.0, 0.5])
    mix_sigma = sigma / r_t
    mix_mean = mu - d_t * mix_sigma
    st = dict(renorm_mean=mix_mean - (1 - w) * mu, renorm_mean_weight=w, renorm_stddev=mix_sigma - (1 - w) * sigma, renorm_stddev_weight=w,
              moving_mean=mu + 0.1, moving_variance=sigma ** 2 * 1.1)
    assert np.all(st["renorm_stddev"] > 0)
    return t, {k: f32(v).astype(np.float64) if np.ndim(v) else float(np.float32(v)) for k, v in st.items()}


def _check_regime_hits(f, regime):
    r, d = f["r"], f["d"]
    if regime == "fresh":
        assert np.all(r == 1.0) and np.all(d == 0.0)
    elif regime == "t100":
        assert np.any(r < 0.7) and np.any(r == 1.0) and np.all(d == 0.0)
    elif regime == "t4500":
        assert np.any(r == 3.0) and np.any(np.abs(r - 0.2) < 0.01) and np.any(d == 5.0) and np.any(d == -5.0) and np.any(np.abs(d - 2.0) < 0.05)


SHAPES = [(8, 32), (18, 8), (512, 192), (4096, 32)]


@pytest.mark.parametrize("route", ["generic", "small"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("P, C", SHAPES)
def test_forward_routes_and_tail_against_reference(L, P, C, dt, route):
    """phx_norm_stats + phx_renorm_apply_fused (generic) / phx_renorm_small_fwd (one launch), then phx_renorm_tail_multi, in the four
    state regimes.  The step value only changes in device memory between the launches; sentinels sit behind every output."""
    rng, x, gamma, beta = _inputs(P, C, dt, 100 + P + C)
    xd = torch.as_tensor(x).to(tdt(dt)).cuda()
    gd, bd = torch.as_tensor(gamma).cuda(), torch.as_tensor(beta).cuda()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()
    for regime in ("fresh", "t100", "t1500", "t4500"):
        t, st = _state_for(rng, x, regime)
        step.fill_(t)
        dev_st = {k: torch.as_tensor(f32(np.atleast_1d(v))).cuda() for k, v in st.items()}
        y = padded(P * C, dt)
        vec = {k: padded(C) for k in ("mean", "rstd", "scale", "shift", "r", "d", "gamma_eff")}
        tail = (p(vec["r"]), p(vec["d"]), p(vec["gamma_eff"]), p(dev_st["renorm_mean"]), p(dev_st["renorm_mean_weight"]), p(dev_st["renorm_stddev"]),
                p(dev_st["renorm_stddev_weight"]), p(step), P, C, 1, S())
        if route == "generic":
            sums, pivot = torch.zeros(2 * C, device="cuda"), torch.zeros(C, device="cuda")
            L.norm_stats(p(xd), dt, p(sums), p(pivot), 1, P, C, S())
            L.renorm_apply_fused(p(xd), dt, p(sums), p(pivot), p(gd), p(bd), 1e-3, p(y), dt, p(vec["mean"]), p(vec["rstd"]), p(vec["scale"]),
                                 p(vec["shift"]), *tail)
        else:
            assert L.renorm_small_supported(P, C, dt, dt) == 1
            L.renorm_small_fwd(p(xd), dt, p(gd), p(bd), 1e-3, p(y), dt, p(vec["mean"]), p(vec["rstd"]), p(vec["scale"]), p(vec["shift"]), *tail)
        torch.cuda.synchronize()
        f = R.forward(x, gamma.astype(np.float64), beta.astype(np.float64), st, t, "relu")
        _check_regime_hits(f, regime)
        what = "%s %s (%d, %d) %s " % (route, "bf16" if dt else "f32", P, C, regime)
        got_y = body(y, P * C).reshape(P, C)
        if dt == F32:
            within(got_y, f["y"], FP32_TOL, what + "y")
        else:
            err = np.abs(got_y - f["y"])
            bound = 2.0 ** -8 * np.abs(f["y"]) + FP32_TOL * np.abs(f["y"]).max()
            print("%-40s worst err / bound %.3f" % (what + "y", (err / bound).max()))
            assert np.all(err <= bound), (what, (err / bound).max())
        got = {k: body(v, C) for k, v in vec.items()}
        for k in vec:
            within(got[k], f[k], FP32_TOL, what + k)
        if regime == "fresh":
            assert np.all(got["r"] == 1.0) and np.all(got["d"] == 0.0), "fresh state: r == 1 and d == 0 exactly"
        for k, v in st.items():                     # the forward launch only reads the state
            assert np.array_equal(dev_st[k].cpu().numpy().astype(np.float64), np.atleast_1d(v)), k
        # ---- the tail launch: corrected gradients onto a non-zero arena, six state updates from the saved mean / rstd
        dgs, dbs = f32(rng.standard_normal(C)), f32(rng.standard_normal(C))
        dgs_d, dbs_d = torch.as_tensor(dgs).cuda(), torch.as_tensor(dbs).cuda()
        dg, db = padded(C), padded(C)
        dg[:C], db[:C] = 0.5, -0.25
        stp = {k: padded(v.numel()) for k, v in dev_st.items()}
        for k, v in dev_st.items():
            stp[k][:v.numel()] = v
        rec = np.zeros(1, dtype=TAIL_DT)
        assert rec.dtype.itemsize == L.renorm_tail_desc_bytes()
        rec[0] = (p(vec["mean"]), p(vec["rstd"]), p(vec["r"]), p(vec["d"]), p(dgs_d), p(dbs_d), p(dg), p(db), p(stp["renorm_mean"]),
                  p(stp["renorm_mean_weight"]), p(stp["renorm_stddev"]), p(stp["renorm_stddev_weight"]), p(stp["moving_mean"]),
                  p(stp["moving_variance"]), C, 1e-3, 1.0 - 0.99, 1.0 - 0.999)
        desc = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        L.renorm_tail_multi(p(desc), 1, S())
        torch.cuda.synchronize()
        within(body(dg, C), 0.5 + got["r"] * dgs + got["d"] * dbs, 1e-6, what + "dgamma")
        within(body(db, C), -0.25 + dbs.astype(np.float64), 1e-6, what + "dbeta")
        want = R.update(st, got["mean"], got["rstd"])                    # the recurrence fed the device's own mean / rstd
        for k in R.STATE:
            n = dev_st[k].numel()
            within(body(stp[k], n), np.atleast_1d(want[k]), ULP8, what + "state " + k)


def test_small_route_refuses_what_it_does_not_support(L):
    """P > 4096, C % 8 != 0, an unknown dtype: the invalid-argument status (-1), nothing launched (tests/test_tail_fusions_gpu.py:102)."""
    from phiseg_code_amd import runtime as rt
    p = lambda t: t.data_ptr()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    for P, C, dt in ((4097, 32, F32), (18, 12, F32), (16, 4, BF16), (16, 16, 2)):
        assert L.renorm_small_supported(P, C, dt, dt if dt < 2 else F32) == 0
        x = torch.ones(P * C, device="cuda")
        y = torch.full((P * C,), SENT, device="cuda")
        v = [torch.full((C,), SENT, device="cuda") for _ in range(7)]
        s = [torch.zeros(C, device="cuda") for _ in range(4)]
        with pytest.raises(rt.PhxError, match=r"\(-1\)"):
            L.renorm_small_fwd(p(x), dt, p(s[0]), p(s[0]), 1e-3, p(y), dt if dt < 2 else F32, *[p(t) for t in v], *[p(t) for t in s], p(step), P, C, 1, S())
        torch.cuda.synchronize()
        assert bool((y == SENT).all()) and all(bool((t == SENT).all()) for t in v)


# ---- a two-layer graph: conv2D(normalisation=batch_renorm) twice, the second on a 4 x 4 map at batch 2 ----------------------------------
def test_two_layer_graph_gradients_against_float64(L):
    """Layer 1 is a strided convolution (a general unit), layer 2 a plain 3x3 on the 4 x 4 map; in an fp32 plan both take the generic
    forward route (the one-launch route belongs to bf16 plans, like batch norm's: the bf16 model test below runs it).  Warm state, t = 4500.  Loss, dgamma, dbeta and both filter gradients (the first layer's carries the second layer's dx) against torch
    float64 convolutions around renorm_ref; after the run the state follows the ref's update."""
    from oracle import tf1_ops as T
    from phiseg_code_amd import engine
    from phiseg_code_amd import graph as G
    from phiseg_code_amd.engine_common import NormRoute
    from phiseg_code_amd.tfwrapper import activations as act
    from phiseg_code_amd.tfwrapper import layers
    from phiseg_code_amd.tfwrapper import normalisation as tfnorm
    B, H, NC, t = 2, 8, 2, 4500
    g = G.reset_default_graph()
    x_inp = G.placeholder(G.KIND_F32, [None, H, H, 3], name="x_input")
    s_inp = G.placeholder(G.KIND_U8, [None, 4, 4], name="s_input")
    with g.variable_scope("net"):
        a1 = layers.conv2D(x_inp, "c1", num_filters=8, strides=(2, 2), normalisation=tfnorm.batch_renorm, training=True)       # 4 x 4
        a2 = layers.conv2D(a1, "c2", num_filters=16, normalisation=tfnorm.batch_renorm, training=True)
        s = layers.conv2D(a2, "head", num_filters=NC, kernel_size=(1, 1), activation=act.identity)
    ce, _ = G.residual_multinoulli([s], s_inp, 1.0)
    loss = G.weighted_sum([ce[0]], [1.0])
    assert "net/c1/b" not in g.variables and "net/c2/batch_renorm/BatchNorm/renorm_stddev_weight" in g.variables
    store = engine.ParamStore(g, seed=3)
    rng = np.random.default_rng(9)
    vals = {}
    for n, v in g.variables.items():
        leaf = n.rsplit("/", 1)[-1]
        val = v.initial_value(3).astype(np.float64)
        if leaf in ("gamma", "beta", "b"):
            val = val + 0.2 * rng.standard_normal(v.shape)
        elif leaf.endswith("_weight"):
            val = np.asarray(0.9)
        elif leaf == "renorm_mean":
            val = 0.9 * 1.5 * rng.standard_normal(v.shape)
        elif leaf == "renorm_stddev":
            val = 0.9 * rng.uniform(0.2, 3.0, v.shape)
        elif leaf == "moving_variance":
            val = rng.uniform(0.5, 2.0, v.shape)
        if leaf == "renorm_stddev":
            val[0] = 0.9 * 0.02                      # r far above rmax: cut to 3
        if leaf == "renorm_mean":
            val[1] = 0.9 * 20.0                      # d far below -dmax: cut to -5
        vals[n] = f32(val)
    store.load(vals)
    store.set_step(t)
    plan = engine.Plan(store, [loss, s], loss=loss, batch=B, training=True, compute_dtype="f32", optimize=False, use_hip_graph=False)
    routes = {op.name: sv.route for op, sv in plan.saved.items() if getattr(sv, "renorm", None) is not None}
    assert sorted(r.name for r in routes.values()) == ["GENERIC", "GENERIC"], routes
    x = f32(rng.standard_normal((B, H, H, 3)))
    lab = rng.integers(0, NC, (B, 4, 4)).astype(np.uint8)
    plan.set_input("x_input", x)
    plan.set_input("s_input", lab)
    plan.run(sync=True)
    got_loss = float(plan.fetch(loss))
    grads = store.export(grads=True)
    after = store.export()
    # ---- float64: torch convolutions, numpy renorm
    v64 = {n: np.asarray(v, dtype=np.float64) for n, v in vals.items()}
    tt = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))

    def state(scope):
        b = scope + "/batch_renorm/BatchNorm/"
        return {k: (float(v64[b + k]) if k.endswith("_weight") else v64[b + k]) for k in R.STATE}, v64[b + "gamma"], v64[b + "beta"], b
    W1, W2 = tt(v64["net/c1/W"]).requires_grad_(True), tt(v64["net/c2/W"]).requires_grad_(True)
    y1 = T.conv2d_general_same(tt(x), W1, (2, 2), (1, 1))
    st1, g1, b1, n1 = state("net/c1")
    f1 = R.forward(y1.detach().numpy().reshape(-1, 8), g1, b1, st1, t, "relu")
    a1_t = tt(f1["y"].reshape(B, 4, 4, 8)).requires_grad_(True)
    y2 = T.conv2d_same(a1_t, W2)
    st2, g2, b2, n2 = state("net/c2")
    f2 = R.forward(y2.detach().numpy().reshape(-1, 16), g2, b2, st2, t, "relu")
    a2_t = tt(f2["y"].reshape(B, 4, 4, 16)).requires_grad_(True)
    Wh, bh = tt(v64["net/head/W"]).requires_grad_(True), tt(v64["net/head/b"]).requires_grad_(True)
    so = T.bias_add(T.conv2d_same(a2_t, Wh), bh)
    ref_loss = T.multinoulli_loss_with_logits(T.one_hot(torch.as_tensor(lab), NC, torch.float64), so)
    ref_loss.backward()
    dy2, dg2, db2 = R.backward(y2.detach().numpy().reshape(-1, 16), g2, b2, st2, t, a2_t.grad.numpy().reshape(-1, 16), "relu")
    y2.backward(tt(dy2.reshape(B, 4, 4, 16)))
    dy1, dg1, db1 = R.backward(y1.detach().numpy().reshape(-1, 8), g1, b1, st1, t, a1_t.grad.numpy().reshape(-1, 8), "relu")
    y1.backward(tt(dy1.reshape(B, 4, 4, 8)))
    assert f1["r"][0] == 3.0 and f2["r"][0] == 3.0 and f1["d"][1] == -5.0 and f2["d"][1] == -5.0 and np.any(f2["r"] < 1.0)
    assert abs(got_loss - float(ref_loss)) <= FP32_TOL * abs(float(ref_loss))
    for name, want in ((n1 + "gamma", dg1), (n1 + "beta", db1), (n2 + "gamma", dg2), (n2 + "beta", db2), ("net/c1/W", W1.grad.numpy()),
                       ("net/c2/W", W2.grad.numpy()), ("net/head/W", Wh.grad.numpy()), ("net/head/b", bh.grad.numpy())):
        within(grads[name], want, FP32_TOL, "grad " + name)
    for (st, f, base) in ((st1, f1, n1), (st2, f2, n2)):
        want = R.update(st, f["mean"], f["rstd"])
        for k in R.STATE:
            within(np.atleast_1d(after[base + k]), np.atleast_1d(want[k]), FP32_TOL, "state " + base + k)


# ---- the tiny PHiSeg configuration ---------------------------------------------------------------------------------------------------------
def _cfg(dtype="f32", renorm=True):
    from phiseg_code_amd.tfwrapper import normalisation as tfnorm
    _, cfg, _ = load_golden("tiny_phiseg_bn")
    c = make_config(cfg, dtype)
    if renorm:
        c.layer_norm = tfnorm.batch_renorm
    c.batch_size = 2
    c.validation_frequency = None
    c.tensorboard_update_frequency = 2
    c.do_image_summaries = False
    c.annotator_range = range(4)
    c.lr_schedule_dict = {0: 1e-3}
    return c, cfg


def _model(dtype="f32", renorm=True):
    from phiseg_code_amd.phiseg import phiseg_model
    c, cfg = _cfg(dtype, renorm)
    return phiseg_model.phiseg(c, rng_seed=cfg["eps_seed"]), c, cfg


def _batch(cfg, step=0):
    from phiseg_code_amd.data import synthetic
    x, s = synthetic.philox_batch(2, cfg["H"], cfg["nlabels"], seed=77, step=step)
    return np.asarray(x, dtype=np.float32).reshape(2, cfg["H"], cfg["H"], 1), np.asarray(s, dtype=np.uint8).reshape(2, cfg["H"], cfg["H"])


def _bn_name(n):
    return n.replace("/batch_renorm/", "/batch_norm/")


def _warm_all(model, rng, w=0.9):
    vals = {}
    for n, v in model.graph.variables.items():
        leaf = n.rsplit("/", 1)[-1]
        if leaf.endswith("_weight") and "/renorm_" in n:
            vals[n] = f32(w)
        elif leaf == "renorm_mean":
            vals[n] = f32(w * 4.0 * rng.standard_normal(v.shape))
        elif leaf == "renorm_stddev":
            vals[n] = f32(w * rng.uniform(0.05, 2.0, v.shape))
    model.set_weights(vals)
    return vals


def _worker(*args):
    """tests/renorm_resume_worker.py under PHX_DETERMINISTIC=1 (read once per process) -> its stdout lines, split"""
    env = dict(os.environ, PYTHONPATH=ROOT, PHX_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "renorm_resume_worker.py")] + [str(a) for a in args], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return [l.split() for l in r.stdout.splitlines()]


def test_step_zero_equals_batch_norm_fp32():
    """Fresh state: r == 1 and d == 0, so at step 0 every loss term and every trainable gradient equals the batch-norm model's from the
    same initial values (fp32 parity bound 1e-4), and the moving mean moves with decay 0.999 where batch norm's moves with 0.99.
    Run in the deterministic mode: in the default mode the fp32 atomics of the statistics and gradient reductions make two runs of the
    BATCH-NORM model differ from each other by up to 7.9e-4 of a variable's largest gradient on this ill-conditioned network (measured;
    renorm against batch norm there: 1.9e-4 in the worst variable, 1.9e-5 in the median, loss terms 1.0e-5), which no comparison at
    1e-4 can see through."""
    line = [l for l in _worker("step0") if l and l[0] == "STEP0"][-1]
    e_loss, e_grad, e_mm, checked = float(line[1]), float(line[2]), float(line[3]), int(line[4])
    print("step 0, renorm against batch norm: loss terms %.2e, gradients %.2e of the variable's max (%d variables), moving mean %.2e"
          % (e_loss, e_grad, checked, e_mm))
    assert checked > 20
    assert e_loss <= FP32_TOL and e_grad <= FP32_TOL and e_mm <= FP32_TOL


def test_schedule_is_followed_under_graph_replay_fp32():
    """Step 2498 -> 2501 (dmax reaches 5 at 2500), warm state, four training steps on ONE plan: eager, capture, two replays.  After every
    step the layer's r and d are the ref's for that step's bounds and its six state vectors follow the ref recurrence fed the device's
    own saved mean / rstd."""
    from phiseg_code_amd.tfwrapper import normalisation as tfnorm
    model, c, cfg = _model()
    rng = np.random.default_rng(3)
    _warm_all(model, rng)
    store = model.sess._ensure_store()
    store.set_step(2498)
    post = [n.rsplit("/", 1)[0] + "/" for n in model.graph.variables if n.startswith("posterior/") and n.endswith("/renorm_mean") and "_pre_" in n]
    bases = [post[1], post[-1]]                     # a 128 x 128 layer and one of the coarsest level
    plans, execs, hit, routes = [], [], set(), set()
    for k in range(4):
        t = 2498 + k
        before = store.export()
        x, s = _batch(cfg, step=k)
        model.sess.run([model.train_step, model.loss_tot], {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: 1e-3})
        assert len(model.sess.plans) == 1
        plan = list(model.sess.plans.values())[0]
        plans.append(plan)
        execs.append(plan._graph_exec)
        after = store.export()
        rmax, dmax = R.clip_bounds(t)
        assert tfnorm.renorm_clip(t) == pytest.approx((rmax, dmax), rel=1e-6)
        for base in bases:
            st0 = {key: (float(before[base + key]) if key.endswith("_weight") else before[base + key].astype(np.float64)) for key in R.STATE}
            sv = [sv for op, sv in plan.saved.items() if getattr(sv, "renorm", None) is not None
                  and op.attrs["norm_vars"]["gamma"].name.startswith(base)][0]
            routes.add(sv.route.name)
            mean, rstd = sv.mean.numpy().astype(np.float64), sv.rstd.numpy().astype(np.float64)
            r, d = R.correction(mean, 1.0 / rstd, st0, t)
            got_r, got_d = sv.renorm.r.numpy().astype(np.float64), sv.renorm.d.numpy().astype(np.float64)
            within(got_r, r, FP32_TOL, "step %d %s r" % (t, base))
            within(got_d, d, FP32_TOL, "step %d %s d" % (t, base))
            hit |= ({"r"} if np.any(np.abs(got_r - rmax) < 1e-6 * rmax) else set()) | ({"d"} if np.any(np.abs(np.abs(got_d) - dmax) < 1e-6 * dmax) else set())
            want = R.update(st0, mean, rstd)
            for key in R.STATE:
                within(np.atleast_1d(after[base + key]), np.atleast_1d(want[key]), ULP8, "step %d %s state %s" % (t, base, key))
    print("routes of the checked layers:", sorted(routes))
    assert hit == {"r", "d"}, "the warm state must put channels on both clip bounds"
    assert all(p is plans[0] for p in plans) and execs[1] is not None and execs[2] is execs[1] and execs[3] is execs[1]
    assert int(store.step.cpu().item()) == 2502


def test_inference_equals_batch_norm_bit_for_bit():
    rn, _, cfg = _model()
    bn, _, _ = _model(renorm=False)
    rng = np.random.default_rng(4)
    _warm_all(rn, rng)
    vals = {}
    for n, v in rn.graph.variables.items():
        if "/renorm_" in n:
            continue
        leaf = n.rsplit("/", 1)[-1]
        val = v.initial_value(0)
        if leaf in ("gamma", "beta", "moving_mean"):
            val = val + f32(0.2 * rng.standard_normal(v.shape))
        elif leaf == "moving_variance":
            val = f32(rng.uniform(0.5, 2.0, v.shape))
        vals[n] = val
    rn.set_weights(vals)
    bn.set_weights({_bn_name(n): v for n, v in vals.items()})
    x, _ = _batch(cfg)
    outs = []
    for m in (rn, bn):
        outs.append(m.sess.run([m.s_out_eval, m.s_out_eval_sm] + list(m.prior_mu_list_gen), {m.x_inp: x, m.training_pl: False}))
        plan = list(m.sess.plans.values())[0]
        assert not any(fn is plan.L.renorm_tail_multi or fn is plan.L.renorm_apply_fused or fn is plan.L.renorm_small_fwd for fn, _ in plan.launches)
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


def test_checkpoints_carry_the_eight_variables(tmp_path, caplog):
    from phiseg_code_amd.phiseg import phiseg_model
    from phiseg_code_amd.tfwrapper import tf_checkpoint
    model, c, cfg = _model()
    x, s = _batch(cfg)
    model.sess.run([model.train_step], {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: 1e-3})
    cur = model.sess.store.export()
    layer = [n for n in cur if n.endswith("/renorm_mean")][0].rsplit("/", 1)[0]
    eight = [layer + "/" + k for k in ("beta", "gamma", "moving_mean", "moving_variance", "renorm_mean", "renorm_mean_weight", "renorm_stddev",
                                       "renorm_stddev_weight")]
    assert cur[layer + "/renorm_mean_weight"].shape == () and abs(float(cur[layer + "/renorm_mean_weight"]) - 0.01) < 1e-6
    model.save_weights(str(tmp_path / "rn.ckpt-1"))
    model.save_weights(str(tmp_path / "rn_tf.ckpt-1"), format="tf")
    npz = np.load(str(tmp_path / "rn.ckpt-1.npz"))
    bundle = tf_checkpoint.read(str(tmp_path / "rn_tf.ckpt-1"))
    for n in model.graph.variables:
        for blob in (npz, bundle):
            assert np.asarray(blob[n]).shape == cur[n].shape and np.array_equal(np.asarray(blob[n]), cur[n]), n
    assert all(n in npz.files and n in bundle for n in eight)
    for path in (str(tmp_path / "rn.ckpt-1"), str(tmp_path / "rn_tf.ckpt-1")):
        m2 = phiseg_model.phiseg(c)
        m2.load_weights(path)
        back = m2.sess.store.export()
        assert all(np.array_equal(back[n], cur[n]) for n in cur) and m2.last_load_missing == []
    # a file without the four new variables: they stay zero, one warning
    np.savez(str(tmp_path / "old.ckpt-1.npz"), **{k: npz[k] for k in npz.files if "/renorm_" not in k})
    m3 = phiseg_model.phiseg(c)
    with caplog.at_level(logging.WARNING):
        m3.load_weights(str(tmp_path / "old.ckpt-1"))
    back = m3.sess.store.export()
    assert all(not back[n].any() for n in back if "/renorm_" in n) and np.array_equal(back[layer + "/gamma"], cur[layer + "/gamma"])
    assert sorted(m3.last_load_missing) == sorted(n for n in cur if "/renorm_" in n) and "keep their values" in caplog.text
    # a batch-norm model's checkpoint into the renorm model (weights only), and the renorm file into a batch-norm model (ignored)
    bn, _, _ = _model(renorm=False)
    bn.sess.run([bn.train_step], {bn.x_inp: x, bn.s_inp: s, bn.training_pl: True, bn.lr_pl: 1e-3})
    bn.save_weights(str(tmp_path / "bn.ckpt-1"))
    bn_vals = bn.sess.store.export()
    m4 = phiseg_model.phiseg(c)
    m4.load_weights(str(tmp_path / "bn.ckpt-1"))
    back = m4.sess.store.export()
    wname = [n for n in back if n.endswith("/W")][0]
    assert np.array_equal(back[wname], bn_vals[wname]) and all(not back[n].any() for n in back if "/renorm_" in n)
    bn.load_weights(str(tmp_path / "rn.ckpt-1"))
    assert np.array_equal(bn.sess.store.export()[wname], cur[wname])


def test_resume_is_bit_identical_in_deterministic_mode(tmp_path):
    """PHX_DETERMINISTIC=1: 2 steps + save + load into a fresh model + 1 step == 3 uninterrupted steps."""
    lines = [l for l in _worker("resume", tmp_path) if l and l[0] == "DIGEST"]
    assert len(lines) == 2 and lines[0][1] == lines[1][1], lines


def test_summaries_carry_the_clip_bounds(tmp_path):
    """train(summaries=True) continued from a checkpoint at step 2498: rmax_clip / dmax_clip at every summary step, equal to
    renorm_clip(step); a batch-norm model's event file has neither tag (tests/test_summary_gpu.py pins its tag set)."""
    from phiseg_code_amd import summary as S
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.tfwrapper import normalisation as tfnorm
    model, c, cfg = _model()
    log_dir = str(tmp_path / "run")
    os.makedirs(log_dir)
    model.sess._ensure_store().set_step(2498)
    model.save_weights(os.path.join(log_dir, "model.ckpt-2498"))
    model.train(synthetic.SyntheticLIDC(c, seed=5, n_validation=3), num_iter=2501, log_every=0, log_dir=log_dir, summaries=True)
    files = [f for f in os.listdir(log_dir + "_cont") if f.startswith("events.out.tfevents.")]
    assert len(files) == 1
    seen = {}
    for e in S.read_events(os.path.join(log_dir + "_cont", files[0])):
        sc = {v["tag"]: v["simple_value"] for v in e.get("values", []) if "simple_value" in v}
        if "batch_total_loss" in sc:
            seen[e["step"]] = (sc["rmax_clip"], sc["dmax_clip"])
    assert sorted(seen) == [2498, 2500]
    for step, got in seen.items():
        want = tfnorm.renorm_clip(step)
        assert got == (float(np.float32(want[0])), float(np.float32(want[1]))), (step, got, want)
    assert seen[2500][1] == 5.0 and seen[2498][1] < 5.0


def test_two_bf16_training_steps_stay_in_the_bf16_band():
    """Two training steps of the tiny configuration in bf16 against the fp32 renorm run (whose correctness the tests above establish) from
    the same state, batches and noise.  Band: the one tests/test_model_gpu.py grants bf16 for batch norm at batch 2, where the coarsest
    level normalises 8 values per channel -- test_loss_curve_n0_32, line 552 (cross-entropy within 6 %) and line 558 (a KL term within
    a factor 3; its single-step spike allowance is not used here).  Every loss is finite."""
    runs = {}
    for dt in ("f32", "bf16"):
        model, c, cfg = _model(dt)
        keys = sorted(model.loss_dict)
        out = []
        for k in range(2):
            x, s = _batch(cfg, step=k)
            v = model.sess.run([model.train_step] + [model.loss_dict[key] for key in keys],
                               {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: 1e-3})
            out.append({key: float(val) for key, val in zip(keys, v[1:])})
        runs[dt] = out
    for k in range(2):
        for key in runs["f32"][k]:
            a, b = runs["bf16"][k][key], runs["f32"][k][key]
            print("step %d %-36s bf16 %.5e fp32 %.5e ratio %.4f" % (k, key, a, b, a / b))
            assert np.isfinite(a) and np.isfinite(b), key
            if key.startswith("KL_"):
                assert 1 / 3.0 <= a / b <= 3.0, (k, key, a, b)
            elif key.startswith("residual_"):
                assert abs(a / b - 1) <= 0.06, (k, key, a, b)
