"""tf.train.MomentumOptimizer on the MI355X: the phx_momentum_tf1 kernel against the TF 1.12 ApplyMomentum formula in float64, the
update identity through the model (eager, hipGraph capture, replay; fp32 and bf16), the split-optimiser plan of the data-parallel
step, and the '<var>/Momentum' checkpoints (npz and TensorFlow bundles, resume, cross-loading with Adam checkpoints).

    accum = momentum * accum + g
    p    -= use_nesterov ? lr * g + lr * momentum * accum (the new accum) : lr * accum

Bound of every comparison with the float64 formula: 8 * 2^-23 of the largest operand.  One launch is at most 5 fp32 roundings of
at most 2^-24 relative each (accum: 2, the step: 3), so three launches stay below 7.5 * 2^-23 and one launch below 2.5 * 2^-23."""
import ctypes
import logging

import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.test_graph_cpu import make_config

pytestmark = pytest.mark.gpu

ULP8 = 8 * 2.0 ** -23
LRS = (0.1, 0.01, 0.05)
SENT = (7.25, -3.5, 11.125)          # sentinel values behind p, g, accum


@pytest.fixture(scope="module")
def L():
    from phiseg_code_amd import runtime as rt
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return rt.lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def _f32(x):
    return float(np.float32(x))


# ---- A. the kernel -----------------------------------------------------------------------------------------------------------
# 8 389 635 = 4 * (8192 * 256 + 256) + 3: the smallest size class that enters the grid-stride loop under the 8192 x 256 cap, with a tail
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 65536, 8389635])
@pytest.mark.parametrize("use_nesterov", [0, 1])
@pytest.mark.parametrize("momentum", [0.9, 0.5, 0.0])
def test_kernel_matches_float64_formula(L, n, use_nesterov, momentum):
    gen = torch.Generator(device="cuda").manual_seed(1000 * use_nesterov + n % 997)
    buf = [torch.empty(n + 8, device="cuda") for _ in range(3)]
    for b, s in zip(buf, SENT):
        b[n:] = s
    p, g, a = (b[:n] for b in buf)
    p.copy_(torch.randn(n, device="cuda", generator=gen))
    a.zero_()
    lr = torch.zeros(1, device="cuda")
    pr, ar = p.double(), a.double()
    mom = _f32(momentum)
    for t in range(3):
        g.copy_(torch.randn(n, device="cuda", generator=gen) * 10.0 ** (t - 1))
        g0 = g.clone()
        lr.fill_(LRS[t])                 # only the DEVICE value changes between the launches
        L.momentum_tf1(p.data_ptr(), g.data_ptr(), a.data_ptr(), n, lr.data_ptr(), momentum, use_nesterov, S())
        torch.cuda.synchronize()
        l, gd = _f32(LRS[t]), g0.double()
        ar = mom * ar + gd
        pr = pr - (l * gd + l * mom * ar if use_nesterov else l * ar)
        assert torch.equal(g, g0), "g was written"
        if t == 0 and momentum == 0.0:
            assert torch.equal(a.view(torch.int32), g0.view(torch.int32)), "momentum 0: accum must be g, bit for bit"
    ep, ea = float((p.double() - pr).abs().max()), float((a.double() - ar).abs().max())
    bp, ba = ULP8 * float(pr.abs().max()), ULP8 * float(ar.abs().max())
    print("n=%d nesterov=%d momentum=%g: p err %.3e (bound %.3e), accum err %.3e (bound %.3e)" % (n, use_nesterov, momentum, ep, bp, ea, ba))
    assert ep <= bp and ea <= ba
    for b, s in zip(buf, SENT):
        assert torch.equal(b[n:], torch.full((8,), s, device="cuda")), "wrote past element n - 1"


@pytest.mark.parametrize("use_nesterov,want", [(1, [(0.5, 0.905), (0.95, 0.7695), (1.355, 0.59755)]),
                                               (0, [(0.5, 0.95), (0.95, 0.855), (1.355, 0.7195)])])
def test_kernel_hand_checked_scalar_run(L, use_nesterov, want):
    p, g, a = torch.ones(4, device="cuda"), torch.full((4,), 0.5, device="cuda"), torch.zeros(4, device="cuda")
    lr = torch.tensor([0.1], device="cuda")
    for acc_w, p_w in want:
        L.momentum_tf1(p.data_ptr(), g.data_ptr(), a.data_ptr(), 1, lr.data_ptr(), 0.9, use_nesterov, S())
        torch.cuda.synchronize()
        assert abs(float(a[0]) - acc_w) <= 1e-6 and abs(float(p[0]) - p_w) <= 1e-6, (float(a[0]), float(p[0]), acc_w, p_w)
    assert float(p[1]) == 1.0 and float(a[1]) == 0.0            # n = 1: the neighbours stay


def test_kernel_rejects_misaligned_and_null_pointers(L):
    from phiseg_code_amd.runtime import PhxError
    p, g, a = (torch.ones(16, device="cuda") for _ in range(3))
    lr = torch.tensor([0.1], device="cuda")
    ptrs = [p.data_ptr(), g.data_ptr(), a.data_ptr()]
    for k in range(3):
        for bad in (ptrs[k] + 4, None):
            args = list(ptrs)
            args[k] = bad
            with pytest.raises(PhxError):
                L.momentum_tf1(args[0], args[1], args[2], 8, lr.data_ptr(), 0.9, 1, S())
    torch.cuda.synchronize()
    for t in (p, g, a):                                          # the argument check rejects the call: nothing was launched
        assert torch.equal(t, torch.ones(16, device="cuda"))


def test_kernel_capture_and_replay_equal_eager(L):
    n = 1027
    gen = torch.Generator(device="cuda").manual_seed(5)
    p, g = torch.randn(n, device="cuda", generator=gen), torch.randn(n, device="cuda", generator=gen)
    a = torch.zeros(n, device="cuda")
    pe, ae = p.clone(), a.clone()
    lr = torch.tensor([0.01], device="cuda")
    for _ in range(2):
        L.momentum_tf1(pe.data_ptr(), g.data_ptr(), ae.data_ptr(), n, lr.data_ptr(), 0.9, 1, S())
    st = ctypes.c_void_p()
    L.stream_create(ctypes.byref(st))
    torch.cuda.synchronize()
    L.graph_begin_capture(st)
    L.momentum_tf1(p.data_ptr(), g.data_ptr(), a.data_ptr(), n, lr.data_ptr(), 0.9, 1, st)
    ge = ctypes.c_void_p()
    L.graph_end_capture(st, ctypes.byref(ge))
    for _ in range(2):
        L.graph_launch(ge, st)
    L.stream_sync(st)
    torch.cuda.synchronize()
    assert torch.equal(p, pe) and torch.equal(a, ae)
    L.graph_destroy(ge)
    L.stream_destroy(st)


# ---- B. the update identity through the model --------------------------------------------------------------------------------
def _check_step(names, p0, acc0, g, p1, acc1, lr, momentum=0.9, nesterov=True):
    """One applied step, per trainable variable, in float64 with fp32-rounded lr / momentum -> the variables that moved by more than
    100x their bound."""
    l, mom = _f32(lr), _f32(momentum)
    moved = set()
    for k in names:
        P0, A0, Gk = p0[k].astype(np.float64), acc0[k]["Momentum"].astype(np.float64), g[k].astype(np.float64)
        P1, A1 = p1[k].astype(np.float64), acc1[k]["Momentum"].astype(np.float64)
        aref = mom * A0 + Gk
        assert np.abs(A1 - aref).max() <= ULP8 * np.abs(aref).max(), (k, "accum", np.abs(A1 - aref).max(), np.abs(aref).max())
        pref = P0 - (l * (Gk + mom * A1) if nesterov else l * A1)
        bound = ULP8 * max(np.abs(P0).max(), l * (np.abs(Gk).max() + np.abs(A1).max()))
        assert np.abs(P1 - pref).max() <= bound, (k, "p", np.abs(P1 - pref).max(), bound)
        if not Gk.any() and not A0.any():                        # a never-consumed branch: nothing moves, bit for bit
            assert np.array_equal(p1[k].view(np.int32), p0[k].view(np.int32)), k
            assert np.array_equal(acc1[k]["Momentum"].view(np.int32), acc0[k]["Momentum"].view(np.int32)), k
        if np.abs(P1 - P0).max() > 100 * bound:
            moved.add(k)
    return moved


def _momentum_model(case, compute_dtype, **kw):
    from oracle import init as oinit
    from phiseg_code_amd import optimizers
    from phiseg_code_amd.phiseg import phiseg_model
    g, cfg, var_order = load_golden(case)
    c = make_config(cfg, compute_dtype)
    c.optimizer = optimizers.MomentumOptimizer
    model = phiseg_model.phiseg(c, rng_seed=cfg["eps_seed"], **kw)
    x_np, s_np = oinit.synthetic_batch(cfg["B"], cfg["H"], cfg["nlabels"], cfg["data_seed"])
    return model, cfg, x_np, s_np


def _live_trainable(model):
    from phiseg_code_amd import engine
    live = engine.live_variables(model.loss_tot)
    return [n for n, v in model.graph.variables.items() if v.trainable and n in live]


@pytest.mark.parametrize("case,compute_dtype", [("tiny_phiseg_bn", "f32"), ("lidc_phiseg_bn", "bf16")])
def test_model_steps_apply_nesterov_momentum(case, compute_dtype):
    model, cfg, x_np, s_np = _momentum_model(case, compute_dtype)
    store = model.sess._ensure_store()
    assert store.adam_m is None and store.adam_v is None and store.slot_arenas() == [store.accum]
    names = [n for n, v in model.graph.variables.items() if v.trainable]
    live = _live_trainable(model)
    for lr in (1e-2, 5e-3, 5e-3):                                # eager, capture, replay; the lr change must reach the device
        p0, acc0 = store.export(), store.export_slots()
        _, loss = model.sess.run([model.train_step, model.loss_tot],
                                 {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: True, model.lr_pl: lr})
        p1, acc1, g = store.export(), store.export_slots(), store.export(grads=True)
        assert np.isfinite(float(loss)), loss
        moved = len(_check_step(names, p0, acc0, g, p1, acc1, lr) & set(live))
        print("%s %s lr %g: loss %.4f, %d of %d live variables moved by more than 100x the bound" % (case, compute_dtype, lr, float(loss), moved, len(live)))
        assert 2 * moved >= len(live), (moved, len(live))
    assert int(store.step.cpu().item()) == 3


# ---- C. the split optimiser of the data-parallel step ----------------------------------------------------------------------
def test_split_optimizer_plan_replays_momentum():
    from phiseg_code_amd import engine
    model, cfg, x_np, s_np = _momentum_model("tiny_phiseg_bn", "f32")
    store = model.sess._ensure_store()
    plan = engine.Plan(store, [model.loss_tot], loss=model.loss_tot, batch=cfg["B"], training=True, compute_dtype="f32",
                       rng_seed=cfg["eps_seed"], split_optimizer=True, optimizer=model.optimizer)
    assert any(fn is plan.L.momentum_tf1 for fn, _ in plan.opt_launches) and not any(fn is plan.L.adam_tf1 for fn, _ in plan.opt_launches)
    assert not any(fn is plan.L.momentum_tf1 for fn, _ in plan.launches)
    plan.set_input("x_input", x_np)
    plan.set_input("s_input", s_np)
    lr = 5e-3
    store.set_lr(lr)
    names = [n for n, v in model.graph.variables.items() if v.trainable]
    live = _live_trainable(model)
    for _ in range(3):                                           # eager, capture, replay -- of both launch lists
        p0, acc0 = store.export(), store.export_slots()
        plan.run_main()
        plan.run_opt()
        plan.sync()
        p1, acc1, g = store.export(), store.export_slots(), store.export(grads=True)
        assert 2 * len(_check_step(names, p0, acc0, g, p1, acc1, lr) & set(live)) >= len(live)
    assert plan._graph_exec_opt is not None and int(store.step.cpu().item()) == 3


def test_plan_rejects_an_optimizer_whose_slots_the_store_lacks():
    from phiseg_code_amd import engine
    from phiseg_code_amd import optimizers
    model, cfg, _, _ = _momentum_model("tiny_phiseg_bn", "f32")
    store = model.sess._ensure_store()
    with pytest.raises(ValueError):                              # (no optimizer argument = Adam)
        engine.Plan(store, [model.loss_tot], loss=model.loss_tot, batch=cfg["B"], training=True)
    adam_store = engine.ParamStore(model.graph, live=engine.live_variables(model.loss_tot))
    assert adam_store.accum is None and adam_store.slot_names == ("Adam", "Adam_1")
    with pytest.raises(ValueError):
        engine.Plan(adam_store, [model.loss_tot], loss=model.loss_tot, batch=cfg["B"], training=True,
                    optimizer=optimizers.MomentumOptimizer(None, 0.9))


# ---- D. checkpoints ---------------------------------------------------------------------------------------------------------
def _ckpt_cfg(momentum=True):
    from phiseg_code_amd import optimizers
    from tests.test_checkpoint_gpu import _cfg
    c = _cfg()
    if momentum:
        c.optimizer = optimizers.MomentumOptimizer
    return c


def _steps(model, batches, lr=1e-3):
    for x, s in batches:
        model.sess.run([model.train_step, model.loss_tot], {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: lr})


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """A Momentum model after 2 steps, written as npz and as a TensorFlow bundle, and an Adam model after 1 step (npz)."""
    from phiseg_code_amd.phiseg import phiseg_model
    from tests.test_checkpoint_gpu import _data
    d = tmp_path_factory.mktemp("momentum_ckpt")
    cfg = _ckpt_cfg()
    data = _data(cfg)
    batches = [data.train.next_batch(cfg.batch_size) for _ in range(3)]
    m = phiseg_model.phiseg(cfg)
    _steps(m, batches[:2])
    m.save_weights(str(d / "mom.ckpt-1"))
    m.save_weights(str(d / "tf" / "mom.ckpt-1"), format="tf")
    adam = phiseg_model.phiseg(_ckpt_cfg(momentum=False))
    _steps(adam, batches[:1])
    adam.save_weights(str(d / "adam.ckpt-0"))
    store = m.sess.store
    return dict(dir=d, cfg=cfg, batches=batches, params=store.export(), slots=store.export_slots(), names=list(m.graph.variables),
                trainable=[n for n, v in m.graph.variables.items() if v.trainable], adam_params=adam.sess.store.export())


def _assert_restored(model, saved):
    store = model.sess.store
    got, gslots = store.export(), store.export_slots()
    for n in saved["names"]:
        assert np.array_equal(got[n].view(np.int32), saved["params"][n].view(np.int32)), n
    assert set(gslots) == set(saved["trainable"])
    for n in saved["trainable"]:
        assert list(gslots[n]) == ["Momentum"]
        assert np.array_equal(gslots[n]["Momentum"].view(np.int32), saved["slots"][n]["Momentum"].view(np.int32)), n
    assert int(store.step.cpu().item()) == 2


def test_npz_checkpoint_holds_momentum_slots_and_resumes(saved):
    from phiseg_code_amd.phiseg import phiseg_model
    ck = np.load(str(saved["dir"] / "mom.ckpt-1.npz"))
    for n in saved["trainable"]:
        assert n + "/Momentum" in ck.files, n
    assert not any(k.endswith(("/Adam", "/Adam_1")) for k in ck.files)
    assert int(ck["__step__"][0]) == 2
    assert max(np.abs(ck[n + "/Momentum"]).max() for n in saved["trainable"]) > 0
    c = phiseg_model.phiseg(saved["cfg"], init_seed=99)           # different initial weights: everything must come from the file
    c.load_weights(str(saved["dir"] / "mom.ckpt-1"))
    _assert_restored(c, saved)
    # one further step uses the LOADED accumulator (a reset one would miss by 0.81 * lr * |acc0|)
    store = c.sess.store
    p0, acc0 = store.export(), store.export_slots()
    _steps(c, saved["batches"][2:3])
    p1, acc1, g = store.export(), store.export_slots(), store.export(grads=True)
    moved = _check_step(saved["trainable"], p0, acc0, g, p1, acc1, 1e-3)
    assert len(moved) > 0 and int(store.step.cpu().item()) == 3


def test_tf_bundle_round_trip_has_no_adam_variables(saved):
    from phiseg_code_amd.phiseg import phiseg_model
    from phiseg_code_amd.tfwrapper import tf_checkpoint as tfc
    prefix = str(saved["dir"] / "tf" / "mom.ckpt-1")
    ck = tfc.read(prefix)
    for n in saved["trainable"]:
        assert n + "/Momentum" in ck, n
    assert int(ck["global_step"]) == 2
    assert "beta1_power" not in ck and "beta2_power" not in ck
    assert not any(k.endswith(("/Adam", "/Adam_1")) for k in ck)
    c = phiseg_model.phiseg(saved["cfg"], init_seed=99)
    c.load_weights(prefix)
    _assert_restored(c, saved)


def test_cross_loading_is_weights_only(saved, caplog):
    from phiseg_code_amd.phiseg import phiseg_model
    # an Adam-written checkpoint into a Momentum model whose state is non-zero
    m = phiseg_model.phiseg(saved["cfg"], init_seed=99)
    _steps(m, saved["batches"][:1])
    assert float(m.sess.store.accum.abs().max().cpu()) > 0 and int(m.sess.store.step.cpu().item()) == 1
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        m.load_weights(str(saved["dir"] / "adam.ckpt-0"))
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "Adam" in warned[0] and "Momentum" in warned[0], warned
    got = m.sess.store.export()
    for n in saved["names"]:
        assert np.array_equal(got[n], saved["adam_params"][n]), n
    assert float(m.sess.store.accum.abs().max().cpu()) == 0.0 and int(m.sess.store.step.cpu().item()) == 0
    # a Momentum-written checkpoint into an Adam model whose state is non-zero
    a = phiseg_model.phiseg(_ckpt_cfg(momentum=False), init_seed=99)
    _steps(a, saved["batches"][:1])
    assert float(a.sess.store.adam_v.abs().max().cpu()) > 0
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        a.load_weights(str(saved["dir"] / "mom.ckpt-1"))
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "Momentum" in warned[0], warned
    got = a.sess.store.export()
    for n in saved["names"]:
        assert np.array_equal(got[n], saved["params"][n]), n
    st = a.sess.store
    assert float(st.adam_m.abs().max().cpu()) == 0.0 and float(st.adam_v.abs().max().cpu()) == 0.0 and int(st.step.cpu().item()) == 0
