"""tfwrapper.losses without a GPU: the numpy restatement (tests/seg_losses_ref.py) against torch float64 autograd of the reference's
formulas, and the host-side surface -- import, signatures, graph ops, label handling, add_loss_term, the declared C symbols."""
import inspect

import numpy as np
import pytest
import torch

from tests import seg_losses_ref as R
from tests.helpers import load_golden
from tests.test_graph_cpu import make_config

from phiseg_code_amd import graph as G

RTOL = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    scale = max(float(np.abs(b).max()), 1e-300)
    assert float(np.abs(a - b).max()) <= RTOL * scale, (what, float(np.abs(a - b).max()) / scale)


# ---- the reference's formulas (tfwrapper/losses.py) written with torch ops, float64 ---------------------------------------------
def t_get_dice(logits, y, epsilon, sum_over_labels, sum_over_batches, use_hard_pred):
    prediction = torch.softmax(logits, dim=-1)
    if use_hard_pred:
        prediction = torch.nn.functional.one_hot(torch.argmax(logits, dim=-1), logits.shape[-1]).to(logits.dtype)
    axes = [1, 2]
    if sum_over_batches:
        axes = [0] + axes
    if sum_over_labels:
        axes += [axes[-1] + 1]
    i, l, r = (prediction * y).sum(dim=axes), prediction.sum(dim=axes), y.sum(dim=axes)
    return 2 * i / (l + r + epsilon)


def t_dice_loss(logits, y, epsilon, sum_over_labels, sum_over_batches, only_foreground):
    d = t_get_dice(logits, y, epsilon, sum_over_labels, sum_over_batches, False)
    if only_foreground:
        return 1 - (d[1:] if sum_over_batches else d[:, 1:]).mean()
    return 1 - d.mean()


def t_xent(logits, y, use_sigmoid=False, class_weights=None):
    if use_sigmoid:
        return torch.nn.functional.binary_cross_entropy_with_logits(logits, y, reduction="mean")
    C = logits.shape[-1]
    fl, fy = logits.reshape(-1, C), y.reshape(-1, C)
    loss_map = -(fy * torch.log_softmax(fl, dim=-1)).sum(dim=1)
    if class_weights is not None:
        loss_map = loss_map * (fy * torch.tensor(np.asarray(class_weights, dtype=np.float32).astype(np.float64))).sum(dim=1)
    return loss_map.mean()


CASES = [((2, 5, 7, 3), "normal"), ((3, 8, 8, 4), "normal"), ((2, 33, 31, 5), "normal"), ((2, 5, 7, 2), "extreme"), ((3, 8, 8, 4), "ties")]


def _torch_inputs(shape, kind):
    lg, lab = R.make_case(shape, seed=3, kind=kind)
    t = torch.tensor(lg.astype(np.float64), requires_grad=True)
    y = torch.tensor(R.one_hot(lab, shape[3], np.float64))
    return lg, lab, t, y


@pytest.mark.parametrize("shape,kind", CASES)
def test_restatement_dice_equals_torch_autograd(shape, kind):
    lg, lab, t, y = _torch_inputs(shape, kind)
    for sol, sob, fg in R.DICE_FLAG_SETS:
        for eps in (1e-10, 1e-3):
            loss, grad = R.dice_loss(lg, lab, eps, sol, sob, fg)
            tl = t_dice_loss(t, y, eps, sol, sob, fg)
            (tg,) = torch.autograd.grad(tl, t)
            _close(loss, tl.detach().numpy(), ("dice_loss", sol, sob, fg))
            _close(grad, tg.numpy(), ("dice_loss gradient", sol, sob, fg))
    for hard in (True, False):
        for sol in (False, True):
            for sob in (False, True):
                got = R.get_dice(lg, lab, 1e-10, sol, sob, hard)
                _close(got, t_get_dice(t, y, 1e-10, sol, sob, hard).detach().numpy(), ("get_dice", hard, sol, sob))
    with pytest.raises(ValueError):
        R.dice_loss(lg, lab, 1e-10, True, False, True)
    with pytest.raises(IndexError):              # what the reference's slice does to a tensor without a label axis
        t_dice_loss(t, y, 1e-10, True, False, True)


@pytest.mark.parametrize("shape,kind", CASES)
def test_restatement_cross_entropy_equals_torch_autograd(shape, kind):
    lg, lab, t, y = _torch_inputs(shape, kind)
    cw = [0.3 + 0.7 * c for c in range(shape[3])]
    for kw in (dict(), dict(use_sigmoid=True), dict(class_weights=cw)):
        loss, grad = R.cross_entropy_loss(lg, lab, **kw)
        tl = t_xent(t, y, **kw)
        (tg,) = torch.autograd.grad(tl, t)
        _close(loss, tl.detach().numpy(), ("xent", kw))
        _close(grad, tg.numpy(), ("xent gradient", kw))


def test_restatement_float32_is_close_and_band_has_a_floor():
    lg, lab = R.make_case((2, 33, 31, 5), seed=1)
    l64, g64 = R.dice_loss(lg, lab)
    l32, g32 = R.dice_loss(lg, lab, dtype=np.float32)
    assert l32.dtype == np.float32 and g32.dtype == np.float32
    assert abs(float(l32) - float(l64)) < 1e-5 and np.abs(g32 - g64).max() < 1e-6 * np.abs(g64).max() + 1e-12
    ok, err, allowed = R.band(np.float32(1.0), 1.0, 1.0)
    assert ok and err == 0.0 and allowed == 4 * float(np.spacing(np.float32(1.0)))
    assert not R.band(1.0 + 1e-5, 1.0, 1.0)[0]
    fine = np.arange(2 * 8 * 8 * 3, dtype=np.float64).reshape(2, 8, 8, 3)
    assert R.nn_resize_adjoint(fine, 3).shape == (2, 1, 1, 3) and R.nn_resize_adjoint(fine, 3)[1, 0, 0, 2] == fine[1, :, :, 2].sum()


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def test_losses_import_and_signatures():
    from phiseg_code_amd.tfwrapper import losses

    def sig(fn):
        return [(p.name, p.default if p.default is not inspect.Parameter.empty else "<none>", p.kind == p.VAR_KEYWORD)
                for p in inspect.signature(fn).parameters.values()]
    assert sig(losses.get_dice) == [("logits", "<none>", False), ("labels", "<none>", False), ("epsilon", 1e-10, False),
                                    ("sum_over_labels", False, False), ("sum_over_batches", False, False), ("use_hard_pred", True, False)]
    assert sig(losses.dice_loss) == [("logits", "<none>", False), ("labels", "<none>", False), ("epsilon", 1e-10, False),
                                     ("kwargs", "<none>", True)]
    assert sig(losses.cross_entropy_loss) == [("logits", "<none>", False), ("labels", "<none>", False), ("use_sigmoid", False, False)]
    assert sig(losses.pixel_wise_cross_entropy_loss_weighted) == [("logits", "<none>", False), ("labels", "<none>", False),
                                                                  ("class_weights", "<none>", False)]


def _toy():
    G.reset_default_graph()
    lg = G.placeholder(G.KIND_F32, [None, 8, 8, 3], name="lg")
    s = G.placeholder(G.KIND_U8, [None, 8, 8], name="s_input")
    return lg, s


def test_graph_ops_shapes_modes_and_label_forms():
    from phiseg_code_amd.tfwrapper import losses
    lg, s = _toy()
    oh = G.one_hot(s, 3)
    assert losses.get_dice(lg, oh).shape == (None, 3)
    assert losses.get_dice(lg, s, sum_over_batches=True).shape == (3,)
    assert losses.get_dice(lg, oh, sum_over_labels=True).shape == (None,)
    assert losses.get_dice(lg, oh, sum_over_labels=True, sum_over_batches=True).shape == ()
    d = losses.get_dice(lg, oh, use_hard_pred=False)
    assert d.op.type == "dice_table" and d.op.inputs[1] is s and d.op.attrs["use_hard_pred"] is False
    want = {"macro": (False, False), "macro_robust": (False, True), "micro": (True, False)}
    for mode, (sol, sob) in want.items():
        t = losses.dice_loss(lg, oh, mode=mode)
        assert t.shape == () and t.op.type == "dice_loss" and t.op.inputs[1] is s
        assert (t.op.attrs["sum_over_labels"], t.op.attrs["sum_over_batches"]) == (sol, sob)
    # mode=None: per_structure has no default and feeds sum_over_labels directly (None counts as False)
    assert losses.dice_loss(lg, oh).op.attrs["sum_over_labels"] is False
    assert losses.dice_loss(lg, oh, per_structure=True, sum_over_batches=True).op.attrs == dict(
        epsilon=1e-10, sum_over_labels=True, sum_over_batches=True, only_foreground=False)
    assert losses.dice_loss(lg, oh, mode="macro", only_foreground=True, epsilon=1e-5).op.attrs["only_foreground"] is True
    with pytest.raises(ValueError, match="Encountered unexpected 'mode' in dice_loss: 'nano'"):
        losses.dice_loss(lg, oh, mode="nano")
    with pytest.raises(ValueError):
        losses.dice_loss(lg, oh, mode="micro", only_foreground=True)
    x = losses.cross_entropy_loss(lg, oh)
    assert x.shape == () and x.op.type == "seg_xent" and x.op.attrs == dict(class_weights=None, use_sigmoid=False)
    assert losses.cross_entropy_loss(lg, s, use_sigmoid=True).op.attrs["use_sigmoid"] is True
    assert losses.pixel_wise_cross_entropy_loss_weighted(lg, oh, [1, 2, 3]).op.attrs["class_weights"] == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        losses.pixel_wise_cross_entropy_loss_weighted(lg, oh, [1, 2])
    with pytest.raises(ValueError):
        losses.cross_entropy_loss(lg, G.one_hot(s, 4))
    # a nearest-resized level is summed to full resolution first, so that its gradient has a path (the resize adjoint)
    coarse = G.placeholder(G.KIND_F32, [None, 4, 4, 3], name="coarse")
    t = losses.dice_loss(G.resize_nearest(coarse, (8, 8)), s, mode="macro")
    assert t.op.inputs[0].op.type == "aggregate" and t.op.inputs[0].shape == (None, 8, 8, 3)


def test_float_one_hot_5d_logits_and_bad_logits_raise():
    from phiseg_code_amd.tfwrapper import losses
    lg, s = _toy()
    soft = G.placeholder(G.KIND_F32, [None, 8, 8, 3], name="soft_labels")
    for fn in (losses.get_dice, losses.dice_loss, losses.cross_entropy_loss):
        with pytest.raises(NotImplementedError, match="one-hot"):
            fn(lg, soft)
    with pytest.raises(NotImplementedError, match="one-hot"):
        losses.pixel_wise_cross_entropy_loss_weighted(lg, soft, [1, 1, 1])
    lg5 = G.placeholder(G.KIND_F32, [None, 4, 8, 8, 3], name="lg5")
    s5 = G.placeholder(G.KIND_U8, [None, 4, 8, 8], name="s5")
    for fn in (losses.get_dice, losses.dice_loss, losses.cross_entropy_loss):
        with pytest.raises(NotImplementedError, match="3-D"):
            fn(lg5, s5)
    with pytest.raises(ValueError):
        losses.dice_loss(G.placeholder(G.KIND_F32, [None, 8, 8, 9], name="wide"), s)
    with pytest.raises(ValueError):
        losses.dice_loss(G.placeholder(G.KIND_ACT, [None, 8, 8, 3], name="act"), s)


def test_add_loss_term_rebuilds_loss_tot():
    import types
    from phiseg_code_amd.phiseg import phiseg_model
    from phiseg_code_amd.tfwrapper import losses
    _, cfg, _ = load_golden("tiny_detunet_bn")
    model = phiseg_model.phiseg(make_config(cfg))
    old_tot, old_step, old_keys = model.loss_tot, model.train_step, set(model.loss_dict)
    old_terms, old_w = list(old_tot.op.inputs), list(old_tot.op.attrs["weights"])
    dice = losses.dice_loss(model.s_out_list[0], model.s_inp_oh, mode="macro")
    assert model.add_loss_term("dice", dice, 0.25) is dice
    assert model.loss_tot is not old_tot and model.loss_tot.op.type == "weighted_sum"
    assert list(model.loss_tot.op.inputs) == old_terms + [dice] and model.loss_tot.op.attrs["weights"] == old_w + [0.25]
    assert model.loss_dict["dice"] is dice and model.loss_dict["total_loss"] is model.loss_tot
    assert set(model.loss_dict) == old_keys | {"dice"}
    assert model.train_step is not old_step and model.train_step.loss is model.loss_tot
    with pytest.raises(ValueError):
        model.add_loss_term("dice", dice)
    with pytest.raises(ValueError):
        model.add_loss_term("table", losses.get_dice(model.s_out_list[0], model.s_inp_oh, sum_over_labels=True, sum_over_batches=True))
    with pytest.raises(ValueError):
        model.add_loss_term("logits", model.s_out_list[0])
    # once the session owns a parameter store (or a plan) the loss is fixed
    model.sess.store = object()
    with pytest.raises(RuntimeError):
        model.add_loss_term("late", losses.cross_entropy_loss(model.s_out_list[0], model.s_inp))
    model.sess.store = None
    # data parallel: batch-summed Dice needs a collective
    model.dist = types.SimpleNamespace(active=True, world=2, rank=0)
    with pytest.raises(NotImplementedError):
        model.add_loss_term("robust", losses.dice_loss(model.s_out_list[0], model.s_inp_oh, mode="macro_robust"))
    model.add_loss_term("micro", losses.dice_loss(model.s_out_list[0], model.s_inp_oh, mode="micro"))
    assert "micro" in model.loss_dict and "robust" not in model.loss_dict


def test_model_without_added_terms_is_unchanged():
    from phiseg_code_amd.phiseg import phiseg_model
    _, cfg, _ = load_golden("tiny_phiseg_bn")
    model = phiseg_model.phiseg(make_config(cfg))
    assert not any(op.type in ("dice_loss", "dice_table", "seg_xent") for op in model.graph.ops)
    assert model.train_step.loss is model.loss_tot and model.loss_dict["total_loss"] is model.loss_tot


def test_new_symbols_are_declared_in_the_header():
    from phiseg_code_amd import runtime as rt
    protos = rt.parse_header()
    for name in ("phx_dice_ws_bytes", "phx_dice_sums", "phx_dice_finish", "phx_dice_grad", "phx_seg_xent_ws_bytes", "phx_seg_xent",
                 "phx_nn_resize_adjoint"):
        assert name in protos, name
    assert len(protos["phx_dice_finish"]) == 16 and len(protos["phx_seg_xent"]) == 16 and len(protos["phx_nn_resize_adjoint"]) == 9
    assert "LOGITS, first maximum winning" in open(rt.HEADER).read()      # the header says which arg-max the hard prediction is
