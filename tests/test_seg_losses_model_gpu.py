"""tfwrapper.losses through the model on the MI355X (fp32 compute dtype, the tiny fixtures): fetched values against the restatement on
the fetched logits, the training wiring of phiseg.add_loss_term on det_unet2D (head-bias gradient) and on PHiSeg (the gradient on
model.s_out reaches every level), the Dice term falling over Adam steps, and the guards."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import seg_losses_ref as R
from tests.helpers import golden_inputs, load_golden
from tests.test_graph_cpu import make_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(np.finfo(np.float32).eps)


def detunet(dist=None):
    from phiseg_code_amd.phiseg import phiseg_model
    _, cfg, var_order = load_golden("tiny_detunet_bn")
    model = phiseg_model.phiseg(make_config(cfg, "f32"), rng_seed=cfg["eps_seed"], dist=dist)
    params, x_np, s_np = golden_inputs(cfg, var_order, dtype=torch.float64)
    return model, cfg, {k: v.detach().numpy() for k, v in params.items()}, x_np, s_np


def check(what, dev, ref64, ref32):
    ok, err, allowed = R.band(dev, ref64, ref32)
    print("%-48s error %.3e  allowed %.3e  ratio %.3f" % (what, err, allowed, err / allowed if allowed else 0.0))
    assert ok, (what, err, allowed)


def test_fetched_losses_equal_the_restatement_on_the_fetched_logits():
    from phiseg_code_amd.tfwrapper import losses
    model, cfg, weights, x_np, s_np = detunet()
    logits_t = model.s_out_list[0]
    cw = [0.25, 1.75]
    fetch = [losses.dice_loss(logits_t, model.s_inp_oh, mode="macro"),
             losses.pixel_wise_cross_entropy_loss_weighted(logits_t, model.s_inp_oh, cw),
             losses.get_dice(logits_t, model.s_inp_oh), logits_t]
    model.set_weights(weights)
    dice, wce, table, lg = model.sess.run(fetch, {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: True})
    assert lg.shape == (cfg["B"], cfg["H"], cfg["H"], cfg["nlabels"]) and table.shape == (cfg["B"], cfg["nlabels"])
    check("dice_loss (macro)", dice, R.dice_loss(lg, s_np)[0], R.dice_loss(lg, s_np, dtype=np.float32)[0])
    check("pixel_wise_cross_entropy_loss_weighted", wce, R.cross_entropy_loss(lg, s_np, class_weights=cw)[0],
          R.cross_entropy_loss(lg, s_np, class_weights=cw, dtype=np.float32)[0])
    check("get_dice (hard)", table, R.get_dice(lg, s_np), R.get_dice(lg, s_np, dtype=np.float32))


def test_dice_term_reaches_the_prediction_bias_gradient():
    """One training step of det_unet2D with the objective CE + w * Dice: the gradient of the `prediction` bias is the per-class pixel
    sum of (1 / B) w_ce (sm - y) + w dDice / dlogits, recomputed in float64 from the logits fetched in that step."""
    from phiseg_code_amd.tfwrapper import losses
    base, cfg, weights, x_np, s_np = detunet()
    base.set_weights(weights)
    feed = lambda m: {m.x_inp: x_np, m.s_inp: s_np, m.training_pl: True, m.lr_pl: 1e-6}      # noqa: E731
    lg0 = base.sess.run(base.s_out_list[0], feed(base))
    B, C = cfg["B"], cfg["nlabels"]
    w_ce = float(base.exp_config.residual_multinoulli_loss_weight)
    y = R.one_hot(s_np, C, np.float64)
    ce_share0 = (w_ce * (R.softmax(lg0.astype(np.float64)) - y) / B).sum(axis=(0, 1, 2))
    dice_share0 = R.dice_loss(lg0, s_np)[1].sum(axis=(0, 1, 2))
    w = float(np.abs(ce_share0).max() / np.abs(dice_share0).max())      # the Dice share of the bias gradient ~ the cross-entropy share

    model, _, _, _, _ = detunet()
    model.add_loss_term("dice", losses.dice_loss(model.s_out_list[0], model.s_inp_oh, mode="macro"), w)
    model.set_weights(weights)
    _, lg, tot, ce, dice = model.sess.run([model.train_step, model.s_out_list[0], model.loss_tot,
                                           model.loss_dict["residual_multinoulli_loss_lvl0"], model.loss_dict["dice"]], feed(model))
    got = model.sess.store.export(grads=True)["likelihood/prediction/b"].astype(np.float64)
    d_ce = w_ce * (R.softmax(lg.astype(np.float64)) - y) / B
    d_dice = w * R.dice_loss(lg, s_np)[1]
    want = (d_ce + d_dice).sum(axis=(0, 1, 2))
    # bound: the bias gradient is an fp32 sum of N = B H W elements per class; each element carries ~8 ulp (two shares, an exp, a
    # division), and a blocked fp32 summation (chains of a few dozen adds per thread, then tree stages) stays within a few dozen eps
    # of the sum of magnitudes -- 64 eps covers both, and is far below N eps, the worst case of one serial chain
    bound = 64 * EPS32 * (np.abs(d_ce) + np.abs(d_dice)).sum(axis=(0, 1, 2))
    ce_share, dice_share = d_ce.sum(axis=(0, 1, 2)), d_dice.sum(axis=(0, 1, 2))
    print("prediction/b gradient %s  want %s  CE share %s  Dice share %s  bound %s  w %.4g" % (got, want, ce_share, dice_share, bound, w))
    assert 0.2 < np.abs(dice_share).max() / np.abs(ce_share).max() < 5.0
    assert (bound < 0.05 * np.abs(dice_share)).all(), "the bound must be able to tell the Dice share from nothing"
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)
    np.testing.assert_allclose(float(tot), w_ce * float(ce) + w * float(dice), rtol=1e-5)


@pytest.mark.parametrize("target", ["s_out", "aggregate", "level0"])
def test_dice_on_summed_logits_reaches_every_level_of_phiseg(target):
    """Two tiny PHiSeg models with equal seeds under PHX_DETERMINISTIC=1 (a process of its own: the variable is read once), one with
    a Dice term on model.s_out: the difference of their logit-head bias gradients is the SAME vector at every level,
    w * sum over pixels of dDice / ds_out -- the gradient went through residual_ce's buffers and the resize adjoint.  The same through
    G.aggregate_logits(model.s_out_list)[0]; a term on model.s_out_list[0] alone changes the finest level's gradient and no other."""
    env = dict(os.environ, PYTHONPATH=ROOT, PHX_DETERMINISTIC="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "seg_losses_worker.py"), "1000", target], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res["rows"]) == 5 and np.abs(res["want"]).max() > 0
    for row in res["rows"]:
        diff, bound, want = np.asarray(row["diff"]), np.asarray(row["bound"]), np.asarray(row["want"])
        print("%s level %d  difference %s  want %s  bound %s  |CE gradient| %s" % (target, row["level"], diff, want, bound, row["ce"]))
        assert (bound < 0.05 * np.abs(res["want"])).all(), "the bound must be able to tell the Dice share from nothing"
        assert (np.abs(diff - want) <= bound).all(), (row["level"], diff, want, bound)
        assert np.array_equal(want, res["want"]) or (target == "level0" and row["level"] > 0 and not want.any())
    assert abs(res["dice"] - res["dice64"]) < 1e-5


def test_twenty_adam_steps_lower_the_dice_term():
    from phiseg_code_amd.tfwrapper import losses
    model, cfg, weights, x_np, s_np = detunet()
    model.add_loss_term("dice", losses.dice_loss(model.s_out_list[0], model.s_inp_oh, mode="macro"), 1.0)
    model.set_weights(weights)
    fd = {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: True, model.lr_pl: 1e-3}
    hist = [float(model.sess.run([model.train_step, model.loss_dict["dice"]], fd)[1]) for _ in range(20)]
    print("dice over 20 Adam steps:", ["%.4f" % v for v in hist])
    assert np.isfinite(hist).all() and hist[-1] < hist[0]


def test_guards():
    from phiseg_code_amd.tfwrapper import losses
    model, cfg, weights, x_np, s_np = detunet()
    late = losses.dice_loss(model.s_out_list[0], model.s_inp_oh, mode="micro")
    model.set_weights(weights)
    model.sess.run(model.loss_tot, {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: True})
    with pytest.raises(RuntimeError):
        model.add_loss_term("late", late)
    assert "late" not in model.loss_dict
    # data parallel: a batch-summed Dice would need a collective -- refused when the term is added and when a plan is lowered
    fake = types.SimpleNamespace(active=True, world=1, rank=0, broadcast_=lambda t: None, sum_float=lambda v: v)
    dp, _, _, _, _ = detunet(dist=fake)
    with pytest.raises(NotImplementedError):
        dp.add_loss_term("robust", losses.dice_loss(dp.s_out_list[0], dp.s_inp_oh, mode="macro_robust"))
    table = losses.get_dice(dp.s_out_list[0], dp.s_inp_oh, sum_over_batches=True)
    with pytest.raises(NotImplementedError):
        dp.sess.run(table, {dp.x_inp: x_np, dp.s_inp: s_np, dp.training_pl: False})
    per_image = losses.get_dice(dp.s_out_list[0], dp.s_inp_oh)
    assert dp.sess.run(per_image, {dp.x_inp: x_np, dp.s_inp: s_np, dp.training_pl: False}).shape == (cfg["B"], cfg["nlabels"])
    # get_dice is a table, not a loss term: a plan whose loss holds one is refused
    from phiseg_code_amd import engine, graph as G
    m2, _, _, _, _ = detunet()
    scalar_table = losses.get_dice(m2.s_out_list[0], m2.s_inp_oh, sum_over_labels=True, sum_over_batches=True)
    bad = G.weighted_sum(list(m2.loss_tot.op.inputs) + [scalar_table], list(m2.loss_tot.op.attrs["weights"]) + [1.0])
    with pytest.raises(ValueError):
        engine.Plan(m2.sess._ensure_store(), [bad], loss=bad, batch=cfg["B"], training=True, compute_dtype="f32", optimize=False)
