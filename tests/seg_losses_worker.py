"""Worker of tests/test_seg_losses_model_gpu.py, started with PHX_DETERMINISTIC=1 in its environment (the engine and the library
read the variable once, at import / first use): two tiny PHiSeg models with equal seeds, one of them with a Dice term on model.s_out
("s_out": through residual_ce's buffers), on G.aggregate_logits(model.s_out_list)[0] ("aggregate": through the backward of the
aggregation) or on model.s_out_list[0] ("level0": the finest level alone, a factor-1 resize view), one training step each.  Prints
one JSON line: per level the difference of the two models' logit-head bias gradients, the vector the restatement predicts for it and
the bound computed from the magnitudes that are subtracted."""
import json
import sys

import numpy as np
import torch

from tests import seg_losses_ref as R
from tests.helpers import golden_inputs, load_golden
from tests.test_graph_cpu import make_config


def main(weight, target):
    from phiseg_code_amd.phiseg import phiseg_model
    from phiseg_code_amd.tfwrapper import losses
    _, cfg, var_order = load_golden("tiny_phiseg_bn")
    params, x_np, s_np = golden_inputs(cfg, var_order, dtype=torch.float64)
    weights = {k: v.detach().numpy() for k, v in params.items()}
    L, B = cfg["latent_levels"], cfg["B"]
    feed = lambda m: {m.x_inp: x_np, m.s_inp: s_np, m.training_pl: True, m.lr_pl: 1e-6}      # noqa: E731

    base = phiseg_model.phiseg(make_config(cfg, "f32"), rng_seed=cfg["eps_seed"])
    base.set_weights(weights)
    out = base.sess.run([base.train_step, base.s_out] + list(base.s_out_list), feed(base))
    s_out0, levels = out[1], out[2:]
    g0 = base.sess.store.export(grads=True)

    model = phiseg_model.phiseg(make_config(cfg, "f32"), rng_seed=cfg["eps_seed"])
    from phiseg_code_amd import graph as G
    logits_t = {"s_out": lambda: model.s_out, "aggregate": lambda: G.aggregate_logits(model.s_out_list)[0],
                "level0": lambda: model.s_out_list[0]}[target]()
    model.add_loss_term("dice", losses.dice_loss(logits_t, model.s_inp_oh, mode="macro"), weight)
    model.set_weights(weights)
    _, s_out1, dice = model.sess.run([model.train_step, model.s_out, model.loss_dict["dice"]], feed(model))
    g1 = model.sess.store.export(grads=True)
    assert np.array_equal(s_out0, s_out1), "equal seeds: the two models see the same logits"

    # the Dice gradient on the summed logits, and (for the bound) the residual-CE gradient of every level at full resolution:
    # d / d s_k = sum_{l <= k} (softmax(A_l) - y) / B with A_l = sum_{j >= l} s_j (phiseg_model.py:229-262)
    dice64, dd = R.dice_loss(levels[0] if target == "level0" else s_out1, s_np)
    want = (weight * dd).sum(axis=(0, 1, 2))
    y = R.one_hot(s_np, cfg["nlabels"], np.float64)
    w_ce = float(getattr(make_config(cfg, "f32"), "residual_multinoulli_loss_weight"))
    acc = np.zeros_like(levels[0], dtype=np.float64)
    G_l = [None] * L
    for l in reversed(range(L)):
        acc = acc + levels[l].astype(np.float64)
        G_l[l] = w_ce * (R.softmax(acc) - y) / B
    eps32 = float(np.finfo(np.float32).eps)
    rows = []
    run = np.zeros_like(acc)
    for k in range(L):
        run = run + G_l[k]
        # each of the two bias gradients is an fp32 sum over the level's pixels of block sums of these elements: 64 eps of the sum of
        # magnitudes each (a blocked fp32 summation with ~8 ulp per element), the same allowance as in the det_unet2D test
        share = weight * dd if (k == 0 or target != "level0") else 0.0 * dd         # "level0": the term stops at the finest level
        bound = 64 * eps32 * (np.abs(run).sum(axis=(0, 1, 2)) + np.abs(run + share).sum(axis=(0, 1, 2)))
        name = "likelihood/y_lvl%d/b" % k
        rows.append(dict(level=k, want=share.sum(axis=(0, 1, 2)).tolist(), bound=bound.tolist(),
                         diff=(g1[name].astype(np.float64) - g0[name].astype(np.float64)).tolist(),
                         ce=np.abs(g0[name]).astype(np.float64).tolist()))
    print(json.dumps(dict(want=want.tolist(), rows=rows, dice=float(dice), dice64=float(dice64))))


if __name__ == "__main__":
    main(float(sys.argv[1]), sys.argv[2])
