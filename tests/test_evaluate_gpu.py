"""Test-set evaluation on the MI355X (phiseg_code_amd/evaluate.py, the two test scripts): evaluate_split scores samples that never leave
the GPU; the same samples are fetched again (noise step rewound, same grouping of images into passes) and scored by the CPU oracle.
Tolerances are those of test_do_validation_matches_oracle_scoring: GED and Dice 1e-6 (integer counts, one float32 store), NCC 2e-5."""
import importlib
import os
import types

import numpy as np
import pytest

from oracle import metrics as om
from tests.helpers import golden_inputs, load_golden
from tests.test_graph_cpu import make_config

pytestmark = pytest.mark.gpu


def _noise_step(model):
    return int(model.sess._ensure_store().noise_step.cpu().item())


def _rewind(model, step):
    import torch
    model.sess._ensure_store().noise_step.fill_(step)
    torch.cuda.synchronize()


def _oracle_rows(model, split, sm_tensor, n, groups, sref, repeat_x):
    """Fetch the samples of every pass again and score them per image -> (ged [n_img], ncc [n_img], dice [n_img, nlabels])"""
    C = model.exp_config.nlabels
    ged, ncc, dice = [], [], []
    for i0, b in groups:
        x = split.images[i0:i0 + b]
        sm = model.sess.run(sm_tensor, {model.training_pl: False, model.x_inp: np.repeat(x, n, axis=0) if repeat_x else x})
        model._advance_noise()
        sm = sm.reshape((b, n) + sm.shape[1:])
        for k in range(b):
            gts = np.ascontiguousarray(split.labels[i0 + k].transpose(2, 0, 1))
            g, c, _ = om.validation_metrics(sm[k], gts, gts[sref[i0 + k]], C)
            ged.append(g)
            ncc.append(c)
            dice.append(om.per_label_dice(sm[k].astype(np.float64).mean(axis=0).argmax(axis=-1), gts[sref[i0 + k]], C))
    return np.asarray(ged), np.asarray(ncc), np.asarray(dice)


def _check(res, ref):
    ged, ncc, dice = ref
    print("GED", res["ged"], ged, "\nNCC", res["ncc"], ncc, "\nDice", res["dice"].tolist(), dice.tolist())
    assert np.isfinite(ged).all() and np.isfinite(ncc).all()
    np.testing.assert_allclose(res["ged"], ged, rtol=0, atol=1e-6)
    np.testing.assert_allclose(res["ncc"], ncc, rtol=0, atol=2e-5)
    np.testing.assert_allclose(res["dice"], dice, rtol=0, atol=1e-6)
    assert ((res["ged"] >= 0) & (res["ged"] <= 2)).all() and (np.abs(res["ncc"]) <= 1 + 1e-6).all()


def test_evaluate_split_matches_oracle_scoring():
    """phiseg_7_5, bf16, 3 images, 8 samples, 2 images per pass: two passes through sampling_graph(8), the second one short."""
    from phiseg_code_amd import evaluate
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    base = importlib.import_module("phiseg_code_amd.phiseg.experiments.phiseg_7_5")
    cfg = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if not k.startswith("_")})
    cfg.compute_dtype = "bf16"
    data = synthetic.SyntheticLIDC(cfg, seed=5, n_validation=3)
    model = phiseg_model.phiseg(cfg, rng_seed=3)
    assert model._one_pass_prior()
    step0 = _noise_step(model)
    np.random.seed(0)
    res = evaluate.evaluate_split(model, data.validation, 8, images_per_pass=2)
    assert _noise_step(model) == step0 + 2
    np.random.seed(0)
    assert res["sref_annot"].tolist() == [np.random.choice(cfg.annotator_range) for _ in range(3)]
    assert res["ged"].shape == res["ncc"].shape == (3,) and res["dice"].shape == (3, cfg.nlabels)
    _rewind(model, step0)
    _check(res, _oracle_rows(model, data.validation, model.sampling_graph(8)[1], 8, [(0, 2), (2, 1)], res["sref_annot"], False))
    # n_images: the first two images alone, in one pass, score as they did above (same noise step, same pass)
    _rewind(model, step0)
    np.random.seed(0)
    two = evaluate.evaluate_split(model, data.validation, 8, images_per_pass=2, n_images=2)
    assert _noise_step(model) == step0 + 1 and two["ged"].shape == (2,)
    for key in ("ged", "ncc", "dice"):
        np.testing.assert_allclose(two[key], res[key][:2], rtol=0, atol=2e-5 if key == "ncc" else 1e-6, err_msg=key)


def _tiny_model(name):
    import torch
    from phiseg_code_amd.phiseg import phiseg_model
    g, cfg, var_order = load_golden(name)
    model = phiseg_model.phiseg(make_config(cfg, "f32"), rng_seed=cfg["eps_seed"])
    params, _, _ = golden_inputs(cfg, var_order, dtype=torch.float64)
    model.set_weights({k: v.detach().numpy() for k, v in params.items()})
    return model, cfg


def _tiny_split(cfg, n_images=3, seed=9):
    from phiseg_code_amd.data import synthetic
    return synthetic._ValidationSplit(cfg["H"], cfg["nlabels"], seed, n_images, 4)


@pytest.mark.parametrize("name, n", [("tiny_probunet_bn", 8), ("tiny_phiseg_bn", 1)])
def test_repeated_x_path_matches_oracle_scoring(name, n):
    """prob_unet2D without one_pass_sampling, and a single sample of any model (how det_unet2D is scored): x repeated on
    s_out_eval_sm.  n0 = 4 fixtures in fp32 keep this at seconds."""
    from phiseg_code_amd import evaluate
    model, cfg = _tiny_model(name)
    assert n == 1 or not model._one_pass_prior()
    split = _tiny_split(cfg)
    step0 = _noise_step(model)
    np.random.seed(1)
    res = evaluate.evaluate_split(model, split, n, images_per_pass=2, annotator_range=range(4))
    assert _noise_step(model) == step0 + 2
    _rewind(model, step0)
    _check(res, _oracle_rows(model, split, model.s_out_eval_sm, n, [(0, 2), (2, 1)], res["sref_annot"], True))


def test_both_mains_end_to_end(tmp_path):
    """Checkpoints written by save_weights, a 3-image test split of a lidc_data built from arrays, 8 samples: the files the reference's
    scripts write, with the values of an evaluate_split call at the same noise step."""
    from phiseg_code_amd import evaluate
    from phiseg_code_amd import phiseg_test_predictions as tp
    from phiseg_code_amd import phiseg_test_quantitative as tq
    from phiseg_code_amd.data.lidc_data import lidc_data
    from phiseg_code_amd.phiseg import phiseg_model
    model, cfg = _tiny_model("tiny_phiseg_bn")
    exp_config = model.exp_config
    model.save_weights(os.path.join(str(tmp_path), "model_best_ged.ckpt-0"))
    model.save_weights(os.path.join(str(tmp_path), "model_best_dice.ckpt-0"))
    parts = {sp: _tiny_split(cfg, n_images=k, seed=20 + k) for sp, k in (("train", 4), ("val", 2), ("test", 3))}
    data = lidc_data(exp_config, source={sp: dict(images=s.images[..., 0], labels=s.labels) for sp, s in parts.items()})
    assert data.test.labels_dev.shape == (3, cfg["H"], cfg["H"], 4)
    nl = cfg["nlabels"]

    np.random.seed(4)
    tq.main(str(tmp_path), exp_config, do_plots=False, n_samples=8, data=data)
    np.random.seed(4)
    tp.main(str(tmp_path), exp_config, n_samples=8, data=data)
    files = [os.path.join(str(tmp_path), f) for f in ("ged8_best_ged.npz", "ncc8_best_ged.npz", "dice_best_dice.npz")]
    arrs = []
    for f, shape in zip(files, ((3,), (3,), (3, nl))):
        assert os.path.exists(f), f
        z = np.load(f)
        assert z.files == ["arr_0"] and z["arr_0"].shape == shape
        arrs.append(z["arr_0"])
    ged, ncc, dice = arrs
    assert ((ged >= 0) & (ged <= 2)).all() and ((ncc >= -1) & (ncc <= 1)).all() and ((dice >= 0) & (dice <= 1)).all()
    # a fresh model on the same checkpoint starts at the same noise step as the one each main builds
    for kind, want in (("best_ged", dict(ged=ged, ncc=ncc)), ("best_dice", dict(dice=dice))):
        m2 = phiseg_model.phiseg(exp_config=exp_config)
        m2.load_weights(str(tmp_path), type=kind)
        np.random.seed(4)
        res = evaluate.evaluate_split(m2, data.test, 8)
        for key, arr in want.items():
            np.testing.assert_allclose(res[key], arr, rtol=0, atol=2e-5 if key == "ncc" else 1e-6, err_msg=key)
