"""PHiSeg with 9 and 19 classes end to end on the MI355X: the tiny net of the goldens' shape family -- n0 = 4,
64 x 64, three latent levels, five resolution levels, B = 2 -- against the float64 oracle, with the bounds the tests of
tests/test_model_gpu.py hold the two-class fixtures to (each test names its model).  Above eight classes the residual_ce, aggregate and
eval_xent operators launch the entries of csrc/many_class.hip and the 1x1 logit heads run on phx_conv2d_direct; the scores of
_do_validation and evaluate_split come from phx_metrics_wide."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import init as oinit
from oracle import metrics as om
from oracle import nets
from oracle import train as otrain
from tests.test_graph_cpu import make_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS_SEED, H, B = 42, 64, 2


def tiny_cfg(C):
    return dict(arch="phiseg", norm="batch_norm", n0=4, zdim0=2, H=H, B=B, nlabels=C, latent_levels=3, resolution_levels=5,
                image_size=(H, H, 1), KL_weight=1.0, CE_weight=1.0, exponential_weighting=True, weight_seed=0, eps_seed=EPS_SEED,
                data_seed=1234)


def labels(C):
    """blocks of 3 x 5 pixels cycling through every class: classes 0 and C - 1 both occur, and a coarse level sees mixed blocks"""
    y, x = np.mgrid[0:H, 0:H]
    s = np.stack([(x // 3 + 3 * (y // 5) + b) % C for b in range(B)]).astype(np.uint8)
    assert set(np.unique(s).tolist()) == set(range(C))
    return s


def build(C, dtype="f32", perturbed=False):
    """-> (model, cfg, oracle parameters in float64 (the reference's initialisation unless perturbed), x, s)"""
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = tiny_cfg(C)
    model = phiseg_model.phiseg(make_config(cfg, dtype), rng_seed=EPS_SEED)
    var_order = [(n, tuple(v.shape)) for n, v in model.graph.variables.items()]
    params = otrain.make_params(var_order, cfg["weight_seed"], torch.float64, perturbed=perturbed)
    model.set_weights({k: v.detach().numpy() for k, v in params.items()})
    x_np, _ = oinit.synthetic_batch(B, H, 2, cfg["data_seed"])
    return model, cfg, params, x_np, labels(C)


def _hip_grads(model, cfg, x_np, s_np):
    from phiseg_code_amd import engine
    store = model.sess._ensure_store()
    plan = engine.Plan(store, [model.loss_tot], loss=model.loss_tot, batch=cfg["B"], training=True,
                       compute_dtype="f32", optimize=False, rng_seed=cfg["eps_seed"], use_hip_graph=False)
    plan.set_input("x_input", x_np)
    plan.set_input("s_input", s_np)
    plan.run(sync=True)
    return store.export(grads=True)


@pytest.mark.parametrize("C", [9, 19])
def test_loss_terms_and_gradients_match_oracle_fp32(C):
    """every ELBO term (5e-4, the bound of the n0 = 4 fixtures) and EVERY variable's gradient against the oracle's autograd: 3e-2 of the
    variable's largest gradient entry + 1e-5 of the largest gradient norm (test_gradients_match_oracle_wellconditioned_fp32)"""
    model, cfg, params, x_np, s_np = build(C)
    out, gref = otrain.loss_and_grads(params, torch.as_tensor(x_np, dtype=torch.float64), torch.as_tensor(s_np),
                                      otrain.torch_eps_fn(EPS_SEED, 0, B), cfg)
    keys = sorted(model.loss_dict)
    assert set(keys) == set(out["loss_dict"])
    got = model.sess.run([model.loss_dict[k] for k in keys], {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: True})
    for k, v in zip(keys, got):
        print("C=%d %-36s HIP %.6f oracle %.6f" % (C, k, float(v), float(out["loss_dict"][k])))
        np.testing.assert_allclose(float(v), float(out["loss_dict"][k]), rtol=5e-4, err_msg=k)
    grads = _hip_grads(model, cfg, x_np, s_np)
    gmax = max(float(v.norm()) for v in gref.values() if v is not None)
    checked, worst = 0, 0.0
    for name, ref in gref.items():
        g = grads[name].astype(np.float64)
        if ref is None:
            assert np.abs(g).max() == 0.0, name
            continue
        r = ref.numpy()
        tol = 3e-2 * np.abs(r).max() + 1e-5 * gmax
        worst = max(worst, np.abs(g - r).max() / tol)
        assert np.abs(g - r).max() <= tol, (name, np.abs(g - r).max(), tol)
        checked += 1
    print("C=%d gradients: %d variables, worst error / bound %.3f" % (C, checked, worst))
    assert checked > 10


@pytest.mark.parametrize("C", [9, 19])
def test_three_adam_steps_match_oracle_fp32(C):
    """eager, hipGraph capture, hipGraph replay against the oracle's TF1-form Adam, by the rule of the test of the same name in
    tests/test_model_gpu.py (lr = 1e-5: a weight whose gradient is round-off-sized may differ by 2 lr per step, no more than 1 % do)"""
    lr = 1e-5
    model, cfg, params, x_np, s_np = build(C, perturbed=True)
    p0 = {k: v.detach().clone().numpy() for k, v in params.items()}
    ref_losses = otrain.train_steps(params, [(x_np, s_np)], cfg, EPS_SEED, lr=lr, n_steps=3)
    losses = []
    for _ in range(3):
        _, lt = model.sess.run([model.train_step, model.loss_tot],
                               {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: True, model.lr_pl: lr})
        losses.append(float(lt))
    np.testing.assert_allclose(losses, [l["total_loss"] for l in ref_losses], rtol=1e-3)
    got = model.sess.store.export()
    n_all = n_off = n_moved = 0
    for name, ref in params.items():
        r = ref.detach().numpy()
        d = np.abs(got[name].astype(np.float64) - r)
        if name.rsplit("/", 1)[-1].startswith("moving_"):
            assert d.max() <= 1e-3 * max(np.abs(r).max(), 1.0), (name, d.max())
            continue
        assert d.max() <= 3 * 2 * lr + 1e-6 * np.abs(r).max(), (name, d.max())
        n_all += d.size
        n_off += int((d > 0.1 * lr + 2e-7 * np.abs(r)).sum())
        n_moved += int((np.abs(r - p0[name]) > 0.5 * lr).sum())
    print("C=%d three Adam steps: %d of %d elements off by more than 0.1 lr" % (C, n_off, n_all))
    assert n_moved > 0.5 * n_all * 0.5
    assert n_off <= 0.01 * n_all, (n_off, n_all)
    assert int(model.sess.store.step.cpu()[0]) == 3


@pytest.mark.parametrize("C", [9, 19])
def test_sampling_softmax_and_eval_xent_match_oracle_fp32(C):
    """s_out_eval_sm and eval_xent (prior in generation mode, likelihood, the aggregate and xent_map operators) against
    oracle.nets.sample: 1e-4 of the largest reference value"""
    model, cfg, params, x_np, s_np = build(C)
    with torch.no_grad():
        ref = nets.sample(params, torch.as_tensor(x_np, dtype=torch.float64), otrain.torch_eps_fn(EPS_SEED, 0, B), cfg)
    sm, xe = model.sess.run([model.s_out_eval_sm, model.eval_xent], {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: False})
    r_sm = ref["s_out_eval_sm"].numpy()
    lg = ref["s_out_eval"]
    r_xe = (torch.logsumexp(lg, dim=-1) - lg.gather(-1, torch.as_tensor(s_np).long()[..., None])[..., 0]).numpy()
    for name, got, r in (("s_out_eval_sm", sm, r_sm), ("eval_xent", xe, r_xe)):
        err = np.abs(got - r).max() / np.abs(r).max()
        print("C=%d %s rel-to-max error %.3e" % (C, name, err))
        assert got.shape == r.shape and err <= 1e-4, (name, err)


def test_bf16_path_19_classes():
    """bf16 storage at C = 19 by the rule of test_bf16_path_lidc: the HIP logits of every level sit within 2x the distance between the
    exact float64 oracle and the oracle with bf16 storage simulated (floor 0.5 % of the logit range), of BOTH oracles; every ELBO term
    within max(5 %, 2.5x what the simulated storage moves it, for a KL level 1.5x the largest such move of any KL level)"""
    C = 19
    model, cfg, params, x_np, s_np = build(C, "bf16")
    L = cfg["latent_levels"]
    xt, st = torch.as_tensor(x_np, dtype=torch.float64), torch.as_tensor(s_np)
    eps = otrain.torch_eps_fn(EPS_SEED, 0, B)
    with torch.no_grad():
        exact = nets.elbo(params, xt, st, eps, cfg, training=True)
        sim = nets.elbo(params, xt, st, eps, cfg, training=True, bf16_sim=True)
    keys = sorted(model.loss_dict)
    s_list, losses = model.sess.run([model.s_out_list, [model.loss_dict[k] for k in keys]],
                                    {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: True})

    def rms(ref, l):
        r = ref["s"][l].numpy()
        return float(np.sqrt(((s_list[l] - r) ** 2).mean()) / np.abs(r).max())
    for l in range(L):
        inherent = float(np.sqrt(((sim["s"][l] - exact["s"][l]) ** 2).mean()) / exact["s"][l].abs().max())
        bound = 2.0 * max(inherent, 0.005)
        print("C=19 bf16 level %d: RMS/max vs simulated %.4f, vs exact %.4f, simulated vs exact %.4f" % (l, rms(sim, l), rms(exact, l), inherent))
        assert rms(sim, l) < bound and rms(exact, l) < bound, (l, rms(sim, l), rms(exact, l), inherent)
    inh = {k: abs(float(sim["loss_dict"][k]) - float(exact["loss_dict"][k])) / abs(float(exact["loss_dict"][k])) for k in keys}
    kl_inh = max([v for k, v in inh.items() if k.startswith("KL_")] or [0.0])
    for k, v in zip(keys, losses):
        ex = float(exact["loss_dict"][k])
        print("C=19 bf16 %-36s exact %.4e HIP %+.2f%% simulated %+.2f%%" % (k, ex, 100 * (float(v) - ex) / ex, 100 * inh[k]))
        np.testing.assert_allclose(float(v), ex, rtol=max(0.05, 2.5 * inh[k], 1.5 * kl_inh if k.startswith("KL_") else 0.0), err_msg=k)


def _digest(C, dtype, steps):
    env = dict(os.environ, PYTHONPATH=ROOT, PHX_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "many_class_model_worker.py"), str(C), dtype, str(steps)], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DIGEST")][-1].split()
    return line[1], float(line[2])


def test_captured_plan_is_bit_identical_in_deterministic_mode():
    """PHX_DETERMINISTIC=1, C = 19, fp32: four training steps (eager, capture, two replays) in two processes give the same digest of
    every loss term, gradient and parameter"""
    a, b = _digest(19, "f32", 4), _digest(19, "f32", 4)
    assert np.isfinite(a[1]) and a == b, (a, b)


def _nine_class_model_and_data(n_validation=3):
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = make_config(tiny_cfg(9), "f32")
    cfg.validation_samples, cfg.num_validation_images = 6, n_validation
    data = synthetic.SyntheticLIDC(cfg, seed=5, n_validation=n_validation)
    return phiseg_model.phiseg(cfg, rng_seed=3), cfg, data


def test_train_two_steps_and_validation_pass_nine_classes():
    """train(data, num_iter=2) on data/synthetic.py data with nine classes runs to the end, and one validation pass scores what the
    oracle scores on the samples it drew (the noise step rewound): GED and Dice 1e-6, NCC 2e-5, as
    test_do_validation_matches_oracle_scoring"""
    model, cfg, data = _nine_class_model_and_data()
    assert int(data.train.next_batch(4)[1].max()) == 8                     # the synthetic labels reach class 8
    losses = model.train(data, num_iter=2)
    assert int(model.sess.store.step.cpu()[0]) == 2
    assert losses is None or np.isfinite(np.asarray(losses, dtype=np.float64)).all()
    np.random.seed(0)
    res = model._do_validation(data)
    assert np.isfinite([res["loss"], res["dice"], res["ged"], res["ncc"]]).all()
    assert 0.0 <= res["ged"] <= 2.0 and -1.0 <= res["ncc"] <= 1.0 and res["per_structure_dice"].shape == (9,)
    np.random.seed(0)
    model.sess.store.noise_step -= cfg.num_validation_images
    geds, nccs, dices = [], [], []
    for ii in range(cfg.num_validation_images):
        s_gt = data.validation.labels[ii]
        s = s_gt[:, :, np.random.choice(cfg.annotator_range)]
        x_b = np.tile(data.validation.images[ii][None], [cfg.validation_samples, 1, 1, 1])
        sm = model.predict_segmentation_sample(x_b, return_softmax=True)
        g, n, d = om.validation_metrics(sm, np.ascontiguousarray(s_gt.transpose(2, 0, 1)), s, 9)
        geds.append(g); nccs.append(n); dices.append(d)
    np.testing.assert_allclose(res["ged"], np.mean(geds), atol=1e-6)
    np.testing.assert_allclose(res["ncc"], np.mean(nccs), atol=2e-5)
    np.testing.assert_allclose(res["per_structure_dice"], np.mean(dices, axis=0), atol=1e-6)


def test_evaluate_split_nine_classes_equals_the_per_image_path():
    """evaluate_split (labels [I][P][M], annotator index, samples scored in place) against the per-image path of _do_validation
    (utils.validation_metrics: labels [I][M][P], reference map) and against the oracle on the same samples, fetched again"""
    from phiseg_code_amd import evaluate, utils
    model, cfg, data = _nine_class_model_and_data()
    n, split = 6, data.validation
    store = model.sess._ensure_store()
    step0 = int(store.noise_step.cpu().item())
    np.random.seed(0)
    res = evaluate.evaluate_split(model, split, n, images_per_pass=2)
    assert res["dice"].shape == (3, 9) and int(store.noise_step.cpu().item()) == step0 + 2
    store.noise_step.fill_(step0)
    torch.cuda.synchronize()
    one_pass = model._one_pass_prior()
    sm_t = model.sampling_graph(n)[1] if one_pass else model.s_out_eval_sm
    row = 0
    for i0, b in [(0, 2), (2, 1)]:
        x = split.images[i0:i0 + b]
        sm = model.sess.run(sm_t, {model.training_pl: False, model.x_inp: x if one_pass else np.repeat(x, n, axis=0)})
        model._advance_noise()
        sm = sm.reshape((b, n) + sm.shape[1:])
        for k in range(b):
            gts = np.ascontiguousarray(split.labels[i0 + k].transpose(2, 0, 1))
            ref = gts[res["sref_annot"][row]]
            ged, ncc, dice = utils.validation_metrics(sm[k][None], gts[None], ref[None], 9)
            o_ged, o_ncc, o_dice = om.validation_metrics(sm[k], gts, ref, 9)
            print("image %d GED %.7f / %.7f / %.7f NCC %.7f / %.7f / %.7f" % (row, res["ged"][row], ged[0], o_ged, res["ncc"][row], ncc[0], o_ncc))
            np.testing.assert_allclose([res["ged"][row], ged[0]], o_ged, rtol=0, atol=1e-6)
            np.testing.assert_allclose([res["ncc"][row], ncc[0]], o_ncc, rtol=0, atol=2e-5)
            np.testing.assert_allclose(res["dice"][row], o_dice, rtol=0, atol=1e-6)
            np.testing.assert_allclose(dice[0], o_dice, rtol=0, atol=1e-6)
            row += 1


def test_train_with_augmentation_on_nine_classes():
    """phiseg.train(data) on a device-resident nine-class data set with rotation, crop-scale and the elastic deformation switched on:
    the steps consume batches whose label maps went through the nearest-neighbour chain (phx_augment_batch_nearest)"""
    from phiseg_code_amd.data import augment as pa
    from phiseg_code_amd.phiseg import phiseg_model
    from tests import augment_nearest_ref as nr
    from tests.test_augment_nearest_gpu import _data
    cfg = make_config(tiny_cfg(9), "f32")
    cfg.batch_size, cfg.annotator_range, cfg.num_labels_per_subject = 2, range(4), 4
    cfg.lr_schedule_dict = {0: 1e-3}
    cfg.augmentation_options = dict(do_rotations=True, do_scaleaug=True, do_elasticaug=True, nlabels=9, augment_every_nth=1)
    parts = {sp: _data(n, H, 9, 4, 40 + n) for sp, n in (("train", 4), ("val", 2))}
    data = pa.lidc_data(cfg, {sp: dict(images=i, labels=l) for sp, (i, l) in parts.items()}, seed=5)
    model = phiseg_model.phiseg(cfg)
    losses = model.train(data, num_iter=2, log_every=0)
    assert len(losses) == 2 and np.all(np.isfinite(losses)) and data.train.step == 2
    x, s = data.train.next_batch(2)
    for j, (d, src, an) in enumerate(zip(data.train.last_decisions, data.train.last_indices, data.train.last_annotators)):
        ref_x, ref_s = nr.augment_pair_nearest(parts["train"][0][src], parts["train"][1][src, ..., an], d)
        assert d["elastic"] is not None and np.array_equal(s[j], ref_s)
        np.testing.assert_allclose(x[j, ..., 0], ref_x, rtol=0, atol=1e-6)
        assert not np.array_equal(s[j], parts["train"][1][src, ..., an])
