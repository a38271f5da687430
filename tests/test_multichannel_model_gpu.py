"""PHiSeg and the probabilistic U-Net on multi-channel images end to end on the MI355X: the tiny net of
tests/test_many_class_model_gpu.py -- n0 = 4, 64 x 64, three latent levels, five resolution levels, B = 2 -- with image_size =
(64, 64, Cx), against the float64 oracle with that file's bounds (the project's bounds for this net family, not new numbers).  x is Cx
stacked oinit.synthetic_batch draws with different seeds.  With Cx > 1 the posterior's input goes through phx_posterior_input_mc, the
producer through phx_augment_batch_mc and the x_inp grids through phx_summary_grid_image_mc; the convolutions pad any input width."""
import io
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
EPS_SEED, H, B, NL = 42, 64, 2, 2


def tiny_cfg(Cx, arch="phiseg"):
    unet = arch == "prob_unet2D"
    return dict(arch=arch, norm="batch_norm", n0=4, zdim0=6 if unet else 2, H=H, B=B, nlabels=NL, latent_levels=1 if unet else 3,
                resolution_levels=5, image_size=(H, H, Cx), KL_weight=1.0, CE_weight=1.0, exponential_weighting=True, weight_seed=0,
                eps_seed=EPS_SEED, data_seed=1234)


def config(Cx, dtype="f32", arch="phiseg"):
    """tests.test_graph_cpu.make_config sets one channel; the third entry of image_size is set afterwards"""
    c = make_config(tiny_cfg(Cx, arch), dtype)
    c.image_size = (H, H, Cx)
    return c


def inputs(Cx, batch=B):
    planes = [oinit.synthetic_batch(batch, H, NL, 1234 + 17 * c) for c in range(Cx)]
    return np.concatenate([p[0] for p in planes], axis=-1), planes[0][1]


def build(Cx, dtype="f32", perturbed=False, arch="phiseg"):
    """-> (model, cfg, oracle parameters in float64, x [B, H, H, Cx], s)"""
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = tiny_cfg(Cx, arch)
    model = phiseg_model.phiseg(config(Cx, dtype, arch), rng_seed=EPS_SEED)
    var_order = [(n, tuple(v.shape)) for n, v in model.graph.variables.items()]
    params = otrain.make_params(var_order, cfg["weight_seed"], torch.float64, perturbed=perturbed)
    model.set_weights({k: v.detach().numpy() for k, v in params.items()})
    x_np, s_np = inputs(Cx)
    assert x_np.shape == (B, H, H, Cx) and s_np.max() == 1
    return model, cfg, params, x_np, s_np


def _hip_grads(model, cfg, x_np, s_np):
    from phiseg_code_amd import engine
    store = model.sess._ensure_store()
    plan = engine.Plan(store, [model.loss_tot], loss=model.loss_tot, batch=cfg["B"], training=True,
                       compute_dtype="f32", optimize=False, rng_seed=cfg["eps_seed"], use_hip_graph=False)
    plan.set_input("x_input", x_np)
    plan.set_input("s_input", s_np)
    plan.run(sync=True)
    return store.export(grads=True), plan


def _launch_names(plan):
    return [getattr(fn, "__name__", repr(fn)) for fn, _ in plan.launches]


def check_loss_terms_and_gradients(arch, Cx):
    """the body of test_loss_terms_and_gradients_match_oracle_fp32; Cx = 1 runs the launches the engine always made"""
    model, cfg, params, x_np, s_np = build(Cx, arch=arch)
    out, gref = otrain.loss_and_grads(params, torch.as_tensor(x_np, dtype=torch.float64), torch.as_tensor(s_np),
                                      otrain.torch_eps_fn(EPS_SEED, 0, B), cfg)
    keys = sorted(model.loss_dict)
    assert set(keys) == set(out["loss_dict"])
    got = model.sess.run([model.loss_dict[k] for k in keys], {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: True})
    for k, v in zip(keys, got):
        print("%s Cx=%d %-36s HIP %.6f oracle %.6f" % (arch, Cx, k, float(v), float(out["loss_dict"][k])))
        np.testing.assert_allclose(float(v), float(out["loss_dict"][k]), rtol=5e-4, err_msg=k)
    grads, plan = _hip_grads(model, cfg, x_np, s_np)
    names = _launch_names(plan)
    mc, one = names.count("phx_posterior_input_mc"), names.count("phx_posterior_input")
    assert (mc, one) == ((1, 0) if Cx > 1 else (0, 1)), (mc, one)
    gmax = max(float(v.norm()) for v in gref.values() if v is not None)
    checked, worst, failed = 0, 0.0, []
    for name, ref in gref.items():
        g = grads[name].astype(np.float64)
        if ref is None:
            assert np.abs(g).max() == 0.0, name
            continue
        r = ref.numpy()
        tol = 3e-2 * np.abs(r).max() + 1e-5 * gmax
        ratio = np.abs(g - r).max() / tol
        if ratio > 0.5:
            print("%s Cx=%d gradient of %s: error / bound %.3f (largest entry %.4g)" % (arch, Cx, name, ratio, np.abs(r).max()))
        worst = max(worst, ratio)
        failed += [(name, np.abs(g - r).max(), tol)] if ratio > 1.0 else []
        checked += 1
    print("%s Cx=%d gradients: %d variables, worst error / bound %.3f" % (arch, Cx, checked, worst))
    assert not failed, failed
    assert checked > 10


@pytest.mark.parametrize("arch,Cx", [("phiseg", 2), ("phiseg", 3), ("prob_unet2D", 3)])
def test_loss_terms_and_gradients_match_oracle_fp32(arch, Cx):
    """every ELBO term at rtol 5e-4 and EVERY variable's gradient against the oracle's autograd: 3e-2 of the variable's largest gradient
    entry + 1e-5 of the largest gradient norm.

    MEASURED (MI355X): phiseg at Cx = 2 and 3 and prob_unet2D at Cx = 2 (worst error / bound 0.41) hold both bounds.  prob_unet2D at
    Cx = 3 holds every loss term and 189 of 190 gradients and MISSES the gradient bound on one variable,
    likelihood/encoder/conv_0_1/batch_norm/BatchNorm/gamma: error 5.85 - 6.04 against a bound of 3.56 (1.70x; largest entry 117).  The
    same body at Cx = 1 -- the launches the engine always made, none of the new kernels -- misses it on 40-odd variables of the
    likelihood's encoder, worst 6.0x (likelihood/encoder/conv_3_3/W): the bound of the three-latent-level PHiSeg family never fit this
    one-latent-level U-Net at n0 = 4 in fp32 (sums of three or four channels in batch-norm gradients that cancel), with or without
    extra channels.  The bound stays as the issue sets it and the prob_unet2D case is left failing."""
    check_loss_terms_and_gradients(arch, Cx)


def test_three_adam_steps_match_oracle_fp32():
    """eager, hipGraph capture, hipGraph replay against the oracle's TF1-form Adam, by the rule of the test of the same name in
    tests/test_model_gpu.py (lr = 1e-5: a weight whose gradient is round-off-sized may differ by 2 lr per step, no more than 1 % do)"""
    lr, Cx = 1e-5, 3
    model, cfg, params, x_np, s_np = build(Cx, perturbed=True)
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
    print("Cx=3 three Adam steps: %d of %d elements off by more than 0.1 lr" % (n_off, n_all))
    assert n_moved > 0.5 * n_all * 0.5
    assert n_off <= 0.01 * n_all, (n_off, n_all)
    assert int(model.sess.store.step.cpu()[0]) == 3


def test_sampling_softmax_and_eval_xent_match_oracle_fp32():
    """PHiSeg, Cx = 3: s_out_eval_sm and eval_xent against oracle.nets.sample: 1e-4 of the largest reference value"""
    model, cfg, params, x_np, s_np = build(3)
    with torch.no_grad():
        ref = nets.sample(params, torch.as_tensor(x_np, dtype=torch.float64), otrain.torch_eps_fn(EPS_SEED, 0, B), cfg)
    sm, xe = model.sess.run([model.s_out_eval_sm, model.eval_xent], {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: False})
    r_sm = ref["s_out_eval_sm"].numpy()
    lg = ref["s_out_eval"]
    r_xe = (torch.logsumexp(lg, dim=-1) - lg.gather(-1, torch.as_tensor(s_np).long()[..., None])[..., 0]).numpy()
    for name, got, r in (("s_out_eval_sm", sm, r_sm), ("eval_xent", xe, r_xe)):
        err = np.abs(got - r).max() / np.abs(r).max()
        print("Cx=3 %s rel-to-max error %.3e" % (name, err))
        assert got.shape == r.shape and err <= 1e-4, (name, err)


def test_probunet_one_pass_sampling_matches_oracle_fp32():
    """prob_unet2D, Cx = 3, through sampling_graph(4) (the one-pass chain: the U-Net once per image): the soft-max of the 2 x 4 rows
    against oracle.nets.sample on np.repeat(x, 4, 0), 1e-4 of the largest reference value"""
    n = 4
    model, cfg, params, x_np, s_np = build(3, arch="prob_unet2D", perturbed=True)
    xt = np.repeat(x_np, n, axis=0)
    with torch.no_grad():
        ref = nets.sample(params, torch.as_tensor(xt, dtype=torch.float64), otrain.torch_eps_fn(EPS_SEED, 0, B * n), dict(cfg, B=B * n))
    sm = model.sess.run(model.sampling_graph(n)[1], {model.training_pl: False, model.x_inp: x_np})
    r = ref["s_out_eval_sm"].numpy()
    err = np.abs(sm - r).max() / np.abs(r).max()
    print("prob_unet2D Cx=3 sampling_graph(4) s_out_eval_sm rel-to-max error %.3e" % err)
    assert sm.shape == r.shape and err <= 1e-4, err
    assert np.abs(sm[0] - sm[1]).max() > 1e-6


def test_bf16_path_three_channels():
    """bf16 storage at Cx = 3 by the rule of test_bf16_path_19_classes: the HIP logits of every level sit within 2x the distance between
    the exact float64 oracle and the oracle with bf16 storage simulated (floor 0.5 % of the logit range), of BOTH oracles; every ELBO term
    within max(5 %, 2.5x what the simulated storage moves it, for a KL level 1.5x the largest such move of any KL level)"""
    model, cfg, params, x_np, s_np = build(3, "bf16")
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
        print("Cx=3 bf16 level %d: RMS/max vs simulated %.4f, vs exact %.4f, simulated vs exact %.4f" % (l, rms(sim, l), rms(exact, l), inherent))
        assert rms(sim, l) < bound and rms(exact, l) < bound, (l, rms(sim, l), rms(exact, l), inherent)
    inh = {k: abs(float(sim["loss_dict"][k]) - float(exact["loss_dict"][k])) / abs(float(exact["loss_dict"][k])) for k in keys}
    kl_inh = max([v for k, v in inh.items() if k.startswith("KL_")] or [0.0])
    for k, v in zip(keys, losses):
        ex = float(exact["loss_dict"][k])
        print("Cx=3 bf16 %-36s exact %.4e HIP %+.2f%% simulated %+.2f%%" % (k, ex, 100 * (float(v) - ex) / ex, 100 * inh[k]))
        np.testing.assert_allclose(float(v), ex, rtol=max(0.05, 2.5 * inh[k], 1.5 * kl_inh if k.startswith("KL_") else 0.0), err_msg=k)


def _digest(Cx, dtype, steps):
    env = dict(os.environ, PYTHONPATH=ROOT, PHX_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multichannel_model_worker.py"), str(Cx), dtype, str(steps)], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DIGEST")][-1].split()
    return line[1], float(line[2])


def test_captured_plan_is_bit_identical_in_deterministic_mode():
    """PHX_DETERMINISTIC=1, Cx = 3, fp32: four training steps (eager, capture, two replays) in two processes give the same digest of
    every loss term, gradient and parameter"""
    a, b = _digest(3, "f32", 4), _digest(3, "f32", 4)
    assert np.isfinite(a[1]) and a == b, (a, b)


SWITCHES = ["PHX_XF", "PHX_DUAL", "PHX_UPCONV", "PHX_HIP_GRAPH"]


@pytest.mark.parametrize("switch", SWITCHES)
def test_plan_rewrites_off_give_the_same_loss_terms(switch, monkeypatch):
    """each default-on plan rewrite at 0 against the default plan, Cx = 3, fp32, same weights, inputs and noise: every loss term agrees
    within the fp32 bound of this file (rtol 5e-4)"""
    res = {}
    for v in (None, "0"):
        if v is None:
            monkeypatch.delenv(switch, raising=False)
        else:
            monkeypatch.setenv(switch, v)
        model, cfg, params, x_np, s_np = build(3, "f32", perturbed=True)
        keys = sorted(model.loss_dict)
        fd = {model.x_inp: x_np, model.s_inp: s_np, model.training_pl: True}
        model.sess.run([model.loss_dict[k] for k in keys], fd)
        res[v] = [float(t) for t in model.sess.run([model.loss_dict[k] for k in keys], fd)]       # (the second run: a replay)
    for k, a, b in zip(keys, res[None], res["0"]):
        print("%s=0 f32 %-36s default %.6f off %.6f" % (switch, k, a, b))
        np.testing.assert_allclose(b, a, rtol=5e-4, err_msg=k)


def _model_and_data(Cx=3, n_validation=3):
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = config(Cx)
    cfg.validation_samples, cfg.num_validation_images = 6, n_validation
    data = synthetic.SyntheticLIDC(cfg, seed=5, n_validation=n_validation)
    return phiseg_model.phiseg(cfg, rng_seed=3), cfg, data


def test_train_with_image_summaries_and_validation_pass(tmp_path):
    """train(SyntheticLIDC, num_iter=2, summaries=True) with do_image_summaries runs; train_x_inp/image/0 of the event file is a
    three-channel PNG of the grid shape holding the grid of the batch; one validation pass scores what the oracle scores on the samples
    it drew (GED and Dice 1e-6, NCC 2e-5, as test_train_two_steps_and_validation_pass_nine_classes)"""
    from PIL import Image
    from phiseg_code_amd import summary as S
    model, cfg, data = _model_and_data()
    cfg.batch_size, cfg.do_image_summaries, cfg.tensorboard_update_frequency, cfg.validation_frequency = 2, True, 1, 2
    cfg.annotator_range, cfg.lr_schedule_dict = range(4), {0: 1e-3}
    log_dir = str(tmp_path / "run")
    losses = model.train(data, num_iter=2, log_every=0, log_dir=log_dir, summaries=True)
    assert int(model.sess.store.step.cpu()[0]) == 2 and np.isfinite(np.asarray(losses, dtype=np.float64)).all()
    files = [f for f in os.listdir(log_dir) if f.startswith("events.out.tfevents.")]
    assert len(files) == 1
    images = {}
    for ev in S.read_events(os.path.join(log_dir, files[0])):
        for v in ev["values"]:
            if "image" in v:
                images.setdefault(v["tag"], v["image"])
    gy, gx = S.factorization(2)
    for tag in ("train_x_inp/image/0", "val_x_inp/image/0", "generated_x_in/image/0"):
        im = images[tag]
        assert (im["height"], im["width"], im["colorspace"]) == ((H + 2) * gy, (H + 2) * gx, 3), (tag, im["height"], im["width"], im["colorspace"])
        pix = np.asarray(Image.open(io.BytesIO(im["png"])))
        assert pix.shape == ((H + 2) * gy, (H + 2) * gx, 3) and pix.max() >= 253 and len(np.unique(pix)) > 100
        assert not np.array_equal(pix[..., 0], pix[..., 1]) and not pix[0].any() and not pix[:, 0].any()
    assert images["train_s_inp/image/0"]["colorspace"] == 1
    np.random.seed(0)
    res = model._do_validation(data)
    assert np.isfinite([res["loss"], res["dice"], res["ged"], res["ncc"]]).all()
    np.random.seed(0)
    model.sess.store.noise_step -= cfg.num_validation_images
    geds, nccs, dices = [], [], []
    for ii in range(cfg.num_validation_images):
        s_gt = data.validation.labels[ii]
        s = s_gt[:, :, np.random.choice(cfg.annotator_range)]
        x_b = np.tile(data.validation.images[ii][None], [cfg.validation_samples, 1, 1, 1])
        assert x_b.shape == (cfg.validation_samples, H, H, 3)
        sm = model.predict_segmentation_sample(x_b, return_softmax=True)
        g, n, d = om.validation_metrics(sm, np.ascontiguousarray(s_gt.transpose(2, 0, 1)), s, NL)
        geds.append(g); nccs.append(n); dices.append(d)
    np.testing.assert_allclose(res["ged"], np.mean(geds), atol=1e-6)
    np.testing.assert_allclose(res["ncc"], np.mean(nccs), atol=2e-5)
    np.testing.assert_allclose(res["per_structure_dice"], np.mean(dices, axis=0), atol=1e-6)


def test_two_channel_summary_shows_channel_zero_in_grey():
    from phiseg_code_amd import summary as S
    from tests.test_summary_gpu import _ref_grid
    x = inputs(2, 6)[0]
    x[0, 0, 0, 0], x[5, 3, 3, 0] = -0.75, 0.875                   # channel 0 holds the extrema: _ref_grid's own reduction is the tensor's
    t = torch.as_tensor(x).cuda()
    st = torch.cuda.current_stream()
    g = S.grid_image_device(t.data_ptr(), 6, H, H, 2, st.cuda_stream)
    st.synchronize()
    want, _ = _ref_grid(x[..., 0])
    assert g.dim() == 2 and np.array_equal(g.cpu().numpy(), want[0, :, :, 0])


def test_train_on_a_device_resident_three_channel_data_set():
    """phiseg.train(data) on a device-resident three-channel data set with rotation, crop-scale and the elastic deformation switched on:
    the steps consume batches that went through phx_augment_batch_mc, and such a batch matches the restatement per channel"""
    from phiseg_code_amd.data import augment as pa
    from phiseg_code_amd.phiseg import phiseg_model
    from tests import elastic_ref as er
    from tests.test_multichannel_kernels_gpu import _data
    cfg = config(3)
    cfg.batch_size, cfg.annotator_range, cfg.num_labels_per_subject = 2, range(4), 4
    cfg.lr_schedule_dict = {0: 1e-3}
    cfg.augmentation_options = dict(do_rotations=True, do_scaleaug=True, do_elasticaug=True, nlabels=NL, augment_every_nth=1)
    parts = {sp: _data(n, H, H, 3, NL, 4, 40 + n) for sp, n in (("train", 4), ("val", 2))}
    data = pa.lidc_data(cfg, {sp: dict(images=i, labels=l) for sp, (i, l) in parts.items()}, seed=5)
    assert data.train.channels == 3 and data.validation.images.shape == (2, H, H, 3)
    model = phiseg_model.phiseg(cfg)
    losses = model.train(data, num_iter=2, log_every=0)
    assert len(losses) == 2 and np.all(np.isfinite(losses)) and data.train.step == 2
    x, s = data.train.next_batch(2)
    assert x.shape == (2, H, H, 3)
    for j, (d, src, an) in enumerate(zip(data.train.last_decisions, data.train.last_indices, data.train.last_annotators)):
        assert d["elastic"] is not None
        for c in range(3):
            ref_x, ref_s = er.augment_pair_elastic(parts["train"][0][src, ..., c], parts["train"][1][src, ..., an], d, NL)
            assert np.array_equal(s[j], ref_s)
            np.testing.assert_allclose(x[j, ..., c], ref_x, rtol=0, atol=1e-6)
            assert not np.array_equal(x[j, ..., c], parts["train"][0][src, ..., c])


def test_evaluate_split_equals_the_per_image_path():
    """evaluate_split at Cx = 3 against the per-image path (utils.validation_metrics) and the oracle on the same samples, fetched again"""
    from phiseg_code_amd import evaluate, utils
    model, cfg, data = _model_and_data()
    n, split = 6, data.validation
    store = model.sess._ensure_store()
    step0 = int(store.noise_step.cpu().item())
    np.random.seed(0)
    res = evaluate.evaluate_split(model, split, n, images_per_pass=2)
    assert res["dice"].shape[0] == 3 and int(store.noise_step.cpu().item()) == step0 + 2
    store.noise_step.fill_(step0)
    torch.cuda.synchronize()
    sm_t = model.sampling_graph(n)[1]
    row = 0
    for i0, b in [(0, 2), (2, 1)]:
        x = split.images[i0:i0 + b]
        sm = model.sess.run(sm_t, {model.training_pl: False, model.x_inp: x})
        model._advance_noise()
        sm = sm.reshape((b, n) + sm.shape[1:])
        for k in range(b):
            gts = np.ascontiguousarray(split.labels[i0 + k].transpose(2, 0, 1))
            ref = gts[res["sref_annot"][row]]
            ged, ncc, dice = utils.validation_metrics(sm[k][None], gts[None], ref[None], NL)
            o_ged, o_ncc, o_dice = om.validation_metrics(sm[k], gts, ref, NL)
            np.testing.assert_allclose([res["ged"][row], ged[0]], o_ged, rtol=0, atol=1e-6)
            np.testing.assert_allclose([res["ncc"][row], ncc[0]], o_ncc, rtol=0, atol=2e-5)
            np.testing.assert_allclose(res["dice"][row][:NL], o_dice, rtol=0, atol=1e-6)
            row += 1


def test_checkpoint_round_trip_and_uncertainty_maps(tmp_path):
    """save_weights then load_weights into a fresh three-channel model gives the same sample; predict_mean_variance_and_error_maps
    returns finite [X, Y] maps"""
    from phiseg_code_amd.phiseg import phiseg_model
    model, cfg, params, x_np, s_np = build(3, perturbed=True)
    fd = {model.x_inp: x_np, model.training_pl: False}
    a = model.sess.run(model.s_out_eval_sm, fd)
    path = str(tmp_path / "model.ckpt-0")
    model.save_weights(path)
    fresh = phiseg_model.phiseg(config(3), rng_seed=EPS_SEED)
    fresh.load_weights(path)
    b = fresh.sess.run(fresh.s_out_eval_sm, {fresh.x_inp: x_np, fresh.training_pl: False})
    assert np.array_equal(a, b)
    am, std, err = model.predict_mean_variance_and_error_maps(s_np[:1], x_np[:1], 4)
    for m in (am, std, err):
        m = np.asarray(m)
        assert m.shape == (H, H) and np.isfinite(m.astype(np.float64)).all()
