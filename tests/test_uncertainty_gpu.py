"""Per-pixel Monte-Carlo maps on the MI355X (phx_mc_stats, phiseg_code_amd/uncertainty.py, the model class's Monte-Carlo methods)
against the fixture written by the reference's own code and against the numpy restatement of tests/uncertainty_ref.py.

The rule for every plane: max |device - golden| <= 4 * max(err_ref32, 2^-23 * max |golden|), err_ref32 being the error of the
restatement run in float32 -- the reference's own working precision -- against the same golden (uncertainty_ref.band).  COV_DET of
soft-max inputs is the determinant of a singular matrix, rounding noise in the reference too: there Hadamard's inequality
|det| <= prod_c var_c is asserted, and the determinant code is pinned by COV_DET_DROP_LAST and by COV_DET of un-normalised inputs."""
import importlib
import os
import types

import numpy as np
import pytest

from tests import uncertainty_ref as U
from tests.helpers import GOLDEN_DIR, load_golden
from tests.test_graph_cpu import make_config

pytestmark = pytest.mark.gpu


def _check(tag, name, dev, golden, ref32):
    tol, err_ref32 = U.band(golden, ref32)
    err_dev = float(np.abs(np.asarray(dev, dtype=np.float64) - golden).max())
    print("%s %-18s max|golden| %.3e  err_dev %.3e  err_ref32 %.3e  band %.3e" % (tag, name, np.abs(golden).max(), err_dev, err_ref32, tol))
    assert err_dev <= tol, (tag, name, err_dev, err_ref32, tol)


def _hadamard(tag, dev, var1):
    bound = np.prod(var1, axis=-1) * (1 + 1e-6)
    bad = int((np.abs(np.asarray(dev, dtype=np.float64)) > bound).sum())
    print("%s cov_det (singular)  max|device| %.3e  max bound %.3e  violations %d" % (tag, np.abs(dev).max(), bound.max(), bad))
    assert bad == 0, (tag, bad)


@pytest.mark.parametrize("k", range(len(U.CASES)))
def test_kernel_matches_reference_goldens(k):
    from phiseg_code_amd import uncertainty as unc
    gold = np.load(os.path.join(GOLDEN_DIR, "uncertainty_cases.npz"))
    logits, sm, gts, s_ref = U.uncertainty_case(k)
    r64 = U.reference_maps(logits, sm, gts, s_ref, np.float64)
    r32 = U.reference_maps(logits, sm, gts, s_ref, np.float32)
    dev = unc.mc_statistics(logits=logits, sm=sm, gts=gts, s_ref=s_ref)
    assert set(U.MAPS) <= set(dev)
    tag = "case %d" % k
    for name in U.MAPS:
        assert dev[name].shape == sm.shape[1:3] and dev[name].dtype == np.float32
        if name == "cov_det":
            _hadamard(tag, dev[name], r64["var1"])
        else:
            _check(tag, name, dev[name], gold["%d/%s" % (k, name)], r32[name])
    _check(tag, "mean_sm", dev["mean_sm"], r64["mean_sm"], r32["mean_sm"])
    m = np.sort(r64["mean_sm"], axis=-1)
    clear = (m[..., -1] - m[..., -2]) > 1e-6
    assert (dev["argmax"][clear] == gold["%d/argmax" % k][clear]).all()
    # the determinant on a well-conditioned matrix: un-normalised samples, replayed through the reference's _bf method
    _, smu, _, _ = U.uncertainty_case(k, unnormalised=True)
    du = unc.mc_statistics(sm=smu, maps=("cov_det",), mean=False)
    _check(tag, "cov_det (unnorm.)", du["cov_det"], gold["%d/cov_det_unnormalised" % k], U.reference_maps(logits, smu, gts, s_ref, np.float32)["cov_det"])
    # the reference's own entry point of the error maps
    e_ss, e_sy, e_yy = unc.generate_error_maps(sm, np.eye(sm.shape[-1], dtype=np.float32)[gts])
    for name, v in (("e_ss", e_ss), ("e_sy", e_sy), ("e_yy", e_yy)):
        np.testing.assert_array_equal(v, dev[name])


def test_kernel_lidc_shape_batch_of_images():
    """I = 3, N = 100, M = 4, 128 x 128, C = 2 (the inputs of test_device_metrics_batch_of_images_lidc_shape) against the float64
    restatement: the oracle forms E_ss / E_sy only inside variance_ncc and does not expose them."""
    from phiseg_code_amd import uncertainty as unc
    logits, sm, gts, s_ref = U.lidc_case()
    dev = unc.mc_statistics(logits=logits, sm=sm, gts=gts, s_ref=s_ref)
    for i in range(sm.shape[0]):
        r64 = U.reference_maps(logits[i], sm[i], gts[i], s_ref[i], np.float64)
        r32 = U.reference_maps(logits[i], sm[i], gts[i], s_ref[i], np.float32)
        for name in U.MAPS:
            assert dev[name].shape == (3, 128, 128)
            if name == "cov_det":
                _hadamard("lidc %d" % i, dev[name][i], r64["var1"])
            else:
                _check("lidc %d" % i, name, dev[name][i], r64[name], r32[name])


def test_map_without_its_input_is_an_error():
    from phiseg_code_amd import runtime as rt
    from phiseg_code_amd import uncertainty as unc
    logits, sm, gts, s_ref = U.uncertainty_case(3)
    with pytest.raises(rt.PhxError):
        unc.mc_statistics(sm=sm, maps=("xent_mean",))                 # no logits, no s_ref
    with pytest.raises(rt.PhxError):
        unc.mc_statistics(logits=logits, s_ref=s_ref, maps=("std_mean",))
    with pytest.raises(rt.PhxError):
        unc.mc_statistics(sm=sm, maps=("e_sy",))                      # no annotations
    with pytest.raises(ValueError):
        unc.mc_statistics(sm=sm[:2], gts=np.stack([gts[0]] * 3), maps=("e_yy",))      # N < M
    with pytest.raises(ValueError):
        unc.generate_error_maps(sm[:1], np.eye(2, dtype=np.float32)[gts])


# ---- model level ----------------------------------------------------------------------------------------------------------------
def _tiny(dtype):
    from phiseg_code_amd.phiseg import phiseg_model
    import torch
    from tests.helpers import golden_inputs
    g, cfg, var_order = load_golden("tiny_phiseg_bn")
    model = phiseg_model.phiseg(make_config(cfg, dtype), rng_seed=cfg["eps_seed"])
    params, x_np, s_np = golden_inputs(cfg, var_order, dtype=torch.float64)
    model.set_weights({k: v.detach().numpy() for k, v in params.items()})
    return model, x_np[:1], s_np[:1], 8


def _lidc(dtype):
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    base = importlib.import_module("phiseg_code_amd.phiseg.experiments.phiseg_7_5")
    cfg = types.SimpleNamespace(**{k: getattr(base, k) for k in dir(base) if not k.startswith("_")})
    cfg.compute_dtype = dtype
    data = synthetic.SyntheticLIDC(cfg, seed=5, n_validation=2)
    model = phiseg_model.phiseg(cfg, rng_seed=3)
    x = data.validation.images[0].reshape((1,) + tuple(cfg.image_size)).astype(np.float32)
    s = data.validation.labels[0][:, :, 0][None].astype(np.uint8)
    return model, x, s, 16


def _replay(model, tensors, fd):
    """sess.run with the noise of the previous Monte-Carlo call: the step is rewound for the run and put back after it."""
    from phiseg_code_amd import engine
    model.sess.store.noise_step -= 1
    engine.device_sync()
    out = model.sess.run(tensors, fd)
    model.sess.store.noise_step += 1
    engine.device_sync()
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("make", [_tiny, _lidc])
def test_model_monte_carlo_methods_match_restatement(make, dtype, monkeypatch):
    """Every Monte-Carlo method equals the restatement applied to the logits / soft-max that sess.run fetches from the SAME graph
    instance with the noise step rewound; fresh noise per call; nothing but the maps crosses to the host (Plan.fetch is never
    called during a method)."""
    from phiseg_code_amd import engine
    model, x, s, n = make(dtype)
    lg_t, sm_t = model.sampling_graph(n)                   # (both nets have the 'phiseg' prior: the one-pass instance)
    fd = {model.training_pl: False, model.x_inp: x}
    calls = []
    real_fetch = engine.Plan.fetch

    def counting_fetch(self, t):
        calls.append(t)
        return real_fetch(self, t)
    monkeypatch.setattr(engine.Plan, "fetch", counting_fetch)
    tag = "%s/%s" % (make.__name__, dtype)

    def restate(lg, sm):
        lg = lg if lg is not None else np.zeros_like(sm)
        sm = sm if sm is not None else np.full_like(lg, 1.0 / lg.shape[-1])
        gts = s.astype(np.uint8)
        return U.reference_maps(lg, sm, gts, s[0], np.float64), U.reference_maps(lg, sm, gts, s[0], np.float32)

    # predict_mean_variance_and_error_maps: fetches [logits, soft-max]
    means, var, err = model.predict_mean_variance_and_error_maps(s, x, n)
    assert not calls
    lg, sm = _replay(model, [lg_t, sm_t], fd)
    assert len(calls) == 2 and lg.shape == (n,) + x.shape[1:3] + (2,)
    r64, r32 = restate(lg, sm)
    assert means.shape == var.shape == err.shape == x.shape[1:3]
    _check(tag, "std_mean", var, r64["std_mean"], r32["std_mean"])
    _check(tag, "xent_mean", err, r64["xent_mean"], r32["xent_mean"])
    m = np.sort(r64["mean_sm"], axis=-1)
    clear = (m[..., -1] - m[..., -2]) > 1e-6
    assert (means[clear] == r64["argmax"][clear]).all()
    means2, var2, err2 = model.predict_mean_variance_and_error_maps(s, x, n)          # fresh noise
    assert np.abs(var2 - var).max() > 0 and np.abs(err2 - err).max() > 0

    # get_crossentropy_error_map: fetches [logits]; [B, X, Y] like the reference
    del calls[:]
    xe = model.get_crossentropy_error_map(s, x, n)
    assert not calls and xe.shape == (1,) + x.shape[1:3]
    lg = _replay(model, [lg_t], fd)[0]
    r64, r32 = restate(lg, None)
    _check(tag, "xent_mean (own)", xe[0], r64["xent_mean"], r32["xent_mean"])

    # the two variance methods
    del calls[:]
    tr = model.predict_segmentation_sample_variance_sm_cov(x, n)
    assert not calls
    lg = _replay(model, [lg_t], fd)[0]
    r64, r32 = restate(lg, None)
    _check(tag, "cov_trace", tr, r64["cov_trace"], r32["cov_trace"])
    del calls[:]
    det = model.predict_segmentation_sample_variance_sm_cov_bf(x, n)
    assert not calls
    sm = _replay(model, [sm_t], fd)[0]
    r64, r32 = restate(None, sm)
    _hadamard(tag, det, r64["var1"])
    del calls[:]
    det1 = model.predict_segmentation_sample_variance_sm_cov_bf(x, n, drop_last_class=True)
    assert not calls
    sm = _replay(model, [sm_t], fd)[0]
    r64, r32 = restate(None, sm)
    _check(tag, "cov_det_drop_last", det1, r64["cov_det_drop_last"], r32["cov_det_drop_last"])
    assert np.abs(model.predict_segmentation_sample_variance_sm_cov(x, n) - tr).max() > 0


def test_tiled_route_of_a_prior_without_shared_encoder():
    """prob_unet2D draws z per image: the Monte-Carlo methods tile x on s_out_eval; checked against that instance."""
    import torch
    from phiseg_code_amd.phiseg import phiseg_model
    from tests.helpers import golden_inputs
    g, cfg, var_order = load_golden("tiny_probunet_bn")
    model = phiseg_model.phiseg(make_config(cfg, "f32"), rng_seed=cfg["eps_seed"])
    params, x_np, s_np = golden_inputs(cfg, var_order, dtype=torch.float64)
    model.set_weights({k: v.detach().numpy() for k, v in params.items()})
    x, s, n = x_np[:2], s_np[:2], 6
    means, var, err = model.predict_mean_variance_and_error_maps(s, x, n)
    assert means.shape == var.shape == err.shape == (2,) + x.shape[1:3]                # B > 1: [B, X, Y]
    lg, sm = _replay(model, [model.s_out_eval, model.s_out_eval_sm], {model.training_pl: False, model.x_inp: np.repeat(x, n, axis=0)})
    for b in range(2):
        sl = slice(b * n, (b + 1) * n)
        r64 = U.reference_maps(lg[sl], sm[sl], s[b:b + 1], s[b], np.float64)
        r32 = U.reference_maps(lg[sl], sm[sl], s[b:b + 1], s[b], np.float32)
        _check("probunet %d" % b, "std_mean", var[b], r64["std_mean"], r32["std_mean"])
        _check("probunet %d" % b, "xent_mean", err[b], r64["xent_mean"], r32["xent_mean"])


def test_eval_xent_tensor():
    """model.eval_xent (added to the graph on first use) is the per-pixel cross entropy of s_out_eval against s_inp."""
    model, x, s, _ = _tiny("f32")
    xe, lg = model.sess.run([model.eval_xent, model.s_out_eval], {model.training_pl: False, model.x_inp: x, model.s_inp: s})
    lg = lg.astype(np.float64)
    mx = lg.max(axis=-1, keepdims=True)
    ref = mx[..., 0] + np.log(np.exp(lg - mx).sum(axis=-1)) - np.take_along_axis(lg, s.astype(np.int64)[..., None], axis=-1)[..., 0]
    assert xe.shape == ref.shape
    np.testing.assert_allclose(xe, ref, rtol=0, atol=4 * 2.0 ** -23 * max(np.abs(lg).max(), 1.0))
    sml = model.sess.run(model.s_out_eval_sm_list, {model.training_pl: False, model.x_inp: x})
    assert len(sml) == len(model.s_out_eval_list) and all(abs(v.sum(axis=-1) - 1).max() < 1e-5 for v in sml)


def test_mc_statistics_on_plan_buffers_equals_host_arrays():
    """mc_statistics takes the engine's device buffers (Session.run_buffers) as they are: same maps as from the fetched host copies."""
    from phiseg_code_amd import uncertainty as unc
    model, x, s, n = _tiny("f32")
    lg_t, sm_t = model.sampling_graph(n)
    fd = {model.training_pl: False, model.x_inp: np.concatenate([x, x[:, ::-1]])}              # two images
    plan, (lg_b, sm_b) = model.sess.run_buffers([lg_t, sm_t], fd)
    gts = np.stack([s, 1 - s], axis=0).reshape(2, 1, *s.shape[1:]).astype(np.uint8)
    dev = unc.mc_statistics(logits=lg_b, sm=sm_b, gts=gts, s_ref=gts[:, 0], num_samples=n, stream=plan.stream)
    lg, sm = plan.fetch(lg_t), plan.fetch(sm_t)
    host = unc.mc_statistics(logits=lg.reshape((2, n) + lg.shape[1:]), sm=sm.reshape((2, n) + sm.shape[1:]), gts=gts, s_ref=gts[:, 0])
    assert set(dev) == set(host) and set(U.MAPS) <= set(dev)
    for name in dev:
        assert dev[name].shape == host[name].shape and dev[name].shape[0] == 2
        np.testing.assert_array_equal(dev[name], host[name], err_msg=name)
    with pytest.raises(ValueError):
        unc.mc_statistics(sm=sm_b)                                                            # device buffers need num_samples + stream
