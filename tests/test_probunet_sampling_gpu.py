"""One-pass sampling of the Probabilistic U-Net on the MI355X: model.sampling_graph(n) runs the prior encoder and the likelihood's U-Net
once per image and only the recombination layers per sample -- on the existing kernels (the generic route) or, where the lowering
recognises the chain, as ONE phx_recomb_samples launch (the fused route).  Reference: oracle.nets.sample in float64 on the
reference's own batching, np.repeat(x, n, 0), with the same Philox noise per (image, sample) row.  The one-pass routes are held
against the error of the tiled route (s_out_eval on the tiled batch, what predict / the Monte-Carlo methods do without
exp_config.one_pass_sampling) measured against the same oracle in the same test."""
import numpy as np
import pytest
import torch

from oracle import init as oinit
from oracle import nets
from oracle import train as otrain
from tests import uncertainty_ref as U
from tests.helpers import golden_inputs, load_golden
from tests.test_graph_cpu import make_config

pytestmark = pytest.mark.gpu

ENTRY = "phx_recomb_samples"
N32 = dict(arch="prob_unet2D", norm="batch_norm", n0=32, zdim0=6, H=64, B=2, nlabels=2, latent_levels=1, resolution_levels=6,
           image_size=(64, 64, 1), KL_weight=1.0, CE_weight=1.0, exponential_weighting=True)
N_SAMPLES = 5


def _launch_names(plan):
    return [getattr(fn, "__name__", repr(fn)) for fn, _ in plan.launches]          # what tools/dump_launches.py prints


def _n32_model(norm, dtype, one_pass=False):
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = dict(N32, norm=norm)
    c = make_config(cfg, dtype)
    if one_pass:
        c.one_pass_sampling = True
    model = phiseg_model.phiseg(c, rng_seed=42)
    var_order = [(nm, v.shape) for nm, v in model.graph.variables.items()]
    params = otrain.make_params(var_order, 0, torch.float64, perturbed=True)
    model.set_weights({k: v.detach().numpy() for k, v in params.items()})
    return model, cfg, params


@pytest.fixture(scope="module")
def n32_oracle():
    """norm -> (x [2, 64, 64, 1], float64 oracle logits and soft-max of the 2 x 5 rows); computed once per normalisation."""
    cache = {}

    def get(norm):
        if norm not in cache:
            _, cfg, params = _n32_model(norm, "f32")
            x, _ = oinit.synthetic_batch(2, 64, 2, 1234)
            xt = np.repeat(x, N_SAMPLES, axis=0)
            with torch.no_grad():
                ref = nets.sample(params, torch.as_tensor(xt, dtype=torch.float64), otrain.torch_eps_fn(42, 0, xt.shape[0]), dict(cfg, B=xt.shape[0]))
            r, rsm = ref["s_out_eval"].numpy(), ref["s_out_eval_sm"].numpy()
            r.setflags(write=False)
            rsm.setflags(write=False)
            cache[norm] = (x, r, rsm)
        return cache[norm]
    return get


def _both_routes(model, x, n):
    """-> (one-pass logits, tiled-route logits, the one-pass plan), both [B n, X, Y, C], at noise step 0"""
    lg_t, sm_t = model.sampling_graph(n)
    fd = {model.training_pl: False, model.x_inp: x}
    one = model.sess.run(lg_t, fd)
    tiled = model.sess.run(model.s_out_eval, {model.training_pl: False, model.x_inp: np.repeat(x, n, axis=0)})
    return one, tiled, model.sess.plan_for([lg_t], False, x.shape[0], False)


def _fp32_criterion(tag, one, tiled, ref):
    err_one, err_tiled = np.abs(one - ref).max(), np.abs(tiled - ref).max()
    print("%s fp32: err_one_pass %.3e  err_tiled %.3e  max|ref| %.3f" % (tag, err_one, err_tiled, np.abs(ref).max()))
    assert err_one <= 2 * err_tiled + 2.0 ** -23 * np.abs(ref).max()


def _bf16_criterion(tag, one, tiled, ref, ref_sm):
    rms = lambda a: float(np.sqrt(((a - ref) ** 2).mean()))
    r_one, r_tiled, rng = rms(one), rms(tiled), float(np.abs(ref).max())
    agree = float((one.argmax(-1) == ref_sm.argmax(-1)).mean())
    print("%s bf16: RMS one-pass %.4e  RMS tiled %.4e  ratio %.3f  of the logit range %.4f  arg-max agreement %.4f"
          % (tag, r_one, r_tiled, r_one / r_tiled, r_one / rng, agree))
    assert r_one <= 1.5 * r_tiled
    assert r_one <= 0.03 * rng
    assert agree > 0.97


def test_tiny_probunet_sampling_graph_rows_and_oracle_fp32():
    """n0 = 4: the chain is 4 wide, the lowering keeps the generic route."""
    from phiseg_code_amd.phiseg import phiseg_model
    g, cfg, var_order = load_golden("tiny_probunet_bn")
    model = phiseg_model.phiseg(make_config(cfg, "f32"), rng_seed=cfg["eps_seed"])
    params, x_np, _ = golden_inputs(cfg, var_order, dtype=torch.float64)
    model.set_weights({k: v.detach().numpy() for k, v in params.items()})
    n, x = 3, x_np[:2]
    one, tiled, plan = _both_routes(model, x, n)
    assert one.shape == (2 * n,) + x.shape[1:3] + (cfg["nlabels"],)
    assert np.abs(one[0] - one[1]).max() > 1e-4 and np.abs(one[n] - one[n + 1]).max() > 1e-4      # the samples of an image differ
    assert ENTRY not in _launch_names(plan)
    xt = np.repeat(x, n, axis=0)
    with torch.no_grad():
        ref = nets.sample(params, torch.as_tensor(xt, dtype=torch.float64), otrain.torch_eps_fn(cfg["eps_seed"], 0, 2 * n), dict(cfg, B=2 * n))
    _fp32_criterion("tiny_probunet_bn", one, tiled, ref["s_out_eval"].numpy())


def test_fused_route_launch_list():
    """batch norm, n0 = 32: the entry exactly once, nothing of the chain launched unit by unit."""
    for dtype in ("bf16", "f32"):
        model, cfg, _ = _n32_model("batch_norm", dtype)
        lg_t, sm_t = model.sampling_graph(N_SAMPLES)
        plan = model.sess.plan_for([lg_t, sm_t], False, 2, False)
        names = _launch_names(plan)
        assert names.count(ENTRY) == 1
        i = names.index(ENTRY)
        chain = ("conv", "head1x1", "affine_act", "concat2", "broadcast_pixels", "pad_channels", "repeat_batch", "residual_ce")
        assert not [nm for nm in names[i + 1:] if any(k in nm for k in chain)], names[i + 1:]      # no launch of the chain behind the U-Net
        # mu and sigma ([B, 6]: 24-byte rows go through the broadcast kernel with n "pixels" per row) are the only tensors repeated:
        # neither the feature map nor z over the image
        assert not any("repeat_batch" in nm for nm in names)
        bc = [args for (fn, args), nm in zip(plan.launches, names) if "broadcast_pixels" in nm]
        assert len(bc) == 2 and all(a[3] == 2 and a[4] == N_SAMPLES and a[5] == 6 for a in bc)


def test_fused_route_vs_oracle_fp32(n32_oracle):
    x, ref, _ = n32_oracle("batch_norm")
    model, cfg, _ = _n32_model("batch_norm", "f32")
    one, tiled, plan = _both_routes(model, x, N_SAMPLES)
    assert _launch_names(plan).count(ENTRY) == 1
    assert one.shape == ref.shape and np.abs(one[0] - one[1]).max() > 1e-4
    _fp32_criterion("fused", one, tiled, ref)


def test_fused_route_vs_oracle_bf16(n32_oracle):
    x, ref, ref_sm = n32_oracle("batch_norm")
    model, cfg, _ = _n32_model("batch_norm", "bf16")
    one, tiled, plan = _both_routes(model, x, N_SAMPLES)
    assert _launch_names(plan).count(ENTRY) == 1
    _bf16_criterion("fused", one, tiled, ref, ref_sm)
    assert np.abs(one[0] - one[1]).max() > 1e-3 * np.abs(ref).max()


def test_generic_route_group_norm_bf16(n32_oracle):
    """group norm has no folded scale / shift: the chain stays on the unit-by-unit kernels, at B n rows behind ONE U-Net pass."""
    x, ref, ref_sm = n32_oracle("group_norm")
    model, cfg, _ = _n32_model("group_norm", "bf16")
    one, tiled, plan = _both_routes(model, x, N_SAMPLES)
    names = _launch_names(plan)
    assert ENTRY not in names and any("repeat_batch" in nm for nm in names)                         # the feature map, repeated for the samples
    _bf16_criterion("generic (group norm)", one, tiled, ref, ref_sm)


def _replay(model, tensors, fd):
    """sess.run with the noise of the previous sampling call (the step is rewound for the run and put back after it)"""
    from phiseg_code_amd import engine
    model.sess.store.noise_step -= 1
    engine.device_sync()
    out = model.sess.run(tensors, fd)
    model.sess.store.noise_step += 1
    engine.device_sync()
    return out


def test_model_api_one_pass_sampling(monkeypatch):
    """exp_config.one_pass_sampling = True: predict and the Monte-Carlo map methods go through sampling_graph(n) (here: the fused route,
    soft-max only / logits + soft-max), nothing but the maps crosses to the host, the noise step advances once per call."""
    from phiseg_code_amd import engine
    model, cfg, _ = _n32_model("batch_norm", "f32", one_pass=True)
    x, s = oinit.synthetic_batch(2, 64, 2, 1234)
    n = N_SAMPLES
    lg_t, sm_t = model.sampling_graph(n)
    fd = {model.training_pl: False, model.x_inp: x}
    step = lambda: int(model.sess._ensure_store().noise_step.cpu().item())
    s0 = step()
    seg, sm_mean = model.predict(x, n, return_softmax=True)
    assert step() == s0 + 1
    assert ENTRY in _launch_names(model.sess.plan_for([sm_t], False, 2, False))
    rows = _replay(model, sm_t, fd).astype(np.float64)
    assert rows.shape == (2 * n, 64, 64, 2)
    want = rows.reshape((2, n) + rows.shape[1:]).mean(axis=1)
    assert np.abs(sm_mean - want).max() <= n * 2.0 ** -24
    assert seg.shape == (2, 64, 64) and (seg == sm_mean.argmax(-1)).all()

    calls = []
    real_fetch = engine.Plan.fetch

    def counting_fetch(self, t):
        calls.append(t)
        return real_fetch(self, t)
    monkeypatch.setattr(engine.Plan, "fetch", counting_fetch)
    s1 = step()
    means, var, err = model.predict_mean_variance_and_error_maps(s, x, n)
    assert not calls and step() == s1 + 1
    assert means.shape == var.shape == err.shape == (2, 64, 64)
    lg, sm = _replay(model, [lg_t, sm_t], fd)
    for b in range(2):
        sl = slice(b * n, (b + 1) * n)
        r64 = U.reference_maps(lg[sl], sm[sl], s[b:b + 1], s[b], np.float64)
        r32 = U.reference_maps(lg[sl], sm[sl], s[b:b + 1], s[b], np.float32)
        for name, dev in (("std_mean", var[b]), ("xent_mean", err[b])):
            tol, err_ref32 = U.band(r64[name], r32[name])
            err_dev = float(np.abs(dev.astype(np.float64) - r64[name]).max())
            print("image %d %-10s err_dev %.3e  err_ref32 %.3e  band %.3e" % (b, name, err_dev, err_ref32, tol))
            assert err_dev <= tol


def test_without_the_switch_the_tiled_route_stays():
    model, cfg, _ = _n32_model("batch_norm", "f32")
    assert not model._one_pass_prior()
    x, _ = oinit.synthetic_batch(2, 64, 2, 1234)
    model.predict(x, 2)
    assert not model._multi                                    # no sampling_graph instance was built: the reference's loop ran
