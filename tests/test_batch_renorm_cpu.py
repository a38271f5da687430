"""Batch renormalisation without a GPU: the clipping schedule against hand values, the float64 restatement (tests/renorm_ref.py) against
finite differences and against plain batch norm, and the graph a layer_norm=batch_renorm configuration builds."""
import numpy as np
import pytest

from tests import renorm_ref as R
from tests.helpers import load_golden
from tests.test_graph_cpu import make_config

from phiseg_code_amd.phiseg import phiseg_model
from phiseg_code_amd.tfwrapper import normalisation as tfnorm

SCHEDULE = [(0, 1.0, 0.0), (499, 1.0, 0.0), (500, 1.0, 0.0), (501, 1.0 + 2.0 / 3500.0, 5.0 / 2000.0), (2500, 1.0 + 2000.0 * 2.0 / 3500.0, 5.0),
            (2501, 1.0 + 2001.0 * 2.0 / 3500.0, 5.0), (4000, 3.0, 5.0), (4001, 3.0, 5.0)]


@pytest.mark.parametrize("t, rmax, dmax", SCHEDULE)
def test_clipping_schedule_hand_values(t, rmax, dmax):
    """The reference's parametrize_variable (normalisation.py:82-126) at both ends of both ramps: the host mirror the summaries use
    (an fp32 evaluation, like the device's) and the float64 restatement."""
    assert R.clip_bounds(t) == pytest.approx((rmax, dmax), rel=1e-15, abs=0.0)
    assert tfnorm.renorm_clip(t) == pytest.approx((rmax, dmax), rel=2.0 ** -22, abs=0.0)
    if t in (0, 499, 500, 4000, 4001):
        assert tfnorm.renorm_clip(t) == (rmax, dmax)


def _warm_case(rng, P, C):
    x = 1.5 * rng.standard_normal((P, C)) + rng.standard_normal(C)
    gamma, beta = 1.0 + 0.3 * rng.standard_normal(C), 0.2 * rng.standard_normal(C)
    mu, sigma = x.mean(0), np.sqrt(x.var(0) + 1e-3)
    w = 1.0 - 0.99 ** 300
    state = dict(renorm_mean=w * (mu + 0.7 * sigma * rng.standard_normal(C)), renorm_mean_weight=w,
                 renorm_stddev=w * sigma * np.exp(0.5 * rng.standard_normal(C)), renorm_stddev_weight=w,
                 moving_mean=mu.copy(), moving_variance=sigma ** 2)
    return x, gamma, beta, state


@pytest.mark.parametrize("act", ["identity", "relu"])
def test_reference_backward_matches_central_differences(act):
    """d loss / d(x, gamma, beta) of loss = sum(dy * y), with r and d held at their forward values, against central differences of the
    same function in float64 (step 1e-6: truncation 1e-12, rounding 1e-10 -- bound 1e-7 of the gradient's largest element)."""
    rng = np.random.default_rng(5)
    x, gamma, beta, state = _warm_case(rng, 24, 5)
    t = 1500
    dy = rng.standard_normal(x.shape)
    f0 = R.forward(x, gamma, beta, state, t, act)
    r, d = f0["r"], f0["d"]
    assert np.any(r < 1.0) and np.any(r > 1.0) and np.any(d != 0.0)

    def loss(x_, g_, b_):          # r, d constant: batch moments of x_, the correction of the unperturbed point
        mu = x_.mean(0)
        sg = np.sqrt(((x_ - mu) ** 2).mean(0) + R.EPS)
        return float((dy * R.act_fwd(g_ * ((x_ - mu) / sg * r + d) + b_, act)).sum())
    dx, dgamma, dbeta = R.backward(x, gamma, beta, state, t, dy, act)
    h = 1e-6

    def fd(arr, which):
        out = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            ap, am = arr.copy(), arr.copy()
            ap[i] += h
            am[i] -= h
            args_p = [x, gamma, beta]
            args_m = [x, gamma, beta]
            args_p[which], args_m[which] = ap, am
            out[i] = (loss(*args_p) - loss(*args_m)) / (2 * h)
        return out
    for name, got, want in (("dx", dx, fd(x, 0)), ("dgamma", dgamma, fd(gamma, 1)), ("dbeta", dbeta, fd(beta, 2))):
        err = np.abs(got - want).max() / np.abs(want).max()
        print("%s %s: %.2e" % (act, name, err))
        assert err < 1e-7, (name, err)


def test_reference_with_zero_state_is_plain_batch_norm():
    rng = np.random.default_rng(6)
    x, gamma, beta, _ = _warm_case(rng, 18, 8)
    for t in (0, 100, 1500, 4500):
        f = R.forward(x, gamma, beta, R.fresh_state(8), t, "relu")
        assert np.all(f["r"] == 1.0) and np.all(f["d"] == 0.0), t
        assert np.array_equal(f["y"], R.batch_norm_forward(x, gamma, beta, "relu")), t
    # the first update from a fresh state: the bias-corrected statistics ARE the batch's
    s = R.update(R.fresh_state(8), f["mean"], f["rstd"])
    np.testing.assert_allclose(s["moving_mean"], 0.001 * f["mean"], rtol=1e-12)
    np.testing.assert_allclose(s["moving_variance"], 0.999 + 0.001 * (1.0 / f["rstd"] ** 2 - 1e-3), rtol=1e-12)
    assert s["renorm_mean_weight"] == pytest.approx(0.01, rel=1e-12)


def _models():
    _, cfg, var_order = load_golden("tiny_phiseg_bn")
    bn = phiseg_model.phiseg(make_config(cfg))
    c = make_config(cfg)
    c.layer_norm = tfnorm.batch_renorm
    return bn, phiseg_model.phiseg(c), cfg


def test_renorm_model_builds_with_tf_variable_names():
    bn, rn, _ = _models()
    want = []
    for name, v in bn.graph.variables.items():
        name = name.replace("/batch_norm/", "/batch_renorm/")
        want.append((name, tuple(v.shape), v.trainable))
        if name.endswith("/moving_variance"):
            C, base = v.shape[0], name.rsplit("/", 1)[0]
            want += [(base + "/renorm_mean", (C,), False), (base + "/renorm_mean_weight", (), False),
                     (base + "/renorm_stddev", (C,), False), (base + "/renorm_stddev_weight", (), False)]
    got = [(n, tuple(v.shape), v.trainable) for n, v in rn.graph.variables.items()]
    assert got == want
    assert any("/batch_renorm/BatchNorm/renorm_mean" in n for n, _, _ in got)
    for n, v in rn.graph.variables.items():
        if "/renorm_" in n:
            val = v.initial_value(0)
            assert val.shape == v.shape and val.dtype == np.float32 and not val.any(), n
    count = lambda m: sum(v.size for v in m.graph.variables.values() if v.trainable)
    assert count(rn) == count(bn)


def test_selector_is_recognised_by_identity():
    assert tfnorm.KIND[tfnorm.batch_renorm] == "renorm" and tfnorm.EPS["renorm"] == 1e-3
    with pytest.raises(NotImplementedError):
        tfnorm.batch_renorm(None, training=True)          # applied through layers.conv2D(normalisation=...), like batch_norm


def test_double_update_with_renorm_raises():
    _, cfg, _ = load_golden("tiny_phiseg_bn")
    c = make_config(cfg)
    c.layer_norm = tfnorm.batch_renorm
    with pytest.raises(NotImplementedError, match="bn_double_update"):
        phiseg_model.phiseg(c, bn_double_update=True)
