"""The 3-D layer functions through the engine: the toy 3-D U-Net of tests/volume_net.py as a training plan against torch autograd
of the float64 oracle (tests/volume_ref.py) -- logits, loss, every gradient, the moving statistics with the BIASED variance update of
a rank-5 batch norm --, normalise_post_activation, the inference plan, the bf16 plan against the storage-policy yardstick, and a
worker process for hipGraph capture under PHX_DETERMINISTIC=1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import volume_net as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_against(got, ref, logits_tol=3e-4, loss_rtol=3e-5, grad_tol=3e-3, min_checked=8):
    loss, logits, grads = got
    np.testing.assert_allclose(logits, ref["logits"], rtol=0, atol=logits_tol * float(np.abs(ref["logits"]).max()))
    np.testing.assert_allclose(loss, ref["loss"], rtol=loss_rtol)
    checked = 0
    for n, r in ref["grads"].items():
        if np.abs(r).max() < 1e-9:
            assert np.abs(grads[n]).max() < 1e-4, n
            continue
        np.testing.assert_allclose(grads[n], r, rtol=0, atol=grad_tol * max(np.abs(r).max(), 1e-6), err_msg=n)
        checked += 1
    assert checked >= min_checked, checked


_CACHE = {}
NORMS = ["identity", "batch_norm"]


def _trained(norm):
    """the fp32 training plan (optimize=False, no hipGraph) of the toy net and the float64 oracle on the same values, computed once
    per normalisation and shared by the tests"""
    if norm not in _CACHE:
        _CACHE[norm] = _train(norm)
    return _CACHE[norm]


def _train(norm):
    g, t = N.build(norm)
    vals = N.values(g)
    x, lab = N.inputs(g, t)
    loss, logits, grads, after = N.run_plan(g, t, vals, x, lab)
    return dict(norm=norm, g=g, t=t, vals=vals, x=x, lab=lab, got=(loss, logits, grads), after=after,
                ref=N.oracle(g, vals, x, lab, norm))


@pytest.mark.parametrize("norm", NORMS)
def test_fp32_training_plan_matches_autograd(norm):
    trained = _trained(norm)
    names = set(trained["g"].variables)
    assert {"net/c1/W", "net/c1/b", "net/tc/W", "net/tc/b", "net/head/W"} <= names
    assert trained["g"].variables["net/tc/W"].shape == (4, 4, 4, 4, 8) and trained["t"]["logits"].shape == (None,) + N.OUT + (N.NCLS,)
    assert ("net/c2/batch_norm/BatchNorm/gamma" in names) == (trained["norm"] == "batch_norm")
    _check_against(trained["got"], trained["ref"])


def test_moving_statistics_follow_the_biased_variance():
    """tf.contrib.layers.batch_norm on rank 5 (non-fused path): the moving variance moves with the biased batch variance.  rtol 1e-5
    against the biased oracle; the Bessel-corrected value -- what the rank-4 path would give -- must lie outside that tolerance for the
    layers whose B D H W is a few hundred (m / (m - 1) - 1 > 1e-3: c2 with 24 and tc with 192 values per channel)."""
    trained = _trained("batch_norm")
    after, ref = trained["after"], trained["ref"]
    small = 0
    for pre, (m, var) in ref["counts"].items():
        print("%s m = %d, batch variance %.3f .. %.3f" % (pre, m, var.min(), var.max()))
        assert 0.05 < var.min() and var.max() < 20.0, "the bound assumes channel variances of order 1"
        biased, bessel = ref["moving"][pre + "moving_variance"]
        np.testing.assert_allclose(after[pre + "moving_variance"], biased, rtol=1e-5, err_msg=pre)
        np.testing.assert_allclose(after[pre + "moving_mean"], ref["moving"][pre + "moving_mean"][0], rtol=1e-5, atol=1e-7, err_msg=pre)
        if m <= 200:
            assert m / (m - 1) - 1 > 1e-3
            assert (np.abs(after[pre + "moving_variance"] - bessel) > 1e-5 * np.abs(bessel)).all(), pre
            small += 1
    assert small >= 2 and len(ref["counts"]) == 3


@pytest.mark.parametrize("norm", ["batch_norm"])
def test_normalise_post_activation(norm):
    g, t = N.build(norm, post=True)
    assert [op.type for op in g.ops if op.name.startswith("net/a/")] == ["conv_unit", "norm_act"]
    vals = N.values(g)
    x, lab = N.inputs(g, t)
    loss, logits, grads, after = N.run_plan(g, t, vals, x, lab)
    ref = N.oracle(g, vals, x, lab, norm, post=True)
    _check_against((loss, logits, grads), ref, min_checked=6)                  # (the graph has six trainable variables)
    pre = "net/a/batch_norm/BatchNorm/"
    np.testing.assert_allclose(after[pre + "moving_variance"], ref["moving"][pre + "moving_variance"][0], rtol=1e-5)


@pytest.mark.parametrize("norm", NORMS)
def test_inference_plan(norm):
    """dropout is the identity, batch norm reads the moving pair (as the training step left it)"""
    trained = _trained(norm)
    state = trained["after"]
    _, logits, _, _ = N.run_plan(trained["g"], trained["t"], state, trained["x"], trained["lab"], training=False)
    ref = N.oracle(trained["g"], state, trained["x"], trained["lab"], trained["norm"], training=False)
    np.testing.assert_allclose(logits, ref["logits"], rtol=0, atol=3e-4 * float(np.abs(ref["logits"]).max()))


@pytest.mark.parametrize("norm", NORMS)
def test_bf16_plan_within_the_storage_policy_band(norm):
    """The bound is the float64 oracle's own sensitivity to the storage policy: the oracle with every stored tensor rounded to bf16
    against the exact one -- max abs over the logits, per gradient tensor over its max.  The bf16 plan must lie within 2x that distance
    of the ROUNDED oracle (2: another summation order flips rounding boundaries).
    Measured (MI355X): see LABBOOK.md, "3-D layer family"."""
    trained = _trained(norm)
    g, t, vals, x, lab = (trained[k] for k in ("g", "t", "vals", "x", "lab"))
    loss, logits, grads, _ = N.run_plan(g, t, vals, x, lab, compute_dtype="bf16")
    exact, rnd = trained["ref"], N.oracle(g, vals, x, lab, norm, stored=N.bf16_round)
    d_logits = float(np.abs(rnd["logits"] - exact["logits"]).max())
    e_logits = float(np.abs(logits - rnd["logits"]).max())
    print("bf16 %s logits: oracle distance %.3e, plan error %.3e" % (norm, d_logits, e_logits))
    fails = []
    if not e_logits <= 2 * d_logits:
        fails.append(("logits", e_logits, d_logits))
    for n, r in rnd["grads"].items():
        if np.abs(exact["grads"][n]).max() < 1e-9:
            # a bias in front of batch norm: its gradient, the channel sum of dy, is zero in exact arithmetic and the relative metric
            # has no scale.  The plan stores dy in bf16 (relative error 2^-9 per element), so |db| <= 2^-9 sum |dy|; margin 2 as below
            bound = 2 * 2.0 ** -9 * rnd["dy_abs"][n]
            print("bf16 %s %s: structurally zero, |db| max %.3e, bound %.3e" % (norm, n, np.abs(grads[n]).max(), bound.min()))
            if not (np.abs(grads[n]) <= bound).all():
                fails.append((n, float(np.abs(grads[n]).max()), float(bound.min())))
            continue
        scale = max(float(np.abs(r).max()), 1e-12)
        d = float(np.abs(r - exact["grads"][n]).max()) / scale
        e = float(np.abs(grads[n] - r).max()) / scale
        print("bf16 %s %s: oracle distance %.3e, plan error %.3e" % (norm, n, d, e))
        if not e <= 2 * d:
            fails.append((n, e, d))
    assert not fails, fails


def test_hip_graph_and_deterministic_mode():
    """use_hip_graph=True with PHX_DETERMINISTIC=1 (read once per process: a worker): two runs of the training plan from the same state
    give bit-identical loss and gradients, equal to the uncaptured plan's."""
    env = dict(os.environ, PYTHONPATH=ROOT, PHX_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "volume_graph_worker.py")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    for norm, row in rep.items():
        assert row["deterministic"] is True, norm
        assert row["repeat_equal"] and row["eager_equal"], (norm, row)
        assert row["ngrads"] >= 8 and np.isfinite(row["loss"])
