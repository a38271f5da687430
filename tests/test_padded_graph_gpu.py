"""VALID padding and the general pooling windows through the engine: the valid-padded U-Net and the smaller mixed network of
tests/padded_net.py as training plans -- loss, logits and the gradient of EVERY trainable variable against float64 autograd of
tests/padded_ref.py, under tfnorm.identity and tfnorm.batch_norm, in fp32 and in bf16 storage, eagerly and captured into a hipGraph.

fp32: the tolerances of tests/test_extra_layers_gpu.py::test_extra_layers_in_a_graph (logits 3e-4 of their maximum, loss rtol 3e-5,
gradients 3e-3 of each tensor's maximum; a structurally zero gradient below 1e-4 absolute).
bf16: those tolerances describe fp32 arithmetic; a tensor stored in bf16 carries 2^-9 per element before anything is computed, so the
yardstick is the one tests/test_volume_graph_gpu.py uses for the same question: the float64 oracle's own sensitivity to the storage
policy (the oracle with every stored tensor rounded to bf16 against the exact one); the bf16 plan must lie within 2x that distance of the
ROUNDED oracle (2: another summation order flips rounding boundaries), and a bias gradient that is zero in exact arithmetic within
2 * 2^-9 sum |dy| (dy is stored in bf16).
Each configuration's captured run (eager warm-up, capture + launch, replay) must give the bits of its eager run: checked in a worker
process under PHX_DETERMINISTIC=1, because outside that mode cross-block reductions of the existing path sum with float atomics
 and no two runs of such a plan agree to the bit, captured or not; the kernels of conv2d_pad.hip have none in
either mode (tests/test_padded_kernels_gpu.py::test_repeats_are_bit_identical)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import padded_net as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMS = ["identity", "batch_norm"]
KINDS = ["unet", "mixed"]
# trainable variables: W and b of every layer, gamma / beta under batch norm -- where conv2D drops its bias, the other layers keep it
NVARS = {("unet", "identity"): 16, ("unet", "batch_norm"): 24, ("mixed", "identity"): 8, ("mixed", "batch_norm"): 13}
_CACHE = {}


def _case(kind, norm):
    """graph, values, inputs and both oracles, computed once per (network, normalisation) and shared, unchanged, by the tests"""
    if (kind, norm) not in _CACHE:
        g, t = N.build(kind, norm)
        vals = N.values(g)
        x, lab = N.inputs(kind)
        _CACHE[(kind, norm)] = dict(g=g, t=t, vals=vals, x=x, lab=lab, exact=N.oracle(kind, vals, x, lab, norm),
                                    rounded=N.oracle(kind, vals, x, lab, norm, stored=N.bf16_round), runs={})
    return _CACHE[(kind, norm)]


def _run(c, dtype, captured):
    key = (dtype, captured)
    if key not in c["runs"]:
        c["runs"][key] = N.run_plan(c["g"], c["t"], c["vals"], c["x"], c["lab"], compute_dtype=dtype, use_hip_graph=captured,
                                    runs=3 if captured else 1)
    return c["runs"][key]


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_graph_builds_the_new_nodes(kind, norm):
    c = _case(kind, norm)
    units = [op for op in c["g"].ops if op.type == "conv_unit"]
    explicit = [op.attrs["explicit"] for op in units if op.attrs.get("explicit") is not None]
    assert len(explicit) == len(units) - 1                                     # everything but the 1x1 logit head
    pools = [op.attrs["mode"] for op in c["g"].ops if op.type == "pool2d"]
    assert pools == (["max"] if kind == "unet" else ["avg", "max"])
    trainable = [n for n, v in c["g"].variables.items() if v.trainable]
    assert len(trainable) == NVARS[(kind, norm)] == len(c["exact"]["grads"])


@pytest.mark.parametrize("captured", [False, True])
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_fp32_plan_matches_autograd(kind, norm, captured):
    c = _case(kind, norm)
    loss, logits, grads = _run(c, "f32", captured)
    ref = c["exact"]
    print("%s %s: loss %.6f (oracle %.6f), logits error %.3e of max" % (kind, norm, loss, ref["loss"],
                                                                     np.abs(logits - ref["logits"]).max() / np.abs(ref["logits"]).max()))
    np.testing.assert_allclose(logits, ref["logits"], rtol=0, atol=3e-4 * float(np.abs(ref["logits"]).max()))
    np.testing.assert_allclose(loss, ref["loss"], rtol=3e-5)
    checked = 0
    for n, r in ref["grads"].items():
        if np.abs(r).max() < 1e-9:                                             # (the bias of `up` / `t` in front of batch norm)
            assert np.abs(grads[n]).max() < 1e-4, n
        else:
            print("  %s: %.3e of max" % (n, np.abs(grads[n] - r).max() / np.abs(r).max()))
            np.testing.assert_allclose(grads[n], r, rtol=0, atol=3e-3 * max(np.abs(r).max(), 1e-6), err_msg=n)
        checked += 1
    assert checked == NVARS[(kind, norm)]                                      # none skipped


@pytest.mark.parametrize("captured", [False, True])
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_bf16_plan_within_the_storage_policy_band(kind, norm, captured):
    c = _case(kind, norm)
    loss, logits, grads = _run(c, "bf16", captured)
    exact, rnd = c["exact"], c["rounded"]
    d_logits = float(np.abs(rnd["logits"] - exact["logits"]).max())
    e_logits = float(np.abs(logits - rnd["logits"]).max())
    print("bf16 %s %s logits: oracle distance %.3e, plan error %.3e" % (kind, norm, d_logits, e_logits))
    fails = [] if e_logits <= 2 * d_logits else [("logits", e_logits, d_logits)]
    checked = 0
    for n, r in rnd["grads"].items():
        checked += 1
        if np.abs(exact["grads"][n]).max() < 1e-9:
            bound = 2 * 2.0 ** -9 * rnd["dy_abs"][n]
            print("bf16 %s %s %s: structurally zero, |db| max %.3e, bound %.3e" % (kind, norm, n, np.abs(grads[n]).max(), bound.min()))
            if not (np.abs(grads[n]) <= bound).all():
                fails.append((n, float(np.abs(grads[n]).max()), float(bound.min())))
            continue
        scale = max(float(np.abs(r).max()), 1e-12)
        d = float(np.abs(r - exact["grads"][n]).max()) / scale
        e = float(np.abs(grads[n] - r).max()) / scale
        print("bf16 %s %s %s: oracle distance %.3e, plan error %.3e" % (kind, norm, n, d, e))
        if not e <= 2 * d:
            fails.append((n, e, d))
    assert checked == NVARS[(kind, norm)] and not fails, fails


def test_captured_and_eager_runs_are_bit_identical():
    """Every configuration, eager against captured, in ONE worker process under PHX_DETERMINISTIC=1 (read once per process): the loss,
    the logits and every gradient carry the same bits."""
    env = dict(os.environ, PYTHONPATH=ROOT, PHX_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "padded_graph_worker.py")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(rep) == sorted("%s/%s/%s" % (k, n, d) for k in KINDS for n in NORMS for d in ("f32", "bf16"))
    for key, row in rep.items():
        print(key, row)
        kind, norm, _ = key.split("/")
        assert row["deterministic"] is True and row["differ"] == [], (key, row)
        assert row["ngrads"] == NVARS[(kind, norm)] and np.isfinite(row["loss"]), (key, row)
