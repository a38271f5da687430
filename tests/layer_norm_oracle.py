"""The float64 oracle of whole nets under layer normalisation (test infrastructure only).

oracle.nets.Ctx.conv treats a normalisation name it does not know as the identity, so the layer-norm branch lives here: a subclass whose
`conv` adds it with the same self.r(...) storage points as group norm (bf16_sim: the stored pre-normalisation tensor and the stored
activation), patched in as oracle.nets.Ctx for the duration of a call.  `ln` wraps tests/layer_norm_ref.py (numpy float64) as a torch
autograd function for the small graphs whose convolutions are torch float64 (oracle.tf1_ops)."""
import contextlib

import numpy as np
import torch

from oracle import nets
from oracle import tf1_ops as T
from tests import layer_norm_ref as R

NORM = "layer_norm"


class LayerNormCtx(nets.Ctx):
    def conv(self, x, scope, act="relu", normalise=True):
        if not normalise or self.norm != NORM:
            return super().conv(x, scope, act, normalise)
        p = self.p
        w = p[scope + "/W"]
        if self.bf16_sim and w.shape[0] == 3 and w.shape[3] % 32 == 0 and (w.shape[2] % 32 == 0 or w.shape[2] < 32):
            x, w = self.r(x), self.r(w)                # MFMA path: bf16 operands (as Ctx.conv)
        y = self.r(T.bias_add(T.conv2d_same(x, w), p[scope + "/b"]))          # the bias stays; stored pre-norm activation
        m = y.mean(dim=(1, 2, 3), keepdim=True)
        v = ((y - m) ** 2).mean(dim=(1, 2, 3), keepdim=True)
        y = (y - m) / torch.sqrt(v + R.EPS)
        if act == "relu":
            y = T.relu(y)
        elif act == "softplus":
            y = T.softplus(y)
        return self.r(y)


@contextlib.contextmanager
def patched():
    """oracle.nets.elbo / sample build their context as nets.Ctx(...): inside this block that is LayerNormCtx."""
    keep = nets.Ctx
    nets.Ctx = LayerNormCtx
    try:
        yield
    finally:
        nets.Ctx = keep


def elbo(params, x, s, eps_fn, cfg, training=True, bf16_sim=False):
    with patched():
        return nets.elbo(params, x, s, eps_fn, dict(cfg, norm=NORM), training=training, bf16_sim=bf16_sim)


class _LN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, act):
        ctx.act = act
        ctx.save_for_backward(y)
        return torch.as_tensor(R.forward(y.detach().numpy(), act)["a"])

    @staticmethod
    def backward(ctx, dA):
        (y,) = ctx.saved_tensors
        return torch.as_tensor(R.backward(y.detach().numpy(), dA.numpy(), ctx.act)), None


def ln(y, act="relu"):
    """act(layer_norm(y)) of a float64 torch tensor [B, ...], forward and backward by tests/layer_norm_ref.py"""
    assert y.dtype == torch.float64
    return _LN.apply(y, act)


def self_check():
    """the autograd wrapper and the Ctx branch state the same function"""
    rng = np.random.default_rng(0)
    y = torch.as_tensor(rng.standard_normal((2, 3, 4, 5))).requires_grad_(True)
    dA = torch.as_tensor(rng.standard_normal((2, 3, 4, 5)))
    (ln(y) * dA).sum().backward()
    g1 = y.grad.clone()
    y.grad = None
    m = y.mean(dim=(1, 2, 3), keepdim=True)
    v = ((y - m) ** 2).mean(dim=(1, 2, 3), keepdim=True)
    (T.relu((y - m) / torch.sqrt(v + R.EPS)) * dA).sum().backward()
    return float((g1 - y.grad).abs().max())
