"""Reference of leaky ReLU for the tests (not a test file): tf.maximum(x, alpha * x) (the reference's tfwrapper/activations.py) with the
gradient TF's MaximumGrad gives it -- the whole gradient to the first argument where x >= alpha * x, a tie included, so 1 at x == 0
and never (1 + alpha) / 2.  torch.maximum's own autograd splits a tie in half and is NOT used: the backward is written out.

    leaky_relu(x, alpha)              torch, any float dtype, differentiable (float64 under the engine tests' oracle)
    forward_f32 / backward_f32        numpy float32, one correctly rounded multiply each: what the kernels must match bit for bit"""
import numpy as np
import torch


class _LeakyReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha):
        ax = alpha * x
        y = torch.where(x >= ax, x, ax)
        ctx.save_for_backward(y)
        ctx.alpha = alpha
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        # for 0 < alpha < 1 the sign of y is the sign of x; y >= 0 holds for -0.0 too, where x = -0.0 ties with alpha * x
        return dy * torch.where(y >= 0, torch.ones_like(y), torch.full_like(y, ctx.alpha)), None


def leaky_relu(x, alpha=0.01):
    assert 0.0 < alpha < 1.0
    return _LeakyReLU.apply(x, float(alpha))


def forward_f32(x, alpha):
    """np.maximum(x, float32(alpha) * x) in float32"""
    x = np.asarray(x, dtype=np.float32)
    return np.maximum(x, np.float32(alpha) * x)


def backward_f32(dy, y, alpha):
    """dy * where(y >= 0, 1, alpha) in float32"""
    dy, y = np.asarray(dy, dtype=np.float32), np.asarray(y, dtype=np.float32)
    return dy * np.where(y >= 0, np.float32(1.0), np.float32(alpha)).astype(np.float32)
