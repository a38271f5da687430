"""Float64 restatement of layer normalisation as layers.conv2D applies it (the reference's tfwrapper/normalisation.py:39-68 with
gamma = beta = None, axes (1, 2, 3), eps 1e-3; layers.py:135: activation(normalisation(op))).  numpy only: it imports nothing of the
code under test.

Per sample b over all N = H W C values:   m = mean(y_b), v = mean((y_b - m)^2), r = 1 / sqrt(v + eps), pre = (y - m) r, a = act(pre)
backward, g = dA act'(pre):               dy = r (g - mean(g) - pre mean(g pre))"""
import numpy as np

EPS = 1e-3


def act_fwd(v, act):
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "softplus":
        return np.logaddexp(0.0, v)
    assert act == "identity", act
    return v


def act_grad(pre, act):
    if act == "relu":
        return (pre > 0.0).astype(np.float64)
    if act == "softplus":
        return 1.0 / (1.0 + np.exp(-pre))
    assert act == "identity", act
    return np.ones_like(pre)


def _axes(y):
    return tuple(range(1, y.ndim))


def forward(y, act="identity", eps=EPS):
    """y [B, ...] -> dict(a, pre, mean [B], rstd [B]) in float64."""
    y = np.asarray(y, dtype=np.float64)
    ax = _axes(y)
    m = y.mean(axis=ax, keepdims=True)
    v = ((y - m) ** 2).mean(axis=ax, keepdims=True)
    r = 1.0 / np.sqrt(v + eps)
    pre = (y - m) * r
    return dict(a=act_fwd(pre, act), pre=pre, mean=m.reshape(-1), rstd=r.reshape(-1))


def backward(y, dA, act="identity", eps=EPS):
    """-> dy, the gradient of sum(dA * a) with respect to y."""
    f = forward(y, act, eps)
    ax = _axes(f["pre"])
    pre, r = f["pre"], f["rstd"].reshape((-1,) + (1,) * len(ax))
    g = np.asarray(dA, dtype=np.float64) * act_grad(pre, act)
    return r * (g - g.mean(axis=ax, keepdims=True) - pre * (g * pre).mean(axis=ax, keepdims=True))
