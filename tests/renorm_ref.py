"""Float64 numpy restatement of batch renormalisation as DESIGN.md section 7f states it (TF 1.12 tf.contrib.layers.batch_norm(renorm=True,
renorm_decay=0.99, epsilon=1e-3, renorm_clipping={'rmax', 'dmax'}) with the reference's clipping schedule).  Imports nothing of the
code under test."""
import numpy as np

EPS = 1e-3
RENORM_DECAY = 0.99
MOVING_DECAY = 0.999
STATE = ("renorm_mean", "renorm_mean_weight", "renorm_stddev", "renorm_stddev_weight", "moving_mean", "moving_variance")


def clip_bounds(t):
    """(rmax, dmax) at global step t."""
    t = float(t)
    rmax = 1.0 if t < 500 else (3.0 if t > 4000 else 1.0 + (t - 500.0) * 2.0 / 3500.0)
    dmax = 0.0 if t < 500 else (5.0 if t > 2500 else (t - 500.0) * 5.0 / 2000.0)
    return rmax, dmax


def fresh_state(C):
    return dict(renorm_mean=np.zeros(C), renorm_mean_weight=0.0, renorm_stddev=np.zeros(C), renorm_stddev_weight=0.0,
                moving_mean=np.zeros(C), moving_variance=np.ones(C))


def act_fwd(v, act):
    return np.maximum(v, 0.0) if act == "relu" else v


def correction(mu, sigma, state, t):
    """r, d from the batch moments and the state BEFORE this step's update."""
    rmax, dmax = clip_bounds(t)
    mix_mean = state["renorm_mean"] + (1.0 - state["renorm_mean_weight"]) * mu
    mix_sigma = state["renorm_stddev"] + (1.0 - state["renorm_stddev_weight"]) * sigma
    r = np.minimum(sigma / mix_sigma, rmax)                       # no lower clip
    d = np.clip((mu - mix_mean) / mix_sigma, -dmax, dmax)
    return r, d


def forward(x, gamma, beta, state, t, act="identity"):
    """x [P, C] -> dict(y, mean, rstd, r, d, scale, shift, gamma_eff, pre)."""
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(axis=0)
    var = ((x - mu) ** 2).mean(axis=0)
    sigma = np.sqrt(var + EPS)
    r, d = correction(mu, sigma, state, t)
    pre = gamma * ((x - mu) / sigma * r + d) + beta
    scale = gamma * r / sigma
    return dict(y=act_fwd(pre, act), pre=pre, mean=mu, rstd=1.0 / sigma, r=r, d=d, scale=scale, shift=beta + gamma * d - mu * scale,
                gamma_eff=gamma * r)


def batch_norm_forward(x, gamma, beta, act="identity"):
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(axis=0)
    var = ((x - mu) ** 2).mean(axis=0)
    return act_fwd(gamma * ((x - mu) / np.sqrt(var + EPS)) + beta, act)


def _assign(v, x, decay):
    return v - (v - x) * (1.0 - decay)


def update(state, mean, rstd):
    """The six state updates of one training step from the step's (mean, rstd) -> new state."""
    sigma = 1.0 / np.asarray(rstd, dtype=np.float64)
    s = dict(state)
    s["renorm_mean"] = _assign(state["renorm_mean"], mean, RENORM_DECAY)
    s["renorm_mean_weight"] = _assign(state["renorm_mean_weight"], 1.0, RENORM_DECAY)
    s["renorm_stddev"] = _assign(state["renorm_stddev"], sigma, RENORM_DECAY)
    s["renorm_stddev_weight"] = _assign(state["renorm_stddev_weight"], 1.0, RENORM_DECAY)
    new_mean = s["renorm_mean"] / s["renorm_mean_weight"]
    new_sigma = s["renorm_stddev"] / s["renorm_stddev_weight"]
    s["moving_mean"] = _assign(state["moving_mean"], new_mean, MOVING_DECAY)
    s["moving_variance"] = _assign(state["moving_variance"], new_sigma ** 2 - EPS, MOVING_DECAY)
    return s


def backward(x, gamma, beta, state, t, dy, act="identity"):
    """Analytic gradients with r and d constant -> (dx, dgamma, dbeta)."""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    f = forward(x, gamma, beta, state, t, act)
    g = dy * (f["pre"] > 0) if act == "relu" else dy
    xhat = (x - f["mean"]) * f["rstd"]
    dbeta = g.sum(axis=0)
    dgamma = (g * (xhat * f["r"] + f["d"])).sum(axis=0)
    dxhat = g * f["gamma_eff"]
    dx = f["rstd"] * (dxhat - dxhat.mean(axis=0) - xhat * (dxhat * xhat).mean(axis=0))
    return dx, dgamma, dbeta
