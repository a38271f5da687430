"""The two toy networks of tests/test_padded_graph_gpu.py (not a test file), written only with the layer functions of
tfwrapper/layers.py, and their float64 oracle (torch autograd over tests/padded_ref.py).

"unet": the classic valid-padded U-Net
    x [B, 28, 28, 1] -> c1, c2 (3x3 VALID, 8 wide: 28 -> 26 -> 24) -> maxpool2D(padding="VALID") (12) -> c3, c4 (3x3 VALID, 16 wide:
    10, 8) -> transposed_conv2D up (2x2 / stride 2, VALID: 16) -> crop_and_concat with c2 (24 -> 16: a real crop of 4) -> c5, c6 (3x3
    VALID: 14, 12) -> 1x1 logit head, 3 classes, against [B, 12, 12] labels.
"mixed": what the U-Net does not reach
    x [B, 17, 17, 4] -> conv2D a (3x3, strides (2, 2), VALID: 8) -> averagepool2D 3x3 / stride 1 (8) and maxpool2D 3x3 (4) on the same
    tensor -> dilated_conv2D d on the average (rate 2, VALID: 4; leaky_relu, normalise_post_activation=True) -> crop_and_concat([d, max])
    -> transposed_conv2D t (3x3 / stride 2, VALID, output_shape 9 x 10 of the legal 9..10) -> 1x1 logit head against [B, 9, 10] labels.
The loss is built as tests/test_extra_layers_gpu.py::test_extra_layers_in_a_graph builds it."""
import numpy as np
import torch

from oracle import tf1_ops as T
from tests import padded_ref as R

B, NCLS = 3, 3
SEED = 4242
SHAPES = {"unet": ((28, 28, 1), (12, 12)), "mixed": ((17, 17, 4), (9, 10))}


def build(kind, norm):
    """-> (graph, dict of tensors)"""
    from phiseg_code_amd import graph as G
    from phiseg_code_amd.tfwrapper import activations as act
    from phiseg_code_amd.tfwrapper import layers
    from phiseg_code_amd.tfwrapper import normalisation as tfnorm
    nfn = getattr(tfnorm, norm)
    kw = dict(normalisation=nfn, training=True)
    g = G.reset_default_graph()
    xs, ls = SHAPES[kind]
    x_inp = G.placeholder(G.KIND_F32, [None] + list(xs), name="x_input")
    s_inp = G.placeholder(G.KIND_U8, [None] + list(ls), name="s_input")
    with g.variable_scope("net"):
        if kind == "unet":
            c1 = layers.conv2D(x_inp, "c1", num_filters=8, padding="VALID", **kw)
            c2 = layers.conv2D(c1, "c2", num_filters=8, padding="VALID", **kw)
            p = layers.maxpool2D(c2, padding="VALID")
            c3 = layers.conv2D(p, "c3", num_filters=16, padding="VALID", **kw)
            c4 = layers.conv2D(c3, "c4", num_filters=16, padding="VALID", **kw)
            up = layers.transposed_conv2D(c4, "up", kernel_size=(2, 2), num_filters=8, padding="VALID", **kw)
            cat = layers.crop_and_concat([up, c2])
            c5 = layers.conv2D(cat, "c5", num_filters=8, padding="VALID", **kw)
            feat = layers.conv2D(c5, "c6", num_filters=8, padding="VALID", **kw)
            assert [t.get_shape().as_list()[1] for t in (c1, c2, p, c3, c4, up, cat, c5, feat)] == [26, 24, 12, 10, 8, 16, 16, 14, 12]
            assert any(op.type == "spatial_window" and op.attrs["off"] == (4, 4) for op in g.ops)
        else:
            a = layers.conv2D(x_inp, "a", num_filters=8, strides=(2, 2), padding="VALID", **kw)
            ap = layers.averagepool2D(a, kernel_size=(3, 3), strides=(1, 1))
            mp = layers.maxpool2D(a, kernel_size=(3, 3))
            d = layers.dilated_conv2D(ap, "d", num_filters=8, rate=2, padding="VALID", activation=act.leaky_relu,
                                      normalise_post_activation=True, **kw)
            cat = layers.crop_and_concat([d, mp])
            feat = layers.transposed_conv2D(cat, "t", kernel_size=(3, 3), num_filters=8, padding="VALID", output_shape=[None, 9, 10, 8], **kw)
            assert [t.get_shape().as_list()[1:3] for t in (a, ap, mp, d, cat, feat)] == [[8, 8], [8, 8], [4, 4], [4, 4], [4, 4], [9, 10]]
        s = layers.conv2D(feat, "head", num_filters=NCLS, kernel_size=(1, 1), activation=act.identity)
    ce, _ = G.residual_multinoulli([s], s_inp, 1.0)
    loss = G.weighted_sum([ce[0]], [1.0])
    return g, dict(x=x_inp, s_inp=s_inp, logits=s, loss=loss)


def values(g, seed=3):
    """initial values with the biases / norm variables moved off their trivial defaults; moving variances positive"""
    rng = np.random.default_rng(7)
    vals = {n: (v.initial_value(seed) + (0.1 * rng.standard_normal(v.shape) if not n.endswith("/W") else 0)).astype(np.float32)
            for n, v in g.variables.items()}
    for n in vals:
        if n.endswith("moving_variance"):
            vals[n] = (np.abs(vals[n]) + 0.5).astype(np.float32)
    return vals


def inputs(kind):
    rng = np.random.default_rng(19)
    xs, ls = SHAPES[kind]
    return rng.standard_normal((B,) + xs).astype(np.float32), rng.integers(0, NCLS, (B,) + ls).astype(np.uint8)


def run_plan(g, t, vals, x, lab, runs=1, **plan_kw):
    """`runs` runs of the training plan over (loss, logits) from the state `vals` (use_hip_graph=True: the first is the eager warm-up, the
    second captures and launches, later ones replay) -> (loss, logits, gradients) of the last one"""
    from phiseg_code_amd import engine
    store = engine.ParamStore(g, seed=3)
    store.load(vals)
    kw = dict(batch=B, training=True, compute_dtype="f32", use_hip_graph=False, rng_seed=SEED)
    kw.update(plan_kw)
    plan = engine.Plan(store, [t["loss"], t["logits"]], loss=t["loss"], optimize=False, **kw)
    plan.set_input("x_input", x)
    plan.set_input("s_input", lab)
    for _ in range(runs):
        plan.run(sync=True)
    return float(plan.fetch(t["loss"])), plan.fetch(t["logits"]), store.export(grads=True)


def bf16_round(y):
    """value after storage in bf16, straight-through for the gradient"""
    return y + (y.detach().to(torch.float32).to(torch.bfloat16).to(torch.float64) - y.detach())


def oracle(kind, vals, x, lab, norm, stored=None):
    """float64 forward + autograd -> dict(loss, logits, grads {name: array} of every trainable variable, dy_abs {bias name: per-channel
    sum of |d loss / d y| over the pre-normalisation tensor of a unit that keeps its bias in front of batch norm}).
    stored: applied to every tensor the plan stores in its compute dtype (bf16_round models the bf16 storage policy), None = exact."""
    st = stored or (lambda v: v)
    p = {n: torch.as_tensor(v, dtype=torch.float64).requires_grad_(not n.rsplit("/", 1)[-1].startswith("moving_")) for n, v in vals.items()}
    pre_norm = {}

    def bn(y, scope):
        out, _, _ = T.batch_norm_train(y, p[scope + "/batch_norm/BatchNorm/gamma"], p[scope + "/batch_norm/BatchNorm/beta"])
        return out

    def unit(y, scope, activation=torch.relu, post=False):
        """y: the convolution's result.  conv2D drops its bias in front of batch norm, the other layers keep theirs."""
        if scope + "/b" in p:
            y = R.bias_add(y, p[scope + "/b"])
            if norm == "batch_norm" and not post:
                y.retain_grad()
                pre_norm[scope + "/b"] = y
        if norm == "identity":
            return st(activation(st(y))) if post else st(activation(y))          # (post: unit with the identity, then the leaky_relu node)
        if post:
            return st(bn(st(activation(st(y))), scope))
        return st(activation(bn(st(y), scope)))

    def conv(v, scope, s=(1, 1), d=(1, 1), **kw):
        return unit(R.conv2d(v, p[scope + "/W"], s, d, "VALID"), scope, **kw)
    xt = torch.as_tensor(x, dtype=torch.float64)
    if kind == "unet":
        c2 = conv(conv(xt, "net/c1"), "net/c2")
        c4 = conv(conv(R.max_pool(c2, (2, 2), (2, 2), "VALID"), "net/c3"), "net/c4")
        up = unit(R.conv2d_transpose(c4, p["net/up/W"], (16, 16), (2, 2), "VALID"), "net/up")
        feat = conv(conv(torch.cat([up, c2[:, 4:20, 4:20]], dim=-1), "net/c5"), "net/c6")
    else:
        a = conv(xt, "net/a", s=(2, 2))
        ap = st(R.avg_pool(a, (3, 3), (1, 1), "SAME"))
        mp = R.max_pool(a, (3, 3), (2, 2), "SAME")
        d = conv(ap, "net/d", d=(2, 2), activation=lambda v: torch.nn.functional.leaky_relu(v, 0.01), post=True)
        feat = unit(R.conv2d_transpose(torch.cat([d, mp], dim=-1), p["net/t/W"], (9, 10), (2, 2), "VALID"), "net/t")
    logits = T.bias_add(T.conv2d_same(feat, p["net/head/W"]), p["net/head/b"])
    loss = T.multinoulli_loss_with_logits(T.one_hot(torch.as_tensor(lab), NCLS, torch.float64), logits)
    loss.backward()
    grads = {n: v.grad.numpy() for n, v in p.items() if v.requires_grad}
    assert all(v.grad is not None for v in p.values() if v.requires_grad)
    dy_abs = {n: y.grad.abs().sum(dim=(0, 1, 2)).numpy() for n, y in pre_norm.items()}
    return dict(loss=float(loss.detach()), logits=logits.detach().numpy(), grads=grads, dy_abs=dy_abs)
