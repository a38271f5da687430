"""The 3-D layer family without a GPU: the signatures the reference's tfwrapper/layers.py fixes, the graph the four layer functions
build (variable names, shapes, collections, output shapes), the refusals, the float64 oracle (tests/volume_ref.py) against
oracle/tf1_ops.py where the two overlap, the header and the checkpoint writer."""
import inspect
import math

import numpy as np
import pytest
import torch

from oracle import tf1_ops as T
from tests import volume_ref as V

from phiseg_code_amd import graph as G
from phiseg_code_amd.tfwrapper import activations as act
from phiseg_code_amd.tfwrapper import layers
from phiseg_code_amd.tfwrapper import normalisation as tfnorm

RNG = np.random.default_rng(5)


def _sig(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items()]


def test_signatures_are_the_references():
    E = inspect.Parameter.empty
    tail = [("activation", layers.STANDARD_NONLINEARITY), ("normalisation", tfnorm.identity), ("normalise_post_activation", False),
            ("dropout_p", None), ("padding", "SAME"), ("weight_init", "he_normal"), ("add_bias", True), ("kwargs", E)]
    assert _sig(layers.conv3D) == [("x", E), ("name", E), ("kernel_size", (3, 3, 3)), ("num_filters", 32), ("strides", (1, 1, 1))] + tail
    assert _sig(layers.transposed_conv3D) == [("bottom", E), ("name", E), ("kernel_size", (4, 4, 4)), ("num_filters", 32),
                                              ("strides", (2, 2, 2)), ("output_shape", None)] + tail
    assert _sig(layers.maxpool3D) == [("x", E), ("kernel_size", (2, 2, 2)), ("strides", (2, 2, 2)), ("padding", "SAME")]
    assert _sig(layers.bilinear_upsample3D) == [("x", E), ("name", E), ("factor", E)]
    assert inspect.signature(layers.conv3D).parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD


def _toy(norm):
    g = G.reset_default_graph()
    x = G.placeholder(G.KIND_F32, [None, 5, 7, 6, 3], name="x_input")
    with g.variable_scope("net"):
        c1 = layers.conv3D(x, "c1", num_filters=8, normalisation=norm, training=True)
        p1 = layers.maxpool3D(c1)
        c2 = layers.conv3D(p1, "c2", num_filters=4, kernel_size=(3, 1, 2), strides=(1, 2, 2), normalisation=norm, training=True)
        up = layers.bilinear_upsample3D(c2, "up", 2)
        tc = layers.transposed_conv3D(c2, "tc", num_filters=6, normalisation=norm, training=True)
        cat = layers.crop_and_concat([c2, up])
        an = layers.maxpool3D(c1, kernel_size=(1, 2, 2), strides=(1, 2, 2))
    return g, dict(x=x, c1=c1, p1=p1, c2=c2, up=up, tc=tc, cat=cat, an=an)


def test_graph_variables_and_shapes():
    g, t = _toy(tfnorm.batch_norm)
    v = g.variables
    assert v["net/c1/W"].shape == (3, 3, 3, 3, 8) and v["net/c2/W"].shape == (3, 1, 2, 8, 4)
    assert v["net/tc/W"].shape == (4, 4, 4, 6, 4)                               # [kd, kh, kw, num_filters, Cin]
    wv = [w.name for w in g.get_collection("weight_variables")]
    assert wv == ["net/c1/W", "net/c2/W", "net/tc/W"]
    for n in ("c1", "c2", "tc"):                                               # the bias stays in front of batch norm
        assert v["net/%s/b" % n].shape == (v["net/%s/W" % n].shape[4 if n != "tc" else 3],)
        for k in ("beta", "gamma", "moving_mean", "moving_variance"):
            assert "net/%s/batch_norm/BatchNorm/%s" % (n, k) in v
    # odd extents, anisotropic strides
    assert t["c1"].shape == (None, 5, 7, 6, 8)
    assert t["p1"].shape == (None, 3, 4, 3, 8)
    assert t["c2"].shape == (None, 3, 2, 2, 4)
    assert t["up"].shape == (None, 6, 4, 4, 4)
    assert t["tc"].shape == (None, 6, 4, 4, 6)
    assert t["cat"].shape == (None, 3, 2, 2, 8)
    assert t["an"].shape == (None, 5, 4, 3, 8)
    crop = [op for op in g.ops if op.type == "spatial_window3d"]
    assert len(crop) == 1 and crop[0].attrs["off"] == (1, 1, 1)                # start = (larger - output) // 2
    g2, _ = _toy(tfnorm.identity)
    assert not any("batch_norm" in n for n in g2.variables) and "net/c1/b" in g2.variables


def test_normalise_post_activation_is_a_composition_under_the_same_scope():
    g = G.reset_default_graph()
    x = G.placeholder(G.KIND_F32, [None, 4, 4, 4, 2], name="x_input")
    y = layers.conv3D(x, "c", num_filters=4, normalisation=tfnorm.batch_norm, normalise_post_activation=True, training=True)
    assert y.op.type == "norm_act" and y.op.attrs["act"] == "identity" and y.op.attrs["norm"] == "batch"
    unit = y.op.inputs[0].op
    assert unit.type == "conv_unit" and unit.attrs["norm"] is None and unit.attrs["act"] == "relu" and unit.attrs["volume"][0] == "conv"
    assert sorted(g.variables) == ["c/W", "c/b"] + ["c/batch_norm/BatchNorm/" + k for k in ("beta", "gamma", "moving_mean", "moving_variance")]
    z = layers.transposed_conv3D(y, "t", num_filters=3, normalisation=tfnorm.batch_norm, normalise_post_activation=True, training=True)
    assert z.op.type == "norm_act" and z.shape == (None, 8, 8, 8, 3) and "t/batch_norm/BatchNorm/gamma" in g.variables


def test_he_normal_fan_in():
    g = G.reset_default_graph()
    x = G.placeholder(G.KIND_F32, [None, 4, 4, 4, 16], name="x_input")
    layers.conv3D(x, "c", num_filters=24, kernel_size=(3, 3, 3))
    layers.transposed_conv3D(x, "t", num_filters=24, kernel_size=(4, 4, 4))
    for name, fan in (("c/W", 27 * 16), ("t/W", 64 * 24)):                      # TF's shape[-2] rule: num_filters for the transposed filter
        w = g.variables[name].initial_value(seed=1)
        std = math.sqrt(1.3 * 2.0 / fan)
        assert np.abs(w).max() <= 2.0 * std * (1 + 1e-6), name                 # truncated at two standard deviations
        assert abs(w.std() / (0.8796 * std) - 1.0) < 0.03, (name, w.std(), std)  # (std of a normal truncated at 2 sigma = 0.8796 sigma)


def test_refusals():
    g = G.reset_default_graph()
    x = G.placeholder(G.KIND_F32, [None, 4, 4, 4, 2], name="x_input")
    for bad in (tfnorm.group_norm2D, tfnorm.instance_norm2D, tfnorm.layer_norm, tfnorm.batch_renorm):
        with pytest.raises(NotImplementedError):
            layers.conv3D(x, "c_" + tfnorm.KIND[bad], normalisation=bad)
        with pytest.raises(NotImplementedError):
            layers.transposed_conv3D(x, "t_" + tfnorm.KIND[bad], normalisation=bad)
    with pytest.raises(NotImplementedError):
        layers.transposed_conv3D(x, "t1", output_shape=[None, 8, 8, 9, 32])
    layers.transposed_conv3D(x, "t2", output_shape=[None, 8, 8, 8, 32])
    with pytest.raises(NotImplementedError):
        layers.bilinear_upsample3D(x, "u", 3)
    with pytest.raises(NotImplementedError):
        layers.maxpool3D(x, kernel_size=(3, 3, 3), strides=(3, 3, 3))
    with pytest.raises(NotImplementedError):
        layers.maxpool3D(x, kernel_size=(2, 2, 2), strides=(1, 1, 1))
    with pytest.raises(NotImplementedError):
        layers.conv3D(x, "v", padding="VALID")
    with pytest.raises(ValueError):
        layers.crop_and_concat([layers.maxpool3D(x), x], axis=1)
    with pytest.raises(ValueError):
        G.concat([x, layers.maxpool3D(x)])                                      # unequal spatial shapes


def test_losses_accept_volumes():
    from phiseg_code_amd.tfwrapper import losses
    g = G.reset_default_graph()
    x = G.placeholder(G.KIND_F32, [None, 4, 6, 5, 1], name="x_input")
    s = G.placeholder(G.KIND_U8, [None, 4, 6, 5], name="s_input")
    lg = layers.conv3D(x, "head", num_filters=3, kernel_size=(1, 1, 1), activation=act.identity)
    assert lg.kind == G.KIND_F32 and lg.shape == (None, 4, 6, 5, 3)
    d = losses.dice_loss(lg, G.one_hot(s, 3))
    ce = losses.pixel_wise_cross_entropy_loss_weighted(lg, G.one_hot(s, 3), [0.2, 0.5, 0.3])
    for t in (d, ce):
        a, b = t.op.inputs
        assert a.op.type == "fold_depth" and a.shape == (None, 24, 5, 3) and a.op.inputs[0] is lg
        assert b.op.type == "fold_depth" and b.shape == (None, 24, 5) and b.op.inputs[0] is s
    with pytest.raises(ValueError):
        losses.dice_loss(lg, G.one_hot(s, 4))
    for bad in (s, G.placeholder(G.KIND_F32, [None, 4, 6, 5, 3], name="soft")):     # any other label form on a volume stays refused
        with pytest.raises(NotImplementedError, match="3-D"):
            losses.dice_loss(lg, bad)


def _t(a):
    return torch.as_tensor(a, dtype=torch.float64)


def test_oracle_agrees_with_tf1_ops_where_they_overlap():
    x = _t(RNG.standard_normal((2, 1, 7, 6, 3)))
    w = _t(RNG.standard_normal((1, 3, 2, 3, 4)))
    got = V.conv3d_same(x, w, (1, 2, 1))[:, 0]
    assert torch.allclose(got, T.conv2d_general_same(x[:, 0], w[0], (2, 1), (1, 1)), rtol=0, atol=1e-12)
    wt = _t(RNG.standard_normal((1, 4, 4, 5, 3)))
    got = V.conv3d_transpose_same(x, wt, (1, 2, 2))[:, 0]
    assert torch.allclose(got, T.conv2d_transpose_same(x[:, 0], wt[0], (2, 2)), rtol=0, atol=1e-12)
    wt = _t(RNG.standard_normal((1, 3, 3, 5, 3)))
    got = V.conv3d_transpose_same(x, wt, (1, 1, 2))[:, 0]
    assert torch.allclose(got, T.conv2d_transpose_same(x[:, 0], wt[0], (1, 2)), rtol=0, atol=1e-12)
    v = _t(RNG.standard_normal((2, 3, 7, 5, 2)))
    got = V.max_pool3d_same(v, (1, 2, 2))
    for z in range(3):
        assert torch.equal(got[:, z], T.max_pool_2x2_same(v[:, z]))
    plane = _t(RNG.standard_normal((2, 5, 4, 3)))
    vol = plane[:, None].expand(2, 3, 5, 4, 3)                                 # constant along D
    up = V.bilinear_up2x_3d(vol)
    assert up.shape == (2, 6, 10, 8, 3)
    want = T.resize_bilinear_legacy(plane, 10, 8)
    for z in range(6):
        assert torch.allclose(up[:, z], want, rtol=0, atol=1e-12)
    # an odd extent under stride 2 pads asymmetrically: 7 -> 4, total 2 - 1 = 1... the extra plane goes to the far side
    assert V.same_pads(7, 3, 2) == (4, 1, 1) and V.same_pads(6, 3, 2) == (3, 0, 1) and V.same_pads(5, 2, 1) == (5, 0, 1)


@pytest.mark.parametrize("case", [
    (2, 3, 4, 5, 3, 4, (4, 4, 4), (2, 2, 2)), (1, 2, 3, 4, 2, 3, (3, 3, 3), (1, 2, 2)), (1, 3, 2, 3, 4, 2, (5, 3, 4), (3, 1, 2)),
    (2, 3, 2, 4, 3, 2, (1, 1, 1), (2, 2, 2)), (1, 2, 3, 3, 2, 3, (2, 1, 3), (3, 2, 2)), (1, 2, 3, 2, 3, 2, (1, 2, 1), (2, 3, 2)),
])
def test_oracle_conv3d_transpose_is_the_input_gradient_of_conv3d(case):
    """The definition of tf.nn.conv3d_transpose (the 3-D twin of test_tconv.py's 2-D test): V.conv3d_transpose_same(x, w, s) is the
    gradient, contracted with x, of the stride-s SAME convolution V.conv3d_same(z, w, s) with respect to its input z of extent in * s,
    the filter [kd, kh, kw, Cout, Cin] read as DHWIO.  The last three geometries have k < s on one or more axes."""
    B, D, H, W, Cin, Cout, k, s = case
    rng = np.random.default_rng(0)
    x = _t(rng.standard_normal((B, D, H, W, Cin)))
    w = _t(rng.standard_normal(tuple(k) + (Cout, Cin)))
    z = torch.zeros(B, D * s[0], H * s[1], W * s[2], Cout, dtype=torch.float64, requires_grad=True)
    y = V.conv3d_same(z, w, s)
    assert y.shape == x.shape
    (y * x).sum().backward()
    got = V.conv3d_transpose_same(x, w, s)
    assert got.shape == z.shape
    np.testing.assert_allclose(got.numpy(), z.grad.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("k,s", [((3, 3, 3), (1, 1, 1)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (1, 2, 3)), ((1, 1, 1), (2, 2, 2))])
def test_impulse_helpers_restate_the_oracle_exactly(k, s):
    """V.impulse_conv3d_same / _adjoint (np.pad and slicing, no convolution) against the oracle under the same one-hot filter: the
    padded shift is exact, and the adjoint is the oracle's input gradient and its transposed convolution."""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 4, 5, 7, 3))
    o = [V.same_pads(n, k[i], s[i])[0] for i, n in enumerate((4, 5, 7))]
    dy = rng.standard_normal((1, *o, 5))
    xs = rng.standard_normal((1, 4, 5, 7, 5))
    for t, tap in enumerate(np.ndindex(*k)):
        a, b = t % 3, (2 * t + 1) % 5
        w = torch.zeros(tuple(k) + (3, 5), dtype=torch.float64)
        w[tap][a, b] = 1.0
        z = _t(x).requires_grad_(True)
        y = V.conv3d_same(z, w, s)
        assert np.array_equal(y.detach().numpy() + 0.0, V.impulse_conv3d_same(x, k, s, tap, a, b, 5)), tap
        (y * _t(dy)).sum().backward()
        assert np.array_equal(z.grad.numpy() + 0.0, V.impulse_conv3d_same_adjoint(dy, (4, 5, 7), k, s, tap, a, b, 3)), tap
        big = (4 * s[0], 5 * s[1], 7 * s[2])                                   # transposed: filter [.., Cout = 3, Cin = 5]
        up = V.conv3d_transpose_same(_t(xs), w, s)
        assert np.array_equal(up.numpy() + 0.0, V.impulse_conv3d_same_adjoint(xs, big, k, s, tap, a, b, 3)), tap


def test_biased_moving_variance_oracle():
    x = _t(RNG.standard_normal((2, 3, 4, 5, 6)))
    y, mean, var = V.batch_norm_train_5d(x, torch.ones(6, dtype=torch.float64), torch.zeros(6, dtype=torch.float64))
    flat = x.reshape(-1, 6)
    assert torch.allclose(var, flat.var(dim=0, unbiased=False)) and torch.allclose(mean, flat.mean(dim=0))
    _, _, var4 = T.batch_norm_train(x.reshape(2, 12, 5, 6), torch.ones(6, dtype=torch.float64), torch.zeros(6, dtype=torch.float64))
    assert torch.allclose(var4, var * 120 / 119)                               # the fused rank-4 path: Bessel's correction


def test_header_and_sources():
    from phiseg_code_amd import runtime as rt
    protos = rt.parse_header()
    want = dict(phx_gconv3d_out_size=9, phx_gconv3d_fwd=20, phx_gconv3d_dgrad=18, phx_gconv3d_wgrad=18, phx_tconv3d_fwd=20,
                phx_tconv3d_dgrad=18, phx_tconv3d_wgrad=18, phx_maxpool3d_fwd=12, phx_maxpool3d_bwd=13, phx_bilinear_up2x_3d_fwd=9,
                phx_bilinear_up2x_3d_bwd=9, phx_bilinear_up2x_3d_bwd_acc=9, phx_spatial_window3d=15, phx_bn_moving_update_biased=8)
    for name, nargs in want.items():
        assert name in protos and len(protos[name]) == nargs, name
    assert "conv3d.hip" in open(rt.HEADER.replace("include/phx.h", "phiseg_code_amd/csrc/SOURCES")).read().split()


def test_five_d_filter_round_trips_through_the_tensor_bundle(tmp_path):
    from phiseg_code_amd.tfwrapper import tf_checkpoint
    tensors = {"net/c1/W": RNG.standard_normal((3, 3, 3, 5, 7)).astype(np.float32),
               "net/tc/W": RNG.standard_normal((4, 4, 4, 6, 2)).astype(np.float32), "net/c1/b": np.arange(7, dtype=np.float32)}
    prefix = str(tmp_path / "model.ckpt-3")
    tf_checkpoint.write(prefix, tensors)
    back = tf_checkpoint.read(prefix)
    assert sorted(back) == sorted(tensors)
    for n, a in tensors.items():
        assert back[n].shape == a.shape and np.array_equal(back[n], a)
