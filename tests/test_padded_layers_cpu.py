"""VALID padding and general pooling windows of the 2-D layers without a GPU: the float64 reference (tests/padded_ref.py) against
oracle/tf1_ops.py where the two overlap (SAME geometry, odd sizes), graph shape inference against the shapes torch returns, the
ValueError cases of TF 1.12's rules, the guard that every call accepted before still builds the node it built before, the header and the
source list."""
import inspect

import numpy as np
import pytest
import torch

from oracle import tf1_ops as T
from tests import padded_ref as R

from phiseg_code_amd import graph as G
from phiseg_code_amd.tfwrapper import activations as act
from phiseg_code_amd.tfwrapper import layers
from phiseg_code_amd.tfwrapper import normalisation as tfnorm

RNG = np.random.default_rng(17)


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def _same(a, b):
    """agreement to float64 rounding: both sides sum the same products, in possibly different order"""
    a, b = a.detach().numpy(), b.detach().numpy()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(b).max()), np.abs(a - b).max()


# ---- the restatement against the pinned oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(7, 9, 3, 3, 1, 1, 1, 1), (7, 9, 3, 3, 2, 2, 1, 1), (6, 5, 5, 3, 2, 1, 1, 1), (9, 7, 3, 3, 1, 1, 2, 2),
                                  (11, 6, 1, 1, 2, 2, 1, 1), (8, 8, 4, 4, 2, 2, 1, 1), (5, 7, 3, 3, 3, 3, 1, 1)])
def test_conv_same_agrees_with_the_oracle(case):
    H, W, kh, kw, sh, sw, dh, dw = case
    x, w = _t(RNG.standard_normal((2, H, W, 3))), _t(RNG.standard_normal((kh, kw, 3, 4)))
    _same(R.conv2d(x, w, (sh, sw), (dh, dw), "SAME"), T.conv2d_general_same(x, w, (sh, sw), (dh, dw)))


@pytest.mark.parametrize("case", [(5, 7, 4, 4, 2, 2), (3, 5, 3, 3, 2, 2), (4, 3, 2, 2, 2, 2), (5, 4, 3, 2, 1, 2), (3, 3, 5, 5, 3, 3)])
def test_conv_transpose_same_agrees_with_the_oracle(case):
    H, W, kh, kw, sh, sw = case
    x, w = _t(RNG.standard_normal((2, H, W, 3))), _t(RNG.standard_normal((kh, kw, 4, 3)))
    _same(R.conv2d_transpose(x, w, (H * sh, W * sw), (sh, sw), "SAME"), T.conv2d_transpose_same(x, w, (sh, sw)))


@pytest.mark.parametrize("hw", [(7, 9), (8, 6), (1, 5), (5, 1)])
def test_pools_2x2_same_agree_with_the_oracle(hw):
    x = _t(RNG.standard_normal((2,) + hw + (3,))).requires_grad_(True)
    x.data[0, :2, :2, 0] = 0.0                                                # a window of ties
    m, mo = R.max_pool(x), T.max_pool_2x2_same(x)
    assert torch.equal(m, mo)
    _same(R.avg_pool(x), T.avg_pool_2x2_same(x))
    dy = _t(RNG.standard_normal(tuple(m.shape)))
    (g,) = torch.autograd.grad((m * dy).sum(), x)
    (go,) = torch.autograd.grad((mo * dy).sum(), x)
    assert torch.equal(g, go)                                                 # ties: the first element of the window, as torch's kernel


def test_max_pool_first_maximum_in_an_overlapping_window():
    x = torch.zeros(1, 3, 3, 1, dtype=torch.float64, requires_grad=True)      # all ties, 3x3 / s1 SAME: 9 overlapping windows
    y = R.max_pool(x, (3, 3), (1, 1), "SAME")
    (g,) = torch.autograd.grad(y.sum(), x)
    # window (oy, ox) starts at (oy - 1, ox - 1); its first tap inside the map is (max(oy - 1, 0), max(ox - 1, 0))
    want = np.zeros((3, 3))
    for oy in range(3):
        for ox in range(3):
            want[max(oy - 1, 0), max(ox - 1, 0)] += 1
    assert np.array_equal(g[0, :, :, 0].numpy(), want)


# ---- shape inference ------------------------------------------------------------------------------------------------------------------
GEOMETRIES = [(28, 3, 1, 1, "VALID"), (7, 3, 2, 1, "VALID"), (8, 3, 2, 1, "VALID"), (9, 3, 1, 2, "VALID"), (5, 5, 1, 1, "VALID"),
              (6, 1, 1, 1, "VALID"), (7, 1, 3, 1, "VALID"), (9, 2, 2, 1, "VALID"), (7, 3, 2, 1, "SAME"), (8, 3, 2, 1, "SAME"),
              (9, 3, 1, 2, "SAME"), (3, 5, 1, 1, "SAME"), (7, 4, 3, 1, "SAME"), (6, 2, 2, 1, "SAME")]


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_graph_shapes_equal_the_shapes_torch_returns(geo):
    H, k, s, d, padding = geo
    W = H + 2                                                                  # (a second extent through the same rule)
    g = G.reset_default_graph()
    x = G.placeholder(G.KIND_F32, [None, H, W, 2], name="x_input")
    xt = _t(RNG.standard_normal((1, H, W, 2)))
    ho, wo, pt, pl = G.conv_geometry(H, W, (k, k), (s, s), (d, d), padding)
    assert (ho, wo, pt, pl) == R.geometry(H, W, (k, k), (s, s), (d, d), padding)
    with g.variable_scope("net"):
        if d == 1:
            c = layers.conv2D(x, "c", num_filters=3, kernel_size=(k, k), strides=(s, s), padding=padding)
            assert c.get_shape().as_list()[1:] == list(R.conv2d(xt, _t(np.zeros((k, k, 2, 3))), (s, s), (1, 1), padding).shape[1:])
            for mode, fn, ref in (("max", layers.maxpool2D, R.max_pool), ("avg", layers.averagepool2D, R.avg_pool)):
                p = fn(x, kernel_size=(k, k), strides=(s, s), padding=padding)
                assert p.get_shape().as_list()[1:] == list(ref(xt, (k, k), (s, s), padding).shape[1:]), mode
            # the transposed layer on the convolution's OUTPUT extent, asked for the convolution's input extent: always legal
            small = G.placeholder(G.KIND_F32, [None, ho, wo, 3], name="small")
            tc = layers.transposed_conv2D(small, "tc", kernel_size=(k, k), num_filters=2, strides=(s, s), padding=padding,
                                          output_shape=[None, H, W, 2])
            ref = R.conv2d_transpose(_t(np.zeros((1, ho, wo, 3))), _t(np.zeros((k, k, 2, 3))), (H, W), (s, s), padding)
            assert tc.get_shape().as_list()[1:] == list(ref.shape[1:]) == [H, W, 2]
        if s == 1:
            dc = layers.dilated_conv2D(x, "d", num_filters=3, kernel_size=(k, k), rate=d, padding=padding)
            assert dc.get_shape().as_list()[1:] == list(R.conv2d(xt, _t(np.zeros((k, k, 2, 3))), (1, 1), (d, d), padding).shape[1:])


# ---- the ValueError cases ---------------------------------------------------------------------------------------------------------------
def test_value_errors_of_the_tf_rules():
    g = G.reset_default_graph()
    x = G.placeholder(G.KIND_F32, [None, 4, 9, 2], name="x_input")
    with g.variable_scope("net"):
        with pytest.raises(ValueError, match="smaller than the window"):
            layers.conv2D(x, "a", kernel_size=(5, 5), padding="VALID")                         # in < k
        with pytest.raises(ValueError, match="smaller than the window"):
            layers.dilated_conv2D(x, "b", kernel_size=(3, 3), rate=2, padding="VALID")           # in = 4 < ke = 5
        with pytest.raises(ValueError, match="smaller than the window"):
            layers.maxpool2D(x, kernel_size=(5, 5), padding="VALID")
        with pytest.raises(ValueError, match="smaller than the window"):
            layers.averagepool2D(x, kernel_size=(5, 2), strides=(1, 1), padding="VALID")
        with pytest.raises(ValueError, match="SAME.*VALID"):
            layers.conv2D(x, "c", padding="FULL")
        with pytest.raises(ValueError, match="SAME.*VALID"):
            layers.maxpool2D(x, padding="FULL")
        # output_shape None is input * strides: under VALID legal only for k <= s, and the message names the legal range
        with pytest.raises(ValueError, match=r"legal output extents are 9\.\.10"):
            layers.transposed_conv2D(x, "d", kernel_size=(3, 3), strides=(2, 2), padding="VALID")   # n = 4: [3 * 2 + 3, + 1]
        with pytest.raises(ValueError, match=r"legal output extents are 10\.\.11"):
            layers.transposed_conv2D(x, "e", kernel_size=(4, 4), strides=(2, 2), padding="VALID")
        ok = layers.transposed_conv2D(x, "f", kernel_size=(2, 2), strides=(2, 2), padding="VALID")   # k == s
        assert ok.get_shape().as_list()[1:3] == [8, 18]
        ok = layers.transposed_conv2D(x, "f1", kernel_size=(1, 1), strides=(2, 2), padding="VALID")  # k < s: the last row is bias only
        assert ok.get_shape().as_list()[1:3] == [8, 18]
        # explicit output shapes: the whole legal range and not one more
        for O, legal in ((9, False), (10, True), (11, True), (12, False)):
            shape = [None, O, (9 - 1) * 2 + 4, 2]                                                # W = 20: the lower end of its range
            if legal:
                t = layers.transposed_conv2D(x, "g%d" % O, kernel_size=(4, 4), strides=(2, 2), padding="VALID", output_shape=shape)
                assert t.get_shape().as_list()[1:3] == [O, 20]
            else:
                with pytest.raises(ValueError, match=r"legal output extents are 10\.\.11"):
                    layers.transposed_conv2D(x, "g%d" % O, kernel_size=(4, 4), strides=(2, 2), padding="VALID", output_shape=shape)
        for O, legal in ((6, False), (7, True), (8, True), (9, False)):                          # SAME: ceil(O / 2) == 4
            shape = [None, O, 18, 2]
            if legal:
                t = layers.transposed_conv2D(x, "h%d" % O, output_shape=shape)
                assert t.get_shape().as_list()[1:3] == [O, 18]
            else:
                with pytest.raises(ValueError, match=r"legal output extents are 7\.\.8"):
                    layers.transposed_conv2D(x, "h%d" % O, output_shape=shape)


def test_reference_refuses_what_the_graph_refuses():
    with pytest.raises(ValueError):
        R.conv2d(_t(np.zeros((1, 4, 9, 2))), _t(np.zeros((5, 5, 2, 1))), padding="VALID")
    with pytest.raises(ValueError):
        R.conv2d_transpose(_t(np.zeros((1, 4, 4, 2))), _t(np.zeros((3, 3, 1, 2))), (8, 8), (2, 2), "VALID")
    for n, k, s in ((4, 4, 2), (3, 3, 2), (5, 2, 2), (2, 5, 3)):
        for padding in ("SAME", "VALID"):
            lo, hi = R.transpose_legal_range(n, k, s, padding)
            legal = [O for O in range(1, 40) if (padding == "SAME" or O >= k) and R.axis_geometry(O, k, s, 1, padding)[0] == n]
            assert legal == list(range(lo, hi + 1)), (n, k, s, padding)


# ---- calls accepted before build the node types they built before (passes with and without the feature) ---------------------------------
def test_calls_accepted_before_build_the_old_nodes():
    g = G.reset_default_graph()
    x = G.placeholder(G.KIND_F32, [None, 9, 7, 4], name="x_input")
    with g.variable_scope("net"):
        m = layers.maxpool2D(x)
        a = layers.averagepool2D(x)
        m2 = layers.maxpool2D(x, kernel_size=(2, 2), strides=(2, 2), padding="SAME")
        c1 = layers.conv2D(x, "c1", kernel_size=(1, 1))
        c3 = layers.conv2D(x, "c3", normalisation=tfnorm.batch_norm, training=True)
        cs = layers.conv2D(x, "cs", strides=(2, 2))
        c5 = layers.conv2D(x, "c5", kernel_size=(5, 5))
        dc = layers.dilated_conv2D(x, "dc", rate=3)
        tc = layers.transposed_conv2D(x, "tc")
        tcs = layers.transposed_conv2D(x, "tcs", kernel_size=(3, 3), strides=(2, 2), output_shape=[None, 18, 14, 32])
        hd = layers.conv2D(x, "hd", kernel_size=(1, 1), num_filters=2, activation=act.identity)
    assert (m.op.type, m.op.attrs) == ("maxpool", {}) and (m2.op.type, m2.op.attrs) == ("maxpool", {})
    assert (a.op.type, a.op.attrs) == ("avgpool", {})
    keys = {"W", "b", "ksize", "norm", "norm_vars", "act", "training", "num_groups", "head", "transposed", "general", "volume"}
    for t in (c1, c3, cs, c5, dc, tc, tcs, hd):
        assert t.op.type == "conv_unit" and set(t.op.attrs) == keys, t
    for t in (c1, c3, hd):                                                     # stride-1 1x1 and 3x3 SAME: the MFMA / direct / head routes
        assert t.op.attrs["general"] is None and t.op.attrs["transposed"] is None and t.op.attrs["volume"] is None
    assert hd.op.attrs["head"] and hd.kind == G.KIND_F32 and c3.op.attrs["norm"] == "batch" and c3.op.attrs["b"] is None
    assert cs.op.attrs["general"] == (3, 3, 2, 2, 1, 1) and c5.op.attrs["general"] == (5, 5, 1, 1, 1, 1)
    assert dc.op.attrs["general"] == (3, 3, 1, 1, 3, 3)
    assert tc.op.attrs["transposed"] == (4, 4, 2, 2) and tcs.op.attrs["transposed"] == (3, 3, 2, 2)
    assert tc.get_shape().as_list() == [None, 18, 14, 32] and cs.get_shape().as_list() == [None, 5, 4, 32]


def test_new_argument_values_build_the_new_nodes():
    g = G.reset_default_graph()
    x = G.placeholder(G.KIND_F32, [None, 9, 7, 4], name="x_input")
    with g.variable_scope("net"):
        c = layers.conv2D(x, "c", num_filters=8, padding="VALID", normalisation=tfnorm.batch_norm, training=True)
        d = layers.dilated_conv2D(x, "d", num_filters=8, rate=2, padding="VALID")
        t = layers.transposed_conv2D(c, "t", kernel_size=(3, 3), num_filters=6, padding="VALID", output_shape=[None, 15, 12, 6])
        h = layers.conv2D(x, "h", num_filters=2, kernel_size=(1, 1), padding="VALID", activation=act.identity)
        p = layers.maxpool2D(x, kernel_size=(3, 3))
        q = layers.averagepool2D(x, kernel_size=(3, 2), strides=(2, 1), padding="VALID")
    assert c.op.attrs["explicit"] == ("conv", 3, 3, 1, 1, 1, 1, 7, 5, 0, 0) and c.get_shape().as_list() == [None, 7, 5, 8]
    assert c.op.attrs["b"] is None and g.variables["net/c/W"].shape == (3, 3, 4, 8)           # conv2D drops the bias in front of batch norm
    assert d.op.attrs["explicit"] == ("conv", 3, 3, 1, 1, 2, 2, 5, 3, 0, 0) and "net/d/b" in g.variables
    assert t.op.attrs["explicit"] == ("tconv", 3, 3, 2, 2, 1, 1, 15, 12, 0, 0) and g.variables["net/t/W"].shape == (3, 3, 6, 8)
    assert t.get_shape().as_list() == [None, 15, 12, 6]
    assert h.kind == G.KIND_ACT and not h.op.attrs["head"]                     # (an explicit unit is a hidden layer: the plan's storage)
    assert (p.op.type, p.op.attrs) == ("pool2d", dict(mode="max", window=(3, 3), strides=(2, 2), pad=(1, 1)))
    assert p.get_shape().as_list() == [None, 5, 4, 4]
    assert (q.op.type, q.op.attrs) == ("pool2d", dict(mode="avg", window=(3, 2), strides=(2, 1), pad=(0, 0)))
    assert q.get_shape().as_list() == [None, 4, 6, 4]
    assert [n for n, prm in inspect.signature(layers.maxpool2D).parameters.items()] == ["x", "kernel_size", "strides", "padding"]


def test_header_and_sources():
    from phiseg_code_amd import runtime as rt
    protos = rt.parse_header()
    want = dict(phx_conv2d_geometry=13, phx_conv2d_pad_fwd=23, phx_conv2d_pad_dgrad=21, phx_conv2d_pad_wgrad=22,
                phx_conv2d_pad_wgrad_ws_floats=7, phx_tconv2d_pad_fwd=23, phx_tconv2d_pad_dgrad=21, phx_tconv2d_pad_wgrad=22,
                phx_pool2d_fwd=17, phx_pool2d_bwd=18, phx_pool2d_bwd_acc=18)
    for name, nargs in want.items():
        assert name in protos and len(protos[name]) == nargs, name
    assert "conv2d_pad.hip" in open(rt.HEADER.replace("include/phx.h", "phiseg_code_amd/csrc/SOURCES")).read().split()
