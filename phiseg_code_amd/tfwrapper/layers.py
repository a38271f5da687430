"""Layer wrappers -- counterpart of the reference's tfwrapper/layers.py with the same signatures.

Hot-path layers (surface B1): ``conv2D`` (layers.py:94-145), ``averagepool2D`` (44-54),
``bilinear_upsample2D`` (336-345), ``global_averagepool2D`` (70-78), ``crop_and_concat`` (586-622),
``nearest_neighbour_upsample2D`` (326-333).  Every call adds nodes to ``phiseg_code_amd.graph``; the arithmetic
runs in hand-written HIP kernels (libphx.so).  The layers that no PHiSeg configuration calls are implemented as well, on direct
kernels: strided / dilated / transposed convolutions, residual units, dense, max pool, pad and crop (csrc/gconv.hip, csrc/tconv.hip),
and the 3-D family -- ``conv3D``, ``transposed_conv3D``, ``maxpool3D``, ``bilinear_upsample3D`` and the 5-D branch of
``crop_and_concat`` on NDHWC tensors [B, D, H, W, C] (csrc/conv3d.hip).  3-D units take tfnorm.identity or
tfnorm.batch_norm; what a layer does not support raises NotImplementedError with the reason.  Every ``activation=`` also takes
``activations.leaky_relu`` (or a ``functools.partial`` of it with ``alpha``): the unit then carries the identity and a
``graph.leaky_relu`` node follows it; ``normalise_post_activation=True`` is the unit without normalisation followed by a
normalisation node (``_unit``).  The 2-D convolutions and pools take ``padding="VALID"`` as well as ``"SAME"``,
``transposed_conv2D`` any legal ``output_shape``, and the pools any window and strides: such a call builds a unit (or a ``pool2d``
node) that carries its whole geometry, by TF 1.12's rule (``graph.conv_geometry``), and runs on csrc/conv2d_pad.hip; what TF refuses
when the graph is built -- an input smaller than the window under VALID, an output shape the forward convolution does not map back to
the input -- is a ValueError here too.  Calls with the values accepted before build the nodes they always built.
"""
import logging

import numpy as np

from phiseg_code_amd import graph as G
from phiseg_code_amd.tfwrapper import activations
from phiseg_code_amd.tfwrapper import normalisation as tfnorm
from phiseg_code_amd.tfwrapper import utils

# Will be used as default in all the layers below (reference: tf.nn.relu)
STANDARD_NONLINEARITY = activations.relu


def averagepool2D(x, kernel_size=(2, 2), strides=(2, 2), padding="SAME"):
    """tf.nn.avg_pool (tfwrapper/layers.py:44-54): any window, strides and padding ("SAME" | "VALID"); a window that reaches into the
    padding divides by the number of taps inside the map.  The default 2x2 / stride 2 / SAME is the hot path's own node; anything else
    is a graph.pool2d node (csrc/conv2d_pad.hip)."""
    if tuple(kernel_size) == (2, 2) and tuple(strides) == (2, 2) and padding == "SAME":
        return G.avg_pool2x2(x)
    return G.pool2d(x, "avg", kernel_size, strides, padding)


def global_averagepool2D(x, name=None):
    return G.global_average_pool(x, name=name)


def global_averagepool3D(x, name=None):
    """tf.reduce_mean(x, axis=(1, 2, 3)) (tfwrapper/layers.py:81-91): [B, D, H, W, C] -> [B, C], as the 2-D pool of the same memory seen
    as [B, D * H, W, C] (fold_depth: a view, no launch)."""
    if len(x.get_shape().as_list()) != 5:
        raise ValueError("global_averagepool3D: a [B, D, H, W, C] tensor is expected, got %r" % (x,))
    return G.global_average_pool(G.fold_depth(x), name=name)


def _check_callables(normalisation, activation):
    if normalisation not in tfnorm.KIND:
        raise ValueError("Unknown normalisation callable %r" % (normalisation,))
    if not activations.known(activation):
        raise ValueError("Unknown activation callable %r" % (activation,))
    alpha = activations.leaky_alpha(activation)
    if alpha is not None and not 0.0 < alpha < 1.0:      # (before any variable is made; graph.leaky_relu has the last word)
        raise ValueError("leaky_relu: alpha must lie in (0, 1), got %r" % (alpha,))


def _leaky(op, alpha):
    """the leaky_relu node behind a unit that carries the identity (alpha None: any other activation, which the unit applied itself)"""
    return op if alpha is None else G.leaky_relu(op, alpha)


def _unit(x, weights, biases, ksize, kind, norm_vars, activation, training, num_groups, head, name, post=False, **geometry):
    """conv -> [bias] -> normalisation -> activation as ONE conv_unit node; or -- `post` (normalise_post_activation) with a normalisation
    to apply -- conv -> [bias] -> activation as the unit and a normalisation node behind it under the same scope (the way _volume_unit
    has always built it).  leaky_relu is a node of its own behind a unit that carries the identity; such a unit is a hidden layer, never
    a head, so it keeps the plan's activation storage."""
    an, alpha = activations.unit_act(activation)
    if post and kind is not None:
        op = G.conv_unit(x, weights, biases, ksize, None, {}, an, training, head=False, name=name, **geometry)
        return G.norm_act(_leaky(op, alpha), kind, norm_vars, 'identity', training, num_groups=num_groups, name='norm')
    op = G.conv_unit(x, weights, biases, ksize, kind, norm_vars, an, training, num_groups=num_groups, head=head and alpha is None,
                     name=name, **geometry)
    return _leaky(op, alpha)


def _valid_geometry(x, what, kernel_size, strides, dilations, padding):
    """None under SAME padding (the layer keeps the unit form it has always built); under VALID the `explicit` geometry of
    graph.conv_unit, form "conv", from graph.conv_geometry."""
    if padding == "SAME":
        return None
    if padding != "VALID":
        raise ValueError("%s: padding must be 'SAME' or 'VALID', got %r" % (what, padding))
    shp = x.get_shape().as_list()
    if len(shp) != 4:
        raise ValueError("%s: a [B, H, W, C] tensor is expected, got %s" % (what, shp))
    k, s, d = (tuple(int(v) for v in t) for t in (kernel_size, strides, dilations))
    return ("conv",) + k + s + d + G.conv_geometry(shp[1], shp[2], k, s, d, "VALID")


def conv2D(x,
           name,
           kernel_size=(3, 3),
           num_filters=32,
           strides=(1, 1),
           activation=STANDARD_NONLINEARITY,
           normalisation=tfnorm.identity,
           normalise_post_activation=False,
           dropout_p=None,
           padding="SAME",
           weight_init='he_normal',
           add_bias=True,
           **kwargs):
    """Standard 2-D convolutional layer: conv -> [bias] -> normalisation -> activation (normalise_post_activation: activation ->
    normalisation) [-> dropout].  kwargs can carry ``training`` and normalisation parameters (``num_groups``).  padding "SAME" or
    "VALID" (out = (in - k) // s + 1, no padding: the unpadded convolutions of the classic U-Net, on csrc/conv2d_pad.hip); an input
    smaller than the kernel under VALID is a ValueError."""
    explicit = _valid_geometry(x, "conv2D", kernel_size, strides, (1, 1), padding)
    # stride 1 with a 1x1 / 3x3 kernel is the hot path (MFMA / direct / head kernels); anything else -- strided convolutions of the
    # residual units, larger kernels -- runs on the general direct kernels of csrc/gconv.hip
    general = None
    if explicit is None and (tuple(strides) != (1, 1) or tuple(kernel_size) not in ((1, 1), (3, 3))):
        general = (int(kernel_size[0]), int(kernel_size[1]), int(strides[0]), int(strides[1]), 1, 1)
    _check_callables(normalisation, activation)

    bottom_num_filters = x.get_shape().as_list()[-1]
    weight_shape = [kernel_size[0], kernel_size[1], bottom_num_filters, num_filters]
    bias_shape = [num_filters]
    g = G.get_default_graph()

    with g.variable_scope(name):
        weights = utils.get_weight_variable(weight_shape, name='W', type=weight_init, regularize=True)
        biases = None
        if add_bias and normalisation in (tfnorm.batch_norm, tfnorm.batch_renorm):
            # (decided before the order of normalisation and activation is looked at, as in the reference: layers.py:126-128.)
            # (batch_renorm: the reference keeps the bias there; with r and d constant for the gradient it gets none and stays at its
            # zero initial value, so leaving it out changes no result -- DESIGN.md section 7f)
            logging.debug('Turning of bias because using batch norm.')
            add_bias = False
        if add_bias:
            biases = utils.get_bias_variable(bias_shape, name='b')
        kind = tfnorm.KIND[normalisation]
        norm_vars = tfnorm.make_variables(kind, num_filters)
        training = kwargs.get('training', True)
        # heads (mu / sigma / logits) keep fp32 storage in the bf16 configuration
        head = kind is None and activation is not activations.relu and general is None and explicit is None
        geometry = dict(general=general) if explicit is None else dict(explicit=explicit)
        op = _unit(x, weights, biases, kernel_size[0], kind, norm_vars, activation, training, kwargs.get('num_groups'), head, 'conv',
                   post=normalise_post_activation, **geometry)
        if dropout_p is not None:
            op = dropout(op, keep_prob=dropout_p, training=training)
        return op


def dilated_conv2D(bottom,
                   name,
                   kernel_size=(3, 3),
                   num_filters=32,
                   rate=2,
                   activation=STANDARD_NONLINEARITY,
                   normalisation=tfnorm.identity,
                   normalise_post_activation=False,
                   dropout_p=None,
                   padding="SAME",
                   weight_init='he_normal',
                   add_bias=True,
                   **kwargs):
    """tfwrapper/layers.py:378-425: tf.nn.atrous_conv2d(bottom, W, rate, SAME) -> [bias] -> normalisation -> activation
    (normalise_post_activation: activation -> normalisation) [-> dropout].  (Unlike conv2D the bias is kept in front of batch_norm,
    layers.py:406-409.)  padding "SAME" or "VALID": the output shrinks by (k - 1) * rate per axis under VALID."""
    explicit = _valid_geometry(bottom, "dilated_conv2D", kernel_size, (1, 1), (rate, rate), padding)
    _check_callables(normalisation, activation)
    cin = bottom.get_shape().as_list()[3]
    g = G.get_default_graph()
    with g.variable_scope(name):
        weights = utils.get_weight_variable([kernel_size[0], kernel_size[1], cin, num_filters], name='W', type=weight_init,
                                            regularize=True)
        biases = utils.get_bias_variable([num_filters], name='b') if add_bias else None
        kind = tfnorm.KIND[normalisation]
        norm_vars = tfnorm.make_variables(kind, num_filters)
        training = kwargs.get('training', True)
        geometry = dict(explicit=explicit) if explicit is not None else \
            dict(general=(int(kernel_size[0]), int(kernel_size[1]), 1, 1, int(rate), int(rate)))
        op = _unit(bottom, weights, biases, kernel_size[0], kind, norm_vars, activation, training, kwargs.get('num_groups'), False,
                   'atrous', post=normalise_post_activation, **geometry)
        if dropout_p is not None:
            op = dropout(op, keep_prob=dropout_p, training=training)
        return op


def dense_layer(bottom,
                name,
                hidden_units=512,
                activation=STANDARD_NONLINEARITY,
                normalisation=tfnorm.batch_norm,
                normalise_post_activation=False,
                dropout_p=None,
                weight_init='he_normal',
                add_bias=True,
                **kwargs):
    """tfwrapper/layers.py:539-582: flatten -> matmul with W [F, hidden_units] -> [bias] -> normalisation -> activation
    (normalise_post_activation: activation -> normalisation) [-> dropout].  Runs as a 1x1 convolution of the flattened input; the
    result keeps two unit axes: [B, 1, 1, hidden_units] (same memory as the reference's [B, hidden_units])."""
    _check_callables(normalisation, activation)
    flat = G.flatten(bottom)
    f = flat.get_shape().as_list()[3]
    g = G.get_default_graph()
    with g.variable_scope(name):
        weights = utils.get_weight_variable([f, hidden_units], name='W', type=weight_init, regularize=True)
        biases = utils.get_bias_variable([hidden_units], name='b') if add_bias else None
        kind = tfnorm.KIND[normalisation]
        norm_vars = tfnorm.make_variables(kind, hidden_units)
        training = kwargs.get('training', True)
        op = _unit(flat, weights, biases, 1, kind, norm_vars, activation, training, kwargs.get('num_groups'), False, 'dense',
                   post=normalise_post_activation, general=(1, 1, 1, 1, 1, 1))
        if dropout_p is not None:
            op = dropout(op, keep_prob=dropout_p, training=training)
        return op


def _conv_norm(x, conv_name, norm_scope, num_filters, strides, kernel_size, normalisation, activation, add_bias, kwargs):
    """conv2D(x, conv_name, activation=identity, add_bias=add_bias) -> normalisation(., scope=norm_scope) -> activation, as the
    residual units spell it (layers.py:452-460): the convolution's variables live under conv_name, the normalisation's under
    norm_scope, and the bias is kept even in front of batch norm."""
    g = G.get_default_graph()
    cin = x.get_shape().as_list()[-1]
    with g.variable_scope(conv_name):
        weights = utils.get_weight_variable([kernel_size[0], kernel_size[1], cin, num_filters], name='W', type='he_normal',
                                            regularize=True)
        biases = utils.get_bias_variable([num_filters], name='b') if add_bias else None
    kind = tfnorm.KIND[normalisation]
    norm_vars = tfnorm.make_variables(kind, num_filters, scope=norm_scope)
    general = None
    if tuple(strides) != (1, 1) or tuple(kernel_size) not in ((1, 1), (3, 3)):
        general = (int(kernel_size[0]), int(kernel_size[1]), int(strides[0]), int(strides[1]), 1, 1)
    return _unit(x, weights, biases, kernel_size[0], kind, norm_vars, activation, kwargs.get('training', True), kwargs.get('num_groups'),
                 False, conv_name, general=general)


def _residual_skip(x, num_filters, down_sample, projection, strides, activation, normalisation, add_bias, kwargs):
    """the skip path both residual units share (layers.py:462-472, 520-530)"""
    cin = x.get_shape().as_list()[-1]
    if cin == num_filters and not down_sample:
        return x
    if projection:
        return _conv_norm(x, 'projection', 'bn_projection', num_filters, strides, (1, 1), normalisation, activation, add_bias, kwargs)
    pad = (num_filters - cin) // 2
    _, h, w, _ = x.get_shape().as_list()
    s = 2 if down_sample else 1
    # tf.pad along the channel axis, then identity[:, ::2, ::2, :]: one strided window
    return G.window4(x, -(-h // s), -(-w // s), cin + 2 * pad, stride=(s, s), off=(0, 0, -pad), name='identity')


def residual_unit2D(x,
                    name,
                    num_filters=32,
                    down_sample=False,
                    projection=False,
                    activation=STANDARD_NONLINEARITY,
                    normalisation=tfnorm.batch_norm,
                    add_bias=True,
                    **kwargs):
    """tfwrapper/layers.py:428-478 (https://arxiv.org/abs/1512.03385): conv1 -> bn1 -> act -> conv2 -> bn2, + skip, -> act."""
    _check_callables(normalisation, activation)
    an, alpha = activations.unit_act(activation)
    strides = (2, 2) if down_sample else (1, 1)
    g = G.get_default_graph()
    with g.variable_scope(name):
        conv1 = _conv_norm(x, 'conv1', 'bn1', num_filters, strides, (3, 3), normalisation, activation, add_bias, kwargs)
        conv2 = _conv_norm(conv1, 'conv2', 'bn2', num_filters, (1, 1), (3, 3), normalisation, activations.identity, add_bias, kwargs)
        skip = _residual_skip(x, num_filters, down_sample, projection, strides, activation, normalisation, add_bias, kwargs)
        if skip.get_shape().as_list()[-1] != num_filters:
            raise ValueError("residual_unit2D: channel padding needs an even difference (%d -> %d)"
                             % (x.get_shape().as_list()[-1], num_filters))
        return _leaky(G.add_act(skip, conv2, an, name='add'), alpha)


def identity_residual_unit2D(x,
                             name,
                             num_filters,
                             down_sample=False,
                             projection=True,
                             activation=STANDARD_NONLINEARITY,
                             normalisation=tfnorm.batch_norm,
                             add_bias=True,
                             **kwargs):
    """tfwrapper/layers.py:481-536 (identity mappings, pre-activation order): bn1 -> act -> conv1 -> bn2 -> act -> conv2, + skip."""
    _check_callables(normalisation, activation)
    cin = x.get_shape().as_list()[-1]
    if not projection:
        assert (cin == num_filters) or (cin * 2 == num_filters), \
            'Number of filters must remain constant, or be increased by a ' \
            'factor of 2. In filters: %d, Out filters: %d' % (cin, num_filters)
    strides = (2, 2) if down_sample else (1, 1)
    training = kwargs.get('training', True)
    kind = tfnorm.KIND[normalisation]
    an, alpha = activations.unit_act(activation)
    g = G.get_default_graph()

    def conv(t, cname, st):
        with g.variable_scope(cname):
            ci = t.get_shape().as_list()[-1]
            weights = utils.get_weight_variable([3, 3, ci, num_filters], name='W', type='he_normal', regularize=True)
            biases = utils.get_bias_variable([num_filters], name='b') if add_bias else None
        general = (3, 3, st[0], st[1], 1, 1) if tuple(st) != (1, 1) else None
        return G.conv_unit(t, weights, biases, 3, None, {}, 'identity', training, head=False, name=cname, general=general)
    with g.variable_scope(name):
        op1 = G.norm_act(x, kind, tfnorm.make_variables(kind, cin, scope='bn1'), an, training, kwargs.get('num_groups'), name='bn1')
        op1 = conv(_leaky(op1, alpha), 'conv1', strides)
        op2 = G.norm_act(op1, kind, tfnorm.make_variables(kind, num_filters, scope='bn2'), an, training, kwargs.get('num_groups'),
                         name='bn2')
        op2 = conv(_leaky(op2, alpha), 'conv2', (1, 1))
        skip = _residual_skip(x, num_filters, down_sample, projection, strides, activation, normalisation, add_bias, kwargs)
        return G.add_act(skip, op2, 'identity', name='add')


def reshape_pool2D_layer(x):
    """tfwrapper/layers.py:57-67: space-to-depth by strided slices, concat([x[:,0::2,0::2], x[:,1::2,0::2], x[:,0::2,1::2],
    x[:,1::2,1::2]], axis=3)."""
    _, h, w, c = x.get_shape().as_list()
    if h % 2 or w % 2:
        raise ValueError("reshape_pool2D_layer: even spatial sizes (tf.concat of unequal slices fails in the reference too)")
    parts = [G.window4(x, h // 2, w // 2, c, stride=(2, 2), off=(oy, ox, 0), name='slice') for (oy, ox) in ((0, 0), (1, 0), (0, 1), (1, 1))]
    out = parts[0]
    for t in parts[1:]:
        out = G.concat([out, t], axis=-1)
    return out


def maxpool2D(x, kernel_size=(2, 2), strides=(2, 2), padding="SAME"):
    """tf.nn.max_pool (tfwrapper/layers.py:18-28): any window, strides and padding ("SAME" | "VALID"); padded taps take no part in the
    maximum and the gradient goes to the first maximum of a window in row-major order.  The reference's default 2x2 / stride 2 / SAME
    keeps its own node; anything else is a graph.pool2d node (csrc/conv2d_pad.hip)."""
    if tuple(kernel_size) == (2, 2) and tuple(strides) == (2, 2) and padding == "SAME":
        return G.max_pool2x2(x)
    return G.pool2d(x, "max", kernel_size, strides, padding)


def pad_to_size(bottom, output_size):
    """tfwrapper/layers.py:625-650: zero-pad the spatial axes of `bottom` to output_size = [B, H, W, C] (the odd pixel goes to the
    bottom / right)."""
    shp = bottom.get_shape().as_list()
    if len(shp) != 4:
        raise NotImplementedError('pad_to_size has not been extended to 3D (neither in the reference)')
    dy, dx = int(output_size[1]) - shp[1], int(output_size[2]) - shp[2]
    if dy < 0 or dx < 0:
        raise ValueError("pad_to_size: output smaller than input")
    return G.spatial_window(bottom, output_size[1], output_size[2], -(dy // 2), -(dx // 2), name='pad_to_size')


def dropout(bottom, keep_prob, training):
    """tfwrapper/layers.py:653-668: tf.nn.dropout(bottom, keep_prob) while training, identity otherwise."""
    g = G.get_default_graph()
    with g.variable_scope('dropout_layer'):
        return G.dropout(bottom, keep_prob, training)


def transposed_conv2D(bottom,
                      name,
                      kernel_size=(4, 4),
                      num_filters=32,
                      strides=(2, 2),
                      output_shape=None,
                      activation=STANDARD_NONLINEARITY,
                      normalisation=tfnorm.identity,
                      normalise_post_activation=False,
                      dropout_p=None,
                      padding="SAME",
                      weight_init='he_normal',
                      add_bias=True,
                      **kwargs):
    """Standard 2-D transposed convolution (tfwrapper/layers.py:197-258): tf.nn.conv2d_transpose with a [kh, kw, num_filters,
    bottom channels] filter, default behaviour up-samples by a factor of 2; -> [bias] -> normalisation -> activation
    (normalise_post_activation: activation -> normalisation) [-> dropout].  Unlike conv2D the reference keeps the bias here even in
    front of batch_norm (layers.py:231-234).  padding "SAME" or "VALID".  output_shape None is input * strides as in the reference (under
    VALID legal only for kernel <= stride, e.g. the 2x2 / stride 2 up-convolution of the classic U-Net); an explicit output_shape
    [B, Ho, Wo, C] may be any extent the forward convolution maps back to the input -- SAME: ceil(O / s) == n; VALID: O in
    [(n - 1) s + k, (n - 1) s + k + s - 1] -- and anything else is a ValueError that names the legal range.  Rows of the output that no
    input reaches hold the bias only."""
    _check_callables(normalisation, activation)
    shp = bottom.get_shape().as_list()
    k, st = tuple(int(v) for v in kernel_size), tuple(int(v) for v in strides)
    explicit = None
    if padding != "SAME" or (output_shape is not None and tuple(output_shape[1:3]) != (shp[1] * st[0], shp[2] * st[1])):
        # (SAME with the default extent keeps the unit form it has always built, on csrc/tconv.hip)
        out_hw = None if output_shape is None else tuple(int(v) for v in output_shape[1:3])
        explicit = ("tconv",) + k + st + (1, 1) + G.conv_transpose_geometry(shp[1], shp[2], k, st, padding, out_hw)
    weight_shape = [kernel_size[0], kernel_size[1], num_filters, shp[3]]
    g = G.get_default_graph()
    with g.variable_scope(name):
        weights = utils.get_weight_variable(weight_shape, name='W', type=weight_init, regularize=True)
        biases = utils.get_bias_variable([num_filters], name='b') if add_bias else None
        kind = tfnorm.KIND[normalisation]
        norm_vars = tfnorm.make_variables(kind, num_filters)
        training = kwargs.get('training', True)
        geometry = dict(explicit=explicit) if explicit is not None else dict(transposed=k + st)
        op = _unit(bottom, weights, biases, kernel_size[0], kind, norm_vars, activation, training, kwargs.get('num_groups'), False,
                   'deconv', post=normalise_post_activation, **geometry)
        if dropout_p is not None:
            op = dropout(op, keep_prob=dropout_p, training=training)
        return op


def nearest_neighbour_upsample2D(x, factor):
    shp = x.get_shape().as_list()
    return G.resize_nearest(x, (shp[1] * factor, shp[2] * factor))


def bilinear_upsample2D(x, name, factor):
    """tf.image.resize_images(x, [f*h, f*w]) = TF 1.12 ResizeBilinear(align_corners=False), legacy coordinates."""
    if factor != 2:
        raise NotImplementedError("hot path: factor 2")
    with G.get_default_graph().variable_scope(name):
        return G.bilinear_up2x(x, name="ResizeBilinear")


def crop_and_concat(inputs, axis=-1):
    """tfwrapper/layers.py:586-622: the first feature map defines the output size, the others are centre-cropped to it
    (start = (larger - output) // 2) and everything is concatenated along the channel axis."""
    if len(inputs[0].get_shape().as_list()) == 5:
        return _crop_and_concat3D(inputs, axis)
    if axis not in (-1, 3):
        raise ValueError("crop_and_concat: channel axis only")
    out_size = inputs[0].get_shape().as_list()[1:3]
    out = inputs[0]
    for t in inputs[1:]:
        larger = t.get_shape().as_list()[1:3]
        if larger != out_size:
            if larger[0] < out_size[0] or larger[1] < out_size[1]:
                raise ValueError("crop_and_concat: %s cannot be cropped to %s" % (larger, out_size))
            t = G.spatial_window(t, out_size[0], out_size[1], (larger[0] - out_size[0]) // 2, (larger[1] - out_size[1]) // 2,
                                 name='crop')
        out = G.concat([out, t], axis=-1)
    return out


def _crop_and_concat3D(inputs, axis):
    """the 5-D branch of crop_and_concat (tfwrapper/layers.py:609-612): centre crop on three axes"""
    if axis not in (-1, 4):
        raise ValueError("crop_and_concat: channel axis only")
    out_size = inputs[0].get_shape().as_list()[1:4]
    out = inputs[0]
    for t in inputs[1:]:
        larger = t.get_shape().as_list()[1:4]
        if larger != out_size:
            if any(l < o for l, o in zip(larger, out_size)):
                raise ValueError("crop_and_concat: %s cannot be cropped to %s" % (larger, out_size))
            t = G.spatial_window3d(t, out_size, [(l - o) // 2 for l, o in zip(larger, out_size)], name='crop')
        out = G.concat([out, t], axis=-1)
    return out


# ---- the 3-D layer family (kernels in csrc/conv3d.hip) -------------------------------------------------------
def maxpool3D(x, kernel_size=(2, 2, 2), strides=(2, 2, 2), padding="SAME"):
    """tf.nn.max_pool3d, SAME (tfwrapper/layers.py:31-41): window = stride, each entry 1 or 2 -- 2x2x2 by default, (1, 2, 2) for
    anisotropic volumes."""
    if tuple(kernel_size) != tuple(strides) or any(k not in (1, 2) for k in kernel_size) or len(kernel_size) != 3 or padding != "SAME":
        raise NotImplementedError("maxpool3D: window = stride with entries 1 or 2, SAME")
    return G.max_pool3d(x, kernel_size)


def _volume_unit(x, name, form, kernel_size, num_filters, strides, activation, normalisation, normalise_post_activation, dropout_p,
                 weight_init, add_bias, kwargs):
    """What conv3D and transposed_conv3D share: W (and b, kept even in front of batch norm: layers.py:178-181, 307-310) under `name`,
    conv -> bias -> normalisation -> activation as one unit, or -- normalise_post_activation -- the unit with the activation and no
    normalisation followed by a normalisation node under the same scope, then dropout."""
    _check_callables(normalisation, activation)
    kind = tfnorm.KIND[normalisation]
    if kind not in (None, "batch"):
        why = {"group": "group_norm2D reshapes a rank-4 tensor and fails on a volume in the reference itself",
               "instance": "instance_norm2D takes its moments over axes (1, 2) only and misreads a volume in the reference itself",
               "layer": "layer_norm's default axes (1, 2, 3) leave out the W axis of a volume",
               "renorm": "batch_renorm on volumes is left for later"}[kind]
        raise NotImplementedError("%s: %s" % (name, why))
    shp = x.get_shape().as_list()
    if len(shp) != 5:
        raise ValueError("%s: a [B, D, H, W, C] tensor is expected, got %s" % (name, shp))
    kd, kh, kw = (int(k) for k in kernel_size)
    cin = shp[4]
    weight_shape = [kd, kh, kw, cin, num_filters] if form == "conv" else [kd, kh, kw, num_filters, cin]
    g = G.get_default_graph()
    training = kwargs.get('training', True)
    volume = (form, kd, kh, kw) + tuple(int(s) for s in strides)
    with g.variable_scope(name):
        weights = utils.get_weight_variable(weight_shape, name='W', type=weight_init, regularize=True)
        biases = utils.get_bias_variable([num_filters], name='b') if add_bias else None
        norm_vars = tfnorm.make_variables(kind, num_filters)
        # heads (identity normalisation, activation other than relu) keep fp32 storage in the bf16 configuration, as in conv2D
        head = kind is None and activation is not activations.relu
        uname = 'conv' if form == "conv" else 'deconv'
        op = _unit(x, weights, biases, kd, kind, norm_vars, activation, training, None, head, uname, post=normalise_post_activation,
                   volume=volume)
        if dropout_p is not None:
            op = dropout(op, keep_prob=dropout_p, training=training)
        return op


def conv3D(x,
           name,
           kernel_size=(3,3,3),
           num_filters=32,
           strides=(1,1,1),
           activation=STANDARD_NONLINEARITY,
           normalisation=tfnorm.identity,
           normalise_post_activation=False,
           dropout_p=None,
           padding="SAME",
           weight_init='he_normal',
           add_bias=True,
           **kwargs):
    """Standard 3-D convolutional layer (tfwrapper/layers.py:148-194): tf.nn.conv3d, SAME -> [bias] -> normalisation -> activation
    (or activation -> normalisation with normalise_post_activation) [-> dropout].  W is [kd, kh, kw, Cin, num_filters]; unlike conv2D
    the reference keeps the bias in front of batch norm here (lines 178-181).  kwargs can carry ``training``."""
    if padding != "SAME":
        raise NotImplementedError("conv3D: SAME padding only")
    return _volume_unit(x, name, "conv", kernel_size, num_filters, strides, activation, normalisation, normalise_post_activation,
                        dropout_p, weight_init, add_bias, kwargs)


def transposed_conv3D(bottom,
                      name,
                      kernel_size=(4,4,4),
                      num_filters=32,
                      strides=(2,2,2),
                      output_shape=None,
                      activation=STANDARD_NONLINEARITY,
                      normalisation=tfnorm.identity,
                      normalise_post_activation=False,
                      dropout_p=None,
                      padding="SAME",
                      weight_init='he_normal',
                      add_bias=True,
                      **kwargs):
    """Standard 3-D transposed convolution (tfwrapper/layers.py:261-323): tf.nn.conv3d_transpose with a [kd, kh, kw, num_filters,
    bottom channels] filter, by default up-sampling by 2; -> [bias] -> normalisation -> activation [-> dropout]."""
    if padding != "SAME":
        raise NotImplementedError("transposed_conv3D: SAME padding (the reference's default) only")
    shp = bottom.get_shape().as_list()
    if output_shape is not None and tuple(output_shape[1:4]) != tuple(n * s for n, s in zip(shp[1:4], strides)):
        raise NotImplementedError("transposed_conv3D: output_shape other than input * strides")
    return _volume_unit(bottom, name, "tconv", kernel_size, num_filters, strides, activation, normalisation, normalise_post_activation,
                        dropout_p, weight_init, add_bias, kwargs)


def bilinear_upsample3D(x, name, factor):
    """tfwrapper/layers.py:348-376: tf.image.resize_bilinear (legacy coordinates) on the (H, W) planes, then along D."""
    if factor != 2:
        raise NotImplementedError("hot path: factor 2")
    with G.get_default_graph().variable_scope(name):
        return G.bilinear_up3d(x, name="ResizeBilinear")
