"""Symbolic graph of the PHiSeg step (the role TF1's graph mode plays in the reference).

The reference builds a static TensorFlow graph once (phiseg/phiseg_model.py:20-157) and then runs it
with ``sess.run``.  This module is the build-time half of the replacement: ``tfwrapper.layers`` /
``phiseg.model_zoo`` (our own code, same call signatures) create ``Op`` nodes over ``Tensor`` handles with
static NHWC shapes (batch dimension ``None``), variables live under nested ``variable_scope`` names that
match the reference's TF variable names.  ``engine.Plan`` then lowers a set of
fetches, for a concrete batch size and training flag, to a fixed list of HIP kernel launches that is
captured into a hipGraph -- HIP streams and graphs instead of a tracing compiler.
"""
import contextlib
import zlib
from collections import OrderedDict

import numpy as np

KIND_ACT, KIND_F32, KIND_U8 = "act", "f32", "u8"     # "act" = stored in the plan's compute dtype


class _Shape(list):
    def as_list(self):
        return list(self)


class Tensor:
    def __init__(self, op, shape, kind=KIND_ACT, name=None):
        self.op = op
        self.shape = tuple(shape)
        self.kind = kind
        self.name = name or (op.name if op is not None else "t")
        self.consumers = []
        self.bmul = 1                   # rows per fed image: > 1 behind tile_batch (n Monte-Carlo samples per image)

    def get_shape(self):
        return _Shape(self.shape)

    # the few arithmetic forms the zoo uses: s_oh - 0.5 ; sigma * eps ; mu + (sigma * eps)
    def __sub__(self, c):
        if not isinstance(c, (int, float)):
            raise NotImplementedError("only tensor - constant is part of the hot path")
        return get_default_graph().add_op("sub_const", [self], dict(c=float(c)), [(self.shape, self.kind)])[0]

    def __mul__(self, o):
        if not isinstance(o, Tensor) or o.shape != self.shape:
            raise NotImplementedError("only same-shape tensor * tensor is part of the hot path")
        return get_default_graph().add_op("mul", [self, o], {}, [(self.shape, KIND_F32)])[0]

    def __add__(self, o):
        if not isinstance(o, Tensor) or o.shape != self.shape:
            raise NotImplementedError("only same-shape tensor + tensor is part of the hot path")
        return get_default_graph().add_op("add", [self, o], {}, [(self.shape, KIND_F32)])[0]

    def __repr__(self):
        return "<Tensor %s %s %s>" % (self.name, self.shape, self.kind)


class Op:
    def __init__(self, type_, inputs, attrs, name):
        self.type = type_
        self.inputs = list(inputs)
        self.attrs = attrs
        self.name = name
        self.outputs = []


class Variable:
    def __init__(self, name, shape, initializer, trainable=True):
        self.name = name
        self.shape = tuple(int(s) for s in shape)
        self.initializer = initializer
        self.trainable = trainable

    @property
    def size(self):
        return int(np.prod(self.shape))

    def initial_value(self, seed=0):
        """Value at initialisation: a function of (seed, variable name, shape) only -- the Philox stream contract of
        phiseg_code_amd/philox_host.py -- so every replica, every run and the CPU oracle start from identical weights."""
        from phiseg_code_amd import philox_host
        rng = philox_host.VariableStream(seed, self.name)
        return np.asarray(self.initializer(self.shape, rng), dtype=np.float32).reshape(self.shape)

    def __bool__(self):
        return True


class _ScopeHandle:
    def __init__(self, graph, name):
        self.graph, self.name = graph, name

    def reuse_variables(self):
        self.graph._reuse[self.name] = True


class Graph:
    def __init__(self):
        self.ops = []
        self.variables = OrderedDict()
        self._scope = []
        self._reuse = {}
        self.collections = {}
        self._names = {}

    # ---- scopes / variables (tf.variable_scope / tf.get_variable) --------------------------------
    def scope_name(self):
        return "/".join(self._scope)

    @contextlib.contextmanager
    def variable_scope(self, name):
        self._scope.append(name)
        full = self.scope_name()
        try:
            yield _ScopeHandle(self, full)
        finally:
            self._scope.pop()

    def _reusing(self):
        return any(self._reuse.get("/".join(self._scope[:i + 1]), False) for i in range(len(self._scope)))

    def get_variable(self, name, shape, initializer, trainable=True):
        full = (self.scope_name() + "/" if self._scope else "") + name
        if full in self.variables:
            if not self._reusing():
                raise ValueError("Variable %s already exists (enter the scope with scope_reuse=True)" % full)
            v = self.variables[full]
            if tuple(shape) != v.shape:
                raise ValueError("Variable %s re-used with shape %s != %s" % (full, tuple(shape), v.shape))
            return v
        if self._reusing():
            raise ValueError("Variable %s does not exist but the scope is in reuse mode" % full)
        v = Variable(full, shape, initializer, trainable)
        self.variables[full] = v
        return v

    def add_to_collection(self, name, v):
        self.collections.setdefault(name, []).append(v)

    def get_collection(self, name):
        return list(self.collections.get(name, []))

    # ---- ops -------------------------------------------------------------------------------------
    def unique_name(self, base):
        k = self._names.get(base, 0)
        self._names[base] = k + 1
        return base if k == 0 else "%s_%d" % (base, k)

    def add_op(self, type_, inputs, attrs, out_specs, name=None):
        op = Op(type_, inputs, attrs, self.unique_name((self.scope_name() + "/" if self._scope else "") + (name or type_)))
        for i, (shape, kind) in enumerate(out_specs):
            op.outputs.append(Tensor(op, shape, kind, op.name + (":%d" % i if len(out_specs) > 1 else "")))
        bm = {t.bmul for t in inputs if t.shape and t.shape[0] is None}
        if len(bm) > 1:
            raise ValueError("op %s mixes tensors with %s rows per image (tile_batch the smaller one first)" % (op.name, sorted(bm)))
        rows = (max(bm) if bm else 1) * (int(attrs.get("tile", 1)) if type_ == "tile_batch" else 1)
        for o in op.outputs:
            o.bmul = rows
        for t in inputs:
            t.consumers.append(op)
        self.ops.append(op)
        return op.outputs


_default = Graph()


def get_default_graph():
    return _default


def set_default_graph(g):
    """Make `g` the graph new ops are added to (a model adding a graph instance after construction)."""
    global _default
    _default = g
    return g


def reset_default_graph():
    global _default
    _default = Graph()
    return _default


def variable_scope(name):
    return get_default_graph().variable_scope(name)


# --------------------------------------------------------------------------------------------------
# op constructors (the symbols our tfwrapper / model_zoo / phiseg_model are written against)
def placeholder(kind, shape, name):
    return get_default_graph().add_op("placeholder", [], dict(), [(tuple(shape), kind)], name=name)[0]


def constant(value):
    """tf.constant(scalar): only ever a placeholder value (the dummy posterior / prior of the deterministic baseline)."""
    return get_default_graph().add_op("constant", [], dict(value=float(value)), [((), KIND_F32)], name="const")[0]


def one_hot(s, depth):
    """tf.one_hot (phiseg_model.py:29): [.., H, W] u8 -> [.., H, W, depth]."""
    return get_default_graph().add_op("one_hot", [s], dict(depth=int(depth)), [(s.shape + (int(depth),), KIND_ACT)])[0]


def concat(values, axis=-1, name=None):
    """tf.concat along the channel axis of exactly two NHWC (or NDHWC) tensors (all the zoo needs)."""
    if len(values) != 2:
        raise NotImplementedError("concat of exactly two tensors")
    a, b = values
    if axis not in (-1, len(a.shape) - 1) or len(a.shape) not in (4, 5) or a.shape[:-1] != b.shape[:-1]:
        raise ValueError("concat: channel axis only, equal spatial shapes (%s vs %s)" % (a.shape, b.shape))
    kind = KIND_F32 if (a.kind == KIND_F32 and b.kind == KIND_F32) else KIND_ACT
    return get_default_graph().add_op("concat", [a, b], {}, [(a.shape[:-1] + (a.shape[-1] + b.shape[-1],), kind)],
                                      name=name or "concat")[0]


def random_normal(like, stream):
    """tf.random_normal(tf.shape(like), 0, 1): the Philox stream id fixes the noise contract
    (oracle/philox.py): stream = 16 * net + level."""
    return get_default_graph().add_op("random_normal", [like], dict(stream=int(stream)), [(like.shape, KIND_F32)])[0]


def conv_geometry(h, w, kernel_size, strides, dilations=(1, 1), padding="SAME"):
    """TF 1.12's rule for one convolution or pooling window (phx_conv2d_geometry is the same rule in C) -> (Ho, Wo, pt, pl).  With the
    effective extent ke = (k - 1) d + 1 per axis, SAME: out = ceil(in / s), total = max((out - 1) s + ke - in, 0), before = total // 2;
    VALID: out = (in - ke) // s + 1, no padding, and in < ke is a ValueError (TF refuses a negative dimension when the graph is built)."""
    if padding not in ("SAME", "VALID"):
        raise ValueError("padding must be 'SAME' or 'VALID', got %r" % (padding,))
    out, before = [], []
    for n, k, s, d in zip((int(h), int(w)), kernel_size, strides, dilations):
        n, k, s, d = int(n), int(k), int(s), int(d)
        if n < 1 or k < 1 or s < 1 or d < 1:
            raise ValueError("conv_geometry: extents, kernel, strides and dilations must be positive")
        ke = (k - 1) * d + 1
        if padding == "VALID":
            if n < ke:
                raise ValueError("VALID padding: an input extent of %d is smaller than the window extent %d (negative output size)" % (n, ke))
            out.append((n - ke) // s + 1)
            before.append(0)
        else:
            o = -(-n // s)
            out.append(o)
            before.append(max((o - 1) * s + ke - n, 0) // 2)
    return out[0], out[1], before[0], before[1]


def conv_transpose_geometry(h, w, kernel_size, strides, padding="SAME", output_hw=None):
    """tf.nn.conv2d_transpose of an [h, w] input -> (Ho, Wo, pt, pl).  An output extent O is legal iff the forward convolution of O gives
    the input extent n -- SAME: ceil(O / s) == n; VALID: O in [(n - 1) s + k, (n - 1) s + k + s - 1] -- and the padding is that
    convolution's on O.  output_hw None is the reference's n * s (under VALID legal only for k <= s).  An illegal one is a ValueError
    that names the legal range."""
    if padding not in ("SAME", "VALID"):
        raise ValueError("padding must be 'SAME' or 'VALID', got %r" % (padding,))
    res = []
    for ax, (n, k, s) in enumerate(zip((int(h), int(w)), kernel_size, strides)):
        n, k, s = int(n), int(k), int(s)
        O = n * s if output_hw is None else int(output_hw[ax])
        lo, hi = ((n - 1) * s + 1, n * s) if padding == "SAME" else ((n - 1) * s + k, (n - 1) * s + k + s - 1)
        if not lo <= O <= hi:
            raise ValueError("conv2d_transpose (%s, kernel %d, stride %d): an output extent of %d%s does not map back to the input extent %d; "
                             "legal output extents are %d..%d -- pass output_shape" % (padding, k, s, O, "" if output_hw is not None else
                                                                                      " (input * strides, the default)", n, lo, hi))
        res.append(O)
    ho, wo, pt, pl = conv_geometry(res[0], res[1], kernel_size, strides, (1, 1), padding)
    assert (ho, wo) == (int(h), int(w))
    return res[0], res[1], pt, pl


def conv_unit(x, W, b, ksize, norm, norm_vars, act, training, num_groups=None, head=False, name="conv", transposed=None,
              general=None, volume=None, explicit=None):
    """conv (SAME, stride 1) -> [+bias] -> [norm] -> act as ONE node (tfwrapper/layers.py:122-135).
    transposed = (kh, kw, sh, sw): tf.nn.conv2d_transpose instead (layers.py:197-258), W is [kh, kw, Cout, Cin] and the output
    is sh x sw times larger.  general = (kh, kw, sh, sw, dh, dw): strided / dilated SAME convolution (conv2D with strides,
    dilated_conv2D, dense_layer as a 1x1 convolution of the flattened input) on the direct kernels of csrc/gconv.hip; the
    output is ceil(H / sh) x ceil(W / sw).  volume = (form, kd, kh, kw, sd, sh, sw) on a 5-D [B, D, H, W, C] input (csrc/conv3d.hip):
    form "conv" is tf.nn.conv3d with W [kd, kh, kw, Cin, Cout] and output ceil(D / sd) x ceil(H / sh) x ceil(W / sw) (conv3D,
    layers.py:148-194), form "tconv" tf.nn.conv3d_transpose with W [kd, kh, kw, Cout, Cin] and output D sd x H sh x W sw
    (transposed_conv3D, layers.py:261-323).  explicit = (form, kh, kw, sh, sw, dh, dw, Ho, Wo, pt, pl): a 2-D unit with its whole geometry
    -- output extent and top / left padding from conv_geometry / conv_transpose_geometry -- on the kernels of csrc/conv2d_pad.hip: form
    "conv" with W [kh, kw, Cin, Cout] (VALID padding of conv2D / dilated_conv2D), form "tconv" with W [kh, kw, Cout, Cin]
    (transposed_conv2D under VALID padding or with an output_shape other than input * strides)."""
    kind = KIND_F32 if head else KIND_ACT
    attrs = dict(W=W, b=b, ksize=int(ksize), norm=norm, norm_vars=norm_vars, act=act, training=training,
                 num_groups=num_groups, head=head, transposed=transposed, general=general, volume=volume)
    if explicit is not None:
        # (the key exists only on the units that use it: every other unit keeps the attributes it has always had)
        if len(x.shape) != 4 or len(W.shape) != 4 or len(explicit) != 11 or explicit[0] not in ("conv", "tconv") \
                or transposed is not None or general is not None or volume is not None:
            raise ValueError("conv_unit: explicit = ('conv' | 'tconv', kh, kw, sh, sw, dh, dw, Ho, Wo, pt, pl) takes a 4-D input and a 4-D filter")
        explicit = (explicit[0],) + tuple(int(v) for v in explicit[1:])
        if tuple(W.shape[:2]) != explicit[1:3] or W.shape[3 if explicit[0] == "tconv" else 2] != x.shape[3]:
            raise ValueError("conv_unit: filter %s does not fit the explicit geometry %s on %r" % (W.shape, explicit, x))
        attrs["explicit"] = explicit
        shape = (x.shape[0], explicit[7], explicit[8], W.shape[2 if explicit[0] == "tconv" else 3])
        return get_default_graph().add_op("conv_unit", [x], attrs, [(shape, kind)], name=name)[0]
    if volume is not None:
        if len(x.shape) != 5 or len(W.shape) != 5 or volume[0] not in ("conv", "tconv") or transposed is not None or general is not None:
            raise ValueError("conv_unit: volume = ('conv' | 'tconv', kd, kh, kw, sd, sh, sw) takes a 5-D input and a 5-D filter")
        if norm not in (None, "batch"):
            raise NotImplementedError("3-D units take tfnorm.identity or tfnorm.batch_norm, not %r" % (norm,))
        st = volume[4:7]
        if volume[0] == "tconv":
            shape = (x.shape[0],) + tuple(n * s for n, s in zip(x.shape[1:4], st)) + (W.shape[3],)
        else:
            shape = (x.shape[0],) + tuple(-(-n // s) for n, s in zip(x.shape[1:4], st)) + (W.shape[4],)
    elif len(x.shape) == 5:
        raise ValueError("conv_unit: a 5-D input needs volume= (conv3D / transposed_conv3D), got %r" % (x,))
    elif transposed is not None:
        kh, kw, sh, sw = transposed
        shape = (x.shape[0], x.shape[1] * sh, x.shape[2] * sw, W.shape[2])
    elif general is not None:
        sh, sw = general[2], general[3]
        shape = (x.shape[0], -(-x.shape[1] // sh), -(-x.shape[2] // sw), W.shape[-1])
    else:
        shape = x.shape[:3] + (W.shape[3],)
    return get_default_graph().add_op("conv_unit", [x], attrs, [(shape, kind)], name=name)[0]


def avg_pool2x2(x):
    n, h, w, c = x.shape
    return get_default_graph().add_op("avgpool", [x], {}, [((n, (h + 1) // 2, (w + 1) // 2, c), x.kind)])[0]


def max_pool2x2(x):
    """tf.nn.max_pool 2x2 / stride 2 / SAME (tfwrapper/layers.py:18-28)."""
    n, h, w, c = x.shape
    return get_default_graph().add_op("maxpool", [x], {}, [((n, (h + 1) // 2, (w + 1) // 2, c), x.kind)])[0]


def pool2d(x, mode, kernel_size=(2, 2), strides=(2, 2), padding="SAME"):
    """tf.nn.max_pool / tf.nn.avg_pool with any window, stride and padding (tfwrapper/layers.py:18-28, 44-54) on csrc/conv2d_pad.hip:
    padded taps take no part in a maximum, an average divides by the number of taps inside the map."""
    if mode not in ("max", "avg"):
        raise ValueError("pool2d: mode 'max' or 'avg', got %r" % (mode,))
    if len(x.shape) != 4 or len(kernel_size) != 2 or len(strides) != 2:
        raise ValueError("pool2d: a [B, H, W, C] tensor and two-entry kernel_size / strides are expected")
    n, h, w, c = x.shape
    k, s = tuple(int(v) for v in kernel_size), tuple(int(v) for v in strides)
    ho, wo, pt, pl = conv_geometry(h, w, k, s, (1, 1), padding)
    return get_default_graph().add_op("pool2d", [x], dict(mode=mode, window=k, strides=s, pad=(pt, pl)), [((n, ho, wo, c), x.kind)],
                                      name=mode + "pool2d")[0]


def max_pool3d(x, window=(2, 2, 2)):
    """tf.nn.max_pool3d, window = stride = `window` (each entry 1 or 2), SAME (tfwrapper/layers.py:31-41)."""
    n, d, h, w, c = x.shape
    pd, ph, pw = (int(v) for v in window)
    if any(v not in (1, 2) for v in (pd, ph, pw)):
        raise ValueError("max_pool3d: window entries 1 or 2, got %s" % (window,))
    return get_default_graph().add_op("max_pool3d", [x], dict(window=(pd, ph, pw)),
                                      [((n, -(-d // pd), -(-h // ph), -(-w // pw), c), x.kind)], name="maxpool3d")[0]


def bilinear_up3d(x, name="ups3d"):
    """bilinear_upsample3D by 2 (tfwrapper/layers.py:348-376): legacy tf.image.resize_bilinear on the planes, then along D."""
    n, d, h, w, c = x.shape
    return get_default_graph().add_op("bilinear_up3d", [x], {}, [((n, 2 * d, 2 * h, 2 * w, c), x.kind)], name=name)[0]


def spatial_window3d(x, out_dhw, off, name="window3d"):
    """out[b, z, y, x] = x[b, z + off_z, y + off_y, x + off_x] inside x, 0 outside: the 5-D centre crop of crop_and_concat
    (layers.py:609-612) for positive offsets, zero padding for negative ones."""
    n, d, h, w, c = x.shape
    return get_default_graph().add_op("spatial_window3d", [x], dict(off=tuple(int(v) for v in off)),
                                      [((n,) + tuple(int(v) for v in out_dhw) + (c,), x.kind)], name=name)[0]


def fold_depth(x):
    """[B, D, H, W, ...] -> [B, D * H, W, ...]: the same memory seen with one spatial axis fewer (a view, no launch).  The per-pixel
    cross-entropies and the per-sample Dice sums of tfwrapper.losses do not depend on the fold."""
    return get_default_graph().add_op("fold_depth", [x], {}, [((x.shape[0], x.shape[1] * x.shape[2]) + tuple(x.shape[3:]), x.kind)],
                                      name="fold_depth")[0]


def spatial_window(x, out_h, out_w, off_y, off_x, name="window"):
    """out[b, y, x] = x[b, y + off_y, x + off_x] inside x, 0 outside: zero padding (pad_to_size, layers.py:625-650) for negative
    offsets, centre crop (crop_and_concat, layers.py:586-622) for positive ones."""
    n, h, w, c = x.shape
    return get_default_graph().add_op("spatial_window", [x], dict(off=(int(off_y), int(off_x))),
                                      [((n, int(out_h), int(out_w), c), x.kind)], name=name)[0]


def dropout(x, keep_prob, training, name="dropout"):
    """tf.nn.dropout(x, keep_prob) in training mode, identity otherwise (layers.py:653-668); the keep mask follows the Philox
    contract with stream id crc32(op name) (oracle.tf1_ops.dropout_keep_mask)."""
    import zlib
    out = get_default_graph().add_op("dropout", [x], dict(keep_prob=float(keep_prob), training=training), [(x.shape, x.kind)],
                                     name=name)[0]
    out.op.attrs["stream"] = zlib.crc32(out.op.name.encode()) & 0x3FFFFFFF
    return out


def window4(x, out_h, out_w, out_c, stride=(1, 1), off=(0, 0, 0), name="window"):
    """out[b, y, x, c] = x[b, y sy + oy, x sx + ox, c + oc] inside x, 0 outside: tf.pad along the channel axis (oc = -pad) and the
    strided slice identity[:, ::2, ::2, :] of the residual units' skip path (tfwrapper/layers.py:465-470)."""
    n = x.shape[0]
    return get_default_graph().add_op("window4", [x], dict(stride=(int(stride[0]), int(stride[1])), off=tuple(int(v) for v in off)),
                                      [((n, int(out_h), int(out_w), int(out_c)), x.kind)], name=name)[0]


def add_act(a, b, act="identity", name="add"):
    """act(a + b): tf.add(skip, conv2) [+ activation] of the residual units (layers.py:474-475, 534)."""
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("add: shapes %s and %s differ" % (a.shape, b.shape))
    return get_default_graph().add_op("add_act", [a, b], dict(act=act), [(a.shape, a.kind)], name=name)[0]


def leaky_relu(x, alpha=0.01, name="leaky_relu"):
    """tf.maximum(x, alpha * x) (tfwrapper/activations.py:8-9) as a node of its own, on a rank-4 or rank-5 tensor of any layout: same shape
    and kind as x.  0 < alpha < 1, so that the sign of the output is the sign of the input and the backward pass needs the output only;
    at x == 0 the whole gradient passes (TF's MaximumGrad on a tie).  DESIGN.md section 7i."""
    alpha = float(alpha)
    if not (0.0 < alpha < 1.0 and 0.0 < float(np.float32(alpha)) < 1.0):     # (a NaN fails every comparison; the kernels take an fp32 alpha)
        raise ValueError("leaky_relu: alpha must lie in (0, 1), got %r" % (alpha,))
    if not isinstance(x, Tensor) or len(x.shape) not in (4, 5) or x.kind == KIND_U8:
        raise ValueError("leaky_relu: a rank-4 or rank-5 activation tensor is expected, got %r" % (x,))
    return get_default_graph().add_op("leaky_relu", [x], dict(alpha=alpha), [(x.shape, x.kind)], name=name)[0]


def norm_act(x, norm, norm_vars, act, training, num_groups=None, name="norm"):
    """act(normalisation(x)) as a node of its own: the pre-activation order of identity_residual_unit2D (layers.py:512-518), where
    the normalisation does not follow a convolution."""
    if len(x.shape) == 5 and norm not in (None, "batch"):
        raise NotImplementedError("a 5-D tensor takes tfnorm.identity or tfnorm.batch_norm, not %r" % (norm,))
    attrs = dict(norm=norm, norm_vars=norm_vars, act=act, training=training, num_groups=num_groups)
    return get_default_graph().add_op("norm_act", [x], attrs, [(x.shape, x.kind)], name=name)[0]


def flatten(x):
    """tfwrapper/utils.py:16-22 flatten: [B, ...] (4-D or 5-D) -> [B, 1, 1, prod(...)] (NHWC memory order kept: a view, no launch); the
    extra unit axes keep every tensor of the engine four-dimensional."""
    n = x.shape[0]
    f = int(np.prod(x.shape[1:]))
    return get_default_graph().add_op("flatten", [x], {}, [((n, 1, 1, f), x.kind)], name="flatten")[0]


def bilinear_up2x(x, name="ups"):
    n, h, w, c = x.shape
    return get_default_graph().add_op("bilinear_up", [x], {}, [((n, 2 * h, 2 * w, c), x.kind)], name=name)[0]


def resize_nearest(x, out_hw):
    """tf.image.resize_images(..., NEAREST_NEIGHBOR) by an integer power-of-two factor (likelihoods.py:221).
    Never materialised: the loss / aggregation kernels read the coarse logits through a shift."""
    n, h, w, c = x.shape
    f = out_hw[0] // h
    if h * f != out_hw[0] or w * f != out_hw[1] or f & (f - 1) or f > 16:
        raise ValueError("nearest resize: integer power-of-two factor <= 16 required (%s -> %s)" % ((h, w), out_hw))
    return get_default_graph().add_op("nn_resize", [x], dict(shift=f.bit_length() - 1),
                                      [((n, out_hw[0], out_hw[1], c), KIND_F32)])[0]


def tile_batch(x, n):
    """[B, ...] -> [B * n, ...], row b * n + k = x[b]: every image's feature map repeated for its n Monte-Carlo samples."""
    if n == 1:
        return x
    return get_default_graph().add_op("tile_batch", [x], dict(tile=int(n)), [(x.shape, x.kind)], name="tile_batch")[0]


def global_average_pool(x, name=None):
    n, h, w, c = x.shape
    return get_default_graph().add_op("global_avgpool", [x], {}, [((n, c), KIND_F32)], name=name or "gap")[0]


def tile_pixels(z, h, w):
    """tf.reshape(z,[bs,1,1,zdim]) + tf.tile (likelihoods.py:147-149): [B, C] -> [B, h, w, C]."""
    n, c = z.shape
    return get_default_graph().add_op("tile_pixels", [z], {}, [((n, h, w, c), KIND_ACT)])[0]


def residual_multinoulli(s_list, labels, weight):
    """phiseg_model.py:229-262 for all levels at once -> (list of per-level loss scalars, s_accum[0])."""
    g = get_default_graph()
    L = len(s_list)
    outs = g.add_op("residual_ce", list(s_list) + [labels], dict(L=L, weight=float(weight)),
                    [((), KIND_F32)] * L + [(s_list[0].shape, KIND_F32)], name="residual_multinoulli")
    return outs[:L], outs[L]


def kl_two_gauss(mu0, sigma0, mu1, sigma1, level_weight, loss_weight):
    """level_weight * KL_two_gauss_with_diag_cov (phiseg_model.py:210-226, 271-279)."""
    return get_default_graph().add_op("kl", [mu0, sigma0, mu1, sigma1],
                                      dict(level_weight=float(level_weight), loss_weight=float(loss_weight)),
                                      [((), KIND_F32)], name="KL")[0]


def l2_of_collection(scale=1.0, name="weight_variables"):
    """scale * sum of tf.nn.l2_loss over a variable collection (phiseg_model.py:290-299, add_weight_decay)."""
    g = get_default_graph()
    return g.add_op("l2_weights", [], dict(vars=list(g.get_collection(name)), scale=float(scale)), [((), KIND_F32)],
                    name="weights_norm")[0]


def aggregate_logits(s_list):
    """_aggregate_output_list(use_softmax=False) + tf.nn.softmax (phiseg_model.py:106-109, 304-311)
    -> (sum of levels, softmax of the sum)."""
    outs = get_default_graph().add_op("aggregate", list(s_list), dict(L=len(s_list)),
                                      [(s_list[0].shape, KIND_F32), (s_list[0].shape, KIND_F32)], name="aggregate")
    return outs[0], outs[1]


def softmax_xent_map(logits, labels):
    """tf.nn.softmax_cross_entropy_with_logits_v2(labels=one_hot(labels), logits=logits) per pixel (eval_xent, phiseg_model.py:111):
    [B, H, W, C] f32 logits, [B, H, W] u8 labels -> [B, H, W] f32."""
    return get_default_graph().add_op("xent_map", [logits, labels], {}, [(logits.shape[:-1], KIND_F32)], name="eval_xent")[0]


# ---- tfwrapper/losses.py: Dice and the cross-entropy family (csrc/seg_losses.hip) ----------------------------------------------
def _seg_loss_inputs(logits, labels, what):
    """-> (full-resolution fp32 logits [B,H,W,C], u8 labels [B,H,W]).  `labels` is the u8 class-index tensor or G.one_hot of it (the
    kernels fold the one-hot into the u8 read); a level stored at a coarser resolution is summed to full resolution first (aggregate_logits)."""
    if len(logits.shape) == 5:
        # a volume [B, D, H, W, C] with labels G.one_hot of a u8 [B, D, H, W] placeholder (the form the reference's losses take: a
        # one-hot tensor of the logits' rank): both seen as [B, D * H, W, ..] (fold_depth: a view, no launch).  Any other label form
        # on 5-D logits stays refused.
        if labels.kind == KIND_U8 or labels.op is None or labels.op.type != "one_hot":
            raise NotImplementedError("%s: 3-D (5-D logits) segmentation takes its labels as G.one_hot of the u8 [B, D, H, W] "
                                      "placeholder; other label forms are not part of this port" % what)
        if labels.op.attrs["depth"] != logits.shape[4]:
            raise ValueError("%s: labels are one-hot of depth %d, the logits have %d classes" % (what, labels.op.attrs["depth"], logits.shape[4]))
        labels = labels.op.inputs[0]
        if logits.kind != KIND_F32 or labels.kind != KIND_U8 or tuple(labels.shape) != tuple(logits.shape[:4]):
            raise ValueError("%s: a volume takes fp32 logits [B, D, H, W, C] and G.one_hot of u8 labels [B, D, H, W], got %r / %r"
                             % (what, logits, labels))
        logits, labels = fold_depth(logits), fold_depth(labels)
    if len(logits.shape) != 4 or logits.kind != KIND_F32 or not 2 <= logits.shape[3] <= 8:
        raise ValueError("%s: logits must be an fp32 [B, H, W, C] tensor (a logit head) with 2 <= C <= 8, got %r" % (what, logits))
    if labels.kind != KIND_U8 and labels.op is not None and labels.op.type == "one_hot":
        if labels.op.attrs["depth"] != logits.shape[3]:
            raise ValueError("%s: labels are one-hot of depth %d, the logits have %d classes" % (what, labels.op.attrs["depth"], logits.shape[3]))
        labels = labels.op.inputs[0]
    if labels.kind != KIND_U8:
        raise NotImplementedError("%s: float one-hot / soft label tensors are not supported -- the loss kernels fold the one-hot into "
                                  "the read of u8 class indices and have no dense label read; pass the u8 [B, H, W] tensor or "
                                  "G.one_hot of it" % what)
    if tuple(labels.shape) != tuple(logits.shape[:3]):
        raise ValueError("%s: labels %s do not match logits %s" % (what, labels.shape, logits.shape))
    if logits.op is not None and logits.op.type == "nn_resize" and logits.op.attrs["shift"] > 0:
        logits = aggregate_logits([logits])[0]           # (a level stored at a coarser resolution: materialised; shift 0 is a plain view)
    return logits, labels


def dice_loss(logits, labels, epsilon=1e-10, sum_over_labels=False, sum_over_batches=False, only_foreground=False):
    """tfwrapper/losses.py:50-119 with the mode resolved to its flags: 1 - mean of the soft Dice -> scalar, differentiable."""
    if only_foreground and sum_over_labels:
        raise ValueError("dice_loss: only_foreground slices a label axis that sum_over_labels removed (the reference fails there too)")
    logits, labels = _seg_loss_inputs(logits, labels, "dice_loss")
    attrs = dict(epsilon=float(epsilon), sum_over_labels=bool(sum_over_labels), sum_over_batches=bool(sum_over_batches),
                 only_foreground=bool(only_foreground))
    return get_default_graph().add_op("dice_loss", [logits, labels], attrs, [((), KIND_F32)], name="dice_loss")[0]


def dice_table(logits, labels, epsilon=1e-10, sum_over_labels=False, sum_over_batches=False, use_hard_pred=True):
    """tfwrapper/losses.py:8-47 get_dice -> [B, C]; [C] with sum_over_batches; [B] with sum_over_labels; a scalar with both.
    Fetch-only: no gradient, and not a term of a loss."""
    logits, labels = _seg_loss_inputs(logits, labels, "get_dice")
    shape = (() if sum_over_batches else (logits.shape[0],)) + (() if sum_over_labels else (logits.shape[3],))
    attrs = dict(epsilon=float(epsilon), sum_over_labels=bool(sum_over_labels), sum_over_batches=bool(sum_over_batches),
                 use_hard_pred=bool(use_hard_pred))
    return get_default_graph().add_op("dice_table", [logits, labels], attrs, [(shape, KIND_F32)], name="dice")[0]


def seg_xent(logits, labels, class_weights=None, use_sigmoid=False):
    """tfwrapper/losses.py:123-159: mean soft-max cross-entropy over all pixels, optionally weighted per class, or the mean sigmoid
    cross-entropy over all pixels and classes -> scalar, differentiable."""
    logits, labels = _seg_loss_inputs(logits, labels, "cross_entropy_loss")
    if class_weights is not None:
        class_weights = [float(w) for w in class_weights]
        if use_sigmoid:
            raise ValueError("seg_xent: class weights belong to the soft-max form")
        if len(class_weights) != logits.shape[3]:
            raise ValueError("pixel_wise_cross_entropy_loss_weighted: %d class weights for %d classes" % (len(class_weights), logits.shape[3]))
    return get_default_graph().add_op("seg_xent", [logits, labels], dict(class_weights=class_weights, use_sigmoid=bool(use_sigmoid)),
                                      [((), KIND_F32)], name="seg_xent")[0]


def weighted_sum(scalars, weights):
    return get_default_graph().add_op("weighted_sum", list(scalars), dict(weights=[float(w) for w in weights]),
                                      [((), KIND_F32)], name="loss_tot")[0]
