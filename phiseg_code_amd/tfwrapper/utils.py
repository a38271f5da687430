"""Variable factories -- counterpart of the reference's tfwrapper/utils.py:214-271.

``get_weight_variable`` / ``get_bias_variable`` keep the reference's signatures.  he_normal follows TF 1.12's
``variance_scaling_initializer(factor=2.0, mode='FAN_IN', uniform=False)``: a truncated normal (resampled
beyond two standard deviations) with stddev sqrt(1.3 * 2 / fan_in), fan_in = kh*kw*Cin.

Random draws come from the build's Philox stream contract (``phiseg_code_amd/philox_host.py``: TensorFlow itself is never
seeded by the reference): a variable's value depends on (seed, TF variable name, shape) only."""
import math

import numpy as np

from phiseg_code_amd import graph as G


def _truncated_normal(shape, std, rng):
    """TF's truncated_normal: draws beyond two standard deviations are re-drawn (rng: philox_host.VariableStream)."""
    return rng.truncated_normal(shape) * std


def _fans(shape):
    rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    return rf * shape[-2], rf * shape[-1]


def _initializer(type_, **kwargs):
    """tfwrapper/utils.py:221-244 of the reference.  he_normal / xavier_normal = TF 1.12's variance_scaling_initializer
    (truncated normal, stddev sqrt(1.3 * factor / fan)); the *_uniform variants draw U(-limit, limit)."""
    if type_ == "he_normal":
        return lambda shape, rng: _truncated_normal(shape, math.sqrt(1.3 * 2.0 / _fans(shape)[0]), rng)
    if type_ == "he_uniform":
        return lambda shape, rng: rng.uniform(-1.0, 1.0, shape) * math.sqrt(3.0 * 2.0 / _fans(shape)[0])
    if type_ == "caffe_uniform":
        return lambda shape, rng: rng.uniform(-1.0, 1.0, shape) * math.sqrt(3.0 * 1.0 / _fans(shape)[0])
    if type_ == "xavier_uniform":
        return lambda shape, rng: rng.uniform(-1.0, 1.0, shape) * math.sqrt(6.0 / sum(_fans(shape)))
    if type_ == "xavier_normal":
        return lambda shape, rng: _truncated_normal(shape, math.sqrt(1.3 * 2.0 / sum(_fans(shape))), rng)
    if type_ == "simple":
        std = kwargs.get("stddev", 0.02)
        return lambda shape, rng: _truncated_normal(shape, std, rng)
    if type_ == "bilinear":
        # tfwrapper/utils.py:275-307: 2-D bilinear interpolation kernel on the diagonal of a transposed-convolution filter
        def bil(shape, rng):
            kh, kw, co, ci = shape
            f = math.ceil(kw / 2.0)
            c = (2 * f - 1 - f % 2) / (2.0 * f)
            k2 = np.array([[(1 - abs(xx / f - c)) * (1 - abs(yy / f - c)) for yy in range(kh)] for xx in range(kw)])
            w = np.zeros(shape, dtype=np.float32)
            for i in range(min(co, ci)):
                w[:, :, i, i] = k2
            return w
        return bil
    raise ValueError("Unknown initialisation requested: %s" % type_)


def get_weight_variable(shape, name=None, type="xavier_uniform", regularize=True, **kwargs):
    if name is None:
        raise NotImplementedError("unnamed variables are not used on the hot path")
    if kwargs.get("init_weights") is not None:
        w0 = np.asarray(kwargs["init_weights"], dtype=np.float32)
        init = lambda shape, rng: w0
    else:
        init = _initializer(type, **kwargs)
    g = G.get_default_graph()
    weight = g.get_variable(name, shape, init)
    if regularize:
        g.add_to_collection("weight_variables", weight)
    return weight


def get_bias_variable(shape, name=None, init_value=0.0, **kwargs):
    if name is None:
        raise NotImplementedError("unnamed variables are not used on the hot path")
    if kwargs.get("init_biases") is not None:
        b0 = np.asarray(kwargs["init_biases"], dtype=np.float32)
        init = lambda shape, rng: b0
    else:
        init = lambda shape, rng: np.full(shape, init_value, dtype=np.float32)
    return G.get_default_graph().get_variable(name, shape, init)


def get_latest_model_checkpoint_path(folder, name):
    """tfwrapper/utils.py:189-210 of the reference: the checkpoint `name`-<iteration> with the highest iteration in
    `folder` (False when there is none).  TF marks a checkpoint by its .meta file; ours is one file <name>-<it>.npz."""
    import glob
    import os
    its = []
    for ext in ('.npz', '.index'):           # ours / a TensorFlow tensor bundle (tf_checkpoint.py; TF marks those by .meta as well)
        for f in glob.glob(os.path.join(folder, '%s-*%s' % (name, ext))):
            tail = os.path.basename(f)[len(name) + 1:-len(ext)]
            if tail.isdigit():
                its.append(int(tail))
    if not its:
        return False
    return os.path.join(folder, name + '-' + str(max(its)))


def put_kernels_on_grid(images, batch_size, pad=1, min_int=None, max_int=None, **kwargs):
    """tfwrapper/utils.py:93-168 of the reference: a batch arranged as one grid image, uint8 [1, (X + 2) * grid_Y, (Y + 2) * grid_X, 1],
    formed on the device (phx_summary_grid_u8; phiseg_code_amd/summary.py)."""
    from phiseg_code_amd import summary
    return summary.put_kernels_on_grid(images, batch_size, pad=pad, min_int=min_int, max_int=max_int, **kwargs)


def print_tensornames_in_checkpoint_file(file_name):
    """tfwrapper/utils.py:171-180 of the reference (pywrap_tensorflow.NewCheckpointReader there)."""
    from phiseg_code_amd.tfwrapper import tf_checkpoint
    for key in sorted(tf_checkpoint.list_variables(file_name)):
        print(" - tensor_name: ", key)


def get_checkpoint_weights(file_name):
    """tfwrapper/utils.py:182-187 of the reference: {name: ndarray} of a TensorFlow checkpoint prefix."""
    from phiseg_code_amd.tfwrapper import tf_checkpoint
    return tf_checkpoint.read(file_name)


def get_rhs_dim(tensor):
    return int(np.prod(tensor.get_shape().as_list()[1:]))


def flatten(tensor):
    raise NotImplementedError("flatten is folded into the KL kernel (phx_kl_diag_gauss)")
