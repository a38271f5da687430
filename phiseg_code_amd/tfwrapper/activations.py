"""Activation markers.  The reference passes ``tf.nn.relu`` / ``tf.nn.softplus`` / ``tf.identity`` callables
to ``layers.conv2D(activation=...)`` (tfwrapper/layers.py:14,99; posteriors.py:105-107).  Here they are
marker callables: ``conv2D`` recognises them by identity and fuses the activation into the conv /
normalisation kernel epilogue.

``leaky_relu`` -- the one function of the reference's tfwrapper/activations.py -- is an ordinary function as well: on a graph
tensor it adds a ``graph.leaky_relu`` node (csrc/leaky_relu.hip).  As ``activation=leaky_relu`` or
``activation=functools.partial(leaky_relu, alpha=a)`` a layer builds its unit with the identity activation and puts that node
behind it."""
import functools


def relu(x):
    raise NotImplementedError("stand-alone relu is not on the hot path; pass it as conv2D(activation=relu)")


def softplus(x):
    raise NotImplementedError("stand-alone softplus is not on the hot path; pass it as conv2D(activation=softplus)")


def identity(x, **kwargs):
    return x


def leaky_relu(x, alpha=0.01):
    """tfwrapper/activations.py:8-9: tf.maximum(x, alpha * x), 0 < alpha < 1."""
    from phiseg_code_amd import graph as G
    return G.leaky_relu(x, alpha)


ACT_NAME = {relu: "relu", softplus: "softplus", identity: "identity"}


def leaky_alpha(activation):
    """alpha if `activation` is leaky_relu itself (0.01, its default) or functools.partial(leaky_relu, alpha=a) -- alpha by keyword: a
    positional argument would be x -- else None."""
    if activation is leaky_relu:
        return 0.01
    if isinstance(activation, functools.partial) and activation.func is leaky_relu and not activation.args \
            and set(activation.keywords) <= {"alpha"}:
        return float(activation.keywords.get("alpha", 0.01))
    return None


def known(activation):
    """Is `activation` one of the callables a layer function takes?  (functools.partial objects do not hash by content, and an
    unhashable callable must be a ValueError like any other unknown one.)"""
    if leaky_alpha(activation) is not None:
        return True
    try:
        return activation in ACT_NAME
    except TypeError:
        return False


def unit_act(activation):
    """-> (the activation name the unit / add_act / norm_act node carries, alpha of the leaky_relu node behind it or None)"""
    alpha = leaky_alpha(activation)
    return ("identity", alpha) if alpha is not None else (ACT_NAME[activation], None)
