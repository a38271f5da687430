"""Optimiser selectors named like the TF classes the reference's experiment configs reference
(phiseg/experiments/*.py:37, phiseg_model.py:137-140).  The update itself is one fused HIP kernel over the flat
parameter arena: phx_adam_tf1 (TF 1.12 epsilon-hat Adam) or phx_momentum_tf1 (TF 1.12 ApplyMomentum).  The instance
only carries the hyper-parameters; engine.Plan lowers it to the launch."""


class AdamOptimizer:
    beta1, beta2, epsilon = 0.9, 0.999, 1e-8

    def __init__(self, learning_rate=1e-3):
        self.learning_rate = learning_rate


class MomentumOptimizer:
    """tf.train.MomentumOptimizer: accum = momentum * accum + g;  p -= lr * accum, or with use_nesterov
    p -= lr * g + lr * momentum * accum.  One slot per variable, '<var>/Momentum'; no non-slot variables."""

    def __init__(self, learning_rate, momentum, use_locking=False, name='Momentum', use_nesterov=False):
        self.learning_rate = learning_rate
        self.momentum = momentum
        self.use_locking = use_locking
        self.name = name
        self.use_nesterov = use_nesterov


def slot_names(optimizer):
    """TF's slot names of an optimiser instance (None: Adam), in the order of ParamStore.slot_arenas()."""
    if isinstance(optimizer, MomentumOptimizer):
        return ('Momentum',)
    if optimizer is None or isinstance(optimizer, AdamOptimizer):
        return ('Adam', 'Adam_1')
    raise ValueError("optimizer must be an AdamOptimizer or a MomentumOptimizer instance, got %r" % (optimizer,))
