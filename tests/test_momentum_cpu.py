"""exp_config.optimizer on the host side: the C ABI declares phx_momentum_tf1, optimizers.MomentumOptimizer carries TF's
hyper-parameters, and the model constructor instantiates the configured optimiser as the reference does
(phiseg/phiseg_model.py:135-141: Momentum with momentum 0.9 and use_nesterov=True, anything else with the learning rate alone)."""
import pytest

from tests.helpers import load_golden
from tests.test_graph_cpu import make_config

from phiseg_code_amd import optimizers
from phiseg_code_amd import runtime as rt
from phiseg_code_amd.phiseg import phiseg_model


def _config():
    return make_config(load_golden("tiny_phiseg_bn")[1])


def test_header_declares_momentum_entry():
    protos = rt.parse_header()
    assert "phx_momentum_tf1" in protos
    assert len(protos["phx_momentum_tf1"]) == 8


def test_momentum_optimizer_selector_and_model_wiring():
    o = optimizers.MomentumOptimizer(1e-3, 0.9, use_nesterov=True)
    assert (o.learning_rate, o.momentum, o.use_nesterov) == (1e-3, 0.9, True)
    assert optimizers.MomentumOptimizer(0.1, 0.5).use_nesterov is False           # TF's default
    c = _config()
    c.optimizer = optimizers.MomentumOptimizer
    model = phiseg_model.phiseg(c)
    assert type(model.optimizer) is optimizers.MomentumOptimizer
    assert model.optimizer.momentum == 0.9
    assert model.optimizer.use_nesterov is True
    assert model.optimizer.learning_rate is model.lr_pl


def test_stock_config_gives_adam():
    c = _config()
    assert c.optimizer is optimizers.AdamOptimizer
    model = phiseg_model.phiseg(c)
    assert isinstance(model.optimizer, optimizers.AdamOptimizer)
    assert model.optimizer.learning_rate is model.lr_pl


def test_config_without_optimizer_gives_adam():
    c = _config()
    del c.optimizer
    model = phiseg_model.phiseg(c)
    assert isinstance(model.optimizer, optimizers.AdamOptimizer)


def test_unknown_optimizer_is_rejected():
    c = _config()
    c.optimizer = object
    with pytest.raises(ValueError):
        phiseg_model.phiseg(c)
    c.optimizer = lambda learning_rate: "sgd"          # a factory whose product is no known optimiser
    with pytest.raises(ValueError):
        phiseg_model.phiseg(c)


def test_subclass_with_fixed_hyperparameters_keeps_them():
    class HeavyBall(optimizers.MomentumOptimizer):
        def __init__(self, learning_rate):
            super().__init__(learning_rate, 0.5, use_nesterov=False)

    c = _config()
    c.optimizer = HeavyBall
    model = phiseg_model.phiseg(c)
    assert isinstance(model.optimizer, optimizers.MomentumOptimizer)
    assert model.optimizer.momentum == 0.5 and model.optimizer.use_nesterov is False
    assert model.optimizer.learning_rate is model.lr_pl
    assert optimizers.slot_names(model.optimizer) == ("Momentum",)
    assert optimizers.slot_names(None) == optimizers.slot_names(optimizers.AdamOptimizer()) == ("Adam", "Adam_1")
