"""Host-side checks of the uncertainty-map feature: the numpy restatement (tests/uncertainty_ref.py) against the fixture written by the
reference's own code (tools/make_goldens_uncertainty.py), the C ABI declarations, the model class's method block and the
latent-feed argument check.  No GPU is touched."""
import inspect
import os

import numpy as np
import pytest

from tests import uncertainty_ref as U
from tests.helpers import GOLDEN_DIR, load_golden
from tests.test_graph_cpu import make_config

GOLD = np.load(os.path.join(GOLDEN_DIR, "uncertainty_cases.npz"))


def test_golden_lists_the_cases():
    assert GOLD["cases"].tolist() == [list(c[:6]) for c in U.CASES]


@pytest.mark.parametrize("k", range(len(U.CASES)))
def test_float64_restatement_reproduces_reference_maps(k):
    """Every plane to 1e-12 of the plane's maximum (float64 sums in another order differ by ~1e-15).  COV_DET on soft-max inputs is
    rounding noise on both sides (singular matrix): only Hadamard's inequality |det| <= prod_c var_c is asserted there; the
    determinant itself is pinned by COV_DET_DROP_LAST and by COV_DET on the un-normalised variant."""
    logits, sm, gts, s_ref = U.uncertainty_case(k)
    r = U.reference_maps(logits, sm, gts, s_ref, np.float64)
    for name in U.MAPS:
        g = GOLD["%d/%s" % (k, name)]
        assert g.shape == r[name].shape == sm.shape[1:3]
        if name == "cov_det":
            bound = np.prod(r["var1"], axis=-1) * (1 + 1e-6)
            assert (np.abs(r[name]) <= bound).all() and (np.abs(g) <= bound).all()
            continue
        err = np.abs(r[name] - g).max()
        print(k, name, "max|golden| %.3e err %.3e" % (np.abs(g).max(), err))
        assert err <= 1e-12 * max(np.abs(g).max(), 1e-300), (name, err)
    # arg-max of the mean soft-max: equal wherever the two largest means are not tied to rounding
    m = np.sort(r["mean_sm"], axis=-1)
    clear = (m[..., -1] - m[..., -2]) > 1e-12
    assert (r["argmax"][clear] == GOLD["%d/argmax" % k][clear]).all()
    _, smu, _, _ = U.uncertainty_case(k, unnormalised=True)
    ru = U.reference_maps(logits, smu, gts, s_ref, np.float64)
    gu = GOLD["%d/cov_det_unnormalised" % k]
    assert np.abs(ru["cov_det"] - gu).max() <= 1e-12 * np.abs(gu).max()


def test_header_declares_the_entry_points():
    from phiseg_code_amd import runtime as rt
    protos = rt.parse_header()
    assert len(protos["phx_mc_stats"]) == 16 and len(protos["phx_mc_stats_ws_bytes"]) == 5
    src = open(rt.HEADER).read()
    for k, name in enumerate(U.MAPS):
        assert "PHX_MC_%s = %d" % (name.upper(), k) in src
    assert "PHX_MC_NMAPS = 8" in src


REFERENCE_METHODS = {
    "generate_samples_from_z": ["z_list", "x_in", "output_all_levels"],
    "generate_samples_from_prior": ["x_in", "output_all_levels"],
    "generate_posterior_samples": ["x_in", "s_in", "return_params"],
    "generate_all_output_levels": ["x_in", "s_in"],
    "get_crossentropy_error_map": ["s_gt", "x_in", "num_samples"],
    "predict_mean_variance_and_error_maps": ["s_gt", "x_in", "num_samples"],
    "predict_segmentation_sample_variance_sm_cov": ["x_in", "num_samples"],
    "predict_segmentation_sample_variance_sm_cov_bf": ["x_in", "num_samples", "drop_last_class"],
}


def test_model_class_has_the_reference_method_block():
    from phiseg_code_amd.phiseg import phiseg_model
    for name, args in REFERENCE_METHODS.items():
        sig = inspect.signature(getattr(phiseg_model.phiseg, name))
        assert list(sig.parameters)[1:] == args, name
    p = inspect.signature(phiseg_model.phiseg.get_crossentropy_error_map).parameters
    assert p["num_samples"].default == 100
    assert inspect.signature(phiseg_model.phiseg.generate_samples_from_z).parameters["output_all_levels"].default is False
    assert inspect.signature(phiseg_model.phiseg.generate_all_output_levels).parameters["s_in"].default is None
    assert inspect.signature(phiseg_model.phiseg.predict_segmentation_sample_variance_sm_cov_bf).parameters["drop_last_class"].default is False


def test_lazy_nodes_leave_the_constructed_graph_alone():
    from phiseg_code_amd.phiseg import phiseg_model
    _, cfg, _ = load_golden("tiny_phiseg_bn")
    model = phiseg_model.phiseg(make_config(cfg))
    names = [op.name for op in model.graph.ops]
    xe = model.eval_xent
    assert xe is model.eval_xent and xe.shape == (None, cfg["H"], cfg["H"])
    assert len(model.s_out_eval_sm_list) == cfg["latent_levels"]
    assert [op.name for op in model.graph.ops][:len(names)] == names          # only appended to


def test_feeding_a_tensor_outside_z_list_raises():
    from phiseg_code_amd.phiseg import phiseg_model
    _, cfg, _ = load_golden("tiny_phiseg_bn")
    model = phiseg_model.phiseg(make_config(cfg))
    x = np.zeros((1, cfg["H"], cfg["H"], 1), np.float32)
    for bad in (model.mu_list[0], model.prior_z_list_gen[0], model.s_out_eval):
        with pytest.raises(ValueError, match="z_list"):
            model.sess.run(model.s_out_list, {model.x_inp: x, model.training_pl: False, bad: np.zeros((1, 2, 2, 2), np.float32)})
    assert model.sess.latent_feeds({model.z_list[2]: 0, model.z_list[0]: 0, model.x_inp: x}) == [model.z_list[0], model.z_list[2]]
