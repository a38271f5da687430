"""The many-class surface without a GPU: the header declares the entries of csrc/many_class.hip, the host picks
an entry by the class count alone, and the two places that stay at eight classes or stop at 256 say so before anything is launched."""
import numpy as np
import pytest

from phiseg_code_amd import many_class
from phiseg_code_amd import runtime as rt
from tests.test_graph_cpu import make_config

ENTRIES = ("phx_residual_ce_wide", "phx_residual_ce_wide_ws_bytes", "phx_softmax_xent_map_wide", "phx_metrics_wide",
           "phx_metrics_wide_ws_bytes", "phx_augment_batch_nearest", "phx_augment_batch_nearest_ws_bytes")


def test_header_declares_the_many_class_entries():
    protos = rt.parse_header()
    for name in ENTRIES:
        assert name in protos, name
    narrow, wide = protos["phx_residual_ce"], protos["phx_residual_ce_wide"]
    assert wide[:len(narrow) - 1] == narrow[:-1] and len(wide) == len(narrow) + 2       # the same arguments + (work, work_bytes)
    assert protos["phx_softmax_xent_map_wide"] == protos["phx_softmax_xent_map"]
    sources = open(rt.HEADER.replace("include/phx.h", "phiseg_code_amd/csrc/SOURCES")).read().split()
    assert "many_class.hip" in sources and "augment_nearest.hip" in sources
    assert protos["phx_augment_batch_nearest"] == protos["phx_augment_batch_elastic"]                     # the same arguments


def test_dispatch_by_class_count():
    for C in range(2, 9):
        assert many_class.residual_ce_entry(C) == "residual_ce"
        assert many_class.xent_map_entry(C) == "softmax_xent_map"
        assert many_class.validation_metrics_entry(C) == "validation_metrics"
        assert many_class.eval_metrics_entry(C) == "eval_metrics"
        assert many_class.metrics_row(C) == 10
    for C in range(9, 257):
        assert many_class.residual_ce_entry(C) == "residual_ce_wide"
        assert many_class.xent_map_entry(C) == "softmax_xent_map_wide"
        assert many_class.validation_metrics_entry(C) == many_class.eval_metrics_entry(C) == "metrics_wide"
        assert many_class.metrics_row(C) == 2 + C
    protos = rt.parse_header()
    for fn in (many_class.residual_ce_entry, many_class.xent_map_entry, many_class.validation_metrics_entry, many_class.eval_metrics_entry):
        assert "phx_" + fn(8) in protos and "phx_" + fn(9) in protos
        for C in (1, 0, 257, 2.5):
            with pytest.raises(ValueError):
                fn(C)


def _cfg(nlabels):
    return make_config(dict(arch="phiseg", norm="batch_norm", n0=4, zdim0=2, H=64, B=2, nlabels=nlabels, latent_levels=3,
                            resolution_levels=5, KL_weight=1.0))


@pytest.mark.parametrize("nlabels", [1, 257])
def test_phiseg_refuses_a_class_count_outside_2_to_256(nlabels):
    from phiseg_code_amd.phiseg import phiseg_model
    with pytest.raises(ValueError, match="nlabels"):
        phiseg_model.phiseg(_cfg(nlabels))


@pytest.mark.parametrize("nlabels", [9, 19, 256])
def test_phiseg_builds_its_graph_with_many_classes(nlabels):
    from phiseg_code_amd.phiseg import phiseg_model
    model = phiseg_model.phiseg(_cfg(nlabels))
    assert model.s_out_eval_sm.shape[-1] == nlabels and all(s.shape[-1] == nlabels for s in model.s_out_list)


def test_mc_statistics_refuses_nine_classes_before_any_launch():
    from phiseg_code_amd import uncertainty
    sm = np.full((3, 4, 4, 9), 1.0 / 9, dtype=np.float32)
    with pytest.raises(ValueError, match="2 <= C <= 8"):
        uncertainty.mc_statistics(sm=sm)
    with pytest.raises(ValueError, match="2 <= C <= 8"):
        uncertainty.mc_stats_device(None, 1, None, None, 1, 3, 0, 16, 9, ("e_ss",), 0)
