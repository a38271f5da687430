"""The account behind the kernel tests' promise: every entry point include/phx.h declares is called by some test under tests/ --
its short name stands there as a call, `.<name>(` -- or is listed below with the reason why not.  Two kinds of reason only: a host
utility (no kernel arithmetic to get wrong), or an entry point the tests reach through the named wrapper, called by the named test.
No GPU, no library: the prototypes come from the parser the binding itself uses (phiseg_code_amd.runtime.parse_header)."""
import glob
import os
import re

from phiseg_code_amd import runtime as rt

TESTS = os.path.dirname(os.path.abspath(__file__))

NOT_CALLED_DIRECTLY = {
    # ---- host utilities -------------------------------------------------------------------------------------------------------------
    "debug_set_trace": "host utility: stores a debug pointer for the tracing tools (tools/trace_*.py); NULL, the default, is off",
    "debug_set_blocklog": "host utility: stores a debug pointer for the tracing tools (tools/blocklog.py); NULL, the default, is off",
    # ---- reached through a wrapper ------------------------------------------------------------------------------------------------------
    "conv3x3_bf16": "through the runtime shims conv3x3_mfma_bf16* (runtime._Lib._conv_shims): test_kernels_gpu.py::test_conv3x3_mfma_fwd_dgrad_wgrad",
    "conv3x3_bf16_plan": "through runtime._Lib.conv3x3_plan and its shims (conv3x3_mfma_ws_bytes, ...): test_kernels_gpu.py::test_conv3x3_mfma_fwd_dgrad_wgrad",
    "unpad_filter_grad_accumulate": "called through an alias, (L.unpad_filter_grad_center if ... else L.unpad_filter_grad_accumulate)(...): test_tail_fusions_gpu.py",
    "avgpool2x2_bwd_acc": "called through the alias fn_acc: test_kernels_gpu.py::test_accumulating_pool_and_resize_gradients",
    "bilinear_up2x_bwd_acc": "called through the alias fn_acc: test_kernels_gpu.py::test_accumulating_pool_and_resize_gradients",
    "tconv3d_dgrad": "called through the alias dgrad of _conv_family: test_volume_kernels_gpu.py, test_direct_kernel_edges_gpu.py",
    "tconv3d_wgrad": "called through the alias wgrad of _conv_family: test_volume_kernels_gpu.py, test_direct_kernel_edges_gpu.py",
    "upconv_pack": "through phiseg_code_amd.upconv.forward: test_kernels_gpu.py::test_upsample_conv_phase_form_vs_oracle",
    "upconv_frame_gather": "through phiseg_code_amd.upconv.forward: test_kernels_gpu.py::test_upsample_conv_phase_form_vs_oracle",
    "upconv_frame_scatter": "through phiseg_code_amd.upconv.forward: test_kernels_gpu.py::test_upsample_conv_phase_form_vs_oracle",
    "upconv_frame_gather_dy": "through phiseg_code_amd.upconv.backward_prepare: test_kernels_gpu.py::test_upsample_conv_phase_form_vs_oracle",
    "upconv_fold_wgrad": "through phiseg_code_amd.upconv.backward_filters: test_kernels_gpu.py::test_upsample_conv_phase_form_vs_oracle",
    "upconv_frame_scatter_dx": "through phiseg_code_amd.upconv.backward_data: test_kernels_gpu.py::test_upsample_conv_phase_form_vs_oracle",
    "mc_stats": "through phiseg_code_amd.uncertainty.mc_statistics: test_uncertainty_gpu.py::test_kernel_matches_reference_goldens",
    "summary_histograms": "through phiseg_code_amd.summary.histograms: test_summary_gpu.py::test_segment_list_lengths",
    "summary_grid_u8": "through phiseg_code_amd.summary.grid_u8_device: test_summary_gpu.py::test_grid_of_every_input_form",
}

# the element-wise, loss and optimiser kernels tests/test_glue_kernel_edges_gpu.py pins: none of them may hide behind a reason
MUST_BE_CALLED = ["act_bwd", "cast", "repeat_batch", "l2_masked", "axpy_masked", "weighted_sum", "softmax_xent_map", "unpad_channels_bf16",
                  "sum_scalars", "concat2", "split2", "broadcast_pixels_fwd", "broadcast_pixels_bwd", "global_avgpool_fwd",
                  "global_avgpool_bwd", "posterior_input", "pad_channels_bf16", "residual_ce", "reparam_fwd", "reparam_bwd", "adam_tf1"]


def _test_sources():
    files = sorted(glob.glob(os.path.join(TESTS, "**", "*.py"), recursive=True))
    assert len(files) > 20
    return {os.path.relpath(f, TESTS): open(f).read() for f in files}


def _called(name, sources):
    """`.name(` preceded by an identifier other than ctypes (ctypes.cast( is not phx_cast)"""
    pat = re.compile(r"(\w+)\.%s\(" % re.escape(name))
    return any(m.group(1) != "ctypes" for src in sources.values() for m in pat.finditer(src))


def test_every_entry_point_is_called_by_a_test_or_listed_with_a_reason():
    protos = rt.parse_header()
    assert len(protos) > 150 and all(n.startswith("phx_") for n in protos)
    sources = _test_sources()
    names = sorted(n[4:] for n in protos)
    missing = [n for n in names if not _called(n, sources) and n not in NOT_CALLED_DIRECTLY]
    assert not missing, "entry points of include/phx.h that no test calls and no reason covers: %s" % ", ".join(missing)


def test_the_list_of_reasons_holds_nothing_stale():
    protos = rt.parse_header()
    sources = _test_sources()
    for name, reason in NOT_CALLED_DIRECTLY.items():
        assert "phx_" + name in protos, "%s is listed but include/phx.h does not declare it" % name
        assert not _called(name, sources), "%s is called by a test now: take it off the list" % name
        assert reason.startswith("host utility: ") or reason.startswith("through ") or reason.startswith("called through "), name
        for ref in re.findall(r"(test_\w+\.py)(?:::(test_\w+))?", reason):         # the named test exists
            assert ref[0] in sources, (name, ref[0])
            assert not ref[1] or ("def %s(" % ref[1]) in sources[ref[0]], (name, ref)


def test_the_glue_kernels_are_called_directly():
    sources = _test_sources()
    for name in MUST_BE_CALLED:
        assert name not in NOT_CALLED_DIRECTLY and _called(name, sources), name
