"""Host-side checks of the test-set evaluation: the C ABI declarations and exports of phx_eval_metrics, its workspace query, and the
command line / output file names of the two test scripts.  No GPU is touched."""
import ctypes
import os
import sys

import pytest


def test_header_declares_and_library_exports_the_entry_points():
    from phiseg_code_amd import runtime as rt
    protos = rt.parse_header()
    assert len(protos["phx_eval_metrics"]) == 13 and len(protos["phx_eval_metrics_ws_bytes"]) == 5
    assert protos["phx_eval_metrics"] == protos["phx_validation_metrics"]          # same argument list as the validation entry
    dll = ctypes.CDLL(rt.LIB_PATH)
    for name in ("phx_eval_metrics", "phx_eval_metrics_ws_bytes"):
        assert getattr(dll, name) is not None
    L = rt.lib()
    assert L.eval_metrics_ws_bytes.restype is ctypes.c_size_t and callable(L.eval_metrics)


def test_workspace_query_is_positive_and_monotone():
    from phiseg_code_amd import runtime as rt
    ws = rt.lib().eval_metrics_ws_bytes
    base = int(ws(1, 100, 4, 16384, 2))
    assert base > 0
    assert int(ws(1, 1, 1, 1, 2)) > 0
    for I in (1, 2, 3, 4, 7):
        assert int(ws(I + 1, 100, 4, 16384, 2)) > int(ws(I, 100, 4, 16384, 2))
    for N in (1, 2, 7, 50, 99, 100):
        assert int(ws(1, N + 1, 4, 16384, 2)) > int(ws(1, N, 4, 16384, 2))
    for P in (1, 63, 64, 65, 100, 4096, 16384, 36864):
        assert int(ws(1, 100, 4, P + 1, 2)) >= int(ws(1, 100, 4, P, 2))
        assert int(ws(1, 100, 4, P + 64, 2)) > int(ws(1, 100, 4, P, 2))
    # the planes alone: (N + 1 + M) masks x C labels x P / 64 words of 8 bytes
    assert base >= (100 + 1 + 4) * 2 * 256 * 8


def test_exp_path_command_line_loads_the_first_config(tmp_path):
    from phiseg_code_amd import evaluate
    (tmp_path / "b_other.py").write_text("experiment_name = 'other'\n")
    (tmp_path / "a_config.py").write_text("experiment_name = 'from_folder'\nnlabels = 3\n")
    (tmp_path / "model_best_ged.ckpt-0.npz").write_bytes(b"")
    model_path, cfg = evaluate.parse_command_line([str(tmp_path)], "test")
    assert model_path == str(tmp_path) and cfg.experiment_name == "from_folder" and cfg.nlabels == 3
    with pytest.raises(SystemExit):
        evaluate.parse_command_line([], "test")                      # EXP_PATH is required
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError):
        evaluate.parse_command_line([str(empty)], "test")


def test_output_file_names_and_sample_counts():
    import types
    from phiseg_code_amd import phiseg_test_predictions as tp
    from phiseg_code_amd import phiseg_test_quantitative as tq
    from phiseg_code_amd.phiseg.model_zoo import likelihoods
    assert tq.N_SAMPLES == 50 and tq.MODEL_SELECTION == "best_ged" and tp.MODEL_SELECTION == "best_dice"
    assert tq.output_files("exp") == (os.path.join("exp", "ged50_best_ged.npz"), os.path.join("exp", "ncc50_best_ged.npz"))
    assert tq.output_files("exp", 8) == (os.path.join("exp", "ged8_best_ged.npz"), os.path.join("exp", "ncc8_best_ged.npz"))
    assert tp.output_file("exp") == os.path.join("exp", "dice_best_dice.npz")
    assert tp.default_num_samples(types.SimpleNamespace(likelihood=likelihoods.phiseg)) == 100
    assert tp.default_num_samples(types.SimpleNamespace(likelihood=likelihoods.det_unet2D)) == 1
    for mod in (tq, tp):
        import inspect
        sig = inspect.signature(mod.main)
        assert list(sig.parameters) == ["model_path", "exp_config", "do_plots", "n_samples", "data"]
        assert sig.parameters["do_plots"].default is False and sig.parameters["n_samples"].default is None


def test_the_scripts_run_as_modules_and_ask_for_exp_path():
    """python -m phiseg_code_amd.<name> without arguments: argparse's usage error (exit status 2) naming EXP_PATH."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("phiseg_test_quantitative", "phiseg_test_predictions"):
        r = subprocess.run([sys.executable, "-m", "phiseg_code_amd." + name], cwd=root, capture_output=True, text=True)
        assert r.returncode == 2 and "EXP_PATH" in r.stderr, r.stderr
