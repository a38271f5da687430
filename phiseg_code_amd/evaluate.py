"""Test-set evaluation: GED, variance-NCC and per-label Dice of every image of a split, scored on the device from the buffers the
sampling pass and the data provider already hold (phx_eval_metrics, csrc/eval_metrics.hip).

The reference scores a test set with phiseg_test_quantitative.py (GED / NCC over 50 samples) and phiseg_test_predictions.py (Dice of the
mean of 100 samples): per image one sess.run, the samples pulled to the host, the IoU loops in Python.  Here a pass feeds
`images_per_pass` images, draws all their samples at once (model.sampling_graph where the prior shares an x-only encoder, x repeated
on s_out_eval_sm otherwise -- the policy of phiseg._mc_maps), and the scoring kernel reads the plan's soft-max buffer in place on the
plan's stream; a pass ends with one wait for its stream (the noise step must not move under it), and only the [n, 2 + max(C, 8)] score table
comes back, once, at the end.  phiseg_test_quantitative / phiseg_test_predictions of this package are the reference's two scripts over
evaluate_split."""
import glob
import importlib.util
import os

import numpy as np

DEFAULT_IMAGES_PER_PASS = 4          # the fastest of 1, 2, 4 measured at 100 samples, 128 x 128 (LABBOOK.md: 306 / 359 / 395 images/s)


def evaluate_split(model, split, num_samples, images_per_pass=DEFAULT_IMAGES_PER_PASS, n_images=None, annotator_range=None):
    """Score the first `n_images` (default: all) images of `split` with `num_samples` segmentation samples each.

    split: anything with .images [n, X, Y, 1] and .labels [n, X, Y, A] (a DeviceBatchProvider's .labels_dev is used as it is, other
    splits' labels are uploaded once).  GED (labels 1 .. nlabels-1) and NCC are taken against all A annotations; the Dice of the
    arg-max of the mean soft-max against the annotation of one annotator per image, np.random.choice(annotator_range) drawn in
    image order before the first pass, as _do_validation draws it (annotator_range: default exp_config.annotator_range).
    The noise step advances once per pass.  -> dict(ged [n], ncc [n], dice [n, nlabels], sref_annot [n])."""
    import torch
    from phiseg_code_amd import many_class
    from phiseg_code_amd import runtime as rt
    L = rt.lib()
    cfg = model.exp_config
    n, ipp = int(num_samples), int(images_per_pass)
    if n < 1 or ipp < 1:
        raise ValueError("num_samples and images_per_pass must be >= 1 (got %d, %d)" % (n, ipp))
    images, labels = split.images, split.labels
    total = int(images.shape[0]) if n_images is None else min(int(n_images), int(images.shape[0]))
    X, Y, A = int(labels.shape[1]), int(labels.shape[2]), int(labels.shape[3])
    P, C = X * Y, int(cfg.nlabels)
    if annotator_range is None:
        annotator_range = getattr(cfg, "annotator_range", range(A))
    annotator_range = list(annotator_range)
    if not annotator_range or min(annotator_range) < 0 or max(annotator_range) >= A:
        raise ValueError("annotator_range %r does not fit %d annotations per image" % (annotator_range, A))
    sref = np.asarray([np.random.choice(annotator_range) for _ in range(total)], dtype=np.int64)
    if total == 0:
        return dict(ged=np.zeros(0, np.float32), ncc=np.zeros(0, np.float32), dice=np.zeros((0, C), np.float32), sref_annot=sref)

    dev = torch.device("cuda", torch.cuda.current_device())
    labels_dev = getattr(split, "labels_dev", None)
    if labels_dev is None:
        labels_dev = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.uint8)).to(dev)
    if labels_dev.dtype != torch.uint8 or tuple(labels_dev.shape) != tuple(labels.shape) or not labels_dev.is_contiguous():
        raise ValueError("labels_dev must be a contiguous uint8 tensor of shape %s" % (tuple(labels.shape),))
    sref_dev = torch.as_tensor(sref.astype(np.uint8)).to(dev)
    wide = many_class.eval_metrics_entry(C) == "metrics_wide"
    row = many_class.metrics_row(C)
    out = torch.empty(total, row, dtype=torch.float32, device=dev)
    wsb = int((L.metrics_wide_ws_bytes if wide else L.eval_metrics_ws_bytes)(min(ipp, total), n, A, P, C))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)       # one scratch for every pass
    one_pass = n > 1 and model._one_pass_prior()
    sm_t = model.sampling_graph(n)[1] if one_pass else model.s_out_eval_sm
    torch.cuda.synchronize()                                   # uploaded on torch's stream, read on the plans'

    for i0 in range(0, total, ipp):
        b = min(ipp, total - i0)
        x = np.asarray(images[i0:i0 + b])
        if not one_pass:
            x = np.repeat(x, n, axis=0)                        # rows i * n + k, as sampling_graph lays them out
        plan, (sm,) = model.sess.run_buffers([sm_t], {model.training_pl: False, model.x_inp: x})
        if sm.dt != rt.F32 or sm.shift or tuple(sm.shape) != (b * n, X, Y, C):
            raise rt.PhxError("evaluate_split: the soft-max buffer is %s (dtype code %d), expected float32 %s"
                              % (sm.shape, sm.dt, (b * n, X, Y, C)))
        if wide:
            L.metrics_wide(sm.ptr, labels_dev.data_ptr() + i0 * P * A, 1, A, None, sref_dev.data_ptr() + i0, ws.data_ptr(), wsb, b, n, A, P,
                           C, 1, out.data_ptr() + i0 * row * 4, plan.stream)
        else:
            L.eval_metrics(sm.ptr, labels_dev.data_ptr() + i0 * P * A, sref_dev.data_ptr() + i0, ws.data_ptr(), wsb, b, n, A, P, C, 1,
                           out.data_ptr() + i0 * row * 4, plan.stream)
        # The pass reads the Philox step word on the device: it must have finished before the word moves (as in phiseg._mc_maps).
        # This wait is the only one of a pass and nothing is copied: the scores stay in `out` until every pass has run.
        plan.sync()
        model._advance_noise()
    res = out.cpu().numpy()
    return dict(ged=res[:, 0].copy(), ncc=res[:, 1].copy(), dice=res[:, 2:2 + C].copy(), sref_annot=sref)


# ---- what the reference's two test scripts share: the EXP_PATH command line and the data set ---------------------------------------
def load_experiment(exp_path):
    """EXP_PATH of the reference's test scripts: the experiment folder holds the checkpoints and a copy of its config module; the
    first *.py in it (by name) is loaded as exp_config.  -> (model_path, exp_config)"""
    configs = sorted(glob.glob(os.path.join(exp_path, "*.py")))
    if not configs:
        raise FileNotFoundError("no experiment config (*.py) in %s" % exp_path)
    name = os.path.splitext(os.path.basename(configs[0]))[0]
    spec = importlib.util.spec_from_file_location(name, configs[0])
    exp_config = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(exp_config)
    return exp_path, exp_config


def parse_command_line(argv, description):
    import argparse
    parser = argparse.ArgumentParser(description=description)
    parser.add_argument("EXP_PATH", type=str, help="Path to experiment folder (assuming you are in the working directory)")
    return load_experiment(parser.parse_args(argv).EXP_PATH)


def load_model_and_test_split(model_path, exp_config, model_selection, data=None):
    """The head of both scripts: build the model, load the `model_selection` checkpoint of the folder, open the data set."""
    from phiseg_code_amd.data.data_switch import data_switch
    from phiseg_code_amd.phiseg.phiseg_model import phiseg
    model = phiseg(exp_config=exp_config)
    model.load_weights(model_path, type=model_selection)
    if data is None:
        data = data_switch(exp_config.data_identifier)(exp_config)
    if getattr(data, "test", None) is None:
        raise ValueError("the data set has no test split")
    return model, data.test
