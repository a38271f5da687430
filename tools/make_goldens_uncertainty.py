#!/usr/bin/env python3
"""Write tests/golden/uncertainty_cases.npz by EXECUTING THE REFERENCE'S OWN, unmodified code (build container only; needs
/root/reference):

* phiseg_model.phiseg.predict_segmentation_sample_variance_sm_cov, .predict_segmentation_sample_variance_sm_cov_bf,
  .get_crossentropy_error_map and .predict_mean_variance_and_error_maps, bound to a stub `self` whose sess.run replays a recorded
  list of FLOAT64 sample arrays (so the stored maps are the exact yardstick); the per-sample eval_xent maps the reference forms
  inside TensorFlow come from tools/tf1_shim's softmax_cross_entropy_with_logits_v2 on the float64 logits;
* generate_error_maps of phiseg_generate_samples.py, imported with empty stand-ins for the modules this image lacks.

Inputs are re-created from seeds (tests/uncertainty_ref.py); only the case list and the expected maps are stored."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "tf1_shim"))
sys.path.insert(0, REF)
os.environ.setdefault("SGE_GPU", "0")

import shim  # noqa: E402

shim.install()
class _Empty(types.ModuleType):
    """Stand-in for a module this image lacks: every attribute (cv2.INTER_LINEAR in a default argument, mpl.use) is a no-op."""

    def __getattr__(self, attr):
        if attr.startswith("__"):
            raise AttributeError(attr)
        return lambda *a, **k: None


for name in ("cv2", "matplotlib", "matplotlib.pyplot", "nibabel", "skimage", "skimage.measure", "skimage.transform", "medpy",
             "medpy.metric", "data", "data.data_switch"):
    sys.modules[name] = _Empty(name)
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
sys.modules["skimage"].measure, sys.modules["skimage"].transform = sys.modules["skimage.measure"], sys.modules["skimage.transform"]
sys.modules["medpy"].metric = sys.modules["medpy.metric"]
sys.modules["data"].data_switch = sys.modules["data.data_switch"]
sys.modules["data.data_switch"].data_switch = None

from phiseg import phiseg_model as ref_model  # noqa: E402          (reference file)
import phiseg_generate_samples as ref_samples  # noqa: E402         (reference file)

from tests import uncertainty_ref as U  # noqa: E402               (seeded inputs, shared with the tests)


class _Replay:
    """sess.run of the stub: the k-th fetch of a tensor returns the k-th recorded array of that tensor."""

    def __init__(self, recorded):
        self.recorded, self.count = recorded, {}

    def _one(self, key):
        k = self.count.get(key, 0)
        self.count[key] = k + 1
        return self.recorded[key][k]

    def run(self, fetches, feed_dict=None):
        if isinstance(fetches, (list, tuple)):
            return [self._one(f) for f in fetches]
        return self._one(fetches)


def stub_model(logits, sm, s_ref, C):
    N, X, Y, _ = sm.shape
    m = types.SimpleNamespace(training_pl="training_pl", x_inp="x_inp", s_inp="s_inp", s_out_eval="s_out_eval", s_out_eval_sm="s_out_eval_sm",
                              eval_xent="eval_xent", exp_config=types.SimpleNamespace(image_size=(X, Y, 1)))
    lg64, sm64 = logits.astype(np.float64), sm.astype(np.float64)
    oh = np.eye(C, dtype=np.float64)[s_ref.astype(np.int64)][None]
    xent = [shim.nn_softmax_xent_v2(labels=torch.from_numpy(oh), logits=torch.from_numpy(lg64[i][None])).v.numpy() for i in range(N)]
    m.sess = _Replay({"s_out_eval": [lg64[i][None] for i in range(N)], "s_out_eval_sm": [sm64[i][None] for i in range(N)],
                      "eval_xent": xent})
    return m


def real(a):
    a = np.asarray(a)
    assert np.abs(a.imag).max() <= 1e-12 if np.iscomplexobj(a) else True
    return np.ascontiguousarray(a.real, dtype=np.float64)


def reference_results(logits, sm, gts, s_ref, C):
    N = sm.shape[0]
    P = ref_model.phiseg
    out = {}
    out["cov_trace"] = real(P.predict_segmentation_sample_variance_sm_cov(stub_model(logits, sm, s_ref, C), None, N))
    out["cov_det"] = real(P.predict_segmentation_sample_variance_sm_cov_bf(stub_model(logits, sm, s_ref, C), None, N))
    out["xent_map"] = real(np.squeeze(P.get_crossentropy_error_map(stub_model(logits, sm, s_ref, C), s_ref[None], None, N)))
    means, std, errs = P.predict_mean_variance_and_error_maps(stub_model(logits, sm, s_ref, C), s_ref[None], None, N)
    out["argmax"], out["std_mean"], out["xent_mean"] = np.asarray(means).astype(np.uint8), real(std), real(errs)
    # the determinant without the last class: the same reference method on samples whose last class was removed
    out["cov_det_drop_last"] = real(P.predict_segmentation_sample_variance_sm_cov_bf(stub_model(logits, sm[..., :-1], s_ref, C), None, N)) \
        if C > 2 else real(np.var(sm[..., 0].astype(np.float64), axis=0, ddof=1))       # (np.cov of one row is a scalar: det rejects it)
    e_ss, e_sy, e_yy = ref_samples.generate_error_maps(sm.astype(np.float64), np.eye(C, dtype=np.float64)[gts.astype(np.int64)])
    out["e_ss"], out["e_sy"], out["e_yy"] = real(e_ss), real(e_sy), real(e_yy)
    return out


if __name__ == "__main__":
    blob = {"cases": np.array([list(c[:6]) for c in U.CASES], dtype=np.int64)}
    for k, case in enumerate(U.CASES):
        C = case[5]
        logits, sm, gts, s_ref = U.uncertainty_case(k)
        r = reference_results(logits, sm, gts, s_ref, C)
        assert np.abs(r["xent_map"] - r["xent_mean"]).max() == 0.0
        del r["xent_map"]
        for name, v in r.items():
            blob["%d/%s" % (k, name)] = v
        _, smu, _, _ = U.uncertainty_case(k, unnormalised=True)
        blob["%d/cov_det_unnormalised" % k] = real(ref_model.phiseg.predict_segmentation_sample_variance_sm_cov_bf(
            stub_model(logits, smu, s_ref, C), None, smu.shape[0]))
        print(case, {n: float(np.abs(v).max()) for n, v in r.items()}, "unnorm det max %.3e" % np.abs(blob["%d/cov_det_unnormalised" % k]).max())
    path = os.path.join(ROOT, "tests", "golden", "uncertainty_cases.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")
