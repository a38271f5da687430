"""Worker of test_summary_gpu.test_losses_are_bit_identical_with_and_without_summaries: the same five training steps with and without
summaries in one process (started with PHX_DETERMINISTIC=1); prints per run the losses' bit patterns and one digest of the parameters,
the moving statistics and the optimiser step."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_dir = sys.argv[1]
    from phiseg_code_amd.phiseg import phiseg_model
    from tests.test_summary_gpu import _cfg, _data
    for name, on in (("on", True), ("off", False)):
        cfg = _cfg()
        model = phiseg_model.phiseg(cfg)
        np.random.seed(5)                                  # (validation draws its annotator from numpy's global stream)
        losses = model.train(_data(cfg), num_iter=5, log_every=0, log_dir=os.path.join(out_dir, name), summaries=on)
        st = model.sess.store
        h = hashlib.sha256()
        blob = st.export()
        for k in sorted(blob):
            h.update(blob[k].tobytes())
        h.update(st.step.cpu().numpy().tobytes())
        print("RUN", name, " ".join(np.float32(l).tobytes().hex() for l in losses), h.hexdigest())


if __name__ == "__main__":
    main()
