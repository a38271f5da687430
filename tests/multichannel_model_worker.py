"""Worker of tests/test_multichannel_model_gpu.py: four training steps (eager, hipGraph capture, two replays) of the tiny PHiSeg on a
multi-channel image, then one digest of every loss term, gradient and parameter.  Started with PHX_DETERMINISTIC=1, twice: the digests
must agree."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    Cx, dtype, steps = int(sys.argv[1]), sys.argv[2], int(sys.argv[3])
    from tests.test_multichannel_model_gpu import build
    model, cfg, params, x, s = build(Cx, dtype=dtype, perturbed=True)
    h = hashlib.sha256()
    keys = sorted(model.loss_dict)
    for _ in range(steps):
        out = model.sess.run([model.train_step] + [model.loss_dict[k] for k in keys],
                             {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: 1e-3})
        h.update(np.asarray(out[1:], dtype=np.float32).tobytes())
    st = model.sess.store
    for blob in (st.export(grads=True), st.export()):
        for k in sorted(blob):
            h.update(blob[k].tobytes())
    print("DIGEST", h.hexdigest(), float(out[-1]))


if __name__ == "__main__":
    main()
