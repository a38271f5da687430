"""Worker of tests/test_layer_norm_gpu.py::test_resume_is_bit_identical_in_deterministic_mode (PHX_DETERMINISTIC is read once per
process): the tiny layer_norm=tfnorm.layer_norm configuration, fp32.
    DIR   two uninterrupted training steps, and one step + save_weights + load_weights into a fresh model + one step: prints one digest
          of the final loss terms, parameters, optimiser slots and step counter for each"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_dir = sys.argv[1]
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    from phiseg_code_amd.tfwrapper import normalisation as tfnorm
    from tests.helpers import load_golden
    from tests.test_graph_cpu import make_config
    _, cfg, _ = load_golden("tiny_phiseg_gn4")
    c = make_config(cfg, "f32")
    c.layer_norm = tfnorm.layer_norm

    def steps(model, k0, k1):
        keys = sorted(model.loss_dict)
        out = None
        for k in range(k0, k1):
            x, s = synthetic.philox_batch(2, cfg["H"], cfg["nlabels"], seed=77, step=k)
            out = model.sess.run([model.train_step] + [model.loss_dict[key] for key in keys],
                                 {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: 1e-3})
        return np.asarray(out[1:], dtype=np.float32)

    def digest(model, losses):
        h = hashlib.sha256(losses.tobytes())
        st = model.sess.store
        blob = st.export()
        for k in sorted(blob):
            h.update(blob[k].tobytes())
        for k, per_var in sorted(st.export_slots().items()):
            for sn in sorted(per_var):
                h.update(per_var[sn].tobytes())
        h.update(st.step.cpu().numpy().tobytes())
        return h.hexdigest()

    a = phiseg_model.phiseg(c, rng_seed=cfg["eps_seed"])
    print("DIGEST", digest(a, steps(a, 0, 2)))
    b = phiseg_model.phiseg(c, rng_seed=cfg["eps_seed"])
    steps(b, 0, 1)
    b.save_weights(os.path.join(out_dir, "resume.ckpt-1"))
    r = phiseg_model.phiseg(c, rng_seed=cfg["eps_seed"])
    r.load_weights(os.path.join(out_dir, "resume.ckpt-1"))
    print("DIGEST", digest(r, steps(r, 1, 2)))


if __name__ == "__main__":
    main()
