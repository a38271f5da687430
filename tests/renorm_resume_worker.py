"""Worker of the batch-renorm tests that need PHX_DETERMINISTIC=1 (read once per process), tiny layer_norm=batch_renorm configuration.
    resume DIR   three uninterrupted training steps, and two steps + save_weights + load_weights into a fresh model + one step: prints
                 one digest of the final loss terms, parameters, state and optimiser slots for each
    step0        one step-0 gradient evaluation of the renorm model and of the batch-norm model from the same initial values: prints the
                 largest relative difference of a loss term, of a trainable gradient (to the variable's max) and of the renorm model's
                 moving mean against a tenth of the batch-norm model's update"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step0(cfg, c_rn, c_bn):
    from phiseg_code_amd import engine
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    x, s = synthetic.philox_batch(2, cfg["H"], cfg["nlabels"], seed=77, step=0)
    res = {}
    for kind, c in (("bn", c_bn), ("rn", c_rn)):
        model = phiseg_model.phiseg(c, rng_seed=cfg["eps_seed"])
        store = model.sess._ensure_store()
        init = store.export()
        keys = sorted(model.loss_dict)
        plan = engine.Plan(store, [model.loss_dict[k] for k in keys], loss=model.loss_tot, batch=2, training=True, compute_dtype="f32",
                           optimize=False, rng_seed=cfg["eps_seed"], use_hip_graph=False)
        plan.set_input("x_input", x)
        plan.set_input("s_input", s)
        plan.run(sync=True)
        res[kind] = dict(loss={k: float(plan.fetch(model.loss_dict[k])) for k in keys}, grads=store.export(grads=True), state=store.export(),
                         init=init, tail=any(fn is plan.L.renorm_tail_multi for fn, _ in plan.launches))
    bn, rn = res["bn"], res["rn"]
    name = lambda n: n.replace("/batch_renorm/", "/batch_norm/")
    assert all(np.array_equal(v, bn["init"][name(n)]) for n, v in rn["init"].items() if name(n) in bn["init"]), "initial values differ"
    assert rn["tail"] and not bn["tail"]
    e_loss = max(abs(rn["loss"][k] - bn["loss"][k]) / abs(bn["loss"][k]) for k in bn["loss"])
    e_grad, checked = 0.0, 0
    for n, g in rn["grads"].items():
        want = bn["grads"][name(n)].astype(np.float64)
        if np.abs(want).max() == 0.0:
            assert np.abs(g).max() == 0.0, n
            continue
        e_grad = max(e_grad, float(np.abs(g - want).max() / np.abs(want).max()))
        checked += 1
    mm = "posterior/z0_pre_1/batch_renorm/BatchNorm/moving_mean"
    want = 0.1 * bn["state"][name(mm)].astype(np.float64)           # 0.001 mu against batch norm's 0.01 mu
    assert np.abs(want).max() > 0
    e_mm = float(np.abs(rn["state"][mm] - want).max() / np.abs(want).max())
    print("STEP0 %.3e %.3e %.3e %d" % (e_loss, e_grad, e_mm, checked))


def main():
    mode = sys.argv[1]
    out_dir = sys.argv[2] if len(sys.argv) > 2 else None
    from phiseg_code_amd.data import synthetic
    from phiseg_code_amd.phiseg import phiseg_model
    from phiseg_code_amd.tfwrapper import normalisation as tfnorm
    from tests.helpers import load_golden
    from tests.test_graph_cpu import make_config
    _, cfg, _ = load_golden("tiny_phiseg_bn")
    c = make_config(cfg, "f32")
    c.layer_norm = tfnorm.batch_renorm
    if mode == "step0":
        return step0(cfg, c, make_config(cfg, "f32"))

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
    print("DIGEST", digest(a, steps(a, 0, 3)))
    b = phiseg_model.phiseg(c, rng_seed=cfg["eps_seed"])
    steps(b, 0, 2)
    b.save_weights(os.path.join(out_dir, "resume.ckpt-2"))
    r = phiseg_model.phiseg(c, rng_seed=cfg["eps_seed"])
    r.load_weights(os.path.join(out_dir, "resume.ckpt-2"))
    print("DIGEST", digest(r, steps(r, 2, 3)))


if __name__ == "__main__":
    main()
