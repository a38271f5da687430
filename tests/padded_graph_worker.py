"""Worker of tests/test_padded_graph_gpu.py, started with PHX_DETERMINISTIC=1 in its environment (the engine and the library read the
variable once, at import / first use; without it cross-block reductions of the existing path sum with float atomics and no two runs
agree to the bit): every (network, normalisation, storage type) of tests/padded_net.py as a training plan run eagerly
and captured into a hipGraph (eager warm-up, capture + launch, replay), from the same state.  Prints one JSON line: per configuration
the names whose values differ between the two, the number of gradients compared and the loss."""
import json

import numpy as np

from tests import padded_net as N


def main():
    from phiseg_code_amd import engine_common
    out = {}
    for kind in ("unet", "mixed"):
        for norm in ("identity", "batch_norm"):
            g, t = N.build(kind, norm)
            vals = N.values(g)
            x, lab = N.inputs(kind)
            for dtype in ("f32", "bf16"):
                eager = N.run_plan(g, t, vals, x, lab, compute_dtype=dtype, use_hip_graph=False)
                captured = N.run_plan(g, t, vals, x, lab, compute_dtype=dtype, use_hip_graph=True, runs=3)
                differ = [n for n in eager[2] if not np.array_equal(eager[2][n], captured[2][n])]
                if eager[0] != captured[0]:
                    differ.append("loss")
                if not np.array_equal(eager[1], captured[1]):
                    differ.append("logits")
                trainable = [n for n, v in g.variables.items() if v.trainable]
                out["%s/%s/%s" % (kind, norm, dtype)] = dict(deterministic=bool(engine_common._DETERMINISTIC), differ=differ,
                                                            ngrads=len([n for n in trainable if n in eager[2]]), loss=eager[0])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
