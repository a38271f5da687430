"""Worker of tests/test_volume_graph_gpu.py, started with PHX_DETERMINISTIC=1 in its environment (the engine and the library read the
variable once, at import / first use): the toy 3-D U-Net's training plan captured into a hipGraph, run twice from the same state, and
once uncaptured.  Prints one JSON line: per normalisation whether loss and every gradient are bit-identical between the two captured
runs and between the captured and the uncaptured plan."""
import json

import numpy as np

from tests import volume_net as N


def main():
    from phiseg_code_amd import engine_common
    out = {}
    for norm in ("identity", "batch_norm"):
        g, t = N.build(norm)
        vals = N.values(g)
        x, lab = N.inputs(g, t)
        runs = [N.run_plan(g, t, vals, x, lab, use_hip_graph=True) for _ in range(2)]
        eager = N.run_plan(g, t, vals, x, lab, use_hip_graph=False)

        def same(a, b):
            return bool(a[0] == b[0] and np.array_equal(a[1], b[1]) and all(np.array_equal(a[2][n], b[2][n]) for n in a[2])
                        and all(np.array_equal(a[3][n], b[3][n]) for n in a[3]))
        out[norm] = dict(deterministic=bool(engine_common._DETERMINISTIC), repeat_equal=same(runs[0], runs[1]),
                         eager_equal=same(runs[0], eager), ngrads=len(runs[0][2]), loss=runs[0][0])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
