"""Worker of tests/test_leaky_relu_gpu.py, started with PHX_DETERMINISTIC=1 in its environment (the engine and the library read the
variable once, at import / first use): the training plan of the 2-D toy net of tests/leaky_net.py built for hipGraph capture and run
three times from the same state -- uncaptured (a plan's first run is always eager), the capture with its first launch, a replay --
with loss, logits and gradients read back after each, and once more as a plan that is never captured.  Prints one JSON line: what is
not bit-identical among them.

(The results of the first run are read back BEFORE the capture, as every caller in this repository does.  A plan that is captured
with nothing read back since its eager run replays differently from its first launch (MI355X, ROCm 7.2) -- the
volume net of tests/volume_net.py and a two-layer conv2D graph do the same, with or without this file's nodes, so it is not what this
worker is about; LABBOOK.md, "leaky_relu end to end", has the figures.)"""
import json

import numpy as np

from tests import leaky_net as N


def main():
    from phiseg_code_amd import engine_common
    g, t = N.build("2d")
    vals = N.values(g)
    x, lab = N.inputs(g, t)
    plan, store = N.make_plan(g, t, vals, x, lab, use_hip_graph=True)
    runs = []
    for _ in range(3):                           # eager, the capture + its first launch, a replay
        plan.run(sync=True)
        runs.append((float(plan.fetch(t["loss"])), plan.fetch(t["logits"]), store.export(grads=True)))
    captured = plan._graph_exec is not None
    eager = N.run_plan(g, t, vals, x, lab, use_hip_graph=False)

    def differing(a, b):
        """what is not bit-identical between two runs, with the largest difference: 'loss', 'logits', gradient names"""
        out = ["loss %.3e" % abs(a[0] - b[0])] if a[0] != b[0] else []
        out += [] if np.array_equal(a[1], b[1]) else ["logits %.3e" % np.abs(a[1] - b[1]).max()]
        return out + sorted("%s %.3e" % (n, np.abs(a[2][n] - b[2][n]).max()) for n in a[2] if not np.array_equal(a[2][n], b[2][n]))
    assert set(runs[0][2]) == set(runs[1][2]) == set(runs[2][2]) == set(eager[2])
    repeat, vs_eager = differing(runs[1], runs[2]), [differing(r, eager) for r in runs]
    print(json.dumps(dict(deterministic=bool(engine_common._DETERMINISTIC), captured=bool(captured), repeat_equal=not repeat,
                          eager_equal=not (vs_eager[0] or vs_eager[1] or vs_eager[2]), repeat_differs=repeat, first_run_vs_eager=vs_eager[0],
                          first_launch_vs_eager=vs_eager[1], replay_vs_eager=vs_eager[2], ngrads=len(runs[0][2]), loss=runs[0][0],
                          leaky_launches=sum(1 for fn, _ in plan.launches if getattr(fn, "__name__", "").startswith("phx_leaky_relu")))))


if __name__ == "__main__":
    main()
