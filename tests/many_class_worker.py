"""Worker of tests/test_many_class_kernels_gpu.py: the residual-CE and metrics cases of csrc/many_class.hip inside ONE process started
with PHX_DETERMINISTIC=1.  Every case is checked against its float64 yardstick, run a second time, and a digest of the bytes it wrote
is printed: the parent runs the same cases with the variable unset and compares -- the wide kernels promise the same bits in every mode.

Output: `CASE <name> <sha256>` per case, then `DONE <count>`.  Any exception ends the process with a non-zero status at once."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RESIDUAL = [(9, 24, 40, (0, 1, 3)), (19, 32, 32, (0, 1, 2, 3, 4)), (256, 24, 40, (0, 1, 3))]
METRICS = [(9, "imp"), (19, "ipm")]


def digests(L):
    from tests import many_class_cases as K
    out = {}
    for C, H, W, sh in RESIDUAL:
        a, b = K.residual_ce_full(L, C, H, W, sh), K.residual_ce_full(L, C, H, W, sh)
        assert a == b, "residual_ce_wide C=%d: two launches differ in bits" % C
        out["residual_ce_wide[%d-%dx%d]" % (C, H, W)] = hashlib.sha256(a).hexdigest()
    for C, layout in METRICS:
        a, b = K.metrics_full(L, C, layout), K.metrics_full(L, C, layout)
        assert a == b, "metrics_wide C=%d: two launches differ in bits" % C
        out["metrics_wide[%d-%s]" % (C, layout)] = hashlib.sha256(a).hexdigest()
    return out


if __name__ == "__main__":
    assert os.environ.get("PHX_DETERMINISTIC") == "1", "start this worker with PHX_DETERMINISTIC=1"
    import torch
    from phiseg_code_amd import runtime as rt
    assert torch.cuda.is_available()
    d = digests(rt.lib())
    for k, v in d.items():
        print("CASE %s %s" % (k, v))
    print("DONE %d" % len(d))
