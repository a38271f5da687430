"""Float64 numpy yardsticks and input builders of the many-class tests (9 <= C <= 256; csrc/many_class.hip).

Nothing here touches the GPU.  The residual multinoulli loss is restated from phiseg_model.py:229-262 as include/phx.h states it for
phx_residual_ce; the metrics yardstick is oracle/metrics.py itself, this module only builds inputs whose arg-max no float32 rounding
can flip (checked here, on the CPU, when a case is built)."""
import functools

import numpy as np

CLASS_COUNTS = (9, 16, 17, 19, 33, 256)      # one chunk + one class, whole chunks, odd strides that break 16-byte alignment, the cap
MAPS = ((32, 32, (0, 1, 2, 3, 4)),           # every shift the kernel takes, the 16x level whose wave sums meet in LDS
        (24, 40, (0, 1, 3)))                 # partial 16 x 16 tiles, a skipped shift
BATCH = 2
WEIGHT = 0.7


def label_maps(B, H, W, C):
    """(x + 3 y + b) % C: classes 0 and C - 1 both occur (oracle.init.synthetic_batch leaves the high classes out).  Where the map is
    too small for the pattern to reach C - 1 (C = 256 on 32 x 32: x + 3 y + b <= 125) the last pixel of every image is set to it."""
    y, x = np.mgrid[0:H, 0:W]
    lab = np.stack([(x + 3 * y + b) % C for b in range(B)]).astype(np.uint8)
    if lab.max() < C - 1:
        lab[:, -1, -1] = C - 1
    return lab


def upsample(a, sh):
    """NEAREST_NEIGHBOR resize by 2^sh of [B, h, w, C]"""
    return a.repeat(1 << sh, axis=1).repeat(1 << sh, axis=2)


def block_sum(a, sh):
    """its adjoint: the sum of every 2^sh x 2^sh block"""
    B, H, W, C = a.shape
    f = 1 << sh
    return a.reshape(B, H // f, f, W // f, f, C).sum(axis=(2, 4))


def softmax_and_lse(a):
    m = a.max(axis=-1, keepdims=True)
    e = np.exp(a - m)
    se = e.sum(axis=-1, keepdims=True)
    return e / se, (m + np.log(se))[..., 0]


def residual_ce(s_list, shifts, labels, weight, inv_batch):
    """s_list[l] [B, H >> shifts[l], W >> shifts[l], C] float64, labels [B, H, W] u8 or None
    -> dict(losses [L] (None without labels), ds [L] (None without labels), s_out, sm)"""
    L = len(s_list)
    full = [upsample(np.asarray(s, np.float64), sh) for s, sh in zip(s_list, shifts)]
    acc, A = None, [None] * L
    for l in reversed(range(L)):
        acc = full[l] if acc is None else acc + full[l]
        A[l] = acc
    sm0, _ = softmax_and_lse(A[0])
    out = dict(s_out=A[0], sm=sm0, losses=None, ds=None)
    if labels is None:
        return out
    C = A[0].shape[-1]
    onehot = np.eye(C)[labels.astype(np.int64)]
    losses, G = [], []
    for l in range(L):
        sm, lse = softmax_and_lse(A[l])
        losses.append(inv_batch * float((lse - (A[l] * onehot).sum(axis=-1)).sum()))
        G.append((sm - onehot) * (weight * inv_batch))
    ds, run = [], 0.0
    for k in range(L):                       # s_k enters A_l for every l <= k
        run = run + G[k]
        ds.append(block_sum(run, shifts[k]))
    out.update(losses=np.asarray(losses), ds=ds)
    return out


@functools.lru_cache(maxsize=None)
def residual_ce_case(C, H, W, shifts):
    """-> (s_list float32, labels, yardstick with labels, yardstick of the sampling form); computed once, read-only"""
    rng = np.random.default_rng([C, H, W, len(shifts)])
    s = [(rng.standard_normal((BATCH, H >> sh, W >> sh, C)) * 1.5).astype(np.float32) for sh in shifts]
    lab = label_maps(BATCH, H, W, C)
    assert {0, C - 1} <= set(np.unique(lab).tolist())
    ref = residual_ce(s, shifts, lab, WEIGHT, 1.0 / BATCH)
    for a in s + [lab, ref["s_out"], ref["sm"], ref["losses"]] + ref["ds"]:
        a.setflags(write=False)
    return s, lab, ref


def xent_map(logits, labels):
    l64 = np.asarray(logits, np.float64)
    _, lse = softmax_and_lse(l64)
    return lse - np.take_along_axis(l64, labels.astype(np.int64)[:, None], axis=1)[:, 0]


# ---- metrics -----------------------------------------------------------------------------------------------------------------------------
METRIC_CASES = ((9, 2), (19, 2))             # (C, images); N = 5 samples, M = 3 annotations, 16 x 24 pixels
MET_N, MET_M, MET_X, MET_Y = 5, 3, 16, 24
ARGMAX_MARGIN = 1e-3                         # a sample's arg-max: float32 soft-max values carry 6e-8 of rounding
MEAN_MARGIN = 1e-6                           # the arg-max of the mean: kernel and oracle both add the SAME float32 values in double (1e-16)


@functools.lru_cache(maxsize=None)
def metrics_case(C, img):
    """-> (sm [N, X, Y, C] float32, gts [M, X, Y] u8, annotator of the Dice reference, oracle GED, NCC, Dice [C]).
    Annotations follow the (x + 3 y + b) % C pattern, with blocks of disagreement between annotators; a sample favours the class of one
    annotation (or a neighbour class) by 1 to 3 logits over the runner-up.  Every sample's arg-max wins by ARGMAX_MARGIN, the arg-max of the mean soft-max by MEAN_MARGIN."""
    from oracle import metrics as om
    rng = np.random.default_rng([C, img, 77])
    y, x = np.mgrid[0:MET_X, 0:MET_Y]
    gts = np.stack([(x + 3 * y + img + np.where((x // 4 + y // 4 + j) % 3 == 0, j, 0)) % C for j in range(MET_M)]).astype(np.uint8)
    assert {0, C - 1} <= set(np.unique(gts).tolist())
    logits = rng.standard_normal((MET_N, MET_X, MET_Y, C))
    for k in range(MET_N):
        fav = (gts[k % MET_M].astype(np.int64) + (rng.random((MET_X, MET_Y)) < 0.25)) % C
        np.put_along_axis(logits[k], fav[..., None], logits[k].max(axis=-1, keepdims=True) + 1.0 + 2.0 * rng.random((MET_X, MET_Y, 1)), axis=-1)
    sm64, _ = softmax_and_lse(logits)
    sm = sm64.astype(np.float32)
    for a, margin in [(k, ARGMAX_MARGIN) for k in sm.astype(np.float64)] + [(sm.astype(np.float64).mean(axis=0), MEAN_MARGIN)]:
        top = np.sort(a, axis=-1)
        assert (top[..., -1] - top[..., -2]).min() > margin, "an arg-max of this case is within rounding of a tie"
    annot = (img + 1) % MET_M
    ged, ncc, dice = om.validation_metrics(sm, gts, gts[annot], C)
    for a in (sm, gts):
        a.setflags(write=False)
    return sm, gts, annot, ged, ncc, np.asarray(dice)
