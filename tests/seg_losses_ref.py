"""numpy restatement of the reference's tfwrapper/losses.py (get_dice, dice_loss, cross_entropy_loss,
pixel_wise_cross_entropy_loss_weighted) with analytic gradients with respect to the logits.

Every function takes logits [B, H, W, C] and u8 labels [B, H, W] (the one-hot is built here) and computes in the dtype given:
np.float64 is the reference the tests compare against, np.float32 the same formulas at the device's precision -- its distance to the
float64 result is the yardstick of the error band.  The hard prediction is the arg-max of the logits as given
(first maximum wins), in every dtype, so that ties are broken on the same numbers the device sees."""
import numpy as np


def one_hot(labels, C, dtype):
    return (np.asarray(labels)[..., None] == np.arange(C)).astype(dtype)


def softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _softmax_vjp(sm, g):
    """g = d loss / d softmax -> d loss / d logits"""
    return sm * (g - (g * sm).sum(axis=-1, keepdims=True))


def dice_modes(mode=None, **kw):
    """losses.py:84-99 -> (sum_over_labels, sum_over_batches)"""
    if mode == 'macro':
        return False, False
    if mode == 'macro_robust':
        return False, True
    if mode == 'micro':
        return True, False
    if mode is None:
        return kw.get('per_structure'), kw.get('sum_over_batches', False)
    raise ValueError("Encountered unexpected 'mode' in dice_loss: '%s'" % mode)


def _dice_parts(prediction, y, sum_over_labels, sum_over_batches):
    axes = (1, 2)
    if sum_over_batches:
        axes = (0,) + axes
    if sum_over_labels:
        axes = axes + (3,)
    return (prediction * y).sum(axis=axes), prediction.sum(axis=axes), y.sum(axis=axes), axes


def get_dice(logits, labels, epsilon=1e-10, sum_over_labels=False, sum_over_batches=False, use_hard_pred=True, dtype=np.float64):
    """losses.py:8-47 -> [B, C]; [C] with sum_over_batches; [B] with sum_over_labels; a scalar with both"""
    C = logits.shape[-1]
    y = one_hot(labels, C, dtype)
    if use_hard_pred:
        prediction = one_hot(np.argmax(logits, axis=-1), C, dtype)
    else:
        prediction = softmax(logits.astype(dtype))
    i, l, r, _ = _dice_parts(prediction, y, sum_over_labels, sum_over_batches)
    return 2 * i / (l + r + dtype(epsilon))


def dice_loss(logits, labels, epsilon=1e-10, sum_over_labels=False, sum_over_batches=False, only_foreground=False,
              dtype=np.float64, with_grad=True):
    """losses.py:50-119 with the mode already resolved (dice_modes) -> (loss, d loss / d logits)"""
    if only_foreground and sum_over_labels:
        raise ValueError("only_foreground slices a label axis that sum_over_labels removed (the reference fails there too)")
    C = logits.shape[-1]
    y = one_hot(labels, C, dtype)
    sm = softmax(logits.astype(dtype))
    i, l, r, axes = _dice_parts(sm, y, sum_over_labels, sum_over_batches)
    D = l + r + dtype(epsilon)
    dice = 2 * i / D
    sel = dice[..., 1:] if only_foreground else dice
    loss = dtype(1) - sel.mean(dtype=dtype)
    if not with_grad:
        return loss, None
    # d loss / d dice = -1 / (number of entries in the mean) on the selected entries
    w = np.zeros_like(dice)
    if only_foreground:
        w[..., 1:] = dtype(-1.0 / sel.size)
    else:
        w[...] = dtype(-1.0 / sel.size)
    alpha = np.expand_dims(w * 2 / D, axes)                     # coefficient of y in d loss / d sm
    beta = np.expand_dims(-w * 2 * i / (D * D), axes)
    g = alpha * y + beta
    return loss, _softmax_vjp(sm, g * np.ones_like(sm))


def cross_entropy_loss(logits, labels, use_sigmoid=False, class_weights=None, dtype=np.float64):
    """losses.py:123-131 (class_weights None) and :135-159 -> (loss, d loss / d logits)"""
    C = logits.shape[-1]
    x = logits.astype(dtype)
    y = one_hot(labels, C, dtype)
    if use_sigmoid:
        assert class_weights is None
        e = np.exp(-np.abs(x))
        loss = (np.maximum(x, 0) - x * y + np.log1p(e)).mean(dtype=dtype)
        s = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
        return loss, (s - y) / dtype(x.size)
    mx = x.max(axis=-1, keepdims=True)
    e = np.exp(x - mx)
    se = e.sum(axis=-1, keepdims=True)
    ce = ((mx + np.log(se)) * y.sum(axis=-1, keepdims=True) - (x * y).sum(axis=-1, keepdims=True))[..., 0]
    w = np.ones(C, dtype) if class_weights is None else np.asarray(class_weights, dtype=np.float32).astype(dtype)
    wmap = (y * w).sum(axis=-1)
    n = dtype(ce.size)
    loss = (ce * wmap).mean(dtype=dtype)
    grad = wmap[..., None] * (e / se * y.sum(axis=-1, keepdims=True) - y) / n
    return loss, grad


def pixel_wise_cross_entropy_loss_weighted(logits, labels, class_weights, dtype=np.float64):
    return cross_entropy_loss(logits, labels, class_weights=class_weights, dtype=dtype)


def nn_resize_adjoint(dfine, shift, dtype=np.float64):
    B, H, W, C = dfine.shape
    f = 1 << shift
    return dfine.astype(dtype).reshape(B, H // f, f, W // f, f, C).sum(axis=(2, 4), dtype=dtype)


# ---- seeded cases ----------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 5, 7, 2), (2, 5, 7, 3), (3, 8, 8, 4), (1, 16, 16, 8), (2, 33, 31, 5), (2, 64, 64, 4)]


def make_case(shape, seed=0, kind="normal"):
    """-> (logits f32 [B,H,W,C], labels u8 [B,H,W]).  Logits N(0, 3); labels uniform, with class C-1 absent from image 0 and, for
    B >= 2, the last image of one class.  kind = "extreme": logits of +-40 (fp32 exp underflows for the losing classes);
    kind = "ties": small integer logits, so that many pixels have exactly tied maxima."""
    B, H, W, C = shape
    rng = np.random.default_rng(1000 + seed)
    if kind == "extreme":
        logits = np.where(rng.random(shape) < 0.5, -40.0, 40.0)
    elif kind == "ties":
        logits = rng.integers(-1, 2, size=shape).astype(np.float64)
    else:
        logits = rng.normal(0.0, 3.0, size=shape)
    labels = rng.integers(0, C, size=(B, H, W))
    labels[0][labels[0] == C - 1] = 0                 # a class absent from one image
    if B >= 2:
        labels[B - 1] = 1                             # an image of a single class
    return logits.astype(np.float32), labels.astype(np.uint8)


DICE_FLAG_SETS = [  # (sum_over_labels, sum_over_batches, only_foreground): macro, macro_robust, micro, both sums; with / without foreground
    (False, False, False), (False, False, True), (False, True, False), (False, True, True), (True, False, False), (True, True, False)]


def band(dev, ref64, ref32, mult=4.0, floor_ulp=4.0):
    """The acceptance band: error of `dev` against the float64 restatement <= mult x the error of the float32 restatement, with a floor
    of floor_ulp fp32 ulps of the largest magnitude compared -> (ok, observed error, allowed error)."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    err = float(np.max(np.abs(np.asarray(dev, dtype=np.float64) - ref64))) if ref64.size else 0.0
    e32 = float(np.max(np.abs(np.asarray(ref32, dtype=np.float64) - ref64))) if ref64.size else 0.0
    big = float(np.max(np.abs(ref64))) if ref64.size else 0.0
    floor = floor_ulp * float(np.spacing(np.float32(big))) if big > 0 else floor_ulp * float(np.finfo(np.float32).tiny)
    allowed = max(mult * e32, floor)
    return err <= allowed, err, allowed
