"""The kernels of csrc/seg_losses.hip on the MI355X through the flat ABI: Dice sums / finish / gradient, the cross-entropy family and
the nearest-neighbour resize adjoint against the float64 restatement (tests/seg_losses_ref.py).

Acceptance (value and gradient): the device's error against float64 is at most 4x the error of the float32 numpy restatement on the same
inputs (a different summation order and the device expf / logf are what the margin is for), with a floor of 4 fp32 ulps of the largest
magnitude compared, for where the float32 restatement happens to be exact.  Every check prints its observed ratio."""
import functools

import numpy as np
import pytest

from tests import seg_losses_ref as R

pytestmark = pytest.mark.gpu
E_INVAL = -1


def _lib():
    from phiseg_code_amd import runtime as rt
    return rt.lib()


def _up(a, dtype):
    import torch
    return torch.tensor(np.array(a, dtype=dtype)).to(torch.device("cuda", torch.cuda.current_device()))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize()


def check(what, dev, ref64, ref32):
    ok, err, allowed = R.band(dev, ref64, ref32)
    print("%-64s error %.3e  allowed %.3e  ratio %.3f" % (what, err, allowed, err / allowed if allowed else 0.0))
    assert np.isfinite(np.asarray(dev, dtype=np.float64)).all(), what
    assert ok, (what, err, allowed)


@functools.lru_cache(maxsize=None)
def case(shape, kind="normal"):
    lg, lab = R.make_case(shape, seed=sum(shape), kind=kind)
    lg.setflags(write=False)
    lab.setflags(write=False)
    return lg, lab


class DiceRun:
    """phx_dice_sums once, then any number of finish / gradient calls on the same workspace."""

    def __init__(self, lg, lab):
        import torch
        self.L, self.shape = _lib(), lg.shape
        B, H, W, C = lg.shape
        self.lg, self.lab = _up(lg, np.float32), _up(lab, np.uint8)
        self.wsb = int(self.L.dice_ws_bytes(B, H, W, C))
        self.ws = torch.zeros(self.wsb, dtype=torch.uint8, device=self.lg.device)
        self.L.dice_sums(self.lg.data_ptr(), self.lab.data_ptr(), self.ws.data_ptr(), self.wsb, B, H, W, C, _stream())
        _sync()

    def finish(self, sol, sob, fg=False, hard=False, eps=1e-10, inv_batch=None):
        """-> (table, loss, coef [B, C, 2])"""
        import torch
        B, H, W, C = self.shape
        n = (1 if sob else B) * (1 if sol else C)
        table = torch.full((n,), np.nan, dtype=torch.float32, device=self.lg.device)
        loss = torch.full((1,), np.nan, dtype=torch.float32, device=self.lg.device)
        coef = torch.full((B, C, 2), np.nan, dtype=torch.float32, device=self.lg.device)
        self.L.dice_finish(self.ws.data_ptr(), self.wsb, B, H, W, C, int(hard), int(sol), int(sob), int(fg), eps,
                           1.0 / B if inv_batch is None else inv_batch, table.data_ptr(), loss.data_ptr(), coef.data_ptr(), _stream())
        _sync()
        shape = (() if sob else (B,)) + (() if sol else (C,))
        return table.cpu().numpy().reshape(shape), float(loss.cpu().numpy()[0]), coef

    def grad(self, coef, scale, prefill=None):
        import torch
        B, H, W, C = self.shape
        d = torch.full(self.shape, np.nan, dtype=torch.float32, device=self.lg.device) if prefill is None else _up(prefill, np.float32)
        self.L.dice_grad(self.lg.data_ptr(), self.lab.data_ptr(), coef.data_ptr(), scale, 0 if prefill is None else 1, d.data_ptr(),
                         B, H, W, C, _stream())
        _sync()
        return d.cpu().numpy()


def xent_device(lg, lab, class_weights=None, use_sigmoid=False, grad_scale=1.0, prefill=None, inv_batch=None, with_grad=True):
    import torch
    L = _lib()
    B, H, W, C = lg.shape
    dlg, dlab = _up(lg, np.float32), _up(lab, np.uint8)
    cw = _up(class_weights, np.float32) if class_weights is not None else None
    wsb = int(L.seg_xent_ws_bytes(B, H, W, C))
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dlg.device)
    loss = torch.full((1,), np.nan, dtype=torch.float32, device=dlg.device)
    d = None
    if with_grad:
        d = torch.full(lg.shape, np.nan, dtype=torch.float32, device=dlg.device) if prefill is None else _up(prefill, np.float32)
    L.seg_xent(dlg.data_ptr(), dlab.data_ptr(), cw.data_ptr() if cw is not None else None, int(use_sigmoid),
               1.0 / B if inv_batch is None else inv_batch, grad_scale, 0 if prefill is None else 1, loss.data_ptr(),
               d.data_ptr() if d is not None else None, ws.data_ptr(), wsb, B, H, W, C, _stream())
    _sync()
    return float(loss.cpu().numpy()[0]), (d.cpu().numpy() if d is not None else None)


CASES = [(s, "normal") for s in R.SHAPES] + [((2, 5, 7, 2), "extreme"), ((2, 33, 31, 5), "extreme")]


@pytest.mark.parametrize("shape,kind", CASES)
def test_dice_loss_table_and_gradient(shape, kind):
    lg, lab = case(shape, kind)
    run = DiceRun(lg, lab)
    rng = np.random.default_rng(5)
    pre = rng.normal(0.0, 1e-3, size=shape).astype(np.float32)
    for sol, sob, fg in R.DICE_FLAG_SETS:
        tag = "%s %s dice_loss sol=%d sob=%d fg=%d" % (shape, kind, sol, sob, fg)
        l64, g64 = R.dice_loss(lg, lab, 1e-10, sol, sob, fg)
        l32, g32 = R.dice_loss(lg, lab, 1e-10, sol, sob, fg, dtype=np.float32)
        _, loss, coef = run.finish(sol, sob, fg)
        check(tag + " value", loss, l64, l32)
        check(tag + " gradient (written)", run.grad(coef, 1.0), g64, g32)
        sc = np.float32(0.7)
        check(tag + " gradient (added, scale 0.7)", run.grad(coef, float(sc), prefill=pre),
              pre.astype(np.float64) + float(sc) * g64, pre + sc * g32)
    for hard in (False, True):
        for sol in (False, True):
            for sob in (False, True):
                t64 = R.get_dice(lg, lab, 1e-10, sol, sob, hard)
                t32 = R.get_dice(lg, lab, 1e-10, sol, sob, hard, dtype=np.float32)
                table, _, _ = run.finish(sol, sob, hard=hard)
                assert table.shape == t64.shape
                check("%s %s get_dice hard=%d sol=%d sob=%d" % (shape, kind, hard, sol, sob), table, t64, t32)
    # a rank's share under data parallel: inv_batch = 1 / (B * world) halves the per-image forms
    _, half, _ = run.finish(False, False, inv_batch=0.5 / shape[0])
    _, full, _ = run.finish(False, False)
    assert abs(half - 0.5 * full) <= 2 * float(np.spacing(np.float32(full)))
    # a larger epsilon enters the table as given
    check("%s %s get_dice soft eps=1e-3" % (shape, kind), run.finish(False, False, eps=1e-3)[0],
          R.get_dice(lg, lab, float(np.float32(1e-3)), use_hard_pred=False), R.get_dice(lg, lab, 1e-3, use_hard_pred=False, dtype=np.float32))


@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (3, 8, 8, 4), (2, 33, 31, 5), (2, 64, 64, 4)])
def test_hard_dice_with_tied_logits_is_the_integer_count_result(shape):
    """Logits with exact ties: the hard prediction is the FIRST maximum of the fp32 logits (tf.argmax), so the hard Dice equals the
    integer-count result exactly -- every pixel takes part."""
    lg, lab = case(shape, "ties")
    B, H, W, C = shape
    assert (np.sort(lg, axis=-1)[..., -1] == np.sort(lg, axis=-1)[..., -2]).mean() > 0.2      # many tied maxima
    run = DiceRun(lg, lab)
    pred = np.argmax(lg, axis=-1)
    eps = float(np.float32(1e-10))
    for sol in (False, True):
        for sob in (False, True):
            axes = ((0,) if sob else ()) + (1, 2) + ((3,) if sol else ())
            p1, y1 = R.one_hot(pred, C, np.int64), R.one_hot(lab, C, np.int64)
            i, l, r = (p1 * y1).sum(axis=axes), p1.sum(axis=axes), y1.sum(axis=axes)
            want = (2.0 * i / ((l + r).astype(np.float64) + eps)).astype(np.float32)
            table, _, _ = run.finish(sol, sob, hard=True)
            assert np.array_equal(table, want), (sol, sob, table, want)


@pytest.mark.parametrize("shape,kind", CASES)
def test_cross_entropy_family(shape, kind):
    lg, lab = case(shape, kind)
    C = shape[3]
    rng = np.random.default_rng(6)
    pre = rng.normal(0.0, 1e-4, size=shape).astype(np.float32)
    cw = [0.3 + 0.7 * c for c in range(C)]
    for name, kw in (("softmax", dict()), ("sigmoid", dict(use_sigmoid=True)), ("weighted", dict(class_weights=cw))):
        tag = "%s %s xent %s" % (shape, kind, name)
        l64, g64 = R.cross_entropy_loss(lg, lab, **kw)
        l32, g32 = R.cross_entropy_loss(lg, lab, dtype=np.float32, **kw)
        loss, d = xent_device(lg, lab, **kw)
        check(tag + " value", loss, l64, l32)
        check(tag + " gradient (written)", d, g64, g32)
        sc = np.float32(1.5)
        loss2, d2 = xent_device(lg, lab, grad_scale=float(sc), prefill=pre, **kw)
        assert loss2 == loss
        check(tag + " gradient (added, scale 1.5)", d2, pre.astype(np.float64) + float(sc) * g64, pre + sc * g32)
        loss3, none = xent_device(lg, lab, with_grad=False, **kw)
        assert loss3 == loss and none is None


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_nn_resize_adjoint(shift):
    import torch
    L = _lib()
    B, H, W, C = 2, 16, 16, 3
    h, w = H >> shift, W >> shift
    rng = np.random.default_rng(40 + shift)
    fine = rng.normal(size=(B, H, W, C)).astype(np.float32)
    pre = rng.normal(size=(B, h, w, C)).astype(np.float32)
    r64, r32 = R.nn_resize_adjoint(fine, shift), R.nn_resize_adjoint(fine, shift, dtype=np.float32)
    dfine = _up(fine, np.float32)
    out = torch.full((B, h, w, C), np.nan, dtype=torch.float32, device=dfine.device)
    L.nn_resize_adjoint(dfine.data_ptr(), out.data_ptr(), B, h, w, C, shift, 0, _stream())
    acc = _up(pre, np.float32)
    L.nn_resize_adjoint(dfine.data_ptr(), acc.data_ptr(), B, h, w, C, shift, 1, _stream())
    _sync()
    check("resize adjoint shift %d (written)" % shift, out.cpu().numpy(), r64, r32)
    check("resize adjoint shift %d (added)" % shift, acc.cpu().numpy(), pre.astype(np.float64) + r64, pre + r32)


def test_two_calls_are_bit_identical(monkeypatch):
    monkeypatch.delenv("PHX_DETERMINISTIC", raising=False)
    shape = (2, 64, 64, 4)
    lg, lab = case(shape)
    outs = []
    for _ in range(2):
        run = DiceRun(lg, lab)
        table, loss, coef = run.finish(False, False)
        hard, _, _ = run.finish(False, True, hard=True)
        g = run.grad(coef, 1.0)
        xl, xg = xent_device(lg, lab, class_weights=[1.0, 2.0, 0.5, 3.0])
        sl, sg = xent_device(lg, lab, use_sigmoid=True)
        outs.append([table, np.float32(loss), coef.cpu().numpy(), hard, g, np.float32(xl), xg, np.float32(sl), sg])
    for a, b in zip(*outs):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_argument_checks_launch_nothing():
    import torch
    L = _lib()
    dll = L._dll                                  # the raw entry points: the status code instead of an exception
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    lab = torch.zeros(1 << 12, dtype=torch.uint8, device=dev)
    out = torch.full((64,), 7.0, dtype=torch.float32, device=dev)
    p, q, o, st = buf.data_ptr(), lab.data_ptr(), out.data_ptr(), _stream()
    big = 1 << 18
    for C in (1, 9):
        assert L.dice_ws_bytes(2, 8, 8, C) == 0 and L.seg_xent_ws_bytes(2, 8, 8, C) == 0
        assert dll.phx_dice_sums(p, q, p, big, 2, 8, 8, C, st) == E_INVAL
        assert dll.phx_dice_finish(p, big, 2, 8, 8, C, 0, 0, 0, 0, 1e-10, 0.5, o, o + 128, None, st) == E_INVAL
        assert dll.phx_dice_grad(p, q, p, 1.0, 0, o, 2, 8, 8, C, st) == E_INVAL
        assert dll.phx_seg_xent(p, q, None, 0, 0.5, 1.0, 0, o, None, p, big, 2, 8, 8, C, st) == E_INVAL
    need = int(L.dice_ws_bytes(2, 8, 8, 3))
    assert need > 0
    assert dll.phx_dice_sums(p, q, p, need - 1, 2, 8, 8, 3, st) == E_INVAL                 # workspace too small
    assert dll.phx_dice_finish(p, need - 1, 2, 8, 8, 3, 0, 0, 0, 0, 1e-10, 0.5, o, None, None, st) == E_INVAL
    assert dll.phx_seg_xent(p, q, None, 0, 0.5, 1.0, 0, o, None, p, int(L.seg_xent_ws_bytes(2, 8, 8, 3)) - 1, 2, 8, 8, 3, st) == E_INVAL
    assert dll.phx_dice_finish(p, need, 2, 8, 8, 3, 0, 1, 0, 1, 1e-10, 0.5, o, None, None, st) == E_INVAL   # only_foreground without a label axis
    assert dll.phx_seg_xent(p, q, p, 1, 0.5, 1.0, 0, o, None, p, big, 2, 8, 8, 3, st) == E_INVAL           # class weights with the sigmoid form
    assert dll.phx_nn_resize_adjoint(p, o, 1, 2, 2, 3, 5, 0, st) == E_INVAL
    _sync()
    assert (out.cpu().numpy() == 7.0).all()       # nothing was launched
    with pytest.raises(Exception, match="workspace too small"):
        L.dice_sums(p, q, p, need - 1, 2, 8, 8, 3, st)
