"""The launches of the many-class kernel tests (csrc/many_class.hip): each function runs one case on the GPU, checks it against the float64
yardstick of tests/many_class_ref.py and returns the raw bytes of everything the kernels wrote, so that a caller can compare bits --
tests/test_many_class_kernels_gpu.py between two calls, tests/many_class_worker.py between a PHX_DETERMINISTIC=1 process and this one.

Bounds (rel-to-max, as tests/test_kernels_gpu.close): those test_residual_ce holds the template kernel to -- losses 2e-5, s_out and
soft-max 1e-5, gradients 3e-5; metrics: those of tests/test_eval_metrics_gpu.py -- GED and Dice 2e-7 (integer counts, exact up to the
float32 store), NCC 1e-5."""
import numpy as np
import torch

from phiseg_code_amd import runtime as rt
from tests import many_class_ref as R

TAIL = 64                                    # sentinels behind every output
NAN = float("nan")


def S():
    return torch.cuda.current_stream().cuda_stream


def out_buf(n):
    return torch.full((n + TAIL,), NAN, dtype=torch.float32, device="cuda")


def tail_kept(t, n, what):
    assert bool(torch.isnan(t[n:]).all()), "%s: the kernel wrote past the end of its output" % what


def close(got, ref, rel, what):
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), "%s: NaN or Inf left in the output" % what
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
    print("MANY %s err=%.3e bound=%.1e" % (what, err, rel))
    assert err <= rel, "%s: rel-to-max err %.3e > %.1e" % (what, err, rel)


def residual_ce_launch(L, C, H, W, shifts, ds_mask, with_labels=True, want_sm=True):
    """One phx_residual_ce_wide call on fresh NaN-filled buffers -> dict(losses, s_out, sm, ds: list (None where not handed over)) of
    host float32 arrays; the sentinels behind every output are checked."""
    s, lab, _ = R.residual_ce_case(C, H, W, shifts)
    B, Ls = R.BATCH, len(shifts)
    sd = [torch.tensor(v).cuda() for v in s]
    labd = torch.tensor(lab).cuda()
    dsd = [out_buf(v.numel()) if m else None for v, m in zip(sd, ds_mask)]
    losses = out_buf(8) if with_labels else None
    s_out, sm = out_buf(B * H * W * C), (out_buf(B * H * W * C) if want_sm else None)
    wsb = int(L.residual_ce_wide_ws_bytes(B, H, W))
    assert wsb == B * ((H + 15) // 16) * ((W + 15) // 16) * 8 * 4
    work = torch.full((wsb // 4 + TAIL,), NAN, device="cuda") if with_labels else None
    L.residual_ce_wide(rt.ptr_array([v.data_ptr() for v in sd]), rt.ptr_array([d.data_ptr() if d is not None else None for d in dsd]),
                       rt.int_array(list(shifts)), Ls, labd.data_ptr() if with_labels else None, B, H, W, C, R.WEIGHT, 1.0 / B,
                       losses.data_ptr() if with_labels else None, s_out.data_ptr(), sm.data_ptr() if want_sm else None,
                       work.data_ptr() if with_labels else None, wsb if with_labels else 0, S())
    torch.cuda.synchronize()
    what = "residual_ce_wide C=%d %dx%d" % (C, H, W)
    tail_kept(s_out, B * H * W * C, what + " s_out")
    if want_sm:
        tail_kept(sm, B * H * W * C, what + " sm_out")
    if with_labels:
        assert bool(torch.isnan(losses[Ls:]).all()), what + ": losses beyond L were written"
        tail_kept(work, wsb // 4, what + " work")
    for d, v in zip(dsd, sd):
        if d is not None:
            tail_kept(d, v.numel(), what + " ds")
    return dict(losses=losses[:Ls].cpu().numpy() if with_labels else None, s_out=s_out[:B * H * W * C].cpu().numpy().reshape(B, H, W, C),
                sm=sm[:B * H * W * C].cpu().numpy().reshape(B, H, W, C) if want_sm else None,
                ds=[d[:v.numel()].cpu().numpy().reshape(tuple(v.shape)) if d is not None else None for d, v in zip(dsd, sd)])


def residual_ce_check(got, C, H, W, shifts, what):
    _, _, ref = R.residual_ce_case(C, H, W, shifts)
    if got["losses"] is not None:
        close(got["losses"], ref["losses"], 2e-5, what + " losses")
    close(got["s_out"], ref["s_out"], 1e-5, what + " s_out")
    if got["sm"] is not None:
        close(got["sm"], ref["sm"], 1e-5, what + " softmax")
    for l, d in enumerate(got["ds"]):
        if d is not None:
            close(d, ref["ds"][l], 3e-5, what + " ds[%d]" % l)


def residual_ce_bytes(got):
    parts = [got["losses"], got["s_out"], got["sm"]] + list(got["ds"])
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts if p is not None)


def residual_ce_full(L, C, H, W, shifts):
    """every ds handed over, labels, s_out and sm_out: checked against float64 -> bytes"""
    got = residual_ce_launch(L, C, H, W, shifts, [True] * len(shifts))
    residual_ce_check(got, C, H, W, shifts, "C=%d %dx%d full" % (C, H, W))
    return residual_ce_bytes(got)


def metrics_launch(L, C, layout, with_sref=True, ws_delta=0):
    """One phx_metrics_wide call over every image of the C-class case -> out [I, 2 + C] float32.
    layout "imp": labels [I][M][P] and the Dice reference a map (what utils._metrics_device passes); "ipm": labels [I][P][M] and the
    Dice reference an annotator index (what evaluate.evaluate_split passes)."""
    I = dict(R.METRIC_CASES)[C]
    cases = [R.metrics_case(C, i) for i in range(I)]
    N, M, P = R.MET_N, R.MET_M, R.MET_X * R.MET_Y
    sm = torch.as_tensor(np.ascontiguousarray(np.stack([c[0] for c in cases]).reshape(I * N, P, C))).cuda()
    g = np.stack([c[1].reshape(M, P) for c in cases])
    if layout == "imp":
        lab, strides = torch.as_tensor(np.ascontiguousarray(g)).cuda(), (P, 1)
        ref_map = torch.as_tensor(np.ascontiguousarray(np.stack([c[1][c[2]].reshape(P) for c in cases]))).cuda()
        sref = (ref_map.data_ptr() if with_sref else None, None)
    else:
        lab, strides = torch.as_tensor(np.ascontiguousarray(g.transpose(0, 2, 1))).cuda(), (1, M)
        ref_idx = torch.as_tensor(np.asarray([c[2] for c in cases], dtype=np.uint8)).cuda()
        sref = (None, ref_idx.data_ptr() if with_sref else None)
    wsb = int(L.metrics_wide_ws_bytes(I, N, M, P, C))
    ws = torch.empty(wsb + TAIL, dtype=torch.uint8, device="cuda")
    ws[wsb:] = 0xA5
    out = out_buf(I * (2 + C))
    L.metrics_wide(sm.data_ptr(), lab.data_ptr(), strides[0], strides[1], sref[0], sref[1], ws.data_ptr(), wsb + ws_delta, I, N, M, P, C, 1,
                   out.data_ptr(), S())
    torch.cuda.synchronize()
    tail_kept(out, I * (2 + C), "metrics_wide out")
    assert bool((ws[wsb:] == 0xA5).all()), "metrics_wide wrote past the end of its workspace"
    return out[:I * (2 + C)].cpu().numpy().reshape(I, 2 + C)


def metrics_check(out, C, with_sref=True):
    for i, row in enumerate(out):
        _, _, _, ged, ncc, dice = R.metrics_case(C, i)
        print("MANY metrics C=%d image %d GED %.9f (oracle %.9f) NCC %.9f (oracle %.9f)" % (C, i, row[0], ged, row[1], ncc))
        assert np.isfinite(row).all()
        np.testing.assert_allclose(row[0], ged, rtol=0, atol=2e-7)
        np.testing.assert_allclose(row[1], ncc, rtol=0, atol=1e-5)
        np.testing.assert_allclose(row[2:], dice if with_sref else np.zeros(C), rtol=0, atol=2e-7)


def metrics_full(L, C, layout):
    out = metrics_launch(L, C, layout)
    metrics_check(out, C)
    return np.ascontiguousarray(out).tobytes()
