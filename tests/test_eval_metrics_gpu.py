"""phx_eval_metrics on the MI355X (csrc/eval_metrics.hip): GED / NCC / Dice read from [I * N, P, C] samples and [I, P, M] annotations
against the reference's own outputs (tests/golden/metrics_cases.npz) and the CPU oracle, with the tolerances of test_metrics_gpu.py:
integer counts make GED and Dice exact up to the final float32 store (2e-7); float32 logs with double sums give 1e-5 on a correlation
coefficient."""
import functools
import os

import numpy as np
import pytest

from oracle import metrics as om
from tests.helpers import METRICS_CASES, metrics_case

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "metrics_cases.npz"), allow_pickle=True)

# (seed, N, M, X, Y, C, mode)
EDGE_CASES = [(31, 1, 1, 10, 10, 2, "plain"),        # one sample, one annotator, P = 100
              (32, 7, 8, 13, 5, 3, "plain"),         # P = 65, M at its limit, N below the wave count
              (33, 9, 2, 8, 8, 8, "plain"),          # C at its limit, P = 64 exactly
              (34, 65, 4, 16, 12, 2, "plain"),       # N one past a multiple of 64
              (35, 17, 3, 24, 24, 4, "empty_fg"),    # empty foreground
              (36, 3, 4, 9, 7, 2, "plain")]          # P < 64


@functools.lru_cache(maxsize=None)
def case_and_oracle(case):
    """-> (sm [N, X, Y, C], gts [M, X, Y], annotator of the Dice reference, oracle GED, NCC, Dice); computed once per case"""
    seed, N, M, X, Y, C, mode = case
    sm, gts = metrics_case(*case)
    a = seed % M
    ged, ncc, _ = om.validation_metrics(sm, gts, gts[a], C)
    dice = om.per_label_dice(sm.astype(np.float64).mean(axis=0).argmax(axis=-1), gts[a], C)
    for arr in (sm, gts):
        arr.setflags(write=False)
    return sm, gts, a, ged, ncc, np.asarray(dice)


def device_scores(sms, gtss, annots, C, label0=1, with_sref=True, ws_delta=0, fill=None):
    """sms: list of [N, X, Y, C], gtss: list of [M, X, Y], annots: list of int -> out [I, 10] float32 of ONE phx_eval_metrics call
    (annotations re-laid to [P, M], as a provider keeps them)"""
    import torch
    from phiseg_code_amd import runtime as rt
    L = rt.lib()
    I = len(sms)
    N, X, Y = sms[0].shape[:3]
    M, P = gtss[0].shape[0], X * Y
    dev = torch.device("cuda", torch.cuda.current_device())
    sm = torch.as_tensor(np.ascontiguousarray(np.concatenate(sms).reshape(I * N, P, -1), dtype=np.float32)).to(dev)
    lab = torch.as_tensor(np.ascontiguousarray(np.stack([g.reshape(M, P).T for g in gtss]), dtype=np.uint8)).to(dev)
    assert tuple(lab.shape) == (I, P, M)
    sr = torch.as_tensor(np.asarray(annots, dtype=np.uint8)).to(dev)
    wsb = int(L.eval_metrics_ws_bytes(I, N, M, P, C))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(I, 10, dtype=torch.float32, device=dev)
    if fill is not None:
        out.fill_(fill)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    try:
        L.eval_metrics(sm.data_ptr(), lab.data_ptr(), sr.data_ptr() if with_sref else None, ws.data_ptr(), wsb + ws_delta, I, N, M, P, C,
                       label0, out.data_ptr(), st)
    finally:
        torch.cuda.synchronize()
        device_scores.last_out = out.cpu().numpy()
    return device_scores.last_out


def check_against_oracle(case, row):
    seed, N, M, X, Y, C, mode = case
    _, _, _, ged, ncc, dice = case_and_oracle(case)
    print(case, "GED %.9f (oracle %.9f)  NCC %.9f (oracle %.9f)  Dice %s (oracle %s)" % (row[0], ged, row[1], ncc, row[2:2 + C], dice))
    assert np.isfinite(row).all() and np.isfinite([ged, ncc]).all()
    np.testing.assert_allclose(row[0], ged, rtol=0, atol=2e-7)
    np.testing.assert_allclose(row[1], ncc, rtol=0, atol=1e-5)
    np.testing.assert_allclose(row[2:2 + C], dice, rtol=0, atol=2e-7)
    assert (row[2 + C:] == 0).all()


@pytest.mark.parametrize("k", range(len(METRICS_CASES)))
def test_fixture_cases_match_reference_and_oracle(k):
    case = METRICS_CASES[k]
    sm, gts, a, _, _, _ = case_and_oracle(case)
    row = device_scores([sm], [gts], [a], case[5])[0]
    np.testing.assert_allclose(row[0], float(GOLD["ged_%d" % k]), rtol=0, atol=2e-7)
    np.testing.assert_allclose(row[1], float(GOLD["ncc_%d" % k]), rtol=0, atol=1e-5)
    check_against_oracle(case, row)


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: "seed%d" % c[0])
def test_edge_shapes_match_oracle(case):
    sm, gts, a, _, _, _ = case_and_oracle(case)
    check_against_oracle(case, device_scores([sm], [gts], [a], case[5])[0])


def test_batch_of_images_equals_single_image_calls_bit_for_bit():
    """Three different images in one call: more than one block per image (P = 260, not a multiple of 64), a different Dice
    annotator each; the planes, moment partials and pair distances of an image must not see its neighbours."""
    cases = [(41, 9, 3, 20, 13, 3, "plain"), (42, 9, 3, 20, 13, 3, "empty_fg"), (43, 9, 3, 20, 13, 3, "plain")]
    data = [case_and_oracle(c) for c in cases]
    batch = device_scores([d[0] for d in data], [d[1] for d in data], [d[2] for d in data], 3)
    assert len({d[2] for d in data}) == 3
    for i, (c, d) in enumerate(zip(cases, data)):
        single = device_scores([d[0]], [d[1]], [d[2]], 3)
        assert batch[i].tobytes() == single[0].tobytes(), (i, batch[i], single[0])
        check_against_oracle(c, batch[i])


def test_two_calls_give_identical_bytes():
    case = (37, 16, 4, 64, 64, 2, "plain")
    sm, gts, a, _, _, _ = case_and_oracle(case)
    first = device_scores([sm], [gts], [a], 2, fill=1.0)
    second = device_scores([sm], [gts], [a], 2, fill=-7.0)        # (every slot of the row is written: the pre-fill does not show)
    assert first.tobytes() == second.tobytes()
    check_against_oracle(case, first[0])


def test_null_sref_scores_ged_and_ncc_and_zeroes_the_dice_slots():
    case = METRICS_CASES[1]
    sm, gts, a, _, _, _ = case_and_oracle(case)
    with_ref = device_scores([sm], [gts], [a], case[5])[0]
    without = device_scores([sm], [gts], [a], case[5], with_sref=False, fill=3.0)[0]
    assert with_ref[:2].tobytes() == without[:2].tobytes()
    assert (without[2:] == 0).all() and (with_ref[2:2 + case[5]] > 0).any()


@pytest.mark.parametrize("what, code", [("C9", -2), ("M9", -2), ("short_ws", -1)])
def test_bad_arguments_raise_and_launch_nothing(what, code):
    from phiseg_code_amd import runtime as rt
    N, X, Y = 3, 8, 8
    C = 9 if what == "C9" else 2
    M = 9 if what == "M9" else 2
    sm = np.full((N, X, Y, C), 1.0 / C, np.float32)
    gts = np.zeros((M, X, Y), np.uint8)
    with pytest.raises(rt.PhxError, match=r"phx_eval_metrics failed \(%d\)" % code):
        device_scores([sm], [gts], [0], C, ws_delta=-1 if what == "short_ws" else 0, fill=5.0)
    assert (device_scores.last_out == 5.0).all()                   # the output is as it was: no kernel ran
