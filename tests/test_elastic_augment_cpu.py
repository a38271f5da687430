"""do_elasticaug on the CPU side: the restatement's identities (tests/elastic_ref.py restates OpenCV's published cubic resize and
fixed-point remap; cv2 is not installed, so parity with it is not pinned), the decisions the provider draws, and the C ABI."""
import numpy as np
import pytest

from tests import elastic_ref as er
from tests.test_augment import _data


@pytest.mark.parametrize("X", [24, 32, 128])
def test_restatement_identities(X):
    img, lab = _data(1, X, 3, 1, X)
    img, lab = img[0], lab[0, ..., 0]
    zero = np.zeros(9)
    out, lbl = er.elastic_warp(img, lab, zero, zero, 3)
    np.testing.assert_array_equal(out, img)                                     # zero field: the identity, bit for bit
    np.testing.assert_array_equal(lbl, lab)
    # a constant control matrix resizes to the constant exactly (the four cubic coefficients sum to 1 by construction) ...
    np.testing.assert_array_equal(er.resize_cubic64(np.full((3, 3), 3.0), X, X), np.full((X, X), 3.0))
    # ... so (dx, dy) = (3, -2) is the reflect-shifted pixel permutation out(y, x) = in(reflect(y - 2), reflect(x + 3))
    stats = {}
    out, lbl = er.elastic_warp(img, lab, np.full(9, 3.0), np.full(9, -2.0), 3, stats)
    yy, xx = er.border_reflect(np.arange(X) - 2, X), er.border_reflect(np.arange(X) + 3, X)
    np.testing.assert_array_equal(out, img[yy][:, xx])
    np.testing.assert_array_equal(lbl, lab[yy][:, xx])
    assert stats["reflected"] > 0


def test_border_reflect_repeats_until_in_range():
    np.testing.assert_array_equal(er.border_reflect([-1, -4, -5, -9, 4, 7, 8, 11, 12], 4), [0, 3, 3, 0, 3, 0, 0, 3, 3])
    np.testing.assert_array_equal(er.border_reflect([-3, 5], 1), [0, 0])


def test_non_square_convention():
    """dx displaces along the column index (axis 1), dy along the row index (axis 0), also where the two extents differ."""
    rng = np.random.default_rng(3)
    img = rng.random((40, 24), dtype=np.float32)
    lab = (rng.random((40, 24)) > 0.5).astype(np.uint8)
    out, lbl = er.elastic_warp(img, lab, np.full(9, 5.0), np.full(9, 1.0), 2)
    yy, xx = er.border_reflect(np.arange(40) + 1, 40), er.border_reflect(np.arange(24) + 5, 24)
    np.testing.assert_array_equal(out, img[yy][:, xx])
    np.testing.assert_array_equal(lbl, lab[yy][:, xx])


def test_draw_decisions_elastic():
    from phiseg_code_amd.data import augment as pa
    base = dict(do_rotations=True, do_scaleaug=True, do_fliplr=True, do_flipud=True, nlabels=2)
    vals, n_aug = [], 0
    for j in range(400):
        d0 = pa.draw_decisions(1234, 3, j, 128, 128, base, 4)
        d1 = pa.draw_decisions(1234, 3, j, 128, 128, dict(base, do_elasticaug=True), 4)
        assert d0["elastic"] is None
        assert (d1["elastic"] is not None) == d1["augment"]
        for k in d1:
            if k != "elastic":
                assert d0[k] == d1[k], (j, k)                                   # every other decision: unchanged by the option
        if d1["augment"]:
            n_aug += 1
            dx, dy = d1["elastic"]
            assert dx.shape == (9,) and dy.shape == (9,) and dx.dtype == np.float64 and dy.dtype == np.float64
            vals += [dx, dy]
    assert 140 < n_aug < 260
    vals = np.concatenate(vals)                                                 # ~3600 values of N(0, 10): bounds ~4 standard errors
    assert abs(vals.mean()) < 0.7 and 9.5 < vals.std() < 10.5
    # the control array of pack_params: [B, 2, 3, 3], dx then dy, and the flag bit
    dec = [pa.draw_decisions(1234, 3, j, 128, 128, dict(base, do_elasticaug=True), 4) for j in range(8)]
    ctrl = np.zeros((8, 2, 3, 3))
    rec = pa.pack_params(dec, list(range(8)), [0] * 8, 128, 128, ctrl)
    for j, d in enumerate(dec):
        assert bool(rec["flags"][j] & pa.ELASTIC) == d["augment"]
        if d["augment"]:
            np.testing.assert_array_equal(ctrl[j].reshape(2, 9), np.stack(d["elastic"]))
        else:
            assert not ctrl[j].any()


def test_header_declares_the_elastic_entries():
    from phiseg_code_amd import runtime as rt
    protos = rt.parse_header()
    assert len(protos["phx_augment_batch_elastic"]) == 14
    assert len(protos["phx_augment_batch_elastic_ws_bytes"]) == 3
    assert len(protos["phx_augment_batch"]) == 11                               # the existing entry: unchanged
