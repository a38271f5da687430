"""The nearest-neighbour label restatement (tests/augment_nearest_ref.py) against its own invariants, and the provider's switch."""
import numpy as np
import pytest

from oracle import augment as oa
from phiseg_code_amd import many_class
from tests import augment_nearest_ref as nr


def _labels(X, Y, C, seed):
    return np.random.default_rng(seed).integers(0, C, (X, Y)).astype(np.uint8)


@pytest.mark.parametrize("X,Y,C", [(32, 32, 5), (48, 40, 19), (17, 23, 256)])
def test_identity_stages_reproduce_the_input(X, Y, C):
    lbl = _labels(X, Y, C, X + C)
    assert np.array_equal(nr.warp_affine_nearest(lbl, oa.rotation_matrix(Y, X, 0.0)), lbl)               # angle 0
    assert np.array_equal(nr.resize_nearest(lbl, X, Y), lbl)                                           # full-size crop
    gy, gx = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    assert np.array_equal(nr.remap_nearest_reflect(lbl, gx.astype(np.float32), gy.astype(np.float32)), lbl)
    zero = np.zeros(9)
    d = dict(augment=True, angle=0.0, r_y=None, p_x=None, p_y=None, elastic=(zero, zero), fliplr=False, flipud=False)
    assert np.array_equal(nr.augment_labels_nearest(lbl, d), lbl)                                      # a zero deformation field
    if X == Y:
        assert np.array_equal(nr.augment_labels_nearest(lbl, dict(d, r_y=X, p_x=0, p_y=0)), lbl)


def test_ninety_degrees_is_rot90_away_from_the_shifted_border():
    """the centre of rotation is (cols / 2, rows / 2), half a pixel off the pixel grid's centre: the fixed-point grid shifts one border
    row out (label 0 comes in), everything else is np.rot90 -- as oracle/augment.py's linear path shows for images"""
    lbl = _labels(32, 32, 19, 3) + 1                              # no label 0: the border fill is recognisable
    r = nr.warp_affine_nearest(lbl.astype(np.uint8), oa.rotation_matrix(32, 32, 90.0))
    assert np.array_equal(r[1:, :], np.rot90(lbl)[:-1, :])
    assert (r[0, :] == 0).all()


def test_crop_scale_and_reflection_rules():
    lbl = _labels(32, 32, 7, 5)
    up = nr.resize_nearest(lbl[4:20, 6:22], 32, 32)               # 16 -> 32: every source pixel twice, no half-pixel centre
    assert np.array_equal(up, lbl[4:20, 6:22].repeat(2, axis=0).repeat(2, axis=1))
    down = nr.resize_nearest(lbl, 16, 16)
    assert np.array_equal(down, lbl[::2, ::2])
    gy, gx = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    out = nr.remap_nearest_reflect(lbl, (gx - 3).astype(np.float32), gy.astype(np.float32))
    assert np.array_equal(out[:, 3:], lbl[:, :-3]) and np.array_equal(out[:, :3], lbl[:, 2::-1])     # reflect, edge included
    half = nr.remap_nearest_reflect(lbl, (gx + 0.5).astype(np.float32), gy.astype(np.float32))         # cvRound: half to even
    assert np.array_equal(half[:, 0], lbl[:, 0]) and np.array_equal(half[:, 1], lbl[:, 2])


def test_label_route_switches_at_five():
    assert [many_class.label_route(n) for n in (2, 3, 4)] == ["onehot"] * 3
    assert [many_class.label_route(n) for n in (5, 9, 19, 256)] == ["nearest"] * 4
    for n in (1, 257):
        with pytest.raises(ValueError):
            many_class.label_route(n)
