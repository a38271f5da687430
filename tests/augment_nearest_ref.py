"""Numpy restatement of the reference's `nlabels > 4` augmentation branch (data/batch_provider.py:204-208, 221-224, 245-248): the image
goes through the linear path (oracle/augment.py, tests/elastic_ref.py), the label map is resampled with cv2.INTER_NEAREST.  Test
infrastructure only; it lives beside the tests because oracle/ is frozen.

OpenCV is NOT installed here.  The three rules below restate OpenCV's published algorithms -- believed, not executable here, the same
standing as oracle/augment.py has for the linear path:
    cv2.warpAffine(..., INTER_NEAREST)        the fixed-point grid of oracle.augment.warp_grid with round_delta = AB_SCALE / 2: source
                                              pixel (X0 + adelta[x]) >> AB_BITS, BORDER_CONSTANT 0 outside
    cv2.resize(crop, INTER_NEAREST)           sx = min(floor(dx * (src / dst)), src - 1) per axis in double; no half-pixel centre
    cv2.remap(INTER_NEAREST, BORDER_REFLECT)  on the float32 maps of deformation_to_transformation (do_optimisation=False: no convertMaps):
                                              cvRound (half to even) of each map value, reflect-including-edge border
All label arithmetic is integer: a device result must be array_equal."""
import numpy as np

from oracle import augment as oa
from tests import elastic_ref as er


def warp_affine_nearest(lbl, M):
    """cv2.warpAffine(lbl, M, (cols, rows), flags=INTER_NEAREST), BORDER_CONSTANT 0"""
    rows, cols = lbl.shape
    iM = oa.invert_affine(M)
    x, y = np.arange(cols), np.arange(rows)
    adelta = oa._cv_round(iM[0, 0] * x * oa.AB_SCALE)
    bdelta = oa._cv_round(iM[1, 0] * x * oa.AB_SCALE)
    rd = oa.AB_SCALE // 2
    X0 = oa._cv_round((iM[0, 1] * y + iM[0, 2]) * oa.AB_SCALE) + rd
    Y0 = oa._cv_round((iM[1, 1] * y + iM[1, 2]) * oa.AB_SCALE) + rd
    sx = (X0[:, None] + adelta[None, :]) >> oa.AB_BITS
    sy = (Y0[:, None] + bdelta[None, :]) >> oa.AB_BITS
    ok = (sx >= 0) & (sx < cols) & (sy >= 0) & (sy < rows)
    return np.where(ok, lbl[np.clip(sy, 0, rows - 1), np.clip(sx, 0, cols - 1)], 0).astype(lbl.dtype)


def resize_nearest(lbl, out_rows, out_cols):
    """cv2.resize(lbl, (out_cols, out_rows), interpolation=INTER_NEAREST)"""
    rows, cols = lbl.shape
    sy = np.minimum(np.floor(np.arange(out_rows) * (rows / float(out_rows))).astype(np.int64), rows - 1)
    sx = np.minimum(np.floor(np.arange(out_cols) * (cols / float(out_cols))).astype(np.int64), cols - 1)
    return lbl[sy][:, sx]


def remap_nearest_reflect(lbl, map_x, map_y):
    """cv2.remap(lbl, map_x, map_y, INTER_NEAREST, borderMode=BORDER_REFLECT) on float32 maps"""
    rows, cols = lbl.shape
    sx = er.border_reflect(np.rint(np.asarray(map_x, dtype=np.float32)).astype(np.int64), cols)
    sy = er.border_reflect(np.rint(np.asarray(map_y, dtype=np.float32)).astype(np.int64), rows)
    return lbl[sy, sx]


def augment_labels_nearest(lbl, d):
    """the label map through rotate, crop-scale, elastic, flips with the decisions d of phiseg_code_amd.data.augment.draw_decisions"""
    lbl = np.asarray(lbl, dtype=np.uint8)
    n_x, n_y = lbl.shape
    if d["augment"]:
        if d.get("angle") is not None:
            lbl = warp_affine_nearest(lbl, oa.rotation_matrix(n_y, n_x, d["angle"]))
        if d.get("r_y") is not None:
            r, px, py = d["r_y"], d["p_x"], d["p_y"]
            lbl = resize_nearest(lbl[py:py + r, px:px + r], n_x, n_y)
        if d.get("elastic") is not None:
            map_x, map_y = er.deformation_maps(d["elastic"][0], d["elastic"][1], n_x, n_y)
            lbl = remap_nearest_reflect(lbl, map_x, map_y)
    if d.get("fliplr"):
        lbl = np.fliplr(lbl)
    if d.get("flipud"):
        lbl = np.flipud(lbl)
    return np.ascontiguousarray(lbl)


def augment_pair_nearest(img, lbl, d):
    """(image [X, Y] float32, label map [X, Y] uint8) -> the image by the linear path, the labels by the nearest-neighbour chain"""
    two = np.zeros(np.shape(lbl), dtype=np.uint8)                  # the image path does not depend on the labels
    ref_x, _ = er.augment_pair_elastic(img, two, d, 2)
    return ref_x, augment_labels_nearest(lbl, d)
