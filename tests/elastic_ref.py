"""Numpy restatement of the reference's random elastic deformation (test infrastructure only; it lives beside the tests because
oracle/ is frozen).

Restates data/batch_provider.py:226-248 (`do_elasticaug`) on the image helpers utils.py:40-67:

    dx_img, dy_img          = cv2.resize(3 x 3 control points, (n_y, n_x), INTER_CUBIC)              (CV_64F)
    dense_image_warp        = cv2.remap(im, *cv2.convertMaps(x + dx_img, y + dy_img, CV_16SC2), INTER_LINEAR, BORDER_REFLECT)
    dense_image_warp_as_onehot = argmax over labels of dense_image_warp(one-hot float64 planes)

OpenCV is NOT installed here: `resize_cubic64` and `remap_linear_reflect` restate OpenCV's published algorithms operation by
operation -- the generic cubic resize (float32 coefficients, A = -0.75, unclamped position, replicated taps, horizontal then
vertical pass, double products added in tap order) and the fixed-point bilinear remap (coordinates rounded half-to-even to 1/32
pixel, float32 table weights, every tap through borderInterpolate(BORDER_REFLECT)).  A restatement, not a parity claim pinned
against cv2 -- the same standing as oracle/augment.py."""
import numpy as np

from oracle import augment as oa

INTER_TAB = 32


def _cubic_coeffs(src, dst):
    """-> (s [dst] int64: floor of the source position, c [dst, 4] float32) of cv2.resize INTER_CUBIC along one axis."""
    d = np.arange(dst)
    f = ((d + 0.5) * (float(src) / dst) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    A, one = np.float32(-0.75), np.float32(1)
    g, h = f + one, one - f
    c = np.empty((dst, 4), dtype=np.float32)
    c[:, 0] = ((A * g - np.float32(5) * A) * g + np.float32(8) * A) * g - np.float32(4) * A
    c[:, 1] = ((A + np.float32(2)) * f - (A + np.float32(3))) * f * f + one
    c[:, 2] = ((A + np.float32(2)) * h - (A + np.float32(3))) * h * h + one
    c[:, 3] = one - c[:, 0] - c[:, 1] - c[:, 2]
    assert c.dtype == np.float32
    return s, c


def resize_cubic64(mat, out_rows, out_cols):
    """cv2.resize(mat, (out_cols, out_rows), interpolation=INTER_CUBIC) of a float64 matrix."""
    mat = np.asarray(mat, dtype=np.float64)
    rows, cols = mat.shape
    sx, cx = _cubic_coeffs(cols, out_cols)
    sy, cy = _cubic_coeffs(rows, out_rows)
    h = np.zeros((rows, out_cols), dtype=np.float64)
    for k in range(4):                                                          # horizontal pass, taps s - 1 .. s + 2 in order
        p = mat[:, np.clip(sx - 1 + k, 0, cols - 1)] * cx[:, k].astype(np.float64)[None, :]
        h = p if k == 0 else h + p
    out = np.zeros((out_rows, out_cols), dtype=np.float64)
    for k in range(4):                                                          # vertical pass
        p = h[np.clip(sy - 1 + k, 0, rows - 1), :] * cy[:, k].astype(np.float64)[:, None]
        out = p if k == 0 else out + p
    return out


def border_reflect(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT) on an integer array: p < 0 -> -p - 1, p >= n -> 2 n - p - 1, until in range."""
    p = np.array(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p = np.where(lo, -p - 1, np.where(hi, 2 * n - p - 1, p))


def fixed_point_maps(map_x, map_y):
    """cv2.convertMaps(map_x, map_y, CV_16SC2): cvRound(map * 32) in float -> integer source (x, y) and the 1/32-pixel fractions."""
    ix = np.rint(np.asarray(map_x, dtype=np.float32) * np.float32(INTER_TAB)).astype(np.int64)
    iy = np.rint(np.asarray(map_y, dtype=np.float32) * np.float32(INTER_TAB)).astype(np.int64)
    return ix >> 5, iy >> 5, ix & (INTER_TAB - 1), iy & (INTER_TAB - 1)


def remap_linear_reflect(img, map_x, map_y, work=np.float32, stats=None):
    """cv2.remap(img, *convertMaps(map_x, map_y), INTER_LINEAR, borderMode=BORDER_REFLECT).  img [rows, cols] (work=float32) or
    [rows, cols, C] float64 planes (work=float64); the table weights are float32.  stats (a dict) receives `reflected`, the share
    of pixels with at least one border-reflected tap."""
    rows, cols = img.shape[:2]
    sx, sy, fx, fy = fixed_point_maps(map_x, map_y)
    tab = np.arange(INTER_TAB, dtype=np.float32) * np.float32(1.0 / INTER_TAB)
    wx1, wy1 = tab[fx], tab[fy]
    wx0, wy0 = np.float32(1) - wx1, np.float32(1) - wy1
    w = [wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1]
    x0, x1, y0, y1 = border_reflect(sx, cols), border_reflect(sx + 1, cols), border_reflect(sy, rows), border_reflect(sy + 1, rows)
    if stats is not None:
        stats["reflected"] = float(np.mean((x0 != sx) | (x1 != sx + 1) | (y0 != sy) | (y1 != sy + 1)))
    src = np.asarray(img).astype(work)
    ex = (lambda t: t) if src.ndim == 2 else (lambda t: t[..., None])
    out = src[y0, x0] * ex(w[0]).astype(work)
    out = out + src[y0, x1] * ex(w[1]).astype(work)
    out = out + src[y1, x0] * ex(w[2]).astype(work)
    out = out + src[y1, x1] * ex(w[3]).astype(work)
    return out.astype(work)


def deformation_maps(dx_ctrl, dy_ctrl, n_x, n_y):
    """utils.deformation_to_transformation on the resized control points: map_x = column + dx_img, map_y = row + dy_img (float32)."""
    dx_img = resize_cubic64(np.reshape(dx_ctrl, (3, 3)), n_x, n_y)
    dy_img = resize_cubic64(np.reshape(dy_ctrl, (3, 3)), n_x, n_y)
    grid_y, grid_x = np.meshgrid(np.arange(n_x), np.arange(n_y), indexing="ij")
    return (grid_x + dx_img).astype(np.float32), (grid_y + dy_img).astype(np.float32)


def elastic_warp(img, lbl, dx_ctrl, dy_ctrl, nlabels, stats=None):
    """batch_provider.py:226-248 for nlabels <= 4 with explicit control points (already multiplied by sigma)."""
    img = np.asarray(img, dtype=np.float32)
    n_x, n_y = img.shape
    map_x, map_y = deformation_maps(dx_ctrl, dy_ctrl, n_x, n_y)
    out = remap_linear_reflect(img, map_x, map_y, np.float32, stats)
    planes = remap_linear_reflect(oa.onehot(np.asarray(lbl, dtype=np.uint8), nlabels), map_x, map_y, np.float64)
    return out, np.argmax(planes, axis=-1).astype(np.uint8)


def augment_pair_elastic(img, lbl, d, nlabels, stats=None):
    """oracle.augment.augment_pair with the elastic deformation d['elastic'] = (dx[9], dy[9]) or None between crop-scale and the
    flips (batch_provider.py:186-262)."""
    img, lbl = oa.augment_pair(img, lbl, dict(d, fliplr=False, flipud=False), nlabels)
    if d["augment"] and d.get("elastic") is not None:
        img, lbl = elastic_warp(img, lbl, d["elastic"][0], d["elastic"][1], nlabels, stats)
    if d.get("fliplr"):
        img, lbl = np.fliplr(img), np.fliplr(lbl)
    if d.get("flipud"):
        img, lbl = np.flipud(img), np.flipud(lbl)
    return np.ascontiguousarray(img), np.ascontiguousarray(lbl)
