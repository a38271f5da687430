"""phx_augment_batch_nearest on the MI355X (csrc/augment_nearest.hip): label maps with more than four labels through the provider, against
the numpy restatement of the reference's cv2.INTER_NEAREST branch (tests/augment_nearest_ref.py).  Labels are integer arithmetic on both
sides: array_equal.  Images take the linear path and match oracle/augment.py + tests/elastic_ref.py within the 1e-6 of
test_device_augmentation_matches_oracle."""
import numpy as np
import pytest

from tests import augment_nearest_ref as nr

pytestmark = pytest.mark.gpu


def _data(n, X, nlabels, annot, seed):
    """images ~ U(-0.5, 0.5); label maps of 3 x 2 pixel blocks cycling through every class, shifted per annotator"""
    rng = np.random.default_rng(seed)
    img = (rng.random((n, X, X), dtype=np.float32) - 0.5).astype(np.float32)
    y, x = np.mgrid[0:X, 0:X]
    lab = np.stack([np.stack([(x // 3 + 5 * (y // 2) + i + 2 * a) % nlabels for a in range(annot)], axis=-1) for i in range(n)]).astype(np.uint8)
    assert lab.min() == 0 and lab.max() == nlabels - 1
    return img, lab


def _check_batches(prov, img, lab, batches, batch_size, X):
    seen = set()
    for _ in range(batches):
        x, s = prov.next_batch(batch_size)
        assert x.shape == (batch_size, X, X, 1) and s.shape == (batch_size, X, X) and s.dtype == np.uint8
        for j, (d, src, an) in enumerate(zip(prov.last_decisions, prov.last_indices, prov.last_annotators)):
            ref_x, ref_s = nr.augment_pair_nearest(img[src], lab[src, ..., an], d)
            assert np.array_equal(s[j], ref_s), (j, d, int((s[j] != ref_s).sum()))
            np.testing.assert_allclose(x[j, ..., 0], ref_x, rtol=0, atol=1e-6, err_msg=str(d))
            seen.add((d["angle"] is not None, d["r_y"] is not None, d["elastic"] is not None, d["fliplr"], d["flipud"]))
    return seen


@pytest.mark.parametrize("X", [32, 48])
@pytest.mark.parametrize("nlabels", [5, 19])
def test_device_nearest_labels_match_restatement(X, nlabels):
    """the option set of test_device_augmentation_matches_oracle: rotation, crop-scale and both flips, every second image augmented"""
    from phiseg_code_amd.data import augment as pa
    img, lab = _data(6, X, nlabels, 4, X + nlabels)
    opts = dict(do_rotations=True, do_scaleaug=True, do_fliplr=True, do_flipud=True, nlabels=nlabels, augment_every_nth=2)
    prov = pa.DeviceBatchProvider(img, lab, do_augmentations=True, augmentation_options=opts, num_labels_per_subject=4,
                                  annotator_range=range(4), seed=99, nlabels=nlabels)
    seen = _check_batches(prov, img, lab, 6, 5, X)
    assert len(seen) >= 4                                            # augmented and untouched, flipped and not


@pytest.mark.parametrize("X,nlabels,resample", [(32, 5, True), (48, 19, True), (32, 19, False),
                                                (160, 5, True)])    # 160 x 160: two fp32 intermediates exceed LDS, the workspace form
def test_device_nearest_labels_elastic_match_restatement(X, nlabels, resample):
    """the elastic producer: the deformation after rotation and crop-scale (or alone), before the flips"""
    from phiseg_code_amd.data import augment as pa
    img, lab = _data(4, X, nlabels, 4, 3 * X + nlabels)
    opts = dict(do_rotations=resample, do_scaleaug=resample, do_elasticaug=True, do_fliplr=True, do_flipud=True, nlabels=nlabels,
                augment_every_nth=2)
    prov = pa.DeviceBatchProvider(img, lab, do_augmentations=True, augmentation_options=opts, num_labels_per_subject=4,
                                  annotator_range=range(4), seed=7, nlabels=nlabels)
    nbatch = 2 if X == 160 else 4
    seen = _check_batches(prov, img, lab, nbatch, 4, X)
    assert any(k[2] for k in seen) and any(not k[2] for k in seen)  # deformed and untouched samples


def test_provider_without_augmentation_hands_out_a_five_class_batch():
    from phiseg_code_amd.data import augment as pa
    img, lab = _data(8, 32, 5, 4, 1)
    prov = pa.DeviceBatchProvider(img, lab, do_augmentations=False, num_labels_per_subject=4, annotator_range=[0, 2], seed=1, nlabels=5)
    x, s = prov.next_batch(4)
    for j, (src, an) in enumerate(zip(prov.last_indices, prov.last_annotators)):
        assert np.array_equal(x[j, ..., 0], img[src]) and np.array_equal(s[j], lab[src, ..., an])


def test_refusals_launch_nothing():
    import torch
    from phiseg_code_amd import runtime as rt
    L = rt.lib()
    B, X, A = 2, 160, 2
    need = int(L.augment_batch_nearest_ws_bytes(B, X, X, 1))
    assert need == B * X * X * 4 and int(L.augment_batch_nearest_ws_bytes(B, X, X, 0)) == 0
    assert int(L.augment_batch_nearest_ws_bytes(B, 128, 128, 1)) == 0
    dev = torch.device("cuda", torch.cuda.current_device())
    img = torch.zeros(B, X, X, device=dev)
    lab = torch.zeros(B, X, X, A, dtype=torch.uint8, device=dev)
    par = torch.zeros(B * L.augment_param_bytes(), dtype=torch.uint8, device=dev)
    ctrl = torch.zeros(B, 2, 3, 3, dtype=torch.float64, device=dev)
    xo = torch.full((B, X, X), 7.0, device=dev)
    so = torch.full((B, X, X), 9, dtype=torch.uint8, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    args = (img.data_ptr(), lab.data_ptr(), par.data_ptr(), ctrl.data_ptr(), xo.data_ptr(), so.data_ptr())
    for w, nb in ((None, 0), (None, need), (ws.data_ptr(), need - 1)):
        with pytest.raises(rt.PhxError, match="workspace"):
            L.augment_batch_nearest(*args, w, nb, B, X, X, A, 5, st)
    for n in (4, 257):
        with pytest.raises(rt.PhxError, match="nlabels"):
            L.augment_batch_nearest(*args, ws.data_ptr(), need, B, X, X, A, n, st)
    with pytest.raises(rt.PhxError, match="null"):
        L.augment_batch_nearest(None, *args[1:], ws.data_ptr(), need, B, X, X, A, 5, st)
    with pytest.raises(rt.PhxError, match="LDS"):
        L.augment_batch_nearest(*args, ws.data_ptr(), need, B, 256, 256, A, 5, st)
    torch.cuda.synchronize()
    assert bool((xo == 7.0).all()) and bool((so == 9).all())
