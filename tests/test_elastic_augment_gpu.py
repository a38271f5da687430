"""do_elasticaug on the device: phx_augment_batch_elastic against the numpy restatement of batch_provider.py:226-248
(tests/elastic_ref.py -- OpenCV's published cubic resize and fixed-point remap restated, cv2 itself is not installed, so this pins
the kernel to the restatement, not to cv2), against properties that do not involve the restatement (zero field, constant integer
field, unflagged samples), the workspace contract, and the provider end to end.

Labels bit-equal, images to 1e-6: the same operations in the same order with no FMA contraction on either side -- the bound
tests/test_augment.py uses for the two other resamplings."""
import os
import types

import numpy as np
import pytest

from tests import elastic_ref as er

pytestmark = pytest.mark.gpu


def _data_xy(n, X, Y, nlabels, annot, seed):
    """tests/test_augment.py:_data for an X x Y image"""
    rng = np.random.default_rng(seed)
    img = (rng.random((n, X, Y), dtype=np.float32) - 0.5).astype(np.float32)
    yy, xx = np.mgrid[0:X, 0:Y]
    lab = np.zeros((n, X, Y, annot), dtype=np.uint8)
    for i in range(n):
        for a in range(annot):
            for k in range(1, nlabels):
                cy, cx, r = rng.uniform(0.3, 0.7) * X, rng.uniform(0.3, 0.7) * Y, rng.uniform(0.08, 0.3) * min(X, Y) / k
                lab[i, ..., a][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
    return img, lab


@pytest.mark.parametrize("X,Y,nlabels,resample", [(24, 24, 2, True),          # displacements of twice the image: repeated reflection
                                                  (64, 64, 4, True),          # four one-hot planes
                                                  (128, 128, 2, True),        # the largest size whose intermediates stay in LDS
                                                  (192, 192, 3, True),        # intermediates in the global workspace
                                                  (40, 24, 2, False)])        # non-square, elastic alone: rows vs columns
def test_device_elastic_matches_restatement(X, Y, nlabels, resample):
    from phiseg_code_amd.data import augment as pa
    img, lab = _data_xy(6, X, Y, nlabels, 4, X + Y)
    # offset: the crop side is drawn from [Y - offset, Y]; the default 30 is meant for 128 pixels and exceeds a 24-pixel image
    opts = dict(do_rotations=resample, do_scaleaug=resample, do_elasticaug=True, do_fliplr=True, do_flipud=True, nlabels=nlabels,
                augment_every_nth=2, offset=min(30, Y // 3))
    prov = pa.DeviceBatchProvider(img, lab, do_augmentations=True, augmentation_options=opts, num_labels_per_subject=4,
                                  annotator_range=range(4), seed=99, nlabels=nlabels)
    assert (prov.L.augment_batch_elastic_ws_bytes(5, X, Y) > 0) == (9 * X * Y > 160 * 1024)
    seen, worst, reflected = set(), 0.0, []
    for _ in range(4):
        x, s = prov.next_batch(5)
        assert x.shape == (5, X, Y, 1) and s.shape == (5, X, Y) and s.dtype == np.uint8
        for j, (d, src, an) in enumerate(zip(prov.last_decisions, prov.last_indices, prov.last_annotators)):
            stats = {}
            ref_x, ref_s = er.augment_pair_elastic(img[src], lab[src, ..., an], d, nlabels, stats)
            worst = max(worst, float(np.abs(x[j, ..., 0] - ref_x).max()))
            reflected.append(stats.get("reflected"))
            assert np.array_equal(s[j], ref_s), (j, d, int((s[j] != ref_s).sum()))
            np.testing.assert_allclose(x[j, ..., 0], ref_x, rtol=0, atol=1e-6, err_msg=str(d))
            seen.add((d["angle"] is not None, d["r_y"] is not None, d["elastic"] is not None, bool(d["fliplr"] or d["flipud"])))
    print("%d x %d: max |image - restatement| = %.3g, border-reflected share %s" %
          (X, Y, worst, np.mean([r for r in reflected if r is not None])))
    # elastic after both resamplings (or, in the last case, with none before it), flipped and not, and untouched samples
    assert {(resample, resample, True, False), (resample, resample, True, True), (False, False, False, False)} <= seen
    assert any(r is not None and r > 0 for r in reflected)                      # the reflecting border was exercised


def _launch(L, img_d, lab_d, rec, ctrl, B, X, Y, A, nlabels, elastic):
    """one direct ABI call on explicit records -> (x [B, X, Y] f32, s [B, X, Y] u8) host arrays"""
    import torch
    dev = img_d.device
    par = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    xo = torch.full((B, X, Y), 7.0, dtype=torch.float32, device=dev)
    so = torch.full((B, X, Y), 9, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    if elastic:
        c = torch.from_numpy(np.ascontiguousarray(ctrl, dtype=np.float64)).to(dev)
        nb = L.augment_batch_elastic_ws_bytes(B, X, Y)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        L.augment_batch_elastic(img_d.data_ptr(), lab_d.data_ptr(), par.data_ptr(), c.data_ptr(), xo.data_ptr(), so.data_ptr(),
                                ws.data_ptr() if nb else None, nb, B, X, Y, A, nlabels, st)
    else:
        L.augment_batch(img_d.data_ptr(), lab_d.data_ptr(), par.data_ptr(), xo.data_ptr(), so.data_ptr(), B, X, Y, A, nlabels, st)
    torch.cuda.synchronize()
    return xo.cpu().numpy(), so.cpu().numpy()


def test_elastic_properties_direct_abi():
    """Independent of the restatement: zero field = phx_augment_batch, a constant integer field = an exact reflect shift,
    unflagged samples = phx_augment_batch."""
    import torch
    from phiseg_code_amd import runtime as rt
    from phiseg_code_amd.data import augment as pa
    L = rt.lib()
    B, X, A, nlabels = 6, 32, 4, 3
    img, lab = _data_xy(B, X, X, nlabels, A, 11)
    img_d, lab_d = torch.as_tensor(img).cuda(), torch.as_tensor(lab).cuda()
    plain = dict(augment=True, angle=None, r_y=None, p_x=None, p_y=None, elastic=None, fliplr=False, flipud=False)
    dec = [dict(plain, angle=7.5, fliplr=True), dict(plain, r_y=20, p_x=5, p_y=9), dict(plain, angle=-9.0, r_y=27, p_x=2, p_y=4, flipud=True),
           dict(plain), dict(plain, fliplr=True, flipud=True), dict(plain, angle=3.0, r_y=31, p_x=1, p_y=0)]
    src, annots = [3, 0, 5, 1, 2, 4], [0, 1, 2, 3, 0, 1]

    def records(decisions, ctrl=None):
        return pa.pack_params(decisions, src, annots, X, X, ctrl)
    zeros = (np.zeros(9), np.zeros(9))
    base_x, base_s = _launch(L, img_d, lab_d, records(dec), None, B, X, X, A, nlabels, False)
    assert not (base_x == 7.0).any() and not (base_s == 9).any()                # every pixel written

    # (a) the elastic bit on every record, all control points zero: phx_augment_batch, bit for bit
    ctrl = np.zeros((B, 2, 3, 3))
    rec = records([dict(d, elastic=zeros) for d in dec], ctrl)
    assert all(rec["flags"] & pa.ELASTIC)
    ax, as_ = _launch(L, img_d, lab_d, rec, ctrl, B, X, X, A, nlabels, True)
    assert np.array_equal(ax, base_x) and np.array_equal(as_, base_s)

    # (b) a constant (dx, dy) = (3, -2), flips cleared: out(y, x) = in(reflect(y - 2), reflect(x + 3)) of the flip-free result
    noflip = [dict(d, fliplr=False, flipud=False) for d in dec]
    nf_x, nf_s = _launch(L, img_d, lab_d, records(noflip), None, B, X, X, A, nlabels, False)
    const = (np.full(9, 3.0), np.full(9, -2.0))
    rec = records([dict(d, elastic=const) for d in noflip], ctrl)
    bx, bs = _launch(L, img_d, lab_d, rec, ctrl, B, X, X, A, nlabels, True)
    yy, xx = er.border_reflect(np.arange(X) - 2, X), er.border_reflect(np.arange(X) + 3, X)
    assert np.array_equal(bx, nf_x[:, yy][:, :, xx]) and np.array_equal(bs, nf_s[:, yy][:, :, xx])

    # (c) the bit on samples 0, 2, 4 only, random control points: 1, 3, 5 are phx_augment_batch bit for bit; 0, 2, 4 (elastic after
    # a rotation alone, after both resamplings, and with none) follow the restatement
    rng = np.random.default_rng(5)
    mixed = [dict(d, elastic=(10.0 * rng.standard_normal(9), 10.0 * rng.standard_normal(9))) if j % 2 == 0 else d for j, d in enumerate(dec)]
    ctrl = rng.standard_normal((B, 2, 3, 3)) * 1e3                              # unflagged rows: never read
    rec = records(mixed, ctrl)
    assert [bool(f & pa.ELASTIC) for f in rec["flags"]] == [True, False] * 3
    cx, cs = _launch(L, img_d, lab_d, rec, ctrl, B, X, X, A, nlabels, True)
    for j in range(B):
        if j % 2:
            assert np.array_equal(cx[j], base_x[j]) and np.array_equal(cs[j], base_s[j]), j
        else:
            ref_x, ref_s = er.augment_pair_elastic(img[src[j]], lab[src[j], ..., annots[j]], mixed[j], nlabels)
            assert np.array_equal(cs[j], ref_s), j
            np.testing.assert_allclose(cx[j], ref_x, rtol=0, atol=1e-6)
            assert not np.array_equal(cx[j], base_x[j])


def test_elastic_workspace_contract():
    """The size query, and a refused call: a status comes back and nothing is launched (the outputs keep their fill)."""
    import torch
    from phiseg_code_amd import runtime as rt
    L = rt.lib()
    assert L.augment_batch_elastic_ws_bytes(4, 128, 128) == 0
    need = L.augment_batch_elastic_ws_bytes(4, 192, 192)
    assert need >= 4 * 192 * 192 * 5
    B, X, A = 4, 192, 1
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
            L.augment_batch_elastic(*args, w, nb, B, X, X, A, 2, st)
    with pytest.raises(rt.PhxError, match="nlabels"):
        L.augment_batch_elastic(*args, ws.data_ptr(), need, B, X, X, A, 5, st)
    with pytest.raises(rt.PhxError, match="null"):
        L.augment_batch_elastic(*args[:3], None, *args[4:], ws.data_ptr(), need, B, X, X, A, 2, st)
    torch.cuda.synchronize()
    assert bool((xo == 7.0).all()) and bool((so == 9).all())


def test_provider_end_to_end_on_the_hdf5_fixture(golden_dir):
    """lidc_data on tests/golden/lidc_like.hdf5 with the shipped experiment's options plus do_elasticaug."""
    from phiseg_code_amd.data import augment as pa
    shipped = {'do_flip_lr': True, 'do_flip_ud': True, 'do_rotations': True, 'do_scaleaug': True, 'nlabels': 2}

    def make(options):
        cfg = types.SimpleNamespace(num_labels_per_subject=4, annotator_range=range(4), nlabels=2, augmentation_options=options)
        # seed 11: every crop side its three batches draw is positive (the shipped options leave `offset` at 30, more than the
        # fixture's 24 pixels, so other seeds draw sides <= 0)
        return pa.lidc_data(cfg, os.path.join(golden_dir, "lidc_like.hdf5"), seed=11)
    a, b, plain = make(dict(shipped, do_elasticaug=True)), make(dict(shipped, do_elasticaug=True)), make(shipped)
    lo, hi = float(a.train.images.min()), float(a.train.images.max())
    assert lo < 0 < hi                                                          # (the rotation pads with 0)
    n_aug = n_diff = 0
    for _ in range(3):
        xa, sa = a.train.next_batch(5)
        xb, sb = b.train.next_batch(5)
        xp, sp = plain.train.next_batch(5)
        assert np.array_equal(xa, xb) and np.array_equal(sa, sb)                # same seed: the same batch, bit for bit
        assert set(np.unique(sa)) <= {0, 1} and xa.min() >= lo - 1e-6 and xa.max() <= hi + 1e-6
        assert list(a.train.last_indices) == list(plain.train.last_indices)
        for j, (d, dp) in enumerate(zip(a.train.last_decisions, plain.train.last_decisions)):
            assert d["augment"] == dp["augment"] and (d["elastic"] is not None) == d["augment"] and dp["elastic"] is None
            if d["augment"]:
                n_aug += 1
                n_diff += not np.array_equal(xa[j], xp[j])
            else:
                assert np.array_equal(xa[j], xp[j]) and np.array_equal(sa[j], sp[j])
    assert n_aug > 0 and n_diff > 0
    xv, _ = a.validation.next_batch(2)                                          # the un-augmented providers never draw a field
    assert all(d["elastic"] is None for d in a.validation.last_decisions) and not a.validation.elastic


def test_train_consumes_deformed_batches():
    """phiseg.train(data) on a config with do_elasticaug: the steps run on batches that went through the third pass."""
    from tests.helpers import load_golden
    from tests.test_graph_cpu import make_config
    from phiseg_code_amd.data import augment as pa
    from phiseg_code_amd.phiseg import phiseg_model
    _, gcfg, _ = load_golden("tiny_phiseg_bn")
    cfg = make_config(gcfg, "f32")
    cfg.batch_size, cfg.annotator_range, cfg.num_labels_per_subject = 2, range(4), 4
    cfg.lr_schedule_dict = {0: 1e-3}
    cfg.augmentation_options = dict(do_rotations=True, do_scaleaug=True, do_elasticaug=True, nlabels=cfg.nlabels, augment_every_nth=1)
    H = gcfg["H"]
    parts = {sp: _data_xy(n, H, H, cfg.nlabels, 4, 40 + n) for sp, n in (("train", 4), ("val", 2))}
    data = pa.lidc_data(cfg, {sp: dict(images=i, labels=l) for sp, (i, l) in parts.items()}, seed=5)
    assert data.train.elastic and not data.validation.elastic
    model = phiseg_model.phiseg(cfg)
    losses = model.train(data, num_iter=2, log_every=0)
    assert len(losses) == 2 and np.all(np.isfinite(losses))
    assert data.train.step == 2 and all(d["elastic"] is not None for d in data.train.last_decisions)
    x, s = data.train.next_batch(2)                                              # ... and such a batch is a deformed one
    for j, (d, src, an) in enumerate(zip(data.train.last_decisions, data.train.last_indices, data.train.last_annotators)):
        ref_x, ref_s = er.augment_pair_elastic(parts["train"][0][src], parts["train"][1][src, ..., an], d, cfg.nlabels)
        assert np.array_equal(s[j], ref_s)
        np.testing.assert_allclose(x[j, ..., 0], ref_x, rtol=0, atol=1e-6)
        assert not np.array_equal(x[j, ..., 0], parts["train"][0][src])
