"""The entries of csrc/multichannel.hip on the MI355X: images with 2 .. 16 channels through the posterior's input,
the mini-batch producer and the image grid of the summaries.

Posterior input and grid: exact against numpy / torch.  Producer: against the EXISTING single-channel entries run on every channel
plane with the same records (labels array_equal, images within the 1e-6 of the existing producer tests; whether the channels were in
fact bit-equal is printed), and per channel against the restatements the existing entries are pinned to."""
import numpy as np
import pytest
import torch

from oracle import augment as oa
from tests import augment_nearest_ref as nr
from tests import elastic_ref as er

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
CAP = 4096 * 256                    # threads of the largest grid phx_grid_for hands out (256-thread blocks)


@pytest.fixture(scope="module")
def L():
    from phiseg_code_amd import runtime as rt
    return rt.lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def _off4(n, dtype, fill=None):
    """a device tensor of n elements whose first byte sits 4 bytes past a 16-byte boundary"""
    es = torch.empty(0, dtype=dtype).element_size()
    base = torch.empty(n + 16, dtype=dtype, device="cuda")
    skip = ((16 - base.data_ptr() % 16) % 16 + 4) // es
    v = base[skip:skip + n]
    assert v.data_ptr() % 16 == 4
    if fill is not None:
        v.fill_(fill)
    return v


# ---- phx_posterior_input_mc --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dt", [F32, BF16])
@pytest.mark.parametrize("nlabels", [2, 5, 9])
@pytest.mark.parametrize("Cx", [2, 3, 4, 16])
def test_posterior_input_mc_is_exact(L, Cx, nlabels, out_dt):
    """[x, one_hot(s) - 0.5] for a Cx-channel x: exactly numpy's (bf16 through torch's rounding), at 37 pixels and above the grid cap
    (the grid-stride loop takes a second trip), every pointer 4 bytes off 16-byte alignment, labels >= nlabels give rows of -0.5, and
    the class columns are bit-equal to those of phx_posterior_input on the same labels"""
    g = torch.Generator(device="cuda").manual_seed(100 * Cx + 10 * nlabels + out_dt)
    tdt = torch.float32 if out_dt == F32 else torch.bfloat16
    C = Cx + nlabels
    for npix in (37, CAP // C + 5):
        assert npix == 37 or npix * C > CAP
        x = _off4(npix * Cx, torch.float32)
        x.copy_(torch.randn(npix * Cx, generator=g, device="cuda"))
        s = _off4(npix, torch.uint8)
        s.copy_(torch.randint(0, nlabels + 3, (npix,), generator=g, device="cuda").to(torch.uint8))
        s[-1] = 255
        out = _off4(npix * C + 8, tdt, fill=7.0)
        L.posterior_input_mc(x.data_ptr(), s.data_ptr(), out.data_ptr(), out_dt, npix, Cx, nlabels, S())
        torch.cuda.synchronize()
        assert bool((out[npix * C:] == 7.0).all())                           # nothing written past the end
        oh = (s.long()[:, None] == torch.arange(nlabels, device="cuda")[None, :]).float() - 0.5
        assert bool((oh[s.long() >= nlabels] == -0.5).all()) and int((s.long() >= nlabels).sum()) > 0
        ref = torch.cat([x.reshape(npix, Cx), oh], dim=1).to(tdt)
        got = out[:npix * C].reshape(npix, C)
        assert torch.equal(got, ref), (Cx, nlabels, out_dt, npix)
        narrow = torch.empty(npix, 1 + nlabels, dtype=tdt, device="cuda")
        x0 = x.reshape(npix, Cx)[:, 0].contiguous()
        L.posterior_input(x0.data_ptr(), s.data_ptr(), narrow.data_ptr(), out_dt, npix, nlabels, S())
        torch.cuda.synchronize()
        assert torch.equal(got[:, Cx:], narrow[:, 1:]) and torch.equal(got[:, 0], narrow[:, 0])


def test_posterior_input_mc_refusals_launch_nothing(L):
    from phiseg_code_amd import runtime as rt
    npix = 64
    x = torch.zeros(npix * 17, device="cuda")
    s = torch.zeros(npix, dtype=torch.uint8, device="cuda")
    out = torch.full((npix * (17 + 300),), 7.0, device="cuda")
    for Cx in (1, 17, 0):
        with pytest.raises(rt.PhxError, match="Cx"):
            L.posterior_input_mc(x.data_ptr(), s.data_ptr(), out.data_ptr(), F32, npix, Cx, 2, S())
    for n in (0, 257):
        with pytest.raises(rt.PhxError, match="nlabels"):
            L.posterior_input_mc(x.data_ptr(), s.data_ptr(), out.data_ptr(), F32, npix, 3, n, S())
    for args in ((None, s.data_ptr(), out.data_ptr()), (x.data_ptr(), None, out.data_ptr()), (x.data_ptr(), s.data_ptr(), None)):
        with pytest.raises(rt.PhxError, match="null"):
            L.posterior_input_mc(*args, F32, npix, 3, 2, S())
    with pytest.raises(rt.PhxError, match="out_dt"):
        L.posterior_input_mc(x.data_ptr(), s.data_ptr(), out.data_ptr(), 5, npix, 3, 2, S())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- phx_augment_batch_mc ----------------------------------------------------------------------------------------------------------------
def _data(n, X, Y, Cx, nlabels, annot, seed):
    """images [n, X, Y, Cx] ~ U(-0.5, 0.5), every channel its own draw; label maps: discs (up to four labels, tests/test_augment.py)
    or 3 x 2 pixel blocks cycling through every class (above, tests/test_augment_nearest_gpu.py)"""
    rng = np.random.default_rng(seed)
    img = (rng.random((n, X, Y, Cx), dtype=np.float32) - 0.5).astype(np.float32)
    yy, xx = np.mgrid[0:X, 0:Y]
    if nlabels > 4:
        lab = np.stack([np.stack([(xx // 3 + 5 * (yy // 2) + i + 2 * a) % nlabels for a in range(annot)], axis=-1) for i in range(n)])
        return img, lab.astype(np.uint8)
    lab = np.zeros((n, X, Y, annot), dtype=np.uint8)
    for i in range(n):
        for a in range(annot):
            for k in range(1, nlabels):
                cy, cx, r = rng.uniform(0.3, 0.7) * X, rng.uniform(0.3, 0.7) * Y, rng.uniform(0.08, 0.3) * min(X, Y) / k
                lab[i, ..., a][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
    return img, lab


def _launch_mc(L, img_d, lab_d, rec, ctrl, nlabels):
    """one direct call of the new entry -> (x [B, X, Y, Cx], s [B, X, Y]) host arrays; every output element is checked to be written"""
    N, X, Y, Cx = img_d.shape
    A, B, dev = lab_d.shape[3], len(rec), img_d.device
    par = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(ctrl, dtype=np.float64)).to(dev) if ctrl is not None else None
    xo = torch.full((B, X, Y, Cx), 7.0, dtype=torch.float32, device=dev)
    so = torch.full((B, X, Y), 251, dtype=torch.uint8, device=dev)
    nb = int(L.augment_batch_mc_ws_bytes(B, X, Y, Cx, nlabels, 1 if ctrl is not None else 0))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    L.augment_batch_mc(img_d.data_ptr(), lab_d.data_ptr(), par.data_ptr(), c.data_ptr() if c is not None else None, xo.data_ptr(),
                       so.data_ptr(), ws.data_ptr() if nb else None, nb, B, X, Y, A, Cx, nlabels, S())
    torch.cuda.synchronize()
    x, s = xo.cpu().numpy(), so.cpu().numpy()
    assert not (x == 7.0).any() and not (s == 251).any()
    return x, s, nb


def _launch_single(L, plane_d, lab_d, rec, ctrl, nlabels):
    """the matching EXISTING entry on one contiguous channel plane [N, X, Y]"""
    N, X, Y = plane_d.shape
    A, B, dev = lab_d.shape[3], len(rec), plane_d.device
    par = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(ctrl, dtype=np.float64)).to(dev) if ctrl is not None else None
    xo = torch.full((B, X, Y), 7.0, dtype=torch.float32, device=dev)
    so = torch.full((B, X, Y), 251, dtype=torch.uint8, device=dev)
    args = (plane_d.data_ptr(), lab_d.data_ptr(), par.data_ptr())
    if nlabels > 4:
        nb = int(L.augment_batch_nearest_ws_bytes(B, X, Y, 1 if c is not None else 0))
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        L.augment_batch_nearest(*args, c.data_ptr() if c is not None else None, xo.data_ptr(), so.data_ptr(), ws.data_ptr() if nb else None,
                                nb, B, X, Y, A, nlabels, S())
    elif c is not None:
        nb = int(L.augment_batch_elastic_ws_bytes(B, X, Y))
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        L.augment_batch_elastic(*args, c.data_ptr(), xo.data_ptr(), so.data_ptr(), ws.data_ptr() if nb else None, nb, B, X, Y, A, nlabels, S())
    else:
        L.augment_batch(*args, xo.data_ptr(), so.data_ptr(), B, X, Y, A, nlabels, S())
    torch.cuda.synchronize()
    return xo.cpu().numpy(), so.cpu().numpy()


def _records(X, Y, nlabels, elastic, scale, seed, batches, B=5, n=6):
    """the records (and control points) of `batches` batches as DeviceBatchProvider draws them: B = 5, augment_every_nth = 2, rotation,
    crop-scale (square images only: the reference draws the crop side from the ROW length and the origin from both extents, so on a
    non-square image the crop leaves the image -- there the four other augmentations run), elastic, both flips"""
    from phiseg_code_amd.data import augment as pa
    opts = dict(do_rotations=True, do_scaleaug=scale, do_elasticaug=elastic, do_fliplr=True, do_flipud=True, nlabels=nlabels,
                augment_every_nth=2, offset=min(30, Y // 3))
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    for t in range(batches):
        dec = [pa.draw_decisions(seed, t, j, X, Y, opts, 4) for j in range(B)]
        src, annots = rng.integers(0, n, B), [d["annot"] for d in dec]
        ctrl = np.zeros((B, 2, 3, 3), dtype=np.float64) if elastic else None
        out.append((pa.pack_params(dec, src, annots, X, Y, ctrl), ctrl, dec, src, annots))
        seen |= {(d["angle"] is not None, d["r_y"] is not None, d["elastic"] is not None, d["fliplr"], d["flipud"]) for d in dec}
    assert len(seen) >= 4, seen                      # augmented and untouched, flipped and not
    return out


def _against_existing(L, X, Y, Cx, nlabels, elastic, scale, batches):
    img, lab = _data(6, X, Y, Cx, nlabels, 4, 1000 * X + 10 * Cx + nlabels)
    img_d, lab_d = torch.as_tensor(img).cuda(), torch.as_tensor(lab).cuda()
    planes = [torch.as_tensor(np.ascontiguousarray(img[..., c])).cuda() for c in range(Cx)]
    bit_equal, worst = True, 0.0
    for rec, ctrl, dec, src, annots in _records(X, Y, nlabels, elastic, scale, 99 + Cx, batches):
        x, s, nb = _launch_mc(L, img_d, lab_d, rec, ctrl, nlabels)
        for c in range(Cx):
            px, ps = _launch_single(L, planes[c], lab_d, rec, ctrl, nlabels)
            assert np.array_equal(s, ps), (c, int((s != ps).sum()))
            np.testing.assert_allclose(x[..., c], px, rtol=0, atol=1e-6)
            bit_equal &= np.array_equal(x[..., c], px)
            worst = max(worst, float(np.abs(x[..., c] - px).max()))
    print("augment_batch_mc %d x %d Cx=%d nlabels=%d %s: channels bit-equal to the single-channel entries: %s (max |diff| %.3g), workspace %d bytes"
          % (X, Y, Cx, nlabels, "elastic" if elastic else "plain", bit_equal, worst, nb))
    return nb


@pytest.mark.parametrize("nlabels", [2, 4, 5, 19])
@pytest.mark.parametrize("Cx", [2, 3, 4])
@pytest.mark.parametrize("X,Y,elastic,scale", [(24, 24, True, True),        # displacements of twice the image: repeated reflection
                                               (24, 24, False, True),       # the plain producer (ctrl_dev NULL)
                                               (32, 40, True, False),       # non-square: a swapped stride shows
                                               (128, 128, True, True)])     # the largest LDS-resident form
def test_producer_equals_the_single_channel_entries(L, X, Y, elastic, scale, Cx, nlabels):
    nb = _against_existing(L, X, Y, Cx, nlabels, elastic, scale, 2 if X == 128 else 4)
    assert nb == 0


@pytest.mark.parametrize("nlabels", [2, 5])
def test_producer_workspace_form_equals_the_single_channel_entries(L, nlabels):
    """160 x 160 elastic: a block's intermediates exceed LDS on either label route and live in the caller's workspace"""
    nb = _against_existing(L, 160, 160, 3, nlabels, True, True, 2)
    assert nb == (5 * 3 * 160 * 160 * 4 + (5 * 160 * 160 if nlabels <= 4 else 0))


@pytest.mark.parametrize("nlabels", [3, 9])
def test_producer_matches_the_restatements_per_channel(L, nlabels):
    """Cx = 3, one case per label route: oracle.augment.augment_pair (plain, up to four labels), tests/elastic_ref.py (elastic, up to four
    labels), tests/augment_nearest_ref.py (above four, plain and elastic), at their bounds: labels equal, images within 1e-6"""
    X, Cx = 48, 3
    img, lab = _data(6, X, X, Cx, nlabels, 4, 77 + nlabels)
    img_d, lab_d = torch.as_tensor(img).cuda(), torch.as_tensor(lab).cuda()
    for elastic in (False, True):
        for rec, ctrl, dec, src, annots in _records(X, X, nlabels, elastic, True, 31 + nlabels, 3):
            x, s, _ = _launch_mc(L, img_d, lab_d, rec, ctrl, nlabels)
            for j, d in enumerate(dec):
                for c in range(Cx):
                    plane, lm = img[src[j], ..., c], lab[src[j], ..., annots[j]]
                    if nlabels > 4:
                        ref_x, ref_s = nr.augment_pair_nearest(plane, lm, d)
                    elif elastic:
                        ref_x, ref_s = er.augment_pair_elastic(plane, lm, d, nlabels)
                    else:
                        ref_x, ref_s = oa.augment_pair(plane, lm, d, nlabels)
                    assert np.array_equal(s[j], ref_s), (j, c, d)
                    np.testing.assert_allclose(x[j, ..., c], ref_x, rtol=0, atol=1e-6, err_msg=str(d))


def test_producer_refusals_launch_nothing(L):
    from phiseg_code_amd import runtime as rt
    B, X, A, Cx = 2, 160, 2, 3
    need = int(L.augment_batch_mc_ws_bytes(B, X, X, Cx, 2, 1))
    assert need == B * Cx * X * X * 4 + B * X * X and int(L.augment_batch_mc_ws_bytes(B, X, X, Cx, 5, 1)) == B * Cx * X * X * 4
    assert int(L.augment_batch_mc_ws_bytes(B, X, X, Cx, 2, 0)) == 0 and int(L.augment_batch_mc_ws_bytes(B, 128, 128, Cx, 2, 1)) == 0
    assert int(L.augment_batch_mc_ws_bytes(B, 136, 136, Cx, 2, 1)) > 0 and int(L.augment_batch_mc_ws_bytes(B, 136, 136, Cx, 5, 1)) == 0
    dev = torch.device("cuda", torch.cuda.current_device())
    img = torch.zeros(B, X, X, 17, device=dev)
    lab = torch.zeros(B, X, X, A, dtype=torch.uint8, device=dev)
    par = torch.zeros(B * L.augment_param_bytes(), dtype=torch.uint8, device=dev)
    ctrl = torch.zeros(B, 2, 3, 3, dtype=torch.float64, device=dev)
    xo = torch.full((B, X, X, 17), 7.0, device=dev)
    so = torch.full((B, X, X), 9, dtype=torch.uint8, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = S()
    args = (img.data_ptr(), lab.data_ptr(), par.data_ptr(), ctrl.data_ptr(), xo.data_ptr(), so.data_ptr())
    for w, nb in ((None, 0), (None, need), (ws.data_ptr(), need - 1)):                 # a missing and a too-small workspace
        with pytest.raises(rt.PhxError, match="workspace"):
            L.augment_batch_mc(*args, w, nb, B, X, X, A, Cx, 2, st)
    for c in (1, 17, 0):
        with pytest.raises(rt.PhxError, match="Cx"):
            L.augment_batch_mc(*args, ws.data_ptr(), need, B, X, X, A, c, 2, st)
    for n in (0, 257):
        with pytest.raises(rt.PhxError, match="nlabels"):
            L.augment_batch_mc(*args, ws.data_ptr(), need, B, X, X, A, Cx, n, st)
    with pytest.raises(rt.PhxError, match="null"):
        L.augment_batch_mc(None, *args[1:], ws.data_ptr(), need, B, X, X, A, Cx, 2, st)
    with pytest.raises(rt.PhxError, match="LDS"):                                       # X * Y * 4 above 160 KiB
        L.augment_batch_mc(*args, ws.data_ptr(), need, B, 256, 256, A, Cx, 2, st)
    torch.cuda.synchronize()
    assert bool((xo == 7.0).all()) and bool((so == 9).all())


# ---- the provider ---------------------------------------------------------------------------------------------------------------------------
def test_provider_hands_out_three_channel_batches():
    """without augmentation next_batch hands out the source pixels unchanged; next_batch_device writes a plan-shaped buffer directly;
    BatchProvider(add_dummy_dimension=False) on the 4-D array gives what DeviceBatchProvider gives"""
    from phiseg_code_amd.data import augment as pa
    from phiseg_code_amd.data import batch_provider
    img, lab = _data(8, 64, 64, 3, 2, 4, 5)
    prov = pa.DeviceBatchProvider(img, lab, do_augmentations=False, num_labels_per_subject=4, annotator_range=[0, 2], seed=1)
    assert prov.channels == 3 and prov.images.shape == (8, 64, 64, 3) and np.array_equal(prov.images, img)
    bp = batch_provider.BatchProvider(img, lab, np.arange(8), add_dummy_dimension=False, num_labels_per_subject=4, annotator_range=[0, 2], seed=1)
    seen = []
    for _ in range(2):
        x, s = prov.next_batch(4)
        assert x.shape == (4, 64, 64, 3) and s.shape == (4, 64, 64)
        seen += list(prov.last_indices)
        for j, (src, an) in enumerate(zip(prov.last_indices, prov.last_annotators)):
            assert np.array_equal(x[j], img[src]) and np.array_equal(s[j], lab[src, ..., an])
        xb, sb = bp.next_batch(4)
        assert np.array_equal(xb, x) and np.array_equal(sb, s)
    assert sorted(seen) == list(range(8))
    xd = torch.zeros(4, 64, 64, 3, device="cuda")
    sd = torch.full((4, 64, 64), 9, dtype=torch.uint8, device="cuda")
    prov.next_batch_device(4, xd.data_ptr(), sd.data_ptr())
    torch.cuda.synchronize()
    for j, (src, an) in enumerate(zip(prov.last_indices, prov.last_annotators)):
        assert np.array_equal(xd[j].cpu().numpy(), img[src]) and np.array_equal(sd[j].cpu().numpy(), lab[src, ..., an])
    with pytest.raises(ValueError):
        batch_provider.BatchProvider(img[..., 0], lab, np.arange(8), add_dummy_dimension=False)
    with pytest.raises(ValueError, match="16"):
        pa.DeviceBatchProvider(np.zeros((2, 8, 8, 17), np.float32), np.zeros((2, 8, 8, 1), np.uint8))


def test_provider_augments_three_channels_like_three_providers():
    """the provider end to end at Cx = 3, all five augmentations: every channel is what a one-channel provider with the same seed gives
    for that plane, the label maps are equal"""
    from phiseg_code_amd.data import augment as pa
    X, nlabels = 32, 3
    img, lab = _data(6, X, X, 3, nlabels, 4, 9)
    opts = dict(do_rotations=True, do_scaleaug=True, do_elasticaug=True, do_fliplr=True, do_flipud=True, nlabels=nlabels,
                augment_every_nth=2, offset=10)
    kw = dict(do_augmentations=True, augmentation_options=opts, num_labels_per_subject=4, annotator_range=range(4), seed=99, nlabels=nlabels)
    prov = pa.DeviceBatchProvider(img, lab, **kw)
    singles = [pa.DeviceBatchProvider(np.ascontiguousarray(img[..., c]), lab, **kw) for c in range(3)]
    for _ in range(3):
        x, s = prov.next_batch(5)
        assert x.shape == (5, X, X, 3)
        for c, sp in enumerate(singles):
            xs, ss = sp.next_batch(5)
            assert list(sp.last_indices) == list(prov.last_indices)
            assert np.array_equal(ss, s)
            np.testing.assert_allclose(x[..., c], xs[..., 0], rtol=0, atol=1e-6)


def test_a_trailing_axis_of_one_keeps_the_old_entries():
    """[N, X, Y, 1] still gives [B, X, Y, 1] through the single-channel entries, checked against the one-channel oracle as
    test_device_augmentation_matches_oracle does"""
    from phiseg_code_amd import multichannel
    from phiseg_code_amd.data import augment as pa
    X, nlabels = 64, 4
    img, lab = _data(6, X, X, 1, nlabels, 4, X)
    opts = dict(do_rotations=True, do_scaleaug=True, do_fliplr=True, do_flipud=True, nlabels=nlabels, augment_every_nth=2)
    prov = pa.DeviceBatchProvider(img, lab, do_augmentations=True, augmentation_options=opts, num_labels_per_subject=4,
                                  annotator_range=range(4), seed=99, nlabels=nlabels)
    assert prov.channels == 1 and prov.images.shape == (6, X, X, 1) and tuple(prov.images_dev.shape) == (6, X, X)
    assert multichannel.augment_entry(prov.channels, nlabels, prov.elastic) == "augment_batch"
    called = []
    orig = prov.L.augment_batch_mc
    prov.L.augment_batch_mc = lambda *a: called.append(a)
    try:
        for _ in range(3):
            x, s = prov.next_batch(5)
            assert x.shape == (5, X, X, 1) and s.shape == (5, X, X)
            for j, (d, src, an) in enumerate(zip(prov.last_decisions, prov.last_indices, prov.last_annotators)):
                ref_x, ref_s = oa.augment_pair(img[src, ..., 0], lab[src, ..., an], d, nlabels)
                assert np.array_equal(s[j], ref_s), (j, d)
                np.testing.assert_allclose(x[j, ..., 0], ref_x, rtol=0, atol=1e-6, err_msg=str(d))
    finally:
        prov.L.augment_batch_mc = orig
    assert not called


# ---- phx_summary_grid_image_mc ---------------------------------------------------------------------------------------------------------
def _grid_mc(L, a, Cout):
    from phiseg_code_amd import summary as Sm
    B, H, W, Cx = a.shape
    gy, gx = Sm.factorization(B)
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    out = torch.full(((H + 2) * gy, (W + 2) * gx, Cout), 77, dtype=torch.uint8, device="cuda")
    work = torch.empty(8, dtype=torch.uint8, device="cuda")
    L.summary_grid_image_mc(t.data_ptr(), B, H, W, Cx, Cout, gy, gx, out.data_ptr(), work.data_ptr(), S())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _ref_grid_mc(a, Cout):
    """the pixel rule of tests.test_summary_gpu._ref_grid (fp32 steps, truncation, NaN -> 0, saturation) with the min / max of the WHOLE
    tensor, stacked per output channel; tile b at row block b % grid_Y, column block b // grid_Y (the test below holds this placement to
    _ref_grid itself, on a channel whose own extrema are the tensor's)"""
    from phiseg_code_amd import summary as Sm
    B, H, W, Cx = a.shape
    gy, gx = Sm.factorization(B)
    v = a.astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = (v - v.min()) / v.max()
        f = f * np.float32(254.0)
    assert f.dtype == np.float32
    u8 = np.where(np.isnan(f), np.float32(0), np.clip(f, 0, 255)).astype(np.uint8)
    g = np.zeros(((H + 2) * gy, (W + 2) * gx, Cout), dtype=np.uint8)
    for b in range(B):
        r0, c0 = (b % gy) * (H + 2) + 1, (b // gy) * (W + 2) + 1
        g[r0:r0 + H, c0:c0 + W] = u8[b, :, :, :Cout]
    return g, f


@pytest.mark.parametrize("Cx,Cout", [(3, 3), (4, 4), (2, 1), (16, 1)])
@pytest.mark.parametrize("hw", [(5, 7), (32, 32)])
@pytest.mark.parametrize("B", [1, 6])
def test_image_grid_of_a_multi_channel_batch(L, B, hw, Cx, Cout):
    from tests.test_summary_gpu import _ref_grid
    H, W = hw
    rng = np.random.RandomState(10 * B + H + Cx)
    a = (rng.rand(B, H, W, Cx) - 0.5).astype(np.float32)
    a[0, 0, 0, Cx - 1], a[B - 1, H - 1, W - 1, Cx - 1] = -0.75, 0.875         # the extrema sit in the LAST channel: whole-tensor min / max
    got = _grid_mc(L, a, Cout)
    want, _ = _ref_grid_mc(a, Cout)
    assert got.shape == want.shape and np.array_equal(got, want)
    # the tile placement is _ref_grid's: a channel whose own extrema are the tensor's goes through _ref_grid itself
    b = a.copy()
    b[..., 0] = a[..., Cx - 1]
    b[..., Cx - 1] = a[..., 0]
    ref0, _ = _ref_grid(b[..., 0])
    assert np.array_equal(_grid_mc(L, b, Cout)[:, :, 0], ref0[0, :, :, 0])


def test_image_grid_where_the_cast_is_undefined(L):
    """the three undefined-cast cases of test_grid_where_the_cast_is_undefined at Cx = 3: all-equal zeros (0 / 0 = NaN -> 0), a negative
    maximum (-> 0), values above 255 (saturate)"""
    B, H, W, Cx = 2, 5, 7, 3
    got = _grid_mc(L, np.zeros((B, H, W, Cx), dtype=np.float32), 3)
    assert got.shape == (H + 2, (W + 2) * 2, 3) and not got.any()
    rng = np.random.RandomState(3)
    neg = (-1.0 - rng.rand(B, H, W, Cx)).astype(np.float32)
    want, f = _ref_grid_mc(neg, 3)
    assert f.max() <= 0
    got = _grid_mc(L, neg, 3)
    assert np.array_equal(got, want) and not got.any()
    sat = (rng.rand(B, H, W, Cx) * 1.5 - 1.0).astype(np.float32)
    want, f = _ref_grid_mc(sat, 3)
    assert f.max() > 255 and sat.max() > 0
    got = _grid_mc(L, sat, 3)
    assert np.array_equal(got, want) and got.max() == 255


def test_image_grid_refusals_launch_nothing(L):
    from phiseg_code_amd import runtime as rt
    B, H, W = 2, 4, 4
    src = torch.zeros(B, H, W, 16, device="cuda")
    out = torch.full(((H + 2), (W + 2) * 2, 4), 77, dtype=torch.uint8, device="cuda")
    work = torch.empty(8, dtype=torch.uint8, device="cuda")
    for Cx, Cout, pat in ((1, 1, "Cx"), (17, 1, "Cx"), (3, 2, "Cout"), (3, 4, "Cout"), (2, 3, "Cout")):
        with pytest.raises(rt.PhxError, match=pat):
            L.summary_grid_image_mc(src.data_ptr(), B, H, W, Cx, Cout, 1, 2, out.data_ptr(), work.data_ptr(), S())
    with pytest.raises(rt.PhxError, match="grid_y"):
        L.summary_grid_image_mc(src.data_ptr(), B, H, W, 3, 3, 2, 2, out.data_ptr(), work.data_ptr(), S())
    with pytest.raises(rt.PhxError, match="null"):
        L.summary_grid_image_mc(None, B, H, W, 3, 3, 1, 2, out.data_ptr(), work.data_ptr(), S())
    torch.cuda.synchronize()
    assert bool((out == 77).all())
