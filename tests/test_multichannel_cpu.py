"""Multi-channel images, the host side without a GPU: the dispatch by channel count, the range check when a model is
built, the variable lists at three channels, the declared entries, colour PNGs and their summary values, and the synthetic data."""
import struct
import zlib

import numpy as np
import pytest

from tests.helpers import load_golden
from tests.test_graph_cpu import make_config

from phiseg_code_amd import multichannel
from phiseg_code_amd import summary as S
from phiseg_code_amd.data import synthetic


def config(case, Cx, dtype="f32"):
    """tests.test_graph_cpu.make_config sets one channel; the third entry of image_size is set afterwards"""
    _, cfg, _ = load_golden(case)
    c = make_config(cfg, dtype)
    c.image_size = (cfg["H"], cfg["H"], Cx)
    return c, cfg


def test_dispatch_by_channel_count():
    assert multichannel.MAX_IMAGE_CHANNELS == 16
    assert multichannel.posterior_input_entry(1) == "posterior_input"
    assert multichannel.summary_grid_entry(1) == "summary_grid_u8" and multichannel.summary_channels(1) == 1
    assert [multichannel.augment_entry(1, n, e) for n, e in ((2, False), (4, True), (5, False), (19, True))] == \
        ["augment_batch", "augment_batch_elastic", "augment_batch_nearest", "augment_batch_nearest"]
    for Cx in range(2, 17):
        assert multichannel.posterior_input_entry(Cx) == "posterior_input_mc"
        assert multichannel.summary_grid_entry(Cx) == "summary_grid_image_mc"
        assert {multichannel.augment_entry(Cx, n, e) for n in (2, 4, 5, 256) for e in (False, True)} == {"augment_batch_mc"}
        assert multichannel.summary_channels(Cx) == (Cx if Cx in (3, 4) else 1)
    for fn in (multichannel.posterior_input_entry, multichannel.augment_entry, multichannel.summary_channels, multichannel.summary_grid_entry,
               multichannel.check_channels):
        for bad in (0, 17, -1, 2.5):
            with pytest.raises(ValueError, match="1 .. 16"):
                fn(bad)
    with pytest.raises(ValueError):
        multichannel.augment_entry(3, 257)


@pytest.mark.parametrize("Cx", [0, 17])
def test_model_build_names_the_channel_range(Cx):
    from phiseg_code_amd.phiseg import phiseg_model
    c, _ = config("tiny_phiseg_bn", Cx)
    with pytest.raises(ValueError, match=r"image_size\[2\].*1 \.\. 16"):
        phiseg_model.phiseg(c)


@pytest.mark.parametrize("case,readers", [
    ("tiny_phiseg_bn", {"posterior/z0_pre_1/W": 1, "prior/z0_pre_1/W": 0}),
    ("tiny_probunet_bn", {"posterior/conv_0_1/W": 1, "prior/conv_0_1/W": 0, "likelihood/encoder/conv_0_1/W": 0})])
def test_variables_at_three_channels(case, readers):
    """the names and the creation order of the one-channel model; only the convolutions that read x change, in their input width:
    the posterior's reads [x, one_hot(s) - 0.5] (3 + nlabels), the prior's and the probabilistic U-Net likelihood's read x (3)"""
    from phiseg_code_amd.phiseg import phiseg_model
    c1, cfg = config(case, 1)
    one = [(n, tuple(v.shape)) for n, v in phiseg_model.phiseg(c1).graph.variables.items()]
    c3, _ = config(case, 3)
    three = [(n, tuple(v.shape)) for n, v in phiseg_model.phiseg(c3).graph.variables.items()]
    assert [n for n, _ in one] == [n for n, _ in three]
    diff = {n: (s1, s3) for (n, s1), (_, s3) in zip(one, three) if s1 != s3}
    assert set(diff) == set(readers)
    for n, with_labels in readers.items():
        extra = cfg["nlabels"] if with_labels else 0
        assert diff[n] == ((3, 3, 1 + extra, cfg["n0"]), (3, 3, 3 + extra, cfg["n0"])), (n, diff[n])


def test_header_declares_the_entries():
    import ctypes
    from phiseg_code_amd import runtime as rt
    protos = rt.parse_header()
    assert len(protos["phx_posterior_input_mc"]) == 8 and protos["phx_posterior_input_mc"][4] is ctypes.c_size_t
    assert len(protos["phx_augment_batch_mc"]) == 15 and protos["phx_augment_batch_mc"][7] is ctypes.c_size_t
    assert protos["phx_augment_batch_mc_ws_bytes"] == [ctypes.c_int] * 6
    assert len(protos["phx_summary_grid_image_mc"]) == 11
    src = open(rt.HEADER).read()
    sec = src[src.index("multi-channel images"):src.index("layer normalisation (tfwrapper")]
    for word in ("2 <= Cx <= 16", "PHX_E_SHAPE", "BELIEVED, NOT EXECUTABLE HERE", "[N][X][Y][Cx]", "Cout in {1, 3, 4}"):
        assert word in sec, word
    sources = open(rt.HEADER.replace("include/phx.h", "phiseg_code_amd/csrc/SOURCES")).read().split()
    assert "multichannel.hip" in sources


def _png_decode(png):
    """the stored image of a PNG written with filter 0 on every row -> (array [H, W] or [H, W, C], colour type)"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(png):
        n, kind = struct.unpack(">I", png[pos:pos + 4])[0], png[pos + 4:pos + 8]
        data = png[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data) & 0xffffffff
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif kind == b"IDAT":
            idat += data
        pos += 12 + n
    w, h, depth, ctype = head[:4]
    assert depth == 8 and head[4:] == (0, 0, 0)
    c = {0: 1, 2: 3, 6: 4}[ctype]
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, w * c + 1)
    assert not raw[:, 0].any()                                   # filter type 0 on every scanline
    img = raw[:, 1:].reshape(h, w, c)
    return (img[:, :, 0] if c == 1 else img), ctype


@pytest.mark.parametrize("C,ctype", [(3, 2), (4, 6)])
def test_colour_png_and_summary_value_round_trip(tmp_path, C, ctype):
    rng = np.random.RandomState(C)
    img = rng.randint(0, 256, size=(7, 11, C)).astype(np.uint8)
    back, ct = _png_decode(S.png_encode(img))
    assert ct == ctype and np.array_equal(back, img)
    gray = img[:, :, 0]
    assert S.png_encode(gray) == S.png_encode_gray8(gray) == S.png_encode(gray[:, :, None])
    for bad in (np.zeros((4, 4, 2), np.uint8), np.zeros((4, 4, 5), np.uint8), np.zeros((0, 4, 3), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            S.png_encode(bad)
    w = S.EventFileWriter(str(tmp_path), wall_time=1.0)
    w.add_summary([S.image_value("colour/image/0", img), S.image_value("grey/image/0", gray)], 5, wall_time=2.0)
    w.close()
    ev = list(S.read_events(w.path))[1]
    colour, grey = ev["values"]
    assert colour["tag"] == "colour/image/0" and colour["image"]["colorspace"] == C
    assert (colour["image"]["height"], colour["image"]["width"]) == (7, 11)
    assert np.array_equal(_png_decode(colour["image"]["png"])[0], img)
    assert grey["image"]["colorspace"] == 1 and np.array_equal(_png_decode(grey["image"]["png"])[0], gray)


@pytest.mark.parametrize("C", [3, 4])
def test_colour_png_is_read_by_pillow(C):
    pil = pytest.importorskip("PIL.Image")
    import io
    img = np.random.RandomState(C).randint(0, 256, size=(7, 11, C)).astype(np.uint8)
    assert np.array_equal(np.asarray(pil.open(io.BytesIO(S.png_encode(img)))), img)


def test_synthetic_data_at_three_channels():
    c, cfg = config("tiny_phiseg_bn", 3)
    data = synthetic.SyntheticLIDC(c, seed=5, n_validation=3)
    x, s = data.train.next_batch(4)
    H = cfg["H"]
    assert x.shape == (4, H, H, 3) and x.dtype == np.float32 and s.shape == (4, H, H) and s.dtype == np.uint8
    assert data.validation.images.shape == (3, H, H, 3) and data.validation.labels.shape[:3] == (3, H, H)
    assert float(np.abs(x).max()) <= 0.5 and not np.array_equal(x[..., 0], x[..., 1])
    xp, sp = synthetic.philox_batch(3, 16, 2, seed=7, step=2, sample_offset=1, channels=3)
    x1, s1 = synthetic.philox_batch(3, 16, 2, seed=7, step=2, sample_offset=1)
    assert xp.shape == (3, 16, 16, 3) and np.array_equal(xp[..., :1], x1) and np.array_equal(sp, s1)
    assert not np.array_equal(xp[..., 1], xp[..., 0]) and not np.array_equal(xp[..., 2], xp[..., 1])
    assert float(np.abs(xp).max()) <= 0.5


def test_one_channel_synthetic_draws_have_not_moved():
    """make_batch and SyntheticLIDC at one channel: the arrays of the generator calls they always made, in their order, for a fixed seed"""
    size, nlabels, batch = 16, 3, 5
    rng = np.random.default_rng(11)
    x_want = (rng.random((batch, size, size, 1), dtype=np.float32) - 0.5).astype(np.float32)
    s_want = np.zeros((batch, size, size), dtype=np.uint8)
    yy, xx = np.mgrid[0:size, 0:size]
    for b in range(batch):
        if rng.random() < 0.25:
            continue
        cy, cx = rng.uniform(0.3125 * size, 0.6875 * size), rng.uniform(0.3125 * size, 0.6875 * size)
        ry, rx = rng.uniform(3, 20) * size / 128.0, rng.uniform(3, 20) * size / 128.0
        for k in range(1, nlabels):
            f = 1.0 - (k - 1) / float(max(nlabels - 1, 1))
            s_want[b][((yy - cy) / (ry * f)) ** 2 + ((xx - cx) / (rx * f)) ** 2 <= 1.0] = k
    x, s = synthetic.make_batch(batch, size, nlabels, np.random.default_rng(11))
    assert x.shape == (batch, size, size, 1) and np.array_equal(x, x_want) and np.array_equal(s, s_want)
    c, cfg = config("tiny_phiseg_bn", 1)
    data = synthetic.SyntheticLIDC(c, seed=11)
    want = synthetic.make_batch(batch, cfg["H"], cfg["nlabels"], np.random.default_rng(11))
    got = data.train.next_batch(batch)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    from phiseg_code_amd import philox_host
    u = philox_host.uniforms(7, 2, 1000 + 0 + 1, 16 * 16 + 8)
    xp, _ = synthetic.philox_batch(1, 16, 2, seed=7, step=2, sample_offset=1)
    assert xp.shape == (1, 16, 16, 1) and np.array_equal(xp[0, ..., 0], (u[:256] - 0.5).astype(np.float32).reshape(16, 16))
