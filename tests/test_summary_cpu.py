"""The host side of the TensorBoard summaries (phiseg_code_amd/summary.py): TensorFlow's default histogram limits, the event-file
writer and its reader, HistogramProto's run-length collapse, and the zlib-only PNG encoder.  Needs the built library for the CRC
only, as the checkpoint tests do."""
import io
import os
import sys

import numpy as np
import pytest

from phiseg_code_amd import summary as S


def test_limits_table():
    lim = S.histogram_limits()
    assert lim.dtype == np.float64 and lim.shape == (1551,)
    assert np.all(np.diff(lim) > 0)
    assert lim[775] == 0.0 and np.array_equal(lim[:775], -lim[:775:-1])       # symmetric about the 0.0 in the middle
    assert lim[-1] == sys.float_info.max
    assert lim[776] == 1e-12
    for i in range(777, 1550):                                                  # each positive entry = its predecessor * 1.1, in double
        assert lim[i] == lim[i - 1] * 1.1, i
    assert lim[1549] < 1e20 <= lim[1549] * 1.1


def _write(tmp_path):
    img = (np.arange(5 * 7, dtype=np.uint32) * 7 % 256).astype(np.uint8).reshape(5, 7)
    counts = np.zeros(1551, dtype=np.int64)
    counts[[3, 776, 777, 900, 1550]] = [2, 90, 1, 4, 3]
    w = S.EventFileWriter(str(tmp_path), wall_time=1234.5)
    w.add_summary([S.scalar_value("batch_total_loss", 3.25), S.scalar_value("learning_rate", 1e-3)], 0, wall_time=1235.0)
    w.add_summary([S.histogram_value("enc/W_0", -2.0, 7.5, 100, 12.5, 99.0, counts), S.image_value("train_x_inp/image/0", img)], 7)
    w.flush()
    w.close()
    return w.path, img, counts


def test_writer_reader_round_trip(tmp_path):
    path, img, counts = _write(tmp_path)
    name = os.path.basename(path)
    assert name.startswith("events.out.tfevents.0000001234.") and len(name) > len("events.out.tfevents.0000001234.")
    assert os.listdir(str(tmp_path)) == [name]
    ev = list(S.read_events(path))
    assert len(ev) == 3
    assert ev[0]["file_version"] == "brain.Event:2" and ev[0]["wall_time"] == 1234.5 and ev[0]["values"] == []
    assert ev[1]["step"] == 0 and ev[1]["wall_time"] == 1235.0
    assert [(v["tag"], v["simple_value"]) for v in ev[1]["values"]] == [("batch_total_loss", 3.25), ("learning_rate", float(np.float32(1e-3)))]
    assert ev[2]["step"] == 7
    h, im = ev[2]["values"]
    assert h["tag"] == "enc/W_0"
    hp = h["histo"]
    assert (hp["min"], hp["max"], hp["num"], hp["sum"], hp["sum_squares"]) == (-2.0, 7.5, 100.0, 12.5, 99.0)
    assert np.array_equal(S.expand_buckets(hp), counts)
    assert im["tag"] == "train_x_inp/image/0" and (im["image"]["height"], im["image"]["width"], im["image"]["colorspace"]) == (5, 7, 1)
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(im["image"]["png"]))), img)


def test_flipped_payload_byte_fails_the_crc(tmp_path):
    path, _, _ = _write(tmp_path)
    raw = bytearray(open(path, "rb").read())
    first = 12 + int.from_bytes(raw[:8], "little") + 4                      # the second record starts here
    for at in (first + 12 + 3, first + 2):                                  # a payload byte, a length byte
        bad = bytearray(raw)
        bad[at] ^= 0x10
        p2 = str(tmp_path / ("bad%d" % at))
        open(p2, "wb").write(bytes(bad))
        with pytest.raises(ValueError):
            list(S.read_events(p2))
    assert len(list(S.read_events(path))) == 3


def test_histogram_encoding_collapses_empty_runs():
    lim = S.histogram_limits()
    counts = np.zeros(1551, dtype=np.int64)
    counts[[10, 11, 776, 1000]] = [5, 1, 40, 2]
    bl, bc = S.collapse_buckets(counts)
    # runs of empties 0..9, 12..775, 777..999, 1001..1550 -> one entry each, carrying the run's LAST limit
    assert bc == [0.0, 5.0, 1.0, 0.0, 40.0, 0.0, 2.0, 0.0]
    assert bl == [lim[9], lim[10], lim[11], lim[775], lim[776], lim[999], lim[1000], lim[1550]]
    assert sum(bc) == counts.sum()
    # nothing to collapse at either end; an all-empty histogram is one entry
    counts[:] = 0
    counts[[0, 1550]] = [1, 1]
    bl, bc = S.collapse_buckets(counts)
    assert bc == [1.0, 0.0, 1.0] and bl == [lim[0], lim[1549], lim[1550]]
    bl, bc = S.collapse_buckets(np.zeros(1551))
    assert bc == [0.0] and bl == [lim[1550]]


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (20, 33), (3, 256)])
def test_png_decodes_to_what_was_encoded(shape):
    from PIL import Image
    rng = np.random.RandomState(shape[0] * 1000 + shape[1])
    a = rng.randint(0, 256, size=shape).astype(np.uint8)
    im = Image.open(io.BytesIO(S.png_encode_gray8(a)))
    assert im.mode == "L" and im.size == (shape[1], shape[0])
    assert np.array_equal(np.asarray(im), a)


def test_factorization_is_the_reference_grid():
    assert [S.factorization(n) for n in (1, 2, 6, 12, 64, 7)] == [(1, 1), (1, 2), (2, 3), (3, 4), (8, 8), (1, 7)]
