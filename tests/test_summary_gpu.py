"""TensorBoard summaries on the device (csrc/summary.hip, phiseg_code_amd/summary.py) and train(summaries=True).

The histogram kernel is compared with a float64 numpy restatement of TensorFlow's bucket lookup (np.searchsorted(limits, v,
side='right') on the widened values), the grid kernel with a numpy restatement of put_kernels_on_grid's pad / reshape / transpose,
and a five-step training run's event file with what the model holds at those steps."""
import io
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests.helpers import load_golden
from tests.test_graph_cpu import make_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 63, 64, 65, 255, 4097, 70001)
# sum / sum_squares are double sums of n terms in an order that varies: |error| <= (n - 1) * 2^-53 * sum|x| to first order (Higham,
# Accuracy and Stability of Numerical Algorithms, eq. 4.4, any order); the squares add one rounding each (widened fp32 / bf16 squares
# are exact in double, the bound keeps the term anyway).  Taken for the longest segment, n = 70 001: 7.8e-12 -- the issue's 1e-12 is
# below what double accumulation guarantees at that length.  The reference sums are exact (math.fsum).
SUM_TOL = 70001 * 2.0 ** -53
SQ_TOL = 70002 * 2.0 ** -53


def _torch():
    import torch
    return torch


def _to_dev(a32, dtype):
    """float32 host array -> (device tensor in the storage dtype, the float64 values it holds)"""
    torch = _torch()
    t = torch.as_tensor(np.ascontiguousarray(a32, dtype=np.float32)).cuda()
    if dtype == "bf16":
        t = t.to(torch.bfloat16)
    return t, t.float().cpu().numpy().astype(np.float64)


def _ref(v64):
    from phiseg_code_amd import summary as S
    fin = v64[np.isfinite(v64)]
    counts = np.bincount(np.searchsorted(S.histogram_limits(), fin, side="right"), minlength=1551)
    return dict(counts=counts, num=fin.size, nonfinite=v64.size - fin.size, min=fin.min() if fin.size else 0.0, max=fin.max() if fin.size else 0.0,
                sum=math.fsum(fin), sq=math.fsum(fin * fin), abs=math.fsum(np.abs(fin)))


def _check(tag, counts, stats, ref):
    from phiseg_code_amd import summary as S
    assert counts.shape == (1551,) and counts.sum() == ref["num"], tag
    bad = np.nonzero(counts != ref["counts"])[0]
    assert bad.size == 0, "%s: buckets %s differ: got %s want %s" % (tag, bad[:6], counts[bad[:6]], ref["counts"][bad[:6]])
    assert stats[S.STAT_NUM] == ref["num"] and stats[S.STAT_NONFINITE] == ref["nonfinite"], tag
    assert stats[S.STAT_MIN] == ref["min"] and stats[S.STAT_MAX] == ref["max"], (tag, stats[:2], ref["min"], ref["max"])
    assert abs(stats[S.STAT_SUM] - ref["sum"]) <= SUM_TOL * ref["abs"], (tag, stats[S.STAT_SUM], ref["sum"])
    assert abs(stats[S.STAT_SUM_SQUARES] - ref["sq"]) <= SQ_TOL * ref["sq"], (tag, stats[S.STAT_SUM_SQUARES], ref["sq"])


def _contents(kind, n, rng):
    if kind == "normal":
        return rng.randn(n)
    if kind == "relu90":                                   # a post-ReLU tensor: 90 % exact zeros
        return np.where(rng.rand(n) < 0.9, 0.0, np.abs(rng.randn(n)))
    if kind == "negative":
        return -np.abs(rng.randn(n)) - 1e-3
    if kind == "extreme":                                  # beyond 1e20, below 1e-12, fp32 denormals, both signs
        mag = np.asarray([1e25, 3e38, 2e20, 1e-13, 1e-20, 1e-39, 1.4e-45, 1e-12, 1e20, 1.0])[rng.randint(0, 10, size=n)]
        return mag * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    if kind == "zeros":                                    # -0.0 and +0.0
        return np.where(rng.rand(n) < 0.5, -0.0, 0.0)
    raise ValueError(kind)


def _boundary(dtype):
    """For every third limit of the table: the storage-format numbers nearest the limit and their two neighbours, both signs --
    widened to double they fall on both sides of the double limit (and a few land on it exactly: 1e-12 * 1.1^k never, 0.0 does)."""
    torch = _torch()
    from phiseg_code_amd import summary as S
    lim = S.histogram_limits()[776:1550:3]
    if dtype == "f32":
        c = lim.astype(np.float32)
        v = np.concatenate([np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))])
    else:
        bits = torch.as_tensor(lim.astype(np.float32)).to(torch.bfloat16).view(torch.int16).numpy().astype(np.int32)
        allb = np.concatenate([bits - 1, bits, bits + 1]).astype(np.int16)
        v = torch.as_tensor(allb).view(torch.bfloat16).float().numpy()
    return np.concatenate([v, -v]).astype(np.float32)


@pytest.fixture(scope="module")
def mixed_call():
    """ONE phx_summary_histograms call over a mixed list: every length x content x dtype, the boundary values, a NaN + Inf segment,
    and three views that start 4, 8 and 12 bytes off a 16-byte boundary."""
    from phiseg_code_amd import runtime as rt
    from phiseg_code_amd import summary as S
    rng = np.random.RandomState(7)
    items = []
    for dtype in ("f32", "bf16"):
        for kind in ("normal", "relu90", "negative", "extreme", "zeros"):
            for n in LENGTHS:
                items.append(("%s/%s/%d" % (dtype, kind, n), _contents(kind, n, rng), dtype))
        items.append((dtype + "/boundary", _boundary(dtype), dtype))
        bad = rng.randn(300)
        bad[17], bad[201] = np.nan, -np.inf
        items.append((dtype + "/nonfinite", bad, dtype))
    keep, segs, refs = [], [], []
    for tag, a, dtype in items:
        t, v64 = _to_dev(a, dtype)
        keep.append(t)
        segs.append((t.data_ptr(), t.numel(), rt.F32 if dtype == "f32" else rt.BF16))
        refs.append((tag, _ref(v64)))
    base, v64 = _to_dev(rng.randn(5000) * np.where(rng.rand(5000) < 0.5, 0.0, 1.0), "f32")
    keep.append(base)
    for off in (1, 2, 3):
        segs.append((base.data_ptr() + 4 * off, 4099, rt.F32))
        refs.append(("f32/offset%d" % off, _ref(v64[off:off + 4099])))
    counts, stats = S.histograms(segs)
    return refs, counts, stats


def test_histograms_of_a_mixed_segment_list(mixed_call):
    refs, counts, stats = mixed_call
    assert counts.shape == (len(refs), 1551) and stats.shape == (len(refs), 8)
    for i, (tag, ref) in enumerate(refs):
        _check(tag, counts[i], stats[i], ref)


def test_boundary_values_straddle_their_limits(mixed_call):
    """the boundary segments do exercise both sides: neighbouring storage values of one limit land in different buckets"""
    refs, counts, _ = mixed_call
    for i, (tag, ref) in enumerate(refs):
        if tag.endswith("/boundary"):
            assert np.count_nonzero(ref["counts"]) > 500, tag
            assert np.array_equal(counts[i], ref["counts"])


def test_nonfinite_values_are_counted_apart(mixed_call):
    from phiseg_code_amd import summary as S
    refs, counts, stats = mixed_call
    for i, (tag, ref) in enumerate(refs):
        if tag.endswith("/nonfinite"):
            assert stats[i][S.STAT_NONFINITE] == 2 and counts[i].sum() == 298 and stats[i][S.STAT_NUM] == 298
            with pytest.raises(FloatingPointError, match="some/tag"):
                S.check_finite(["some/tag"], stats[i:i + 1])


@pytest.mark.parametrize("nseg", [1, 300])
def test_segment_list_lengths(nseg):
    from phiseg_code_amd import runtime as rt
    from phiseg_code_amd import summary as S
    rng = np.random.RandomState(nseg)
    base, v64 = _to_dev(rng.randn(64 * 1024) * 3.0, "f32")
    segs, refs = [], []
    for i in range(nseg):
        off, n = 4 * ((i * 211) % 8000), 1 + (i * 37) % 500 if nseg > 1 else 20000
        segs.append((base.data_ptr() + 4 * off, n, rt.F32))
        refs.append(_ref(v64[off:off + n]))
    counts, stats = S.histograms(segs)
    for i in range(nseg):
        _check("seg%d" % i, counts[i], stats[i], refs[i])


# ---- the grid kernel ------------------------------------------------------------------------------------------------------------
def _ref_grid(vals):
    """put_kernels_on_grid's 'image' branch for displayed values vals [B, H, W] float32 (fp32 arithmetic, truncation; NaN -> 0 and
    saturation where the cast is undefined), then its pad / reshape / transpose."""
    from phiseg_code_amd import summary as S
    B, H, W = vals.shape
    gy, gx = S.factorization(B)
    v = vals.astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = (v - v.min()) / v.max()
        f = f * np.float32(254.0)
    assert f.dtype == np.float32
    u8 = np.where(np.isnan(f), np.float32(0), np.clip(f, 0, 255)).astype(np.uint8)
    x = np.pad(u8[..., None], [[0, 0], [1, 1], [1, 1], [0, 0]], mode="constant")
    Y, X = H + 2, W + 2
    x = x.reshape(gx, Y * gy, X, 1).transpose(0, 2, 1, 3).reshape(1, X * gx, Y * gy, 1).transpose(0, 2, 1, 3)
    return x, f


def _grid(a, form, B, H, W, C, shift=0):
    torch = _torch()
    from phiseg_code_amd import summary as S
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    st = torch.cuda.current_stream()
    out = S.grid_u8_device(t.data_ptr(), form, B, H, W, C, st.cuda_stream, shift=shift)
    st.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("hw", [(8, 8), (5, 7)])
@pytest.mark.parametrize("B", [1, 2, 6, 12])
def test_grid_of_every_input_form(B, hw):
    from phiseg_code_amd import summary as S
    H, W = hw
    rng = np.random.RandomState(B * 100 + H)
    gy, gx = S.factorization(B)
    for C in (2, 4):                                       # logits drawn from three values: ties everywhere, the first maximum wins
        lg = rng.randint(0, 3, size=(B, H, W, C)).astype(np.float32)
        lg[0, 0, 0, :] = [5.0] + [0.0] * (C - 1)           # class 0 and class C - 1 both occur: min 0, max C - 1 > 0
        lg[0, 0, 1, :] = [0.0] * (C - 1) + [5.0]
        want, f = _ref_grid(np.argmax(lg, axis=-1).astype(np.float32))
        assert f.min() >= 0 and f.max() <= 254
        got = _grid(lg, S.GRID_LOGITS_F32, B, H, W, C)
        assert got.shape == ((H + 2) * gy, (W + 2) * gx)
        assert np.array_equal(got, want[0, :, :, 0]), "logits C=%d" % C
    lab = rng.randint(0, 4, size=(B, H, W)).astype(np.uint8)
    lab[0, 0, 0], lab[0, 0, 1] = 0, 3
    want, f = _ref_grid(lab.astype(np.float32))
    assert f.min() >= 0 and f.max() <= 254
    assert np.array_equal(_grid(lab, S.GRID_LABELS_U8, B, H, W, 1), want[0, :, :, 0])
    img = rng.rand(B, H, W, 1).astype(np.float32) + 0.25
    want, f = _ref_grid(img[..., 0])
    assert f.min() >= 0 and f.max() <= 254 and img.max() > 0
    assert np.array_equal(_grid(img, S.GRID_IMAGE_F32, B, H, W, 1), want[0, :, :, 0])
    # through the reference's name and signature
    from phiseg_code_amd.tfwrapper import utils as tfutils
    assert np.array_equal(tfutils.put_kernels_on_grid(img, B), want)


def test_grid_where_the_cast_is_undefined():
    """all-background labels: 0 / 0 = NaN -> 0; an image whose maximum is negative: (v - min) / max <= 0 -> 0; an image whose minimum is
    negative and whose maximum is small: values above 255 saturate.  (tf.cast(float -> uint8) is undefined for all three: a deliberate
    choice)"""
    from phiseg_code_amd import summary as S
    B, H, W = 2, 5, 7
    got = _grid(np.zeros((B, H, W), dtype=np.uint8), S.GRID_LABELS_U8, B, H, W, 1)
    assert got.shape == (H + 2, (W + 2) * 2) and not got.any()
    rng = np.random.RandomState(3)
    neg = (-1.0 - rng.rand(B, H, W)).astype(np.float32)
    want, f = _ref_grid(neg)
    assert f.max() <= 0
    got = _grid(neg, S.GRID_IMAGE_F32, B, H, W, 1)
    assert np.array_equal(got, want[0, :, :, 0]) and not got.any()
    sat = (rng.rand(B, H, W) * 1.5 - 1.0).astype(np.float32)
    want, f = _ref_grid(sat)
    assert f.max() > 255 and sat.max() > 0
    got = _grid(sat, S.GRID_IMAGE_F32, B, H, W, 1)
    assert np.array_equal(got, want[0, :, :, 0]) and got.max() == 255


def test_grid_of_a_nearest_neighbour_view():
    """the coarse output levels are stored at (H >> shift) x (W >> shift) and displayed at H x W"""
    from phiseg_code_amd import summary as S
    B, H, W, C = 6, 8, 12, 3
    rng = np.random.RandomState(11)
    small = rng.randn(B, H // 4, W // 4, C).astype(np.float32)
    small[0, 0, 0], small[0, 0, 1] = [9, 0, 0], [0, 0, 9]
    full = np.repeat(np.repeat(small, 4, axis=1), 4, axis=2)
    want, _ = _ref_grid(np.argmax(full, axis=-1).astype(np.float32))
    assert np.array_equal(_grid(small, S.GRID_LOGITS_F32, B, H, W, C, shift=2), want[0, :, :, 0])


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _cfg(dtype="f32"):
    g, cfg, _ = load_golden("tiny_phiseg_bn")
    c = make_config(cfg, dtype)
    c.batch_size = 2
    c.validation_frequency = 2
    c.tensorboard_update_frequency = 2
    c.do_image_summaries = True
    c.validation_samples = 4
    c.num_validation_images = 2
    c.annotator_range = range(4)
    c.lr_schedule_dict = {0: 1e-3, 3: 5e-4}
    return c


def _data(cfg, seed=1234):
    from phiseg_code_amd.data import synthetic
    return synthetic.SyntheticLIDC(cfg, seed=seed, n_validation=3)


def _events(log_dir):
    from phiseg_code_amd import summary as S
    files = [f for f in os.listdir(log_dir) if f.startswith("events.out.tfevents.")]
    assert len(files) == 1, files
    return list(S.read_events(os.path.join(log_dir, files[0])))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = _cfg()
    model = phiseg_model.phiseg(cfg)
    model.keep_checkpoint_every_n_hours = 0.0              # keep model.ckpt-0 / -2 / -4: the variables as they were at each summary
    log_dir = str(tmp_path_factory.mktemp("summaries") / "run")
    losses = model.train(_data(cfg), num_iter=5, log_every=0, log_dir=log_dir, summaries=True)
    return types.SimpleNamespace(cfg=cfg, model=model, log_dir=log_dir, losses=losses, events=_events(log_dir))


def _by_kind(ev):
    sc = {v["tag"]: v["simple_value"] for v in ev["values"] if "simple_value" in v}
    hi = {v["tag"]: v["histo"] for v in ev["values"] if "histo" in v}
    im = {v["tag"]: v["image"] for v in ev["values"] if "image" in v}
    return sc, hi, im


def test_training_summaries_at_every_update_step(run):
    from PIL import Image
    from phiseg_code_amd import summary as S
    m, cfg = run.model, run.cfg
    L, B, H = cfg.latent_levels, cfg.batch_size, cfg.image_size[0]
    assert run.events[0]["file_version"] == "brain.Event:2"
    train_ev = [e for e in run.events if any(v.get("tag") == "batch_total_loss" for v in e["values"])]
    assert [e["step"] for e in train_ev] == [0, 2, 4]
    want_scalars = {"batch_total_loss", "learning_rate"} | {"average_%s_lvl%d" % (k, i) for k in ("mu", "sigma", "prior_mu", "prior_sigma")
                                                            for i in range(L)}
    var_tags = {n + "_0" for n, v in m.graph.variables.items() if n.endswith("/W") or n.endswith("/b")}
    units = m._summary_spec()["units"]
    act_tags = {tag for tag, _ in units}
    assert len(act_tags) == len(units) > 10 and all(t.endswith("/activations") for t in act_tags)
    want_images = {"train_%s/image/0" % n for n in ["x_inp", "s_inp", "s_out"] + ["s_out_list_%d" % i for i in range(L)] +
                   ["s_accum_list_%d" % i for i in range(L)]}
    gy, gx = S.factorization(B)
    for e in train_ev:
        sc, hi, im = _by_kind(e)
        assert set(sc) == want_scalars
        assert set(hi) == var_tags | act_tags
        assert set(im) == want_images
        lr = 1e-3 if e["step"] < 3 else 5e-4
        assert sc["learning_rate"] == float(np.float32(lr))
        assert np.isfinite(sc["batch_total_loss"]) and sc["average_sigma_lvl0"] > 0
        ck = np.load(os.path.join(run.log_dir, "model.ckpt-%d.npz" % e["step"]))
        for tag in var_tags:                               # every filter / bias histogram = the numpy histogram of the variable at this step
            v = ck[tag[:-2]].astype(np.float64).reshape(-1)
            h = hi[tag]
            want = np.bincount(np.searchsorted(S.histogram_limits(), v, side="right"), minlength=1551)
            assert np.array_equal(S.expand_buckets(h), want), tag
            assert h["num"] == v.size and h["min"] == v.min() and h["max"] == v.max(), tag
            assert abs(h["sum"] - math.fsum(v)) <= SUM_TOL * math.fsum(np.abs(v)) and sum(h["bucket"]) == v.size, tag
        for tag, t in units:                               # every activation histogram counts the unit's whole output
            n = B * int(np.prod(t.shape[1:]))
            assert hi[tag]["num"] == n and sum(hi[tag]["bucket"]) == n, tag
        for tag, image in im.items():
            a = np.asarray(Image.open(io.BytesIO(image["png"])))
            assert a.shape == ((H + 2) * gy, (H + 2) * gx) == (image["height"], image["width"]) and a.dtype == np.uint8, tag


def test_validation_summaries(run):
    cfg, m = run.cfg, run.model
    L = cfg.latent_levels
    val_ev = [e for e in run.events if any(v.get("tag") == "validation_GED" for v in e["values"])]
    assert [e["step"] for e in val_ev] == [0, 2, 4]
    want = {"val_batch_%s" % n for n in m.loss_dict} | {"validation_dice_tot_score", "validation_dice_mean_score", "validation_neg_elbo",
                                                         "validation_GED", "validation_NCC"}
    names = ["x_inp", "s_inp", "s_out"] + ["s_out_list_%d" % i for i in range(L)] + ["s_accum_list_%d" % i for i in range(L)]
    want_images = {"val_%s/image/0" % n for n in names} | {"generated_seg/image/0", "generated_x_in/image/0"}
    for e in val_ev:
        sc, hi, im = _by_kind(e)
        assert want <= set(sc) and not hi
        lbl = sorted(t for t in sc if t.startswith("validation_dice_lbl_"))
        assert lbl and lbl[0] == "validation_dice_lbl_0" and set(sc) == want | set(lbl)
        assert all(np.isfinite(v) for v in sc.values())
        assert set(im) == want_images
    tr_ev = [e for e in run.events if any(v.get("tag") == "train_batch_total_loss" for v in e["values"])]
    assert [e["step"] for e in tr_ev] == [0, 2, 4]
    for e in tr_ev:
        assert {v["tag"] for v in e["values"]} == {"train_batch_%s" % n for n in m.loss_dict}


def test_summaries_off_writes_no_event_file(tmp_path):
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = _cfg()
    model = phiseg_model.phiseg(cfg)
    log_dir = str(tmp_path / "run")
    model.train(_data(cfg), num_iter=3, log_every=0, log_dir=log_dir)
    assert not [f for f in os.listdir(log_dir) if "tfevents" in f]
    assert getattr(model, "_summary_spec_cache", None) is None           # and no summary plan was compiled


def test_losses_are_bit_identical_with_and_without_summaries(tmp_path):
    """PHX_DETERMINISTIC=1 (read once per process: a fresh one): the same five steps with summaries=True and with summaries=False
    return the same losses bit for bit, and leave the same parameters, moving statistics and optimiser step."""
    env = dict(os.environ, PYTHONPATH=ROOT, PHX_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "summary_worker.py"), str(tmp_path)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = {l.split()[1]: l.split()[2:] for l in r.stdout.splitlines() if l.startswith("RUN ")}
    assert set(lines) == {"on", "off"} and len(lines["on"]) == 5 + 1
    assert lines["on"] == lines["off"], lines
    assert [f for f in os.listdir(str(tmp_path / "on")) if "tfevents" in f] and not [f for f in os.listdir(str(tmp_path / "off")) if "tfevents" in f]


def test_bf16_plan_buffers():
    """one summary write of a bf16 model: the activation segments are the plan's own bf16 buffers"""
    from phiseg_code_amd import runtime as rt
    from phiseg_code_amd import summary as S
    from phiseg_code_amd.phiseg import phiseg_model
    cfg = _cfg("bf16")
    model = phiseg_model.phiseg(cfg)
    d = _data(cfg)
    x, s = d.train.next_batch(cfg.batch_size)
    model.sess.run([model.train_step, model.loss_tot], {model.x_inp: x, model.s_inp: s, model.training_pl: True, model.lr_pl: 1e-3})
    loss, hist, grids = model._summary_run(x, s, 1e-3, histograms=True)
    spec = model._summary_spec()
    plan = [p for p in model.sess.plans.values() if id(p) in spec["hist"]][0]
    dts = [plan.val[t].dt for _, t in spec["units"]]
    assert rt.BF16 in dts and rt.F32 in dts                # the relu units are bf16, the mu / sigma / logit heads fp32
    tags, counts, stats = hist["act"]
    for i, (tag, t) in enumerate(spec["units"]):
        b = plan.val[t]
        n = cfg.batch_size * int(np.prod(t.shape[1:]))
        assert stats[i][S.STAT_NUM] == n and counts[i].sum() == n, tag
        v = b.numpy().astype(np.float64).reshape(-1)       # the buffer as the plan left it
        assert np.array_equal(counts[i], np.bincount(np.searchsorted(S.histogram_limits(), v, side="right"), minlength=1551)), tag
        assert stats[i][S.STAT_MIN] == v.min() and stats[i][S.STAT_MAX] == v.max(), tag
    assert np.isfinite(loss) and len(grids) == 3 + 2 * cfg.latent_levels
