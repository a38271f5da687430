"""The small kernels that run between the convolutions of every step -- csrc/elementwise.hip, the scalar and masked kernels of
csrc/losses_opt.hip, k_softmax_xent_map (csrc/mc_stats.hip), the channel pad / unpad pair (csrc/conv_mfma.hip) -- through the C ABI at
the edges the whole-model tests and the friendly shapes of tests/test_kernels_gpu.py never reach: every dtype instantiation, the scalar
and the 16-byte paths, NULL outputs, the second trip of every block-stride loop, and the grid-stride step behind the block cap of
phx_grid_for (A-G, L), the masked weight-decay pair on arena sizes around its 256 x 256 grid (H), the scalar sums (I), the per-pixel
cross-entropy map (J), the part of phx_residual_ce's contract no other test exercises: ds levels nullable one by one, shift lists
other than 0 .. L-1, eight levels (K), Adam on arenas shorter than one float4 (M), and the host-side entry points -- copies, events,
queries, the clock stamp -- that nothing called by name (N).

References are plain torch / numpy float64 on the operands as stored (rounded to their storage type first).  Bounds are those of
tests/test_kernels_gpu.py: exact for whatever only moves or converts data, 1e-5 relative to the largest reference value for fp32
arithmetic, 2^-8 for a result stored in bf16; the sums of H and I have bounds derived in their tests.  Every output buffer starts
NaN- or sentinel-filled and carries TAIL sentinel elements past its end that must survive.  Every check prints
`GLUE <group> <what> <error / bound>` before it asserts (pytest -s shows them)."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

from oracle import philox
from oracle import tf1_ops as T
from phiseg_code_amd import runtime as rt
from tests.det_kernels_worker import RESIDUAL_CE_CONTRACT, residual_ce_contract
from tests.test_kernels_gpu import BF16, F32, L, S, close, dev, host, rounded, tdt  # noqa: F401 (L: the fixture)

pytestmark = pytest.mark.gpu

CAP = 4096 * 256             # phx_grid_for(n, 256): items of one grid-stride trip behind its default cap of 4096 blocks
CAP_8192 = 8192 * 256        # phx_grid_for(n, 256, 8192): pad_channels / unpad_channels (and adam_tf1, in float4 items)
CAP_2048 = 2048 * 256        # phx_grid_for(n, 256, 2048): axpy_masked
TAIL = 64                    # sentinel elements past the end of every output buffer
NAN = float("nan")
U = 2.0 ** -24               # unit round-off of fp32
TOL = {F32: 1e-5, BF16: 2.0 ** -8}


def _header_constants():
    """PHX_* enumerators as include/phx.h states them (act codes, error codes): read, not guessed"""
    src = re.sub(r"/\*.*?\*/", "", open(rt.HEADER).read(), flags=re.S)
    return {k: int(v) for k, v in re.findall(r"\b(PHX_[A-Z0-9_]+)\s*=\s*(-?\d+)", src)}


H = _header_constants()
ACTS = {"identity": H["PHX_ACT_ID"], "relu": H["PHX_ACT_RELU"], "softplus": H["PHX_ACT_SOFTPLUS"]}
assert (H["PHX_F32"], H["PHX_BF16"]) == (F32, BF16)


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def buf(n, dtype=torch.float32, fill=NAN):
    """an output buffer of n elements + TAIL sentinels, all `fill`"""
    return torch.full((n + TAIL,), fill, dtype=dtype, device="cuda")


def tail_kept(t, n, fill=NAN):
    torch.cuda.synchronize()
    tail = t[n:]
    assert tail.numel() >= TAIL
    ok = torch.isnan(tail).all() if fill != fill else (tail == fill).all()
    assert bool(ok), "the kernel wrote past the end of its output"


def report(group, what, err, bound):
    print("GLUE %s %s err=%.3e bound=%.3e frac=%.4f" % (group, what, err, bound, err / bound if bound > 0 else (0.0 if err == 0 else np.inf)))
    assert err <= bound, "%s %s: error %.3e > bound %.3e" % (group, what, err, bound)


def rel_to_max(group, what, got, ref, rel):
    """the metric of tests/test_kernels_gpu.close: max abs error over max abs reference"""
    got, ref = got.double(), ref.double()
    assert not bool(torch.isnan(got).any()), "%s %s: NaN left in the output" % (group, what)
    scale = max(float(ref.abs().max()), 1e-30)
    report(group, what, float((got - ref).abs().max()) / scale, rel)


def exact(group, what, got, ref):
    print("GLUE %s %s exact" % (group, what))
    assert got.dtype == ref.dtype and torch.equal(got, ref), "%s %s: not bit-for-bit" % (group, what)


def refused(code, fn, *args):
    """the call comes back with the error code `code` of include/phx.h (the binding raises PhxError with it); nothing is launched"""
    with pytest.raises(rt.PhxError, match=r"\(%d\)" % H[code]):
        fn(*args)


# ---- A. phx_act_bwd: dpre = dy * act'(y) from the stored OUTPUT ---------------------------------------------------------------------
def _act_y(n, y_dt, g):
    """+0, -0, the smallest positive fp32 denormal / bf16 denormal / normal value, then soft-plus outputs of pre-activations over
    [-10, 25] (both sides of the kernel's `v > 20` shortcut); the specials stand at both ends, so every grid-stride trip meets some"""
    special = torch.tensor([0.0, -0.0, 2.0 ** -149, 2.0 ** -133, 2.0 ** -126], dtype=torch.float64)
    pre = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 35.0 - 10.0
    if n >= 2:
        pre[0], pre[-1] = -10.0, 25.0
    y = torch.nn.functional.softplus(pre).float()
    k = min(n, special.numel())
    y[:k] = special[:k].float().cuda()
    if n >= 16:
        y[-8:-3] = special.float().cuda()
    return y.to(tdt(y_dt)).contiguous()


@pytest.mark.parametrize("act", ["relu", "softplus", "identity"])
@pytest.mark.parametrize("y_dt", [F32, BF16])
@pytest.mark.parametrize("d_dt", [F32, BF16])
def test_act_bwd_every_instantiation_and_the_grid_stride_trip(L, d_dt, y_dt, act):
    g = gen(100 + 10 * d_dt + y_dt)
    for n in (1, 255, 257, CAP + 3):
        y = _act_y(n, y_dt, g)
        dy = torch.randn(n, generator=g, device="cuda").to(tdt(d_dt)).contiguous()
        out = buf(n, tdt(d_dt))
        L.act_bwd(dy.data_ptr(), d_dt, y.data_ptr(), y_dt, out.data_ptr(), d_dt, n, ACTS[act], S())
        tail_kept(out, n)
        y64, dy64 = y.double(), dy.double()
        what = "%s dy=%d y=%d n=%d" % (act, d_dt, y_dt, n)
        if act == "softplus":
            rel_to_max("A", what, out[:n], dy64 * (1.0 - torch.exp(-y64)), TOL[d_dt])
        else:                    # a product with 1 or 0: nothing is rounded
            ref = dy64 * (y64 > 0).double() if act == "relu" else dy64
            exact("A", what, out[:n], ref.to(tdt(d_dt)))


def test_act_bwd_refusals(L):
    t = torch.zeros(8, device="cuda")
    out = buf(8)
    refused("PHX_E_INVAL", L.act_bwd, t.data_ptr(), F32, t.data_ptr(), F32, out.data_ptr(), BF16, 8, ACTS["relu"], S())
    refused("PHX_E_INVAL", L.act_bwd, t.data_ptr(), BF16, t.data_ptr(), F32, out.data_ptr(), F32, 8, ACTS["relu"], S())
    refused("PHX_E_INVAL", L.act_bwd, t.data_ptr(), 7, t.data_ptr(), F32, out.data_ptr(), 7, 8, ACTS["relu"], S())
    refused("PHX_E_INVAL", L.act_bwd, t.data_ptr(), F32, t.data_ptr(), 7, out.data_ptr(), F32, 8, ACTS["relu"], S())
    tail_kept(out, 0)


# ---- B. phx_cast ----------------------------------------------------------------------------------------------------------------------
# fp32 bit patterns: round-to-nearest-even ties towards the even neighbour below (0x3F808000 -> 0x3F80) and above (0x3F818000 -> 0x3F82),
# both signs, one bit to either side of a tie, denormals (a tie among them), +-0, +-inf, the largest finite fp32 (-> +inf in bf16), the
# largest value that stays finite, quiet and signalling NaNs of both signs (0x7F800001: a truncating cast would turn it into +inf)
CAST_F32_BITS = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,
                 0x00000001, 0x007FFFFF, 0x80000001, 0x00008000, 0x00018000, 0x00017FFF, 0x00000000, 0x80000000,
                 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001]
CAST_BF16_BITS = [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x0080, 0x3F80, 0xBF80, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81]


def _cast_source(n, dt, rng):
    """n elements of random bit patterns (every exponent, NaNs included) and ordinary values, the hand-made vector at both ends"""
    if dt == F32:
        bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        bits[::2] = rng.standard_normal((n + 1) // 2).astype(np.float32).view(np.uint32)
        hand = np.array(CAST_F32_BITS, dtype=np.uint32)
    else:
        bits = rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
        hand = np.array(CAST_BF16_BITS, dtype=np.uint16)
    k = min(n, hand.size)
    bits[:k] = hand[:k]
    if n >= 2 * hand.size:
        bits[-hand.size:] = hand
    t = torch.from_numpy(bits.view(np.int32 if dt == F32 else np.int16).copy())
    return t.view(tdt(dt))


@pytest.mark.parametrize("dst_dt", [F32, BF16])
@pytest.mark.parametrize("src_dt", [F32, BF16])
def test_cast_bit_for_bit(L, src_dt, dst_dt):
    rng = np.random.default_rng([31, src_dt, dst_dt])
    ibits = {F32: torch.int32, BF16: torch.int16}
    for n in (1, 257, CAP + 5, len(CAST_F32_BITS)):
        src = _cast_source(n, src_dt, rng)
        ref = src.to(tdt(dst_dt))                                   # torch on the CPU: round to nearest even
        srcd = src.cuda()
        out = buf(n, tdt(dst_dt), fill=3.0)
        L.cast(srcd.data_ptr(), src_dt, out.data_ptr(), dst_dt, n, S())
        tail_kept(out, n, fill=3.0)
        got = out[:n].cpu()
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(got), nan), "cast %d -> %d, n = %d: a NaN did not stay NaN (or one appeared)" % (src_dt, dst_dt, n)
        gb, rb = got.view(ibits[dst_dt]), ref.view(ibits[dst_dt])
        exact("B", "%d->%d n=%d" % (src_dt, dst_dt, n), gb[~nan], rb[~nan])
    if (src_dt, dst_dt) == (F32, BF16):                               # the reference itself does what the comment above says
        hand = _cast_source(len(CAST_F32_BITS), F32, rng).to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint16)
        assert list(hand[:4]) == [0x3F80, 0x3F82, 0xBF80, 0xBF82] and hand[18] == 0x7F80 and hand[19] == 0xFF80 and hand[20] == 0x7F7F


def test_cast_refuses_an_unknown_dtype(L):
    t, out = torch.zeros(8, device="cuda"), buf(8)
    refused("PHX_E_INVAL", L.cast, t.data_ptr(), 7, out.data_ptr(), F32, 8, S())
    refused("PHX_E_INVAL", L.cast, t.data_ptr(), F32, out.data_ptr(), 7, 8, S())
    tail_kept(out, 0)


# ---- C. phx_concat2 / phx_split2 ------------------------------------------------------------------------------------------------------
def _concat_case(L, Ca, Cb, dt, npix):
    """values that name their position (a >= 0, b < 0, both exact in bf16): concat against torch.cat; split2 into both outputs, then
    with a = NULL and with b = NULL -- the other output exact, its sentinels and the input untouched"""
    ia, ib = torch.arange(npix * Ca, device="cuda"), torch.arange(npix * Cb, device="cuda")
    a = (ia % 251).to(tdt(dt)).reshape(npix, Ca)
    b = (-(ib % 241) - 1).to(tdt(dt)).reshape(npix, Cb)
    C, what = Ca + Cb, "(%d,%d) dt=%d npix=%d" % (Ca, Cb, dt, npix)
    out = buf(npix * C, tdt(dt))
    L.concat2(a.data_ptr(), Ca, b.data_ptr(), Cb, out.data_ptr(), npix, dt, S())
    tail_kept(out, npix * C)
    cat = torch.cat([a, b], dim=1)
    exact("C", "concat2 " + what, out[:npix * C].reshape(npix, C), cat)
    for (wa, wb) in ((True, True), (False, True), (True, False)):
        keep = cat.clone()
        a2, b2 = buf(npix * Ca, tdt(dt)), buf(npix * Cb, tdt(dt))
        L.split2(cat.data_ptr(), a2.data_ptr() if wa else None, Ca, b2.data_ptr() if wb else None, Cb, npix, dt, S())
        tail_kept(a2, npix * Ca if wa else 0)
        tail_kept(b2, npix * Cb if wb else 0)
        if wa:
            exact("C", "split2 a %s (b %s)" % (what, "too" if wb else "NULL"), a2[:npix * Ca].reshape(npix, Ca), a)
        if wb:
            exact("C", "split2 b %s (a %s)" % (what, "too" if wa else "NULL"), b2[:npix * Cb].reshape(npix, Cb), b)
        assert torch.equal(cat, keep), "split2 changed its input"


@pytest.mark.parametrize("Ca,Cb,dt", [(4, 4, BF16), (8, 3, BF16), (3, 8, BF16), (1, 1, BF16), (16, 4, BF16),        # k_concat2<bf16_t>
                                      (4, 3, F32), (3, 4, F32), (5, 1, F32),                                          # k_concat2<float>
                                      (8, 8, BF16), (8, 24, BF16), (4, 8, F32), (16, 8, BF16), (8, 4, F32)])          # 16-byte chunks, one and two per pixel of a
def test_concat_split_scalar_and_vector_paths(L, Ca, Cb, dt):
    for npix in (1, 37, 300):
        _concat_case(L, Ca, Cb, dt, npix)


@pytest.mark.parametrize("Ca,Cb,dt,npix", [(1, 1, BF16, CAP // 2 + 3), (5, 1, F32, CAP // 6 + 3),                     # scalar: npix * C items
                                           (8, 8, BF16, CAP // 2 + 3), (4, 8, F32, CAP // 3 + 3)])                    # 16-byte: npix * C / per16
def test_concat_split_above_the_grid_cap(L, Ca, Cb, dt, npix):
    per = 1 if (Ca % (16 // rt.DT_SIZE[dt]) or Cb % (16 // rt.DT_SIZE[dt])) else 16 // rt.DT_SIZE[dt]
    assert npix * (Ca + Cb) // per > CAP
    _concat_case(L, Ca, Cb, dt, npix)


# ---- D. phx_broadcast_pixels_fwd/bwd, phx_global_avgpool_fwd/bwd ------------------------------------------------------------------------
def _bcast_gap_case(L, B, P, C, g):
    what = "B=%d P=%d C=%d" % (B, P, C)
    z = torch.randn(B, C, generator=g, device="cuda")
    exp = z[:, None, :].expand(B, P, C)
    fwd = {}
    for dt in (F32, BF16):
        out = buf(B * P * C, tdt(dt))
        L.broadcast_pixels_fwd(z.data_ptr(), out.data_ptr(), dt, B, P, C, S())
        tail_kept(out, B * P * C)
        fwd[dt] = out[:B * P * C].reshape(B, P, C)
        exact("D", "broadcast_pixels_fwd dt=%d %s" % (dt, what), fwd[dt], exp.to(tdt(dt)).contiguous())
    gr = torch.randn(B, P, C, generator=g, device="cuda")
    bwd = {}
    for dt in (F32, BF16):
        gd = gr.to(tdt(dt)).contiguous()
        dz = buf(B * C)
        L.broadcast_pixels_bwd(gd.data_ptr(), dt, dz.data_ptr(), B, P, C, S())
        tail_kept(dz, B * C)
        bwd[dt] = dz[:B * C].reshape(B, C)
        rel_to_max("D", "broadcast_pixels_bwd dt=%d %s" % (dt, what), bwd[dt], gd.double().sum(dim=1), 1e-5)
    # <fwd(z), g> = <z, bwd(g)>: fwd is exact, so the two sides differ by the error of bwd, at most 1e-5 max |dz| on each element
    lhs, rhs = float((fwd[F32].double() * gr.double()).sum()), float((z.double() * bwd[F32].double()).sum())
    report("D", "adjoint broadcast " + what, abs(lhs - rhs), 1e-5 * float(gr.double().sum(dim=1).abs().max()) * float(z.double().abs().sum()))
    y = buf(B * C)
    L.global_avgpool_fwd(gr.data_ptr(), y.data_ptr(), B, P, C, S())
    tail_kept(y, B * C)
    rel_to_max("D", "global_avgpool_fwd " + what, y[:B * C].reshape(B, C), gr.double().mean(dim=1), 1e-5)
    dx = buf(B * P * C)
    L.global_avgpool_bwd(z.data_ptr(), dx.data_ptr(), B, P, C, S())
    tail_kept(dx, B * P * C)
    dxr = (z.double() / P)[:, None, :].expand(B, P, C)
    rel_to_max("D", "global_avgpool_bwd " + what, dx[:B * P * C].reshape(B, P, C), dxr, 1e-5)
    # <gap_fwd(x), dy> = <x, gap_bwd(dy)>: each side carries its kernel's error, bounded as above
    lhs = float((y[:B * C].reshape(B, C).double() * z.double()).sum())
    rhs = float((gr.double() * dx[:B * P * C].reshape(B, P, C).double()).sum())
    bound = 1e-5 * (float(gr.double().mean(dim=1).abs().max()) * float(z.double().abs().sum()) +
                    float(dxr.abs().max()) * float(gr.double().abs().sum()))
    report("D", "adjoint global_avgpool " + what, abs(lhs - rhs), bound)


@pytest.mark.parametrize("B", [1, 3])
def test_broadcast_and_global_pool_block_loops(L, B):
    """P around the 64 threads of k_gap_fwd and the 256 of k_bcast_bwd: one trip, exactly one, one element into the second, four trips"""
    g = gen(40 + B)
    for C in (1, 6, 32):
        for P in (1, 63, 64, 65, 256, 257, 1000):
            _bcast_gap_case(L, B, P, C, g)


def test_broadcast_and_global_pool_above_the_grid_cap(L):
    B, P, C = 3, 58257, 6
    assert B * P * C > CAP
    _bcast_gap_case(L, B, P, C, gen(49))


# ---- E. phx_posterior_input -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dt", [BF16, F32])
@pytest.mark.parametrize("nlabels", [1, 2, 4, 8])
def test_posterior_input_labels_out_of_range_and_grid_stride(L, nlabels, out_dt):
    """[x, one_hot(s) - 0.5]: a label >= nlabels gives a row of -0.5, as tf.one_hot gives a zero row"""
    g = gen(50 + nlabels)
    for npix in (1, 257, CAP + 3):
        x = torch.randn(npix, generator=g, device="cuda")
        s = torch.randint(0, nlabels + 3, (npix,), generator=g, device="cuda").to(torch.uint8)
        s[-1] = 255 if npix > 1 else nlabels
        C = 1 + nlabels
        out = buf(npix * C, tdt(out_dt))
        L.posterior_input(x.data_ptr(), s.data_ptr(), out.data_ptr(), out_dt, npix, nlabels, S())
        tail_kept(out, npix * C)
        oh = (s.long()[:, None] == torch.arange(nlabels, device="cuda")[None, :]).float() - 0.5
        assert bool((oh[s.long() >= nlabels] == -0.5).all())
        ref = torch.cat([x[:, None], oh], dim=1).to(tdt(out_dt))
        exact("E", "nlabels=%d dt=%d npix=%d" % (nlabels, out_dt, npix), out[:npix * C].reshape(npix, C), ref)


# ---- F. phx_repeat_batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
def test_repeat_batch_bit_for_bit(L, dt):
    g, es, B = gen(60 + dt), rt.DT_SIZE[dt], 3
    cases = [(n, nbytes) for n in (1, 2, 5) for nbytes in (16, 48)] + [(2, 16 * (CAP // 6 + 3))]
    assert cases[-1][1] // 16 * B * 2 > CAP
    for (n, nbytes) in cases:
        per = nbytes // es
        x = torch.randn(B, per, generator=g, device="cuda").to(tdt(dt)).contiguous()
        out = buf(B * n * per, tdt(dt))
        L.repeat_batch(x.data_ptr(), out.data_ptr(), B, nbytes, n, S())
        tail_kept(out, B * n * per)
        exact("F", "dt=%d n=%d bytes=%d" % (dt, n, nbytes), out[:B * n * per].reshape(B * n, per), torch.repeat_interleave(x, n, 0))


def test_repeat_batch_refusals(L):
    x, out = torch.zeros(64, device="cuda"), buf(64)
    refused("PHX_E_SHAPE", L.repeat_batch, x.data_ptr(), out.data_ptr(), 3, 24, 2, S())
    refused("PHX_E_SHAPE", L.repeat_batch, x.data_ptr(), out.data_ptr(), 3, 16, 0, S())
    refused("PHX_E_ALIGN", L.repeat_batch, x.data_ptr() + 4, out.data_ptr(), 3, 16, 2, S())
    refused("PHX_E_ALIGN", L.repeat_batch, x.data_ptr(), out.data_ptr() + 4, 3, 16, 2, S())
    tail_kept(out, 0)


# ---- G. phx_pad_channels_bf16 / phx_unpad_channels_bf16 ---------------------------------------------------------------------------------
def _pad_case(L, C, Cpad, dt, npix, g):
    what = "C=%d Cpad=%d dt=%d npix=%d" % (C, Cpad, dt, npix)
    x = torch.randn(npix, C, generator=g, device="cuda").to(tdt(dt)).contiguous()
    xb = x.to(torch.bfloat16)
    padded = buf(npix * Cpad, torch.bfloat16)
    L.pad_channels_bf16(x.data_ptr(), dt, C, padded.data_ptr(), Cpad, npix, S())
    tail_kept(padded, npix * Cpad)
    pv = padded[:npix * Cpad].reshape(npix, Cpad)
    exact("G", "pad, real lanes " + what, pv[:, :C].contiguous(), xb)
    assert bool((pv.view(torch.int16)[:, C:] == 0).all()), "pad lanes are not +0: " + what
    src = torch.full((npix, Cpad), NAN, dtype=torch.bfloat16, device="cuda")             # pad lanes hold NaN: none of it may leak
    src[:, :C] = xb
    for (s, name) in ((src, "unpad of NaN-padded "), (pv, "round trip ")):
        back = buf(npix * C, tdt(dt))
        L.unpad_channels_bf16(s.data_ptr(), back.data_ptr(), dt, C, Cpad, npix, S())
        tail_kept(back, npix * C)
        exact("G", name + what, back[:npix * C].reshape(npix, C), xb.to(tdt(dt)))


@pytest.mark.parametrize("dt", [F32, BF16])
def test_pad_unpad_channels(L, dt):
    """(C = 33 only fits Cpad = 64)"""
    g = gen(70 + dt)
    for C in (1, 3, 5, 33):
        for Cpad in (32, 64):
            if C <= Cpad:
                _pad_case(L, C, Cpad, dt, 37, g)


@pytest.mark.parametrize("C,Cpad,dt,npix", [(3, 32, F32, CAP_8192 // 32 + 3),        # pad: npix * Cpad items
                                            (5, 32, BF16, CAP_8192 // 5 + 3)])       # unpad: npix * C items
def test_pad_unpad_channels_above_the_grid_cap(L, C, Cpad, dt, npix):
    assert npix * (Cpad if C == 3 else C) > CAP_8192
    _pad_case(L, C, Cpad, dt, npix, gen(75))


@pytest.mark.parametrize("Cin,Cpad,Cout", [(1, 32, 32), (3, 32, 64), (38, 64, 32)])
def test_pack_conv3x3_bf16_pad_layout(L, Cin, Cpad, Cout):
    """the single-filter form of the padded pack (the engine packs through phx_pack_conv3x3_bf16_multi): the layout include/phx.h
    documents, element (tap t, row n, channel k) at (((k / 32) * 9 + t) * N + n) * 32 + k % 32 with zero rows / channels for the pad,
    written out in numpy; and bit for bit what the multi-filter launch gives for the same record"""
    g = gen(78)
    w = torch.randn(3, 3, Cin, Cout, generator=g, device="cuda")
    wb = w.to(torch.bfloat16).cpu().view(torch.int16).numpy()
    n = 9 * Cpad * Cout
    ref_f, ref_d = np.zeros(n, dtype=np.int16), np.zeros(n, dtype=np.int16)
    for kh in range(3):
        for kw in range(3):
            for ci in range(Cin):
                co = np.arange(Cout)
                ref_f[(((ci // 32) * 9 + kh * 3 + kw) * Cout + co) * 32 + ci % 32] = wb[kh, kw, ci]                    # N = Cout, K = Cin_pad
                ref_d[(((co // 32) * 9 + (2 - kh) * 3 + (2 - kw)) * Cpad + ci) * 32 + co % 32] = wb[kh, kw, ci]       # N = Cin_pad, K = Cout
    wf, wd = buf(n, torch.bfloat16), buf(n, torch.bfloat16)
    L.pack_conv3x3_bf16_pad(w.data_ptr(), wf.data_ptr(), wd.data_ptr(), Cin, Cpad, Cout, S())
    tail_kept(wf, n)
    tail_kept(wd, n)
    exact("G", "pack_pad fwd (%d,%d,%d)" % (Cin, Cpad, Cout), wf[:n].view(torch.int16).cpu(), torch.from_numpy(ref_f))
    exact("G", "pack_pad dgrad (%d,%d,%d)" % (Cin, Cpad, Cout), wd[:n].view(torch.int16).cpu(), torch.from_numpy(ref_d))
    wf2, wd2 = buf(n, torch.bfloat16), buf(n, torch.bfloat16)
    desc = np.zeros(1, dtype=[("w", "<u8"), ("wf", "<u8"), ("wd", "<u8"), ("cin", "<i4"), ("cpad", "<i4"), ("cout", "<i4"), ("k1", "<i4")])
    desc[0] = (w.data_ptr(), wf2.data_ptr(), wd2.data_ptr(), Cin, Cpad, Cout, 0)
    dd = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    L.pack_conv3x3_bf16_multi(dd.data_ptr(), 1, S())
    torch.cuda.synchronize()
    assert torch.equal(wf.view(torch.int16), wf2.view(torch.int16)) and torch.equal(wd.view(torch.int16), wd2.view(torch.int16))
    wf3 = buf(n, torch.bfloat16)                                     # wpk_dgrad is nullable
    L.pack_conv3x3_bf16_pad(w.data_ptr(), wf3.data_ptr(), None, Cin, Cpad, Cout, S())
    torch.cuda.synchronize()
    assert torch.equal(wf.view(torch.int16), wf3.view(torch.int16))
    refused("PHX_E_SHAPE", L.pack_conv3x3_bf16_pad, w.data_ptr(), wf.data_ptr(), wd.data_ptr(), Cin, 48, Cout, S())
    refused("PHX_E_SHAPE", L.pack_conv3x3_bf16_pad, w.data_ptr(), wf.data_ptr(), wd.data_ptr(), Cpad + 1, Cpad, Cout, S())


# ---- H. phx_l2_masked / phx_axpy_masked -------------------------------------------------------------------------------------------------
MASKED_N = [1, 255, 65535, 65536, 65537, 3 * 65536 + 5]                      # around the 256 x 256 threads of k_l2_masked_partial


def _mask(kind, n):
    if kind == "ones":
        return torch.ones(n, device="cuda")
    if kind == "zeros":
        return torch.zeros(n, device="cuda")
    runs, edges = (100, 14, 206, 6, 2, 58), [0, 37]            # 0 / 1 runs of even length behind an odd one: every edge is odd,
    while edges[-1] < n:                                       # a multiple of neither 4 nor 64
        edges.append(edges[-1] + runs[len(edges) % len(runs)])
    assert all(e % 4 and e % 64 for e in edges[1:])
    m = torch.zeros(n, device="cuda")
    for k in range(0, len(edges) - 1, 2):
        m[edges[k]:edges[k + 1]] = 1.0
    return m


def _masked_params(kind, n, g):
    """in-mask parameters of order one, masked-out ones large but finite (1e3): a dropped mask shows"""
    m = _mask(kind, n)
    p = torch.randn(n, generator=g, device="cuda")
    return torch.where(m > 0, p, torch.full_like(p, 1e3)), m


@pytest.mark.parametrize("kind", ["ones", "zeros", "runs"])
def test_l2_masked_sum_bound_and_fixed_order(L, kind):
    """out = scale / 2 * sum mask p^2.  The order is fixed and readable (k_l2_masked_partial, k_l2_masked_finish): a thread adds its
    T = ceil(n / 65536) terms, wave_sum 6 more levels, the four wave sums meet in 2, the finishing thread adds 256 / 64 = 4 partials,
    wave_sum 6 more: T + 18 additions on the longest path, so |error| <= (T + 18) * 2^-24 * |scale| / 2 * sum mask p^2.  (The products
    add no term of their own: mask * p is exact for a 0 / 1 mask, its product with p and the addition are one fma, 0.5 * scale is
    exact.)  Two launches: equal bits."""
    g = gen(80)
    for n in MASKED_N:
        p, m = _masked_params(kind, n, g)
        terms = float((m.double() * p.double() ** 2).sum())
        for scale in (-0.3, 0.0, 1.7):
            runs = []
            for _ in range(2):
                work, out = buf(256), buf(1)
                L.l2_masked(p.data_ptr(), m.data_ptr(), n, scale, work.data_ptr(), out.data_ptr(), S())
                tail_kept(work, 256)
                tail_kept(out, 1)
                runs.append((work[:256].clone(), out[:1].clone()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "l2_masked: two launches differ in bits"
            got = float(runs[0][1][0])
            T_ = -(-n // 65536)
            report("H", "l2_masked %s n=%d scale=%g" % (kind, n, scale), abs(got - 0.5 * scale * terms), (T_ + 18) * U * 0.5 * abs(scale) * terms)
            if kind == "zeros":
                assert got == 0.0


@pytest.mark.parametrize("kind", ["ones", "zeros", "runs"])
def test_axpy_masked_keeps_what_it_must(L, kind):
    """g += alpha * mask * p: masked-out elements and the elements past n keep their bits; in-mask ones to the fp32 bound"""
    gn = gen(85)
    for n in MASKED_N + [CAP_2048 + 7]:
        p, m = _masked_params(kind, n, gn)
        g0 = torch.randn(n + TAIL, generator=gn, device="cuda")
        for alpha in (-0.25, 0.0, 0.6):
            runs = []
            for _ in range(2):
                gd = g0.clone()
                L.axpy_masked(gd.data_ptr(), p.data_ptr(), m.data_ptr(), n, alpha, S())
                torch.cuda.synchronize()
                runs.append(gd)
            gd = runs[0]
            assert torch.equal(runs[0], runs[1]), "axpy_masked: two launches differ in bits"
            assert torch.equal(gd[n:].view(torch.int32), g0[n:].view(torch.int32)), "axpy_masked wrote past n"
            out_of_mask = m == 0
            assert torch.equal(gd[:n][out_of_mask].view(torch.int32), g0[:n][out_of_mask].view(torch.int32)), "a masked-out element changed"
            if kind != "zeros":
                ref = g0[:n].double() + alpha * m.double() * p.double()
                rel_to_max("H", "axpy_masked %s n=%d alpha=%g" % (kind, n, alpha), gd[:n][~out_of_mask], ref[~out_of_mask], 1e-5)
            elif alpha == 0.6:
                print("GLUE H axpy_masked zeros n=%d exact" % n)


def test_masked_pair_refuses_null_arguments(L):
    t, out = torch.zeros(256, device="cuda"), buf(1)
    refused("PHX_E_INVAL", L.l2_masked, t.data_ptr(), None, 8, 1.0, t.data_ptr(), out.data_ptr(), S())
    refused("PHX_E_INVAL", L.l2_masked, t.data_ptr(), t.data_ptr(), 8, 1.0, None, out.data_ptr(), S())
    refused("PHX_E_INVAL", L.axpy_masked, t.data_ptr(), None, t.data_ptr(), 8, 1.0, S())
    tail_kept(out, 0)


# ---- I. phx_weighted_sum / phx_sum_scalars ------------------------------------------------------------------------------------------------
def test_weighted_sum_and_sum_scalars(L):
    """out = sum_i w[i] * *ptrs[i] (k_weighted_sum: one thread, acc = 0, then acc += w[i] * v[i] in order, each step one fused
    multiply-add, so one rounding): n additions on the path, |error| <= n * 2^-24 * sum |w[i] v[i]|.  k_sum_scalars: n additions,
    |error| <= n * 2^-24 * sum |v[i]|."""
    g = gen(90)
    pool = torch.randn(4096, generator=g, device="cuda") * 3.0
    rng = np.random.default_rng(91)
    for n in (1, 2, 16):
        idx = [int(i) for i in rng.integers(0, 4096, n)]            # scalars scattered in a larger tensor
        if n > 1:
            idx[-1] = idx[0]                                          # one pointer repeated
        w = [float(np.float32(v)) for v in rng.standard_normal(n)]
        if n > 1:
            w[0], w[1] = -1.5, 0.0                                    # a negative and a zero weight
        else:
            w[0] = -1.5
        out = buf(1)
        warr = (ctypes.c_float * n)(*w)
        L.weighted_sum(rt.ptr_array([pool.data_ptr() + 4 * i for i in idx]), ctypes.cast(warr, ctypes.c_void_p), n, out.data_ptr(), S())
        tail_kept(out, 1)
        v = pool.double().cpu().numpy()[idx]
        report("I", "weighted_sum n=%d" % n, abs(float(out[0]) - float(np.dot(w, v))), n * U * float(np.abs(np.array(w) * v).sum()))
    for n in (1, 7):
        out = buf(1)
        L.sum_scalars(pool.data_ptr() + 4 * 100, n, out.data_ptr(), S())
        tail_kept(out, 1)
        v = pool.double().cpu().numpy()[100:100 + n]
        report("I", "sum_scalars n=%d" % n, abs(float(out[0]) - float(v.sum())), n * U * float(np.abs(v).sum()))
    out = buf(1)
    p1, w1 = rt.ptr_array([pool.data_ptr()] * 17), (ctypes.c_float * 17)(*([1.0] * 17))
    refused("PHX_E_SHAPE", L.weighted_sum, p1, ctypes.cast(w1, ctypes.c_void_p), 0, out.data_ptr(), S())
    refused("PHX_E_SHAPE", L.weighted_sum, p1, ctypes.cast(w1, ctypes.c_void_p), 17, out.data_ptr(), S())
    tail_kept(out, 0)


# ---- J. phx_softmax_xent_map --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 4, 5, 6, 7, 8])
def test_softmax_xent_map_against_float64_logsumexp(L, C):
    g = gen(110 + C)
    for npix in (1, 255, 257, 70001):
        logits = torch.randn(npix, C, generator=g, device="cuda") * 3.0
        if npix > 1:                                                  # +-80 and +-100: a naive exp loses the small terms, then overflows
            logits[1::7, 0] = 80.0
            logits[2::7, C - 1] = -80.0
            logits[3::7, :] = -80.0
            logits[3::7, 1] = 80.0
            logits[4::7, C - 1] = 100.0                                 # (e^80 itself still fits fp32; e^100 does not, e^-100 is zero)
            logits[5::7, 0] = -100.0
        else:
            logits[0, 0], logits[0, 1] = -80.0, 80.0
        ar = torch.arange(npix, device="cuda")
        lab = ((ar + ar // C) % C).to(torch.uint8)                    # every class occurs, in a pattern that is not the logits'
        if npix >= C:
            assert set(lab.cpu().tolist()) == set(range(C))
        out = buf(npix)
        L.softmax_xent_map(logits.data_ptr(), lab.data_ptr(), out.data_ptr(), npix, C, S())
        tail_kept(out, npix)
        l64 = logits.double()
        ref = torch.logsumexp(l64, dim=1) - l64.gather(1, lab.long()[:, None])[:, 0]
        rel_to_max("J", "C=%d npix=%d" % (C, npix), out[:npix], ref, 1e-5)


@pytest.mark.parametrize("C", [2, 3, 4, 5, 6, 7, 8])
def test_softmax_xent_map_mean_agrees_with_residual_ce(L, C):
    """the map's sum over a sample batch / B = losses[0] of phx_residual_ce on the same logits with L = 1 (both fp32; the 2e-5 the
    residual_ce tests ask of the loss scalars)"""
    B, Hh, Ww = 2, 16, 48
    g = gen(120 + C)
    logits = torch.randn(B, Hh, Ww, C, generator=g, device="cuda") * 3.0
    lab = torch.randint(0, C, (B, Hh, Ww), generator=g, device="cuda").to(torch.uint8)
    out = buf(B * Hh * Ww)
    L.softmax_xent_map(logits.data_ptr(), lab.data_ptr(), out.data_ptr(), B * Hh * Ww, C, S())
    losses = torch.full((8 + 512,), NAN, device="cuda")
    L.residual_ce(rt.ptr_array([logits.data_ptr()]), None, rt.int_array([0]), 1, lab.data_ptr(), B, Hh, Ww, C, 1.0, 1.0 / B,
                  losses.data_ptr(), None, None, S())
    torch.cuda.synchronize()
    a, b = float(out[:B * Hh * Ww].double().sum()) / B, float(losses[0])
    report("J", "mean vs residual_ce C=%d" % C, abs(a - b) / abs(a), 2e-5)


def test_softmax_xent_map_refusals(L):
    t, lab, out = torch.zeros(64, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda"), buf(8)
    refused("PHX_E_SHAPE", L.softmax_xent_map, t.data_ptr(), lab.data_ptr(), out.data_ptr(), 4, 1, S())
    refused("PHX_E_SHAPE", L.softmax_xent_map, t.data_ptr(), lab.data_ptr(), out.data_ptr(), 4, 9, S())
    refused("PHX_E_SHAPE", L.softmax_xent_map, t.data_ptr(), lab.data_ptr(), out.data_ptr(), 0, 4, S())
    tail_kept(out, 0)


# ---- K. phx_residual_ce: levels of ds nullable one by one, other shift lists, eight levels ------------------------------------------------
@pytest.mark.parametrize("case", RESIDUAL_CE_CONTRACT, ids=lambda c: "-".join(str(v) for v in c))
def test_residual_ce_partial_ds_and_shift_lists(L, case):
    """the cases of tests/det_kernels_worker.RESIDUAL_CE_CONTRACT (which runs them again under PHX_DETERMINISTIC=1), here in the default
    mode: the oracle construction and bounds of test_residual_ce (tests/test_kernels_gpu.py); every level handed over is written,
    whichever levels they are (include/phx.h: ds[l] nullable), the launch with the others NULL runs clean and leaves losses, s_out
    and softmax within their bounds"""
    # (bitwise = True in the default mode too: the loss partials are float atomics into 64 slots there, and these maps give at most
    # 3 x 6 = 18 blocks, one add per slot -- a case of more than 64 blocks would have to drop the bit comparison of the losses here)
    residual_ce_contract(L, *case)
    print("GLUE K %s within the bounds of test_residual_ce" % "-".join(str(v) for v in case))


def test_residual_ce_refusals(L):
    s, lab, losses = torch.zeros(3 * 16 * 16 * 8, device="cuda"), torch.zeros(3 * 16 * 16, dtype=torch.uint8, device="cuda"), buf(8 + 512)

    def call(Ls, C, shifts, H_=16, W_=16):
        n = max(Ls, 1)
        L.residual_ce(rt.ptr_array([s.data_ptr()] * n), None, rt.int_array(shifts), Ls, lab.data_ptr(), 3, H_, W_, C, 1.0, 1.0 / 3,
                      losses.data_ptr(), None, None, S())
    refused("PHX_E_SHAPE", call, 0, 2, [0])
    refused("PHX_E_SHAPE", call, 9, 2, [0] * 9)
    refused("PHX_E_SHAPE", call, 1, 1, [0])
    refused("PHX_E_SHAPE", call, 1, 9, [0])
    refused("PHX_E_SHAPE", call, 2, 2, [0, 5], 32, 32)
    refused("PHX_E_SHAPE", call, 2, 2, [0, 2], 18, 16)
    refused("PHX_E_SHAPE", call, 2, 2, [0, 2], 16, 18)
    tail_kept(losses, 0)


# ---- L. phx_reparam_fwd / phx_reparam_bwd -------------------------------------------------------------------------------------------------
SEED = 42 + (1 << 40)


@functools.lru_cache(maxsize=None)
def _eps(step, stream, B, per, off):
    """the oracle's Philox normals, computed once and shared (read-only)"""
    e = philox.normal(SEED, step, stream, B, per, sample_offset=off, dtype=np.float64)
    e.setflags(write=False)
    return e


def _reparam_case(L, B, per, stream, off, g):
    what = "B=%d per=%d off=%d" % (B, per, off)
    step = torch.tensor([7], dtype=torch.int32, device="cuda")
    eps = torch.from_numpy(_eps(7, stream, B, per, off).copy()).cuda()             # (the cached array itself stays read-only)
    mu = torch.randn(B, per, generator=g, device="cuda")
    sg = torch.rand(B, per, generator=g, device="cuda") + 0.1
    for (m, s, name) in ((mu, sg, "mu and sigma"), (mu, None, "mu only"), (None, sg, "sigma only")):
        z = buf(B * per)
        L.reparam_fwd(m.data_ptr() if m is not None else None, s.data_ptr() if s is not None else None, z.data_ptr(), B, per, SEED,
                      step.data_ptr(), stream, off, S())
        tail_kept(z, B * per)
        ref = (m.double() if m is not None else 0.0) + (s.double() if s is not None else 1.0) * eps
        rel_to_max("L", "reparam_fwd %s %s" % (name, what), z[:B * per].reshape(B, per), ref, 1e-5)
    dz = torch.randn(B, per, generator=g, device="cuda")
    ds = buf(B * per)
    L.reparam_bwd(dz.data_ptr(), ds.data_ptr(), B, per, SEED, step.data_ptr(), stream, off, S())
    tail_kept(ds, B * per)
    rel_to_max("L", "reparam_bwd " + what, ds[:B * per].reshape(B, per), dz.double() * eps, 1e-5)


def test_reparam_null_operands_and_sample_offset(L):
    g = gen(130)
    _reparam_case(L, 3, 37, 5, 0, g)
    _reparam_case(L, 3, 37, 5, 11, g)
    _reparam_case(L, 1, 5, 2, 3, g)
    a, b = _eps(7, 5, 3, 37, 0), _eps(7, 5, 3, 37, 11)
    assert not np.array_equal(a, b) and np.array_equal(_eps(7, 5, 14, 37, 0)[11:], b)     # the offset is a sample index


def test_reparam_above_the_grid_cap(L):
    """B * ceil(per / 4) Philox blocks > CAP with per % 4 != 0 (the last block of a sample is cut), every sample against the oracle"""
    B, per = 2, 4 * (CAP // 2 + 2) - 1
    assert B * ((per + 3) // 4) > CAP and per % 4
    _reparam_case(L, B, per, 9, 1, gen(131))


# ---- M. phx_adam_tf1 on arenas shorter than, equal to and one past a float4 -------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_adam_short_arenas(L, n):
    g = gen(140 + n)
    sent = 12345.0
    bufs = [buf(n, fill=sent) for _ in range(4)]                      # p, g, m, v: 16-byte aligned, neighbours past n are sentinels
    p0, g0 = torch.randn(n, generator=g, device="cuda"), torch.randn(n, generator=g, device="cuda")
    bufs[0][:n], bufs[1][:n], bufs[2][:n], bufs[3][:n] = p0, g0, 0.0, 0.0
    step, lr = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.tensor([1e-3], device="cuda")
    pr, gr, mr, vr = p0.double().cpu(), g0.double().cpu(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(3):
        L.adam_tf1(*[b.data_ptr() for b in bufs], n, lr.data_ptr(), 0.9, 0.999, 1e-8, step.data_ptr(), S())
        L.step_increment(step.data_ptr(), S())
        pr, mr, vr = T.adam_tf1_step(pr, gr, mr, vr, t + 1, 1e-3)
    for b in bufs:
        tail_kept(b, n, fill=sent)
    report("M", "adam n=%d" % n, float((bufs[0][:n].double().cpu() - pr).abs().max()), 2e-6)
    assert torch.equal(bufs[1][:n], g0)
    assert float((bufs[2][:n].double().cpu() - mr).abs().max()) <= 1e-5 * float(mr.abs().max())
    assert float((bufs[3][:n].double().cpu() - vr).abs().max()) <= 1e-4 * float(vr.abs().max())


def test_adam_refuses_a_misaligned_arena(L):
    b = [buf(8, fill=1.0) for _ in range(4)]
    step, lr = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.tensor([1e-3], device="cuda")
    for k in range(4):
        ptrs = [t.data_ptr() + (4 if i == k else 0) for i, t in enumerate(b)]
        refused("PHX_E_ALIGN", L.adam_tf1, *ptrs, 4, lr.data_ptr(), 0.9, 0.999, 1e-8, step.data_ptr(), S())
    for t in b:
        tail_kept(t, 0, fill=1.0)


# ---- N. host-side entry points: stream copies, events, device and size queries, the clock stamp -------------------------------------------
def test_stamp_writes_an_advancing_clock(L):
    out = torch.zeros(2 + TAIL, dtype=torch.int64, device="cuda")
    out[2:] = -7
    L.stamp(out.data_ptr(), S())
    L.stamp(out.data_ptr() + 8, S())                                  # the same stream: the second stamp is taken after the first
    torch.cuda.synchronize()
    a, b = int(out[0]), int(out[1])
    assert 0 < a <= b, (a, b)
    assert b - a < 100e6 * 10, "two back-to-back stamps lie more than ten seconds apart on a 100 MHz clock"
    assert bool((out[2:] == -7).all())


def test_stream_copies_memset_and_events(L):
    n = 4096 + 3
    src = (ctypes.c_ubyte * n)(*[(7 * i + 1) % 251 for i in range(n)])
    back = (ctypes.c_ubyte * n)()
    d0 = torch.full((n + TAIL,), 9, dtype=torch.uint8, device="cuda")
    d1 = torch.full((n + TAIL,), 9, dtype=torch.uint8, device="cuda")
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        L.event_create(ctypes.byref(e))
        assert e.value
    st = ctypes.c_void_p()
    L.stream_create(ctypes.byref(st))
    torch.cuda.synchronize()                                          # (the fills above ran on torch's stream)
    L.event_record(ev[0], st)
    L.memset(d1.data_ptr(), 0x5A, n, st)
    L.memcpy_h2d(d0.data_ptr(), ctypes.cast(src, ctypes.c_void_p), n, st)
    L.event_record(ev[1], st)
    L.stream_wait_event(S(), ev[1])                                   # torch's stream waits for the copies of the other stream
    torch.cuda.synchronize()
    assert bool((d1[:n] == 0x5A).all()) and bool((d1[n:] == 9).all())
    assert bytes(d0[:n].cpu().numpy()) == bytes(src) and bool((d0[n:] == 9).all())
    L.memcpy_d2d(d1.data_ptr(), d0.data_ptr(), n, st)
    L.memcpy_d2h(ctypes.cast(back, ctypes.c_void_p), d1.data_ptr(), n, st)
    L.stream_sync(st)
    assert bytes(back) == bytes(src) and bool((d1[n:] == 9).all())
    L.event_sync(ev[1])
    ms = ctypes.c_float(-1.0)
    L.event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms))
    assert 0.0 <= ms.value < 10e3, ms.value
    for e in ev:
        L.event_destroy(e)
    L.stream_destroy(st)


def test_device_info_last_error_and_size_queries(L):
    cu, khz, hbm, name = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.create_string_buffer(128)
    L.device_info(ctypes.byref(cu), ctypes.byref(khz), ctypes.byref(hbm), name, 128)
    props = torch.cuda.get_device_properties(torch.cuda.current_device())
    assert cu.value == props.multi_processor_count and hbm.value == props.total_memory and khz.value > 0
    assert props.name in name.value.decode() and "gfx950" in name.value.decode()
    L.device_info(None, None, None, None, 0)                          # every output is optional
    t, out = torch.zeros(8, device="cuda"), buf(8)
    refused("PHX_E_SHAPE", L.repeat_batch, t.data_ptr(), out.data_ptr(), 1, 24, 1, S())
    msg = ctypes.create_string_buffer(512)
    L.last_error(msg, 512)
    assert "repeat_batch" in msg.value.decode()
    L.comm_load_api()                                                 # binds the collective library's symbols; raises if one is missing
    assert L.conv3x3_desc_bytes() == ctypes.sizeof(rt.Conv3x3Desc) == 224        # include/phx.h: "224 bytes"
    # the phase-form predicate on the shapes tests/test_kernels_gpu.test_upsample_conv_phase_form_vs_oracle runs, and off the matrix
    # kernels' channel multiple (phx_upconv_pack refuses those)
    assert L.upconv_supported(2, 16, 16, 32, 32) == 1 and L.upconv_supported(2, 4, 4, 32, 32) == 1
    assert L.upconv_supported(2, 16, 16, 24, 32) == 0 and L.upconv_supported(2, 16, 16, 32, 40) == 0 and L.upconv_supported(0, 16, 16, 32, 32) == 0
    # workspace sizes: what the launches accept (their own tests pass exactly these), growing with the problem
    small, big = L.validation_metrics_ws_bytes(1, 4, 2, 64, 2), L.validation_metrics_ws_bytes(3, 16, 4, 128 * 128, 2)
    assert 0 < small < big
    assert L.summary_histograms_ws_bytes(0) == 0 and 0 < L.summary_histograms_ws_bytes(1) and \
        L.summary_histograms_ws_bytes(10) == 10 * L.summary_histograms_ws_bytes(1)
    assert L.mc_stats_ws_bytes(2, 16, 4, 192 * 192, 4) == 0           # (the samples are combined inside the block: no scratch)
