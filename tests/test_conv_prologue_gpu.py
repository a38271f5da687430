"""The first-chunk loads of k_conv3x3_mfma (MI355X): the smallest shapes that reach every path on which the kernel's prologue -- filter
slab first, then every input-patch piece as soon as its offset is known -- could go wrong: a piece's offset, its tensor (dual input),
its range check, the first chunk's index (split-K).  Every launcher form, against the float64 convolution of the bf16-rounded operands
with the bounds tests/test_kernels_gpu.py applies to the same entry point and form; no write outside what the launch owns; the plan
(tiles, split-K factor, workspace) unchanged.  (That the loads DO come first is a property of the compiled code: LABBOOK.md,
tools/conv_prologue_asm_table.py -- no test reads the assembly.)"""
import numpy as np
import pytest
import torch

from oracle import tf1_ops as T

pytestmark = pytest.mark.gpu

#        (B, H, W, K, N)        -> what the parent commit's phx_conv3x3_bf16_plan reports: (tiles, ksplit, ws_bytes)
CASES = {
    (1, 1, 1, 32, 32): (1, 1, 0),           # 1 x 1 x 256 tile: 36 pieces per thread, more than the kernel's 16 -- refused (see launched())
    (3, 4, 4, 32, 32): (1, 1, 0),           # 4 x 4 x 16 tile, 9 of 16 pieces, three images in a 16-image tile, a single chunk
    (40, 2, 2, 32, 32): (1, 1, 0),          # 2 x 2 x 64 tile, all 16 pieces, a single chunk (only the prologue's loads exist)
    (3, 2, 2, 64, 32): (1, 2, 3072),        # 2 x 2 x 64 tile partly filled, two chunks, split-K = 2
    (5, 3, 5, 32, 64): (1, 1, 0),           # map not a power of two (4 x 8 x 8 tile larger than the image), 64-channel block
    (17, 4, 4, 96, 96): (2, 3, 313344),     # B not a multiple of the 16-image tile, three chunks
    (9, 8, 8, 160, 64): (3, 5, 737280),     # 8 x 8 x 4 tiles, last tile partial, five chunks
    (2, 8, 32, 32, 32): (2, 1, 0),          # tiles with neighbours in x (the halo is real data), not the 16 x 16 path
    (2, 16, 16, 64, 32): (2, 2, 131072),    # 16 x 16 tiles
    (1, 32, 16, 32, 64): (2, 1, 0),         # 16 x 16 tiles, two in y
}
SLACK = 4                                   # pixels of slack behind every buffer
K1_DUAL, N1_DUAL = 32, 8
BF16_BOUND, F32_BOUND, DUAL_BOUND = 6e-3, 2e-5, 1.5e-2      # test_kernels_gpu.py: _mfma_case, test_conv3x3_mfma_fp32_output, test_conv3x3_concat_free
PARTIAL_STATS_BOUND, ATOMIC_STATS_BOUND = 1e-3, 2e-5        # ... _mfma_case, test_conv3x3_mfma_statistics_by_atomics


@pytest.fixture(scope="module")
def L():
    from phiseg_code_amd import runtime as rt
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return rt.lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def close(got, ref, rel, what):
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30)
    assert err <= rel, "%s: rel-to-max err %.3e > %.1e" % (what, err, rel)


def pieces_per_thread(case):
    """16-byte input-patch pieces a thread stages per chunk on the case's 256-pixel tile (conv_mfma.hip: NA)"""
    B, H, W, K, N = case
    tw = min(16, 1 << max(W - 1, 0).bit_length())
    th = min(16, 1 << max(H - 1, 0).bit_length())
    return (256 // (tw * th) * (tw + 2) * (th + 2) * 4 + 255) // 256


def launched(case, call, *bufs):
    """Run the launch.  A tile geometry beyond the kernel's 16 pieces per thread (a 1 x 1 map: 256 images x 3 x 3 patch pixels) never
    reaches the kernel: the launcher refuses it, as it did before the prologue was reordered, and must leave every buffer alone."""
    if pieces_per_thread(case) <= 16:
        call()
        return True
    from phiseg_code_amd.runtime import PhxError
    with pytest.raises(PhxError, match="unexpected tile geometry"):
        call()
    torch.cuda.synchronize()
    for b in bufs:
        assert torch.equal(b.t.view(torch.int16 if b.t.element_size() == 2 else torch.int32), b.t0), "a refused launch wrote to a buffer"
    return False


class Guarded:
    """A device buffer of `n` elements the launch owns plus `slack` behind them; both start as `fill`, the slack stays NaN."""
    def __init__(self, n, slack, dtype, fill=float("nan")):
        self.n = n
        self.t = torch.full((n + slack,), float("nan"), dtype=dtype, device="cuda")
        self.t[:n] = fill
        self.t0 = self.t.view(torch.int16 if self.t.element_size() == 2 else torch.int32).clone()      # (bit pattern at the start)
        self.ptr = self.t.data_ptr()

    def owned(self, what, allow_nan=False):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.t[self.n:]).all()), "%s: written behind the buffer" % what
        if not allow_nan:
            assert not bool(torch.isnan(self.t[:self.n]).any()), "%s: a NaN is left in what the launch owns" % what
        return self.t[:self.n]


_SETUP = {}


def setup(L, case):
    """operands, packed filter and the float64 reference of a case: made once, shared by its tests, never written to"""
    if case not in _SETUP:
        B, H, W, K, N = case
        rng = np.random.default_rng(sum(c * 131 ** i for i, c in enumerate(case)))
        x = torch.as_tensor(rng.standard_normal((B, H, W, K)), dtype=torch.float32).to(torch.bfloat16)
        w = torch.as_tensor(rng.standard_normal((3, 3, K, N)) / np.sqrt(9 * K), dtype=torch.float32)
        ref = T.conv2d_same(x.double(), w.to(torch.bfloat16).double()).numpy()
        xd, wd = x.cuda().contiguous(), w.cuda().contiguous()
        wf = torch.empty(9 * N * K, dtype=torch.bfloat16, device="cuda")
        L.pack_conv3x3_bf16(wd.data_ptr(), wf.data_ptr(), None, K, N, S())
        scale = torch.as_tensor(1.0 + 0.2 * rng.standard_normal(N), dtype=torch.float32)
        shift = torch.as_tensor(0.3 * rng.standard_normal(N), dtype=torch.float32)
        torch.cuda.synchronize()
        _SETUP[case] = dict(x=xd, wf=wf, ref=ref, scale=scale, shift=shift, P=B * H * W)
    return _SETUP[case]


def workspace(case):
    nb = CASES[case][2]
    ws = Guarded(nb // 4, SLACK * case[4], torch.float32)
    return ws, (ws.ptr if nb else None), nb


@pytest.mark.parametrize("case", list(CASES))
def test_plan_is_the_parents(L, case):
    pl = L.conv3x3_plan(*case)
    assert (pl.tiles, pl.ksplit, int(pl.ws_bytes)) == CASES[case]


@pytest.mark.parametrize("case", list(CASES))
def test_plain_bf16_output(L, case):
    B, H, W, K, N = case
    s = setup(L, case)
    y = Guarded(s["P"] * N, SLACK * N, torch.bfloat16)
    if not launched(case, lambda: L.conv3x3_mfma_bf16(s["x"].data_ptr(), s["wf"].data_ptr(), y.ptr, None, 0, None, B, H, W, K, N, S()), y):
        return
    close(y.owned("plain").float().cpu().numpy().reshape(s["ref"].shape), s["ref"], BF16_BOUND, "plain bf16 output")


@pytest.mark.parametrize("with_ws", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_bias_relu_oscale(L, case, with_ws):
    """y = relu(conv * oscale + bias): in the kernel's own epilogue (no workspace) and, where the plan splits K, in the finishing pass"""
    B, H, W, K, N = case
    s = setup(L, case)
    ref = np.maximum(s["ref"] * s["scale"].double().numpy() + s["shift"].double().numpy(), 0.0)
    sc, sh = s["scale"].cuda(), s["shift"].cuda()
    ws, wsp, wsb = workspace(case)
    y = Guarded(s["P"] * N, SLACK * N, torch.bfloat16)
    if not launched(case, lambda: L.conv3x3_mfma_bf16_affine(s["x"].data_ptr(), s["wf"].data_ptr(), y.ptr, sc.data_ptr(), sh.data_ptr(), 1,
                                                             wsp if with_ws else None, wsb if with_ws else 0, B, H, W, K, N, S()), y, ws):
        return
    close(y.owned("affine").float().cpu().numpy().reshape(ref.shape), ref, BF16_BOUND, "bias + ReLU + oscale")
    ws.owned("affine workspace", allow_nan=not (with_ws and wsb))


@pytest.mark.parametrize("mode", ["per-tile", "atomic"])
@pytest.mark.parametrize("case", list(CASES))
def test_statistics(L, case, mode):
    B, H, W, K, N = case
    s = setup(L, case)
    tiles = CASES[case][0]
    y = Guarded(s["P"] * N, SLACK * N, torch.bfloat16)
    if mode == "per-tile":
        st = Guarded(tiles * 2 * N, SLACK * N, torch.float32)
        if not launched(case, lambda: L.conv3x3_mfma_bf16(s["x"].data_ptr(), s["wf"].data_ptr(), y.ptr, None, 0, st.ptr, B, H, W, K, N, S()), y, st):
            return
        got = st.owned("per-tile statistics").double().cpu().numpy().reshape(tiles, 2, N).sum(0)
        bound = PARTIAL_STATS_BOUND
    else:
        assert L.conv3x3_plan(*case).stats_atomic_ok == 1
        st = Guarded(N * 2, SLACK * N, torch.float32, fill=0.0)                 # accumulated (+=)
        if not launched(case, lambda: L.conv3x3_mfma_bf16_stats_atomic(s["x"].data_ptr(), s["wf"].data_ptr(), y.ptr, None, 0, st.ptr,
                                                                       B, H, W, K, N, S()), y, st):
            return
        got = st.owned("atomic statistics").double().cpu().numpy().reshape(N, 2).T
        bound = ATOMIC_STATS_BOUND
    yf = y.owned("output of the statistics launch").float().cpu().double().numpy().reshape(-1, N)
    close(yf.reshape(s["ref"].shape), s["ref"], BF16_BOUND, "output of the statistics launch")
    close(got[0], yf.sum(0), bound, "sum y (%s)" % mode)
    close(got[1], (yf ** 2).sum(0), bound, "sum y^2 (%s)" % mode)


@pytest.mark.parametrize("case", list(CASES))
def test_split_k_with_finish(L, case):
    B, H, W, K, N = case
    s = setup(L, case)
    ws, wsp, wsb = workspace(case)
    y = Guarded(s["P"] * N, SLACK * N, torch.bfloat16)
    if not launched(case, lambda: L.conv3x3_mfma_bf16_ws(s["x"].data_ptr(), s["wf"].data_ptr(), y.ptr, None, 0, None, wsp, wsb,
                                                         B, H, W, K, N, S()), y, ws):
        return
    close(y.owned("split-K").float().cpu().numpy().reshape(s["ref"].shape), s["ref"], BF16_BOUND, "split-K with finish")
    ws.owned("split-K workspace")            # every slice element is written, nothing behind the slices


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_output_and_kept_slices(L, case):
    B, H, W, K, N = case
    s = setup(L, case)
    nz = CASES[case][1]
    ws, wsp, wsb = workspace(case)
    y1 = Guarded(s["P"] * N, SLACK * N, torch.float32)
    def f32out(y, sum_slices, p, nb):
        return lambda: L.conv3x3_mfma_bf16_f32out(s["x"].data_ptr(), None, 0, s["wf"].data_ptr(), y.ptr, sum_slices, p, nb, B, H, W, K, N, S())
    if not launched(case, f32out(y1, 1, wsp, wsb), y1, ws):
        assert not launched(case, f32out(y1, 0, wsp, wsb), y1, ws)
        return
    summed = y1.owned("fp32 output, slices summed").clone()
    close(summed.cpu().numpy().reshape(s["ref"].shape), s["ref"], F32_BOUND, "fp32 output")
    ws.owned("fp32-output workspace")
    ws0, wsp0, wsb0 = workspace(case)
    y0 = Guarded(s["P"] * N, SLACK * N, torch.float32)
    f32out(y0, 0, wsp0, wsb0)()
    if nz > 1:                               # the slices stay in the workspace, y_f32 is not touched
        sl = ws0.owned("kept slices").view(nz, s["P"] * N)
        acc = sl[0].clone()
        for z in range(1, nz):
            acc += sl[z]                     # the order of the finishing pass
        assert torch.equal(acc, summed), "sum of the kept slices differs from the summed output"
        assert bool(torch.isnan(y0.owned("y_f32 of a kept-slices launch", allow_nan=True)).all())
    else:                                    # a single slice goes straight to y_f32
        assert torch.equal(y0.owned("fp32 output, single slice"), summed)


@pytest.mark.parametrize("with_ws", [False, True])
@pytest.mark.parametrize("case", [c for c in CASES if c[3] >= 64])
def test_dual_input(L, case, with_ws):
    """reduction channels [0, 32) from one tensor, the rest from another: the launch on the concatenation, bit for bit"""
    B, H, W, K, N = case
    s = setup(L, case)
    xa, xb = s["x"][..., :K1_DUAL].contiguous(), s["x"][..., K1_DUAL:].contiguous()
    ws, wsp, wsb = workspace(case)
    if not with_ws:
        wsp, wsb = None, 0
    y_ref = Guarded(s["P"] * N, SLACK * N, torch.bfloat16)
    L.conv3x3_mfma_bf16_ws(s["x"].data_ptr(), s["wf"].data_ptr(), y_ref.ptr, None, 0, None, wsp, wsb, B, H, W, K, N, S())
    y = Guarded(s["P"] * N, SLACK * N, torch.bfloat16)
    L.conv3x3_mfma_bf16_dual(xa.data_ptr(), xb.data_ptr(), K1_DUAL, s["wf"].data_ptr(), y.ptr, None, 0, None, None, 0, None, 0, wsp, wsb,
                             B, H, W, K, N, S())
    got = y.owned("dual input")
    assert torch.equal(got, y_ref.owned("single input"))
    close(got.float().cpu().numpy().reshape(s["ref"].shape), s["ref"], DUAL_BOUND, "dual input vs concat + conv")
    ws.owned("dual-input workspace", allow_nan=not wsb)
    if wsb:                                  # fp32 output of the dual input (the split-K instantiation picks each chunk's tensor)
        ws2, wsp2, wsb2 = workspace(case)
        yf = Guarded(s["P"] * N, SLACK * N, torch.float32)
        L.conv3x3_mfma_bf16_f32out(xa.data_ptr(), xb.data_ptr(), K1_DUAL, s["wf"].data_ptr(), yf.ptr, 1, wsp2, wsb2, B, H, W, K, N, S())
        close(yf.owned("dual input, fp32 output").cpu().numpy().reshape(s["ref"].shape), s["ref"], F32_BOUND, "dual input, fp32 output")
        ws2.owned("dual-input fp32 workspace")


@pytest.mark.parametrize("with_ws", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_dual_output(L, case, with_ws):
    """output channels [0, 8) to one tensor, the rest to another: the two halves of the plain launch's output, bit for bit"""
    B, H, W, K, N = case
    s = setup(L, case)
    ws, wsp, wsb = workspace(case)
    if not with_ws:
        wsp, wsb = None, 0
    y_ref = Guarded(s["P"] * N, SLACK * N, torch.bfloat16)
    g1 = Guarded(s["P"] * N1_DUAL, SLACK * N1_DUAL, torch.bfloat16)
    g2 = Guarded(s["P"] * (N - N1_DUAL), SLACK * (N - N1_DUAL), torch.bfloat16)
    if not launched(case, lambda: L.conv3x3_mfma_bf16_dual(s["x"].data_ptr(), None, 0, s["wf"].data_ptr(), g1.ptr, g2.ptr, N1_DUAL, None, None,
                                                           0, None, 0, wsp, wsb, B, H, W, K, N, S()), g1, g2, ws):
        return
    L.conv3x3_mfma_bf16_ws(s["x"].data_ptr(), s["wf"].data_ptr(), y_ref.ptr, None, 0, None, wsp, wsb, B, H, W, K, N, S())
    ref = y_ref.owned("single output").view(s["P"], N)
    close(ref.float().cpu().numpy().reshape(s["ref"].shape), s["ref"], BF16_BOUND, "single output")
    assert torch.equal(g1.owned("dual output, first tensor").view(s["P"], N1_DUAL), ref[:, :N1_DUAL])
    assert torch.equal(g2.owned("dual output, second tensor").view(s["P"], N - N1_DUAL), ref[:, N1_DUAL:])
    ws.owned("dual-output workspace", allow_nan=not wsb)
