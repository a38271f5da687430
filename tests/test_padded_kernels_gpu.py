"""csrc/conv2d_pad.hip through the C ABI against the float64 reference (tests/padded_ref.py, a torch-CPU restatement independent of the
kernels): convolution and transposed convolution with explicit geometry -- forward, data gradient and accumulating filter gradient on
the vector path and the scalar route, fp32 and bf16 storage -- the general pools, the SAME cases against the kernels of gconv.hip,
bit-identical repeats and the refusals.  The metric and the convolution bounds are those of
tests/test_extra_layers_gpu.py::test_general_conv_fwd_dgrad_wgrad (the same arithmetic class): max abs error over max abs reference,
operands rounded to the storage type before the reference sees them; 2e-5 (fp32) / 8e-3 (bf16) forward and data gradient, 3e-5 / 2e-5
filter gradient.  Pools: a maximum is exact (1e-7, as the existing max-pool test has it); an average in fp32 is taps additions and one
division, (taps + 2) * 2^-24 of max |x| per element, plus one output rounding, 2^-8 of |reference|, in bf16 storage."""
import ctypes

import numpy as np
import pytest
import torch

from tests import padded_ref as R

pytestmark = pytest.mark.gpu
F32, BF16 = 0, 1
SAME, VALID = 0, 1
MAX, AVG = 0, 1
RNG = np.random.default_rng(29)
PHX_E_SHAPE = -2
FWD_TOL = {F32: 2e-5, BF16: 8e-3}
WGRAD_TOL = {F32: 3e-5, BF16: 2e-5}


@pytest.fixture(scope="module")
def L():
    from phiseg_code_amd import runtime as rt
    return rt.lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def tdt(dt):
    return torch.float32 if dt == F32 else torch.bfloat16


def dev(a, dt=F32):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(tdt(dt)).cuda()


def rounded(a, dt):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(tdt(dt)).double()


def host(t):
    return t.float().cpu().numpy()


def close(a, b, tol, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() / max(1e-12, np.abs(b).max())
    print("%s: %.3e (bound %.1e)" % (what, err, tol))
    assert err < tol, (what, err)


def c_geometry(L, H, W, k, s, d, padding):
    o = [ctypes.c_int() for _ in range(4)]
    L.conv2d_geometry(H, W, *k, *s, *d, SAME if padding == "SAME" else VALID, *[ctypes.byref(v) for v in o])
    got = tuple(v.value for v in o)
    assert got == R.geometry(H, W, k, s, d, padding), (got, H, W, k, s, d, padding)
    return got


def workspace(L, B, Hs, Ws, Ca, Cb, k):
    """(tensor kept alive, pointer or None) for the filter gradient over the small side [B, Hs, Ws] with reduced channels Ca x Cb"""
    n = int(L.conv2d_pad_wgrad_ws_floats(B, Hs, Ws, Ca, Cb, *k))
    ws = torch.full((max(n, 1),), float("nan")).cuda()                        # (need not be cleared: NaN would show a read before a write)
    return ws, (ws.data_ptr() if n else None), n


def conv_case(L, B, H, W, Ci, Co, k, s, d, padding, dt):
    """forward (bias + ReLU epilogue), data gradient into a sentinel-filled dx, filter gradient accumulating into a pre-filled dw
    -> (host y, host dx, host dw increment, geometry)"""
    Ho, Wo, pt, pl = c_geometry(L, H, W, k, s, d, padding)
    x = RNG.standard_normal((B, H, W, Ci))
    w = RNG.standard_normal(tuple(k) + (Ci, Co)) / np.sqrt(k[0] * k[1] * Ci)
    b = RNG.standard_normal(Co) * 0.3
    xr = rounded(x, dt).requires_grad_(True)
    wr = torch.as_tensor(w, dtype=torch.float32).double().requires_grad_(True)
    pre = R.conv2d(xr, wr, s, d, padding)
    assert tuple(pre.shape) == (B, Ho, Wo, Co)
    yr = torch.relu(R.bias_add(pre, torch.as_tensor(b, dtype=torch.float32).double()))
    xd, wd, bd = dev(x, dt), dev(w), dev(b)
    geo = (B, H, W, Ci, Co, *k, *s, *d, Ho, Wo, pt, pl)
    y = torch.empty(B, Ho, Wo, Co, dtype=tdt(dt)).cuda()
    L.conv2d_pad_fwd(xd.data_ptr(), dt, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), dt, *geo, 1, S())
    close(host(y), yr.detach().numpy(), FWD_TOL[dt], "conv fwd")
    dy = RNG.standard_normal((B, Ho, Wo, Co))
    (pre * rounded(dy, dt)).sum().backward()                                  # gradients of the un-activated convolution
    dyd = dev(dy, dt)
    dx = torch.full_like(xd, 7.0)
    L.conv2d_pad_dgrad(dyd.data_ptr(), dt, wd.data_ptr(), dx.data_ptr(), dt, *geo, S())
    close(host(dx), xr.grad.numpy(), FWD_TOL[dt], "conv dgrad")
    dwd = torch.full(tuple(w.shape), 0.25, dtype=torch.float32).cuda()
    keep, ws, n = workspace(L, B, Ho, Wo, Ci, Co, k)
    L.conv2d_pad_wgrad(xd.data_ptr(), dt, dyd.data_ptr(), dt, dwd.data_ptr(), ws, *geo, S())
    close(host(dwd) - 0.25, wr.grad.numpy(), WGRAD_TOL[dt], "conv wgrad (accumulates, %d workspace floats)" % n)
    return host(y), host(dx), host(dwd) - 0.25, (xd, wd, bd, dyd, geo)


def tconv_case(L, B, H, W, Ci, Co, k, s, padding, out_hw, dt):
    """the transposed layer: x [B, H, W, Ci] is the small side, y [B, Ho, Wo, Co] the big one, filter HWOI"""
    Ho, Wo = out_hw
    back = c_geometry(L, Ho, Wo, k, s, (1, 1), padding)                        # the forward convolution ON the output extent
    assert back[:2] == (H, W), (back, H, W)
    pt, pl = back[2:]
    x = RNG.standard_normal((B, H, W, Ci))
    w = RNG.standard_normal(tuple(k) + (Co, Ci)) / np.sqrt(k[0] * k[1] * Ci)
    b = RNG.standard_normal(Co) * 0.3
    xr = rounded(x, dt).requires_grad_(True)
    wr = torch.as_tensor(w, dtype=torch.float32).double().requires_grad_(True)
    pre = R.conv2d_transpose(xr, wr, out_hw, s, padding)
    assert tuple(pre.shape) == (B, Ho, Wo, Co)
    yr = torch.relu(R.bias_add(pre, torch.as_tensor(b, dtype=torch.float32).double()))
    xd, wd, bd = dev(x, dt), dev(w), dev(b)
    geo = (B, H, W, Ci, Co, *k, *s, 1, 1, Ho, Wo, pt, pl)
    y = torch.empty(B, Ho, Wo, Co, dtype=tdt(dt)).cuda()
    L.tconv2d_pad_fwd(xd.data_ptr(), dt, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), dt, *geo, 1, S())
    close(host(y), yr.detach().numpy(), FWD_TOL[dt], "tconv fwd")
    dy = RNG.standard_normal((B, Ho, Wo, Co))
    (pre * rounded(dy, dt)).sum().backward()
    dyd = dev(dy, dt)
    dx = torch.full_like(xd, 7.0)
    L.tconv2d_pad_dgrad(dyd.data_ptr(), dt, wd.data_ptr(), dx.data_ptr(), dt, *geo, S())
    close(host(dx), xr.grad.numpy(), FWD_TOL[dt], "tconv dgrad")
    dwd = torch.full(tuple(w.shape), 0.25, dtype=torch.float32).cuda()
    keep, ws, n = workspace(L, B, H, W, Co, Ci, k)
    L.tconv2d_pad_wgrad(xd.data_ptr(), dt, dyd.data_ptr(), dt, dwd.data_ptr(), ws, *geo, S())
    close(host(dwd) - 0.25, wr.grad.numpy(), WGRAD_TOL[dt], "tconv wgrad (accumulates, %d workspace floats)" % n)
    return host(y), np.maximum(np.float32(b), 0)


# (B, H, W, Cin, Cout, kernel, strides, dilations): VALID padding
FAST_EDGES = [
    (2, 7, 7, 8, 12, (3, 3), (1, 1), (1, 1)),       # Wo = 5 (not a multiple of 4); Cout = 12: channel padding in LDS; one reduction slice
    (2, 3, 3, 8, 8, (3, 3), (1, 1), (1, 1)),        # H == ke: a 1 x 1 output, Wo = 1, one filter-gradient chunk
    (2, 6, 9, 24, 16, (3, 3), (1, 1), (1, 1)),      # Cin = 24: three reduction slices
    (1, 7, 8, 32, 64, (5, 5), (1, 1), (1, 1)),      # 5 x 5, 32 -> 64: 25 taps do not fit one staging pass (16 fit)
    (2, 9, 8, 3, 5, (3, 3), (1, 1), (1, 1)),        # Cin = 3: the scalar route
    (2, 6, 7, 4, 8, (3, 3), (1, 1), (1, 1)),        # Cin = 4: scalar in bf16, fast in fp32
    (1, 6, 6, 40, 72, (3, 3), (1, 1), (1, 1)),      # two channel tiles of the filter gradient on both sides, Cout > 64
]
VALID_GEOMETRY = [
    (2, 8, 10, 8, 8, (3, 3), (2, 2), (1, 1)),       # (H - k) % s != 0 on both axes: the last row and column are read by nothing
    (2, 9, 8, 8, 16, (3, 3), (1, 1), (2, 2)),       # dilation 2
    (2, 5, 6, 8, 4, (1, 1), (1, 1), (1, 1)),        # 1 x 1
    (3, 9, 7, 16, 8, (5, 3), (2, 1), (1, 1)),       # a 5 x 3 filter with strides (2, 1)
    (2, 11, 9, 8, 8, (3, 3), (3, 2), (1, 2)),       # stride 3, mixed dilation: every stride and dilation takes the vector path
]


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("case", FAST_EDGES + VALID_GEOMETRY)
def test_conv_valid_fwd_dgrad_wgrad(L, case, dt):
    B, H, W, Ci, Co, k, s, d = case
    _, dx, _, _ = conv_case(L, B, H, W, Ci, Co, k, s, d, "VALID", dt)
    # rows / columns no window reaches get a ZERO data gradient (dx was filled with a sentinel)
    Ho, Wo, _, _ = R.geometry(H, W, k, s, d, "VALID")
    used_h, used_w = (Ho - 1) * s[0] + (k[0] - 1) * d[0] + 1, (Wo - 1) * s[1] + (k[1] - 1) * d[1] + 1
    assert not dx[:, used_h:].any() and not dx[:, :, used_w:].any()
    if case == VALID_GEOMETRY[0]:
        assert (used_h, used_w) == (7, 9) and dx[:, :7, :9].any()


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("case", [
    (2, 8, 7, 8, 8, (3, 3), (2, 2), (1, 1)),        # H = 8: total padding 1, pt = 0 != pb = 1; W = 7: 1 / 1
    (2, 9, 7, 5, 6, (3, 3), (1, 1), (2, 2)),        # dilated, scalar route
    (2, 6, 9, 16, 8, (5, 3), (2, 1), (1, 1)),       # H = 6, k = 5, s = 2: total 3, pt = 1 != pb = 2
])
def test_same_through_the_new_entries_equals_the_general_kernels(L, case, dt):
    B, H, W, Ci, Co, k, s, d = case
    y, dx, dw, (xd, wd, bd, dyd, geo) = conv_case(L, B, H, W, Ci, Co, k, s, d, "SAME", dt)
    old = geo[:11]
    y0 = torch.empty(y.shape, dtype=tdt(dt)).cuda()
    L.gconv2d_fwd(xd.data_ptr(), dt, wd.data_ptr(), bd.data_ptr(), y0.data_ptr(), dt, *old, 1, S())
    close(y, host(y0), FWD_TOL[dt], "fwd against gconv2d")
    dx0 = torch.empty_like(xd)
    L.gconv2d_dgrad(dyd.data_ptr(), dt, wd.data_ptr(), dx0.data_ptr(), dt, *old, S())
    close(dx, host(dx0), FWD_TOL[dt], "dgrad against gconv2d")
    dw0 = torch.zeros(tuple(wd.shape)).cuda()
    L.gconv2d_wgrad(xd.data_ptr(), dt, dyd.data_ptr(), dt, dw0.data_ptr(), *old, S())
    close(dw, host(dw0), WGRAD_TOL[dt], "wgrad against gconv2d")


# (B, H, W, Cin, Cout, kernel, strides, padding, output extent)
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("case", [
    (2, 4, 5, 8, 6, (2, 2), (2, 2), "VALID", (8, 10)),        # k2 / s2: no overlap
    (2, 4, 5, 8, 6, (3, 3), (2, 2), "VALID", (9, 11)),        # k3 / s2: overlap, O = 2 n + 1
    (2, 4, 5, 8, 16, (4, 4), (2, 2), "VALID", (10, 12)),      # k4 / s2: the lower end of the legal range
    (2, 4, 5, 8, 16, (4, 4), (2, 2), "VALID", (11, 13)),      # ... and the upper end: the last row and column are bias only
    (2, 4, 5, 8, 6, (4, 4), (2, 2), "SAME", (7, 9)),          # SAME with O = n s - 1
    (2, 3, 4, 5, 3, (3, 3), (2, 2), "SAME", (6, 8)),          # SAME, the default extent, scalar routes
    (1, 4, 4, 16, 8, (1, 1), (2, 2), "VALID", (8, 8)),        # k < s: every second row is bias only
])
def test_tconv_fwd_dgrad_wgrad(L, case, dt):
    B, H, W, Ci, Co, k, s, padding, out_hw = case
    y, relu_b = tconv_case(L, B, H, W, Ci, Co, k, s, padding, out_hw, dt)
    if padding == "VALID" and out_hw[0] == (H - 1) * s[0] + k[0] + s[0] - 1:
        want = host(dev(relu_b, dt))                                           # bias only, exactly: act(0 + b) in the storage type
        assert np.array_equal(y[:, -1], np.broadcast_to(want, y[:, -1].shape))
        assert np.array_equal(y[:, :, -1], np.broadcast_to(want, y[:, :, -1].shape))


# ---- pools ------------------------------------------------------------------------------------------------------------------------------
# (B, H, W, C, window, strides, padding)
POOLS = [
    (2, 7, 9, 6, (2, 2), (2, 2), "SAME"),           # the old kernels' geometry, odd sizes
    (2, 7, 6, 1, (2, 2), (2, 2), "VALID"),          # odd H under VALID: the last row is dropped
    (2, 8, 7, 6, (3, 3), (2, 2), "SAME"),           # even H: pt = 0; odd W: pl = 1
    (2, 5, 6, 6, (3, 3), (1, 1), "SAME"),           # overlap, padding on both sides
    (2, 7, 6, 1, (3, 2), (2, 1), "VALID"),          # a 3 x 2 window with strides (2, 1)
    (1, 3, 2, 6, (5, 5), (1, 1), "SAME"),           # a window larger than the map
    (2, 4, 5, 1, (5, 4), (2, 2), "SAME"),
]


def pool_input(B, H, W, C):
    x = RNG.standard_normal((B, H, W, C))
    x[0] = np.maximum(x[0], 0.0)                                              # ReLU zeros: ties everywhere in sample 0
    x[-1, :3, :3, 0] = 0.0                                                    # and a whole window of exact ties
    return x


def avg_close(got, ref, scale, taps, dt, what):
    """|got - ref| <= (taps + 2) 2^-24 max|operand| [+ 2^-8 |ref| in bf16 storage], per element"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = (taps + 2) * 2.0 ** -24 * scale + (2.0 ** -8 * np.abs(ref) if dt == BF16 else 0.0)
    print("%s: worst error / bound %.3f" % (what, float((np.abs(got - ref) / bound).max())))
    assert (np.abs(got - ref) <= bound).all(), what


def pool_geo(L, B, H, W, C, k, s, padding):
    Ho, Wo, pt, pl = c_geometry(L, H, W, k, s, (1, 1), padding)
    return (B, H, W, C, *k, *s, pt, pl, Ho, Wo)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("case", POOLS)
def test_max_pool_fwd_bwd(L, case, dt):
    B, H, W, C, k, s, padding = case
    geo = pool_geo(L, B, H, W, C, k, s, padding)
    x = pool_input(B, H, W, C)
    xr = rounded(x, dt).requires_grad_(True)
    yr = R.max_pool(xr, k, s, padding)
    xd = dev(x, dt)
    y = torch.empty(tuple(yr.shape), dtype=tdt(dt)).cuda()
    L.pool2d_fwd(xd.data_ptr(), dt, y.data_ptr(), MAX, *geo, S())
    close(host(y), yr.detach().numpy(), 1e-7, "max pool fwd")
    dy = RNG.standard_normal(tuple(yr.shape))
    (yr * rounded(dy, dt)).sum().backward()
    dyd = dev(dy, dt)
    dx = torch.full_like(xd, 7.0)
    L.pool2d_bwd(xd.data_ptr(), dyd.data_ptr(), dt, dx.data_ptr(), MAX, *geo, S())
    # without overlap an element takes one dy unchanged: exact.  With overlap it is the fp32 sum of up to nsum = ceil(k / s)^2 of them
    # (partial sums below nsum max|dy|, one rounding per addition), rounded once more in bf16 storage: the average's bound at that scale
    nsum = -(-k[0] // s[0]) * -(-k[1] // s[1])
    dymax = float(np.abs(host(dyd)).max())
    if nsum == 1:
        close(host(dx), xr.grad.numpy(), 1e-7, "max pool bwd")
    else:
        avg_close(host(dx), xr.grad.numpy(), nsum * dymax, nsum, dt, "max pool bwd (overlapping windows)")
    if padding == "VALID" and (H - k[0]) % s[0]:
        assert not host(dx)[:, H - (H - k[0]) % s[0]:].any()                  # the dropped rows: zero gradient, written
    if dt == F32:                                                              # the accumulating form: one more addition, onto 0.5
        acc = torch.full_like(xd, 0.5)
        L.pool2d_bwd_acc(xd.data_ptr(), dyd.data_ptr(), dt, acc.data_ptr(), MAX, *geo, S())
        avg_close(host(acc) - 0.5, xr.grad.numpy(), nsum * dymax + 0.5, nsum + 1, dt, "max pool bwd (accumulates)")
    if case == POOLS[0]:                                                       # bit-equal to the 2 x 2 kernels of gconv.hip
        y0, dx0 = torch.empty_like(y), torch.full_like(xd, 3.0)
        L.maxpool2x2_fwd(xd.data_ptr(), dt, y0.data_ptr(), B, H, W, C, S())
        L.maxpool2x2_bwd(xd.data_ptr(), dyd.data_ptr(), dt, dx0.data_ptr(), B, H, W, C, S())
        assert torch.equal(y, y0) and torch.equal(dx, dx0)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("case", POOLS)
def test_avg_pool_fwd_bwd(L, case, dt):
    B, H, W, C, k, s, padding = case
    geo = pool_geo(L, B, H, W, C, k, s, padding)
    taps = k[0] * k[1]
    x = pool_input(B, H, W, C)
    xr = rounded(x, dt).requires_grad_(True)
    yr = R.avg_pool(xr, k, s, padding)
    xd = dev(x, dt)
    y = torch.empty(tuple(yr.shape), dtype=tdt(dt)).cuda()
    L.pool2d_fwd(xd.data_ptr(), dt, y.data_ptr(), AVG, *geo, S())
    avg_close(host(y), yr.detach().numpy(), float(np.abs(host(xd)).max()), taps, dt, "avg pool fwd")
    dy = RNG.standard_normal(tuple(yr.shape))
    (yr * rounded(dy, dt)).sum().backward()
    dyd = dev(dy, dt)
    dx = torch.full_like(xd, 7.0)
    L.pool2d_bwd(None, dyd.data_ptr(), dt, dx.data_ptr(), AVG, *geo, S())     # (the average's gradient does not read x)
    avg_close(host(dx), xr.grad.numpy(), float(np.abs(host(dyd)).max()), taps, dt, "avg pool bwd")
    if padding == "VALID" and (H - k[0]) % s[0]:
        assert not host(dx)[:, H - (H - k[0]) % s[0]:].any()
    if dt == F32:                                                              # the accumulating form adds the same values
        acc = torch.full_like(xd, 0.5)
        L.pool2d_bwd_acc(None, dyd.data_ptr(), dt, acc.data_ptr(), AVG, *geo, S())
        avg_close(host(acc) - 0.5, xr.grad.numpy(), float(np.abs(host(dyd)).max()) + 0.5, taps, dt, "avg pool bwd (accumulates)")
    if case == POOLS[0]:                                                       # the existing 2 x 2 kernel, within the same bound
        y0 = torch.empty_like(y)
        L.avgpool2x2_fwd(xd.data_ptr(), dt, y0.data_ptr(), B, H, W, C, S())
        avg_close(host(y), host(y0), float(np.abs(host(xd)).max()), taps, dt, "avg pool fwd against avgpool2x2")


# ---- repeats and refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
def test_repeats_are_bit_identical(L, dt):
    B, H, W, Ci, Co, k, s, d = 2, 13, 11, 16, 24, (3, 3), (2, 1), (1, 1)
    Ho, Wo, pt, pl = R.geometry(H, W, k, s, d, "VALID")
    geo = (B, H, W, Ci, Co, *k, *s, *d, Ho, Wo, pt, pl)
    xd, wd, bd = dev(RNG.standard_normal((B, H, W, Ci)), dt), dev(RNG.standard_normal(k + (Ci, Co)) / 12), dev(RNG.standard_normal(Co))
    dyd = dev(RNG.standard_normal((B, Ho, Wo, Co)), dt)
    # the transposed layer reads the SAME tensors the other way round: dyd is its input, xd-shaped its output, wd its HWOI filter
    tgeo = (B, Ho, Wo, Co, Ci, *k, *s, *d, H, W, pt, pl)
    pgeo = (B, H, W, Ci, 3, 3, 2, 2, 1, 1, (H + 1) // 2, (W + 1) // 2)
    runs = []
    for _ in range(2):
        out = []
        y = torch.empty(B, Ho, Wo, Co, dtype=tdt(dt)).cuda()
        L.conv2d_pad_fwd(xd.data_ptr(), dt, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), dt, *geo, 1, S())
        dx = torch.empty_like(xd)
        L.conv2d_pad_dgrad(dyd.data_ptr(), dt, wd.data_ptr(), dx.data_ptr(), dt, *geo, S())
        dw = torch.zeros(k + (Ci, Co)).cuda()
        keep, ws, n = workspace(L, B, Ho, Wo, Ci, Co, k)
        assert n > 0                                                           # the two-stage form
        L.conv2d_pad_wgrad(xd.data_ptr(), dt, dyd.data_ptr(), dt, dw.data_ptr(), ws, *geo, S())
        ty = torch.empty_like(xd)
        L.tconv2d_pad_fwd(dyd.data_ptr(), dt, wd.data_ptr(), None, ty.data_ptr(), dt, *tgeo, 0, S())
        tdx = torch.empty_like(dyd)
        L.tconv2d_pad_dgrad(xd.data_ptr(), dt, wd.data_ptr(), tdx.data_ptr(), dt, *tgeo, S())
        tdw = torch.zeros(k + (Ci, Co)).cuda()
        L.tconv2d_pad_wgrad(dyd.data_ptr(), dt, xd.data_ptr(), dt, tdw.data_ptr(), ws, *tgeo, S())
        out += [y, dx, dw, ty, tdx, tdw]
        for mode in (MAX, AVG):
            p = torch.empty(B, pgeo[-2], pgeo[-1], Ci, dtype=tdt(dt)).cuda()
            L.pool2d_fwd(xd.data_ptr(), dt, p.data_ptr(), mode, *pgeo, S())
            g = torch.empty_like(xd)
            L.pool2d_bwd(xd.data_ptr(), p.data_ptr(), dt, g.data_ptr(), mode, *pgeo, S())
            ga = torch.ones_like(xd)
            L.pool2d_bwd_acc(xd.data_ptr(), p.data_ptr(), dt, ga.data_ptr(), mode, *pgeo, S())
            out += [p, g, ga]
        runs.append(out)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][2].abs().max()) > 0 and torch.equal(runs[0][2], runs[0][5])      # one filter gradient, reached from both layers


def test_bad_geometry_returns_the_shape_status_and_launches_nothing(L):
    dll = L._dll                                                               # the raw entry points: the status instead of an exception
    x = torch.ones(2 * 6 * 6 * 8, device="cuda")
    w = torch.ones(9 * 8 * 8, device="cuda")
    out = torch.full((2 * 6 * 6 * 8,), 5.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(S())
    good = (2, 6, 6, 8, 8, 3, 3, 1, 1, 1, 1, 4, 4, 0, 0)
    for pos, bad in [(0, 0), (1, -1), (2, 0), (3, 0), (4, -2), (5, 0), (6, 0), (7, 0), (8, -1), (9, 0), (10, 0), (11, 0), (12, -4), (13, -1), (14, -1)]:
        geo = good[:pos] + (bad,) + good[pos + 1:]
        assert dll.phx_conv2d_pad_fwd(p(x), F32, p(w), None, p(out), F32, *geo, 0, s) == PHX_E_SHAPE, geo
        assert dll.phx_conv2d_pad_dgrad(p(x), F32, p(w), p(out), F32, *geo, s) == PHX_E_SHAPE, geo
        assert dll.phx_conv2d_pad_wgrad(p(x), F32, p(x), F32, p(out), None, *geo, s) == PHX_E_SHAPE, geo
        assert dll.phx_tconv2d_pad_fwd(p(x), F32, p(w), None, p(out), F32, *geo, 0, s) == PHX_E_SHAPE, geo
        assert dll.phx_tconv2d_pad_dgrad(p(x), F32, p(w), p(out), F32, *geo, s) == PHX_E_SHAPE, geo
        assert dll.phx_tconv2d_pad_wgrad(p(x), F32, p(x), F32, p(out), None, *geo, s) == PHX_E_SHAPE, geo
    pgood = (2, 6, 6, 8, 3, 3, 2, 2, 0, 0, 3, 3)
    for pos, bad in [(0, 0), (1, 0), (2, -1), (3, 0), (4, 0), (5, -1), (6, 0), (7, 0), (8, -1), (9, -1), (10, 0), (11, -3)]:
        geo = pgood[:pos] + (bad,) + pgood[pos + 1:]
        for mode in (MAX, AVG):
            assert dll.phx_pool2d_fwd(p(x), F32, p(out), mode, *geo, s) == PHX_E_SHAPE, geo
            assert dll.phx_pool2d_bwd(p(x), p(x), F32, p(out), mode, *geo, s) == PHX_E_SHAPE, geo
            assert dll.phx_pool2d_bwd_acc(p(x), p(x), F32, p(out), mode, *geo, s) == PHX_E_SHAPE, geo
    o = [ctypes.c_int(77) for _ in range(4)]
    refs = [ctypes.byref(v) for v in o]
    assert dll.phx_conv2d_geometry(4, 9, 3, 3, 1, 1, 2, 2, VALID, *refs) == PHX_E_SHAPE      # 4 < ke = 5 under VALID
    assert dll.phx_conv2d_geometry(0, 9, 3, 3, 1, 1, 1, 1, SAME, *refs) == PHX_E_SHAPE
    assert dll.phx_conv2d_geometry(9, 9, 3, 3, 0, 1, 1, 1, SAME, *refs) == PHX_E_SHAPE
    assert int(L.conv2d_pad_wgrad_ws_floats(0, 4, 4, 8, 8, 3, 3)) == 0
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())                                            # the output buffer is untouched
    with pytest.raises(Exception, match="conv2d_pad"):
        L.conv2d_pad_fwd(x.data_ptr(), F32, w.data_ptr(), None, out.data_ptr(), F32, 2, 6, 6, 8, 8, 3, 3, 1, 1, 1, 1, 0, 4, 0, 0, 0, S())
