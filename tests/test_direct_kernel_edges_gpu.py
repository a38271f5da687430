"""The direct (non-MFMA) layer kernels -- csrc/conv3d.hip, gconv.hip, tconv.hip -- through the C ABI at the edges the friendly shapes of
tests/test_volume_kernels_gpu.py, test_extra_layers_gpu.py and test_tconv.py never reach: the sliced LDS filter stage of k_conv3_vec
(A), the 32-channel chunk loop of the three filter-gradient kernels (B), the grid-stride step behind the 8192-block cap of every
one-thread-per-element launcher (C), padding and offsets pinned exactly by one-hot filters against a reference that holds no
convolution (D), transposed geometries with k < s (E), the epilogue branches and the mixed dtype pairs (F),
phx_bn_moving_update_biased (G), pools and up-sampling on axes of extent 1 (H).

Helpers, metric (max abs error over max abs reference, operands rounded to their storage type before the float64 oracle sees them)
and bounds are those of the files the cases extend: 3-D 4e-5 (fp32) / 1.6e-2 (bf16) forward and data gradient, 6e-5 filter gradient;
2-D general convolution 2e-5 / 8e-3 and 3e-5 (fp32) / 2e-5 (bf16) filter gradient; 2-D transposed 1e-5 / 8e-3 and 2e-5.  D is exact;
G has a bound derived in its test."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import tf1_ops as T
from tests import test_volume_kernels_gpu as K
from tests import volume_ref as V
from tests.test_volume_kernels_gpu import BF16, F32, L, S, _conv_family, close, dev, host, rounded, tdt  # noqa: F401 (L: the fixture)

pytestmark = pytest.mark.gpu
RNG = np.random.default_rng(29)
PHX_E_INVAL = -1
CAP = 8192 * 256                                                               # phx_grid_for(n, 256, 8192): elements of one grid-stride trip


def _v3_constants():
    """V3_LDS, V3_RK, V3_CPT as csrc/conv3d.hip states them: the slicing asserted below follows the source, not a copy of it"""
    from phiseg_code_amd import runtime as rt
    src = open(os.path.join(os.path.dirname(rt.__file__), "csrc", "conv3d.hip")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1)) for n in ("V3_LDS", "V3_RK", "V3_CPT"))


def _stage(taps, cr, cq, dt):
    """-> (taps per staged slice, vector path taken) of k_conv3_vec for `cr` reduction and `cq` output channels (v3_vec_ok, conv3d.hip)"""
    lds, rk, cpt = _v3_constants()
    cqp = -(-cq // cpt) * cpt
    vec = cr % (8 if dt == BF16 else 4) == 0 and rk * cqp <= lds
    return min(taps, lds // (rk * cqp)), vec


def _taps(k):
    return k[0] * k[1] * k[2]


# ---- A. tap slicing of the LDS filter stage, the vector / scalar boundary, the half-load, dead threads ------------------------------
# (case, taps per slice of the forward pass, of the data gradient; None: that pass runs the scalar kernel)
CONV_A = [
    ((1, 3, 4, 9, 8, 40, (3, 3, 3), (1, 1, 1), F32), 25, 27),                 # forward slices 25 + 2
    ((1, 3, 4, 5, 16, 44, (3, 3, 3), (1, 1, 1), BF16), 21, None),             # cqp = 48: Cq % 8 != 0 inside a sliced stage
    ((2, 3, 5, 6, 64, 64, (3, 3, 3), (1, 1, 1), BF16), 16, 16),               # the width of a real U-Net: 16 + 11, both passes
    ((2, 3, 5, 6, 64, 64, (3, 3, 3), (1, 1, 1), F32), 16, 16),
    ((1, 4, 5, 7, 16, 72, (3, 3, 3), (2, 2, 2), F32), 14, 27),                # 14 + 13 under stride and asymmetric padding
    ((1, 2, 2, 4, 8, 1024, (3, 3, 3), (1, 1, 1), F32), 1, 27),                # 27 slices of one tap: the last vector-path width
    ((1, 2, 2, 4, 8, 1025, (3, 3, 3), (1, 1, 1), F32), None, None),           # the first width v3_vec_ok refuses: scalar kernels
    ((1, 3, 3, 5, 12, 8, (3, 3, 3), (1, 1, 1), F32), 27, 27),                 # `second` false on the last trip (r0 = 8)
    ((1, 3, 3, 5, 20, 8, (3, 3, 3), (1, 1, 1), F32), 27, 27),                 # ... (r0 = 16)
    ((1, 1, 1, 1, 8, 8, (3, 3, 3), (1, 1, 1), BF16), 27, 27),                 # one live thread of 256, the rest pass the barriers dead
    ((1, 1, 1, 2, 8, 8, (3, 3, 3), (1, 1, 1), BF16), 27, 27),
    ((1, 1, 1, 3, 8, 8, (3, 3, 3), (1, 1, 1), BF16), 27, 27),
]
TCONV_A = [
    ((1, 2, 3, 3, 16, 24, (4, 4, 4), (2, 2, 2), BF16), 42, 64),               # forward UP sliced 42 + 22
    ((1, 2, 3, 3, 24, 16, (4, 4, 4), (2, 2, 2), BF16), 64, 42),               # data gradient DOWN sliced 42 + 22
]


@pytest.mark.parametrize("case,tk_fwd,tk_dgrad", CONV_A)
def test_conv3d_sliced_stage_and_vector_path_edges(L, case, tk_fwd, tk_dgrad):
    B, D, H, W, Ci, Co, k, s, dt = case
    for (cr, cq, want) in ((Ci, Co, tk_fwd), (Co, Ci, tk_dgrad)):               # forward reduces Cin, the data gradient Cout
        tk, vec = _stage(_taps(k), cr, cq, dt)
        assert (tk if vec else None) == want, (cr, cq, tk, vec)
    _conv_family(L, False, B, D, H, W, Ci, Co, k, s, dt)


@pytest.mark.parametrize("case,tk_fwd,tk_dgrad", TCONV_A)
def test_tconv3d_sliced_stage(L, case, tk_fwd, tk_dgrad):
    B, D, H, W, Ci, Co, k, s, dt = case
    for (cr, cq, want) in ((Ci, Co, tk_fwd), (Co, Ci, tk_dgrad)):               # forward (UP) reduces Cin, the data gradient (DOWN) Cout
        tk, vec = _stage(_taps(k), cr, cq, dt)
        assert vec and tk == want, (cr, cq, tk, vec)
    _conv_family(L, True, B, D, H, W, Ci, Co, k, s, dt)


def test_both_directions_are_seen_sliced():
    """DOWN and UP fill the stage in different index orders: the cases above slice conv3D forward (DOWN) and its data gradient (UP),
    transposed_conv3D forward (UP) and its data gradient (DOWN)"""
    down = [c for c, f, d in CONV_A if f is not None and f < _taps(c[6])] + [c for c, f, d in TCONV_A if d < _taps(c[6])]
    up = [c for c, f, d in CONV_A if d is not None and d < _taps(c[6])] + [c for c, f, d in TCONV_A if f < _taps(c[6])]
    assert len(down) >= 2 and len(up) >= 2
    assert _stage(27, 8, 1024, F32) == (1, True) and not _stage(27, 8, 1025, F32)[1]


# ---- B. the 32-channel chunk loop of the direct filter gradients ---------------------------------------------------------------------
def _prefill(shape):
    """a pre-filled dw that differs from element to element, in eighths: fp32 sums onto it lose nothing the bound would see"""
    return (np.arange(int(np.prod(shape))) % 7).reshape(shape).astype(np.float32) * 0.125


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("inner", [33, 40, 64, 72])
@pytest.mark.parametrize("transposed", [False, True])
def test_volume_wgrad_channel_chunks(L, transposed, inner, dt):
    """phx_gconv3d_wgrad (inner = Cout) and phx_tconv3d_wgrad (inner = Cin): k_conv3_wgrad takes its second and third trip over Cb"""
    B, D, H, W = 2, 2, 3, 5
    if transposed:
        Ci, Co, k, s = inner, 3, (4, 4, 4), (2, 2, 2)
        xs, ys, ws = (B, D, H, W, Ci), (B, D * 2, H * 2, W * 2, Co), k + (Co, Ci)
        conv, fn = V.conv3d_transpose_same, L.tconv3d_wgrad
    else:
        Ci, Co, k, s = 3, inner, (3, 3, 3), (1, 1, 1)
        xs, ys, ws = (B, D, H, W, Ci), (B, D, H, W, Co), k + (Ci, Co)
        conv, fn = V.conv3d_same, L.gconv3d_wgrad
    x, dy = RNG.standard_normal(xs), RNG.standard_normal(ys)
    wr = torch.zeros(ws, dtype=torch.float64, requires_grad=True)
    (conv(rounded(x, dt), wr, s) * rounded(dy, dt)).sum().backward()
    pre = _prefill(ws)
    dw = dev(pre)
    xd, dyd = dev(x, dt), dev(dy, dt)
    fn(xd.data_ptr(), dt, dyd.data_ptr(), dt, dw.data_ptr(), B, D, H, W, Ci, Co, *k, *s, S())
    close(host(dw) - pre, wr.grad.numpy(), 6e-5, "wgrad over %d inner channels (accumulates)" % inner)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("inner", [40, 72])
def test_gconv2d_wgrad_channel_chunks(L, inner, dt):
    B, H, W, Ci, Co, geo = 2, 5, 6, 3, inner, (3, 3, 2, 1, 1, 2)                # kh, kw, sh, sw, dh, dw
    x = RNG.standard_normal((B, H, W, Ci))
    wr = torch.zeros(3, 3, Ci, Co, dtype=torch.float64, requires_grad=True)
    yr = T.conv2d_general_same(rounded(x, dt), wr, geo[2:4], geo[4:6])
    dy = RNG.standard_normal(tuple(yr.shape))
    (yr * rounded(dy, dt)).sum().backward()
    pre = _prefill((3, 3, Ci, Co))
    dw = dev(pre)
    xd, dyd = dev(x, dt), dev(dy, dt)
    L.gconv2d_wgrad(xd.data_ptr(), dt, dyd.data_ptr(), dt, dw.data_ptr(), B, H, W, Ci, Co, *geo, S())
    close(host(dw) - pre, wr.grad.numpy(), 3e-5 if dt == F32 else 2e-5, "gconv2d wgrad over %d output channels" % inner)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("inner", [40, 72])
def test_tconv2d_wgrad_channel_chunks(L, inner, dt):
    B, H, W, Ci, Co, geo = 2, 5, 6, inner, 3, (4, 4, 2, 2)                      # kh, kw, sh, sw
    x, dy = RNG.standard_normal((B, H, W, Ci)), RNG.standard_normal((B, 2 * H, 2 * W, Co))
    wr = torch.zeros(4, 4, Co, Ci, dtype=torch.float64, requires_grad=True)
    (T.conv2d_transpose_same(rounded(x, dt), wr, (2, 2)) * rounded(dy, dt)).sum().backward()
    pre = _prefill((4, 4, Co, Ci))
    dw = dev(pre)
    xd, dyd = dev(x, dt), dev(dy, dt)
    L.tconv2d_wgrad(xd.data_ptr(), dt, dyd.data_ptr(), dt, dw.data_ptr(), B, H, W, Ci, Co, *geo, S())
    close(host(dw) - pre, wr.grad.numpy(), 2e-5, "tconv2d wgrad over %d input channels" % inner)


# ---- C. past the grid cap: the grid-stride step of every one-thread-per-element launcher --------------------------------------------
def _capped(n, ragged=True):
    """n elements need a second grid-stride trip, and (where the case can choose) end in a partial block"""
    assert CAP < n <= 2 * CAP + CAP // 64, n
    assert not ragged or n % 256 != 0, n


def _fwd_dgrad(L, transposed, B, D, H, W, Ci, Co, k, s, dt, dgrad=True, bias=True, act=1, out_dt=None, bias_values=None):
    """forward (optional bias, any activation) and data gradient of one 3-D layer, each into a buffer pre-filled with 7.0;
    dt: storage of the tensors read, out_dt: of those written (the bound follows it).  -> (oracle pre-activation, kernel output)"""
    out_dt = dt if out_dt is None else out_dt
    x = RNG.standard_normal((B, D, H, W, Ci))
    w = RNG.standard_normal(tuple(k) + ((Co, Ci) if transposed else (Ci, Co))) / np.sqrt(_taps(k) * Ci)
    b = RNG.standard_normal(Co) * 0.3 if bias_values is None else np.asarray(bias_values, dtype=np.float64)
    xr = rounded(x, dt).requires_grad_(True)
    wr = torch.as_tensor(w, dtype=torch.float32).double()
    pre = (V.conv3d_transpose_same if transposed else V.conv3d_same)(xr, wr, s)
    full = V.bias_add(pre, torch.as_tensor(b, dtype=torch.float32).double()) if bias else pre
    yr = full if act == 0 else torch.relu(full) if act == 1 else torch.nn.functional.softplus(full, threshold=1e9)
    fwd, dgr = (L.tconv3d_fwd, L.tconv3d_dgrad) if transposed else (L.gconv3d_fwd, L.gconv3d_dgrad)
    xd, wd, bd = dev(x, dt), dev(w), dev(b)
    y = torch.full(tuple(yr.shape), 7.0, dtype=tdt(out_dt)).cuda()
    geo = (B, D, H, W, Ci, Co, *k, *s)
    fwd(xd.data_ptr(), dt, wd.data_ptr(), bd.data_ptr() if bias else None, y.data_ptr(), out_dt, *geo, act, S())
    tol = 4e-5 if out_dt == F32 else 1.6e-2
    close(host(y), yr.detach().numpy(), tol, "fwd")
    if dgrad:                                                                 # dy in the input's storage, dx in the output's
        dy = RNG.standard_normal(tuple(yr.shape))
        (pre * rounded(dy, dt)).sum().backward()
        dx = torch.full(tuple(x.shape), 7.0, dtype=tdt(out_dt)).cuda()
        dyd = dev(dy, dt)
        dgr(dyd.data_ptr(), dt, wd.data_ptr(), dx.data_ptr(), out_dt, *geo, S())
        close(host(dx), xr.grad.numpy(), tol, "dgrad")
    return full.detach().numpy(), host(y)


def test_grid_cap_conv3d_scalar_fwd_dgrad(L):
    """k_conv3_down / k_conv3_up; 2 600 960 elements each way (this shape's count is a multiple of 256: the ragged tails are the
    other cases').  No filter gradient here: it has no capped grid."""
    case = (2, 16, 128, 127, 5, 5, (3, 3, 3), (1, 1, 1), F32)
    _capped(2 * 16 * 128 * 127 * 5, ragged=False)
    assert not _stage(27, 5, 5, F32)[1]
    _fwd_dgrad(L, False, *case)


def test_grid_cap_tconv3d_scalar_fwd(L):
    """k_conv3_up as the transposed layer's forward pass, 2 580 480 outputs"""
    case = (1, 8, 64, 63, 3, 10, (4, 4, 4), (2, 2, 2), F32)
    _capped(16 * 128 * 126 * 10, ragged=False)
    assert not _stage(64, 3, 10, F32)[1]
    _fwd_dgrad(L, True, *case, dgrad=False)


def test_grid_cap_maxpool3d(L):
    B, D, H, W, C, win = 1, 6, 129, 1301, 5, (1, 1, 2)
    _capped(B * D * H * ((W + 1) // 2) * C)                                    # the launch counts OUTPUT elements
    x = RNG.standard_normal((B, D, H, W, C))
    xr = rounded(x, F32).requires_grad_(True)
    yr = V.max_pool3d_same(xr, win)
    xd = dev(x)
    y = torch.full(tuple(yr.shape), 7.0).cuda()
    L.maxpool3d_fwd(xd.data_ptr(), F32, y.data_ptr(), B, D, H, W, C, *win, S())
    assert torch.equal(y.cpu().double(), yr.detach())
    dy = RNG.standard_normal(tuple(yr.shape))
    (yr * rounded(dy, F32)).sum().backward()
    dx = torch.full_like(xd, 7.0)
    dyd = dev(dy)
    L.maxpool3d_bwd(xd.data_ptr(), dyd.data_ptr(), F32, dx.data_ptr(), B, D, H, W, C, *win, S())
    assert torch.equal(dx.cpu().double(), xr.grad)


def test_grid_cap_bilinear_up3d(L):
    """forward (the launch counts the 8x output), adjoint and its accumulating form (they count the input): one oracle for the three"""
    B, D, H, W, C = 1, 3, 90, 101, 77
    _capped(B * D * H * W * C)
    x = RNG.standard_normal((B, D, H, W, C))
    xr = rounded(x, F32).requires_grad_(True)
    yr = V.bilinear_up2x_3d(xr)
    xd = dev(x)
    y = torch.full(tuple(yr.shape), 7.0).cuda()
    L.bilinear_up2x_3d_fwd(xd.data_ptr(), F32, y.data_ptr(), B, D, H, W, C, S())
    close(host(y), yr.detach().numpy(), 1e-6, "up3d fwd")
    dy = RNG.standard_normal(tuple(yr.shape)).astype(np.float32)
    yr.backward(torch.as_tensor(dy).double())
    dyd = dev(dy)
    dx = torch.full_like(xd, 7.0)
    L.bilinear_up2x_3d_bwd(dyd.data_ptr(), F32, dx.data_ptr(), B, D, H, W, C, S())
    close(host(dx), xr.grad.numpy(), 1e-6, "up3d bwd")
    acc = torch.full_like(xd, 0.5)
    L.bilinear_up2x_3d_bwd_acc(dyd.data_ptr(), F32, acc.data_ptr(), B, D, H, W, C, S())
    close(host(acc) - 0.5, xr.grad.numpy(), 1e-6, "up3d bwd (accumulates)")


def _window(x, out_shape, off):
    """dst[b, i.., :] = src[b, i + off.., :] inside the source, 0 outside: numpy slices over any number of spatial axes"""
    want = np.zeros((x.shape[0],) + tuple(out_shape) + (x.shape[-1],), dtype=x.dtype)
    d, s = [slice(None)], [slice(None)]
    for n_dst, n_src, o in zip(out_shape, x.shape[1:-1], off):
        lo, hi = max(0, -o), min(n_dst, n_src - o)
        assert lo < hi
        d.append(slice(lo, hi)), s.append(slice(lo + o, hi + o))
    want[tuple(d)] = x[tuple(s)]
    return want


def test_grid_cap_spatial_window3d(L):
    src, dst, off = (20, 129, 99), (21, 131, 97), (-1, 1, 2)
    _capped(21 * 131 * 97 * 8)
    x = RNG.standard_normal((1,) + src + (8,)).astype(np.float32)
    out = torch.full((1,) + dst + (8,), 7.0).cuda()
    xd = dev(x)
    L.spatial_window3d(xd.data_ptr(), out.data_ptr(), F32, 1, *src, *dst, 8, *off, S())
    assert np.array_equal(out.cpu().numpy(), _window(x, dst, off))


def test_grid_cap_gconv2d_fwd_dgrad(L):
    B, H, W, Ci, Co, geo = 3, 401, 351, 5, 5, (3, 3, 1, 1, 1, 1)
    _capped(B * H * W * Co)
    x = RNG.standard_normal((B, H, W, Ci))
    w = RNG.standard_normal((3, 3, Ci, Co)) / np.sqrt(9 * Ci)
    b = RNG.standard_normal(Co) * 0.3
    xr = rounded(x, F32).requires_grad_(True)
    wr = torch.as_tensor(w, dtype=torch.float32).double()
    pre = T.conv2d_general_same(xr, wr, (1, 1), (1, 1))
    yr = T.relu(pre + torch.as_tensor(b, dtype=torch.float32).double())
    xd, wd, bd = dev(x), dev(w), dev(b)
    y = torch.full((B, H, W, Co), 7.0).cuda()
    L.gconv2d_fwd(xd.data_ptr(), F32, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), F32, B, H, W, Ci, Co, *geo, 1, S())
    close(host(y), yr.detach().numpy(), 2e-5, "gconv2d fwd")
    dy = RNG.standard_normal((B, H, W, Co))
    (pre * rounded(dy, F32)).sum().backward()
    dx = torch.full_like(xd, 7.0)
    dyd = dev(dy)
    L.gconv2d_dgrad(dyd.data_ptr(), F32, wd.data_ptr(), dx.data_ptr(), F32, B, H, W, Ci, Co, *geo, S())
    close(host(dx), xr.grad.numpy(), 2e-5, "gconv2d dgrad")


def test_grid_cap_tconv2d_fwd_dgrad(L):
    B, H, W, Ci, Co, geo = 1, 401, 527, 10, 3, (4, 4, 2, 2)
    _capped(B * 2 * H * 2 * W * Co), _capped(B * H * W * Ci)
    x = RNG.standard_normal((B, H, W, Ci))
    w = RNG.standard_normal((4, 4, Co, Ci)) / np.sqrt(16 * Ci)
    b = RNG.standard_normal(Co) * 0.3
    xr = rounded(x, F32).requires_grad_(True)
    wr = torch.as_tensor(w, dtype=torch.float32).double()
    pre = T.conv2d_transpose_same(xr, wr, (2, 2))
    yr = T.relu(pre + torch.as_tensor(b, dtype=torch.float32).double())
    xd, wd, bd = dev(x), dev(w), dev(b)
    y = torch.full((B, 2 * H, 2 * W, Co), 7.0).cuda()
    L.tconv2d_fwd(xd.data_ptr(), F32, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), F32, B, H, W, Ci, Co, *geo, 1, S())
    close(host(y), yr.detach().numpy(), 1e-5, "tconv2d fwd")
    dy = RNG.standard_normal((B, 2 * H, 2 * W, Co))
    (pre * rounded(dy, F32)).sum().backward()
    dx = torch.full_like(xd, 7.0)
    dyd = dev(dy)
    L.tconv2d_dgrad(dyd.data_ptr(), F32, wd.data_ptr(), dx.data_ptr(), F32, B, H, W, Ci, Co, *geo, S())
    close(host(dx), xr.grad.numpy(), 1e-5, "tconv2d dgrad")


def test_grid_cap_maxpool2x2(L):
    B, H, W, C = 3, 801, 701, 5
    _capped(B * 401 * 351 * C)
    x = RNG.standard_normal((B, H, W, C))
    xr = rounded(x, F32).requires_grad_(True)
    yr = T.max_pool_2x2_same(xr)
    xd = dev(x)
    y = torch.full(tuple(yr.shape), 7.0).cuda()
    L.maxpool2x2_fwd(xd.data_ptr(), F32, y.data_ptr(), B, H, W, C, S())
    assert torch.equal(y.cpu().double(), yr.detach())
    dy = RNG.standard_normal(tuple(yr.shape))
    (yr * rounded(dy, F32)).sum().backward()
    dx = torch.full_like(xd, 7.0)
    dyd = dev(dy)
    L.maxpool2x2_bwd(xd.data_ptr(), dyd.data_ptr(), F32, dx.data_ptr(), B, H, W, C, S())
    assert torch.equal(dx.cpu().double(), xr.grad)


def test_grid_cap_spatial_window_and_window4(L):
    src, dst, off = (399, 353), (401, 351), (-1, 1)
    _capped(3 * 401 * 351 * 5)
    x = RNG.standard_normal((3,) + src + (5,)).astype(np.float32)
    out = torch.full((3,) + dst + (5,), 7.0).cuda()
    xd = dev(x)
    L.spatial_window(xd.data_ptr(), out.data_ptr(), F32, 3, *src, *dst, 5, *off, S())
    assert np.array_equal(out.cpu().numpy(), _window(x, dst, off))
    # zero-padded channels (1 in front, 1 behind) + [:, :, ::2, :]: the forward counts the destination, the gradient the source
    Bs, Hs, Ws, Cs, Wd, Cd = 3, 401, 701, 5, 351, 7
    _capped(Bs * Hs * Wd * Cd), _capped(Bs * Hs * Ws * Cs)
    x = RNG.standard_normal((Bs, Hs, Ws, Cs)).astype(np.float32)
    geo = (Bs, Hs, Ws, Cs, Hs, Wd, Cd, 1, 2, 0, 0, -1)
    out = torch.full((Bs, Hs, Wd, Cd), 7.0).cuda()
    xd = dev(x)
    L.window4_fwd(xd.data_ptr(), out.data_ptr(), F32, *geo, S())
    assert np.array_equal(out.cpu().numpy(), np.pad(x, ((0, 0), (0, 0), (0, 0), (1, 1)))[:, :, ::2, :])
    d = RNG.standard_normal((Bs, Hs, Wd, Cd)).astype(np.float32)
    dx = torch.full((Bs, Hs, Ws, Cs), 7.0).cuda()
    dd = dev(d)
    L.window4_bwd(dd.data_ptr(), dx.data_ptr(), F32, *geo, S())
    ref = np.zeros_like(x)
    ref[:, :, ::2, :] = d[..., 1:6]
    assert np.array_equal(dx.cpu().numpy(), ref)


def test_grid_cap_add_act(L):
    n = CAP + 2849
    _capped(n)
    a, b = dev(RNG.standard_normal(n)), dev(RNG.standard_normal(n))
    y = torch.full_like(a, 7.0)
    L.add_act(a.data_ptr(), b.data_ptr(), y.data_ptr(), F32, n, 1, S())
    assert torch.equal(y, torch.relu(a + b))


def test_grid_cap_dropout(L):
    """The launch counts Philox blocks of four elements: 2 x 4 200 003 elements are 2 100 002 blocks, each sample ending in a partial
    one.  The host Philox oracle (oracle.tf1_ops.dropout_keep_mask) takes 1.2 s for this size on the CPU
    (0.26 s for the whole case on the GPU machine's host), under the 5 s that decide whether dropout is part of this group."""
    B, per = 2, 4200003
    _capped(B * ((per + 3) // 4))
    x = RNG.standard_normal((B, per)).astype(np.float32)
    xd = dev(x)
    step = torch.tensor([4], dtype=torch.int32).cuda()
    y = torch.full_like(xd, 7.0)
    L.dropout(xd.data_ptr(), y.data_ptr(), F32, per, B, 0.7, 1234567890123, step.data_ptr(), 99, 5, S())
    keep = T.dropout_keep_mask((B, per), 0.7, 1234567890123, 4, 99, sample_offset=5)
    close(y.cpu().numpy(), np.where(keep, x / np.float32(0.7), np.float32(0.0)), 1e-6, "dropout")


# ---- D. geometry by one-hot filters, exact --------------------------------------------------------------------------------------------
IMPULSE_SETS = [((3, 3, 3), (1, 1, 1)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (1, 2, 3)), ((1, 1, 1), (2, 2, 2))]


def _np_storage(a, dt):
    """values representable in the storage type, as fp32 numpy"""
    return torch.as_tensor(a, dtype=torch.float32).to(tdt(dt)).float().numpy()


@pytest.mark.parametrize("entry", ["gconv3d_fwd", "gconv3d_dgrad", "tconv3d_fwd"])
@pytest.mark.parametrize("k,s", IMPULSE_SETS)
@pytest.mark.parametrize("path", ["vector", "scalar"])
def test_impulse_filters_pin_padding_and_offsets_exactly(L, path, k, s, entry):
    """Every tap of the set as the one-hot filter w[tap][a][b] = 1, NULL bias, act = 0: the kernel's output is fmaf(x, 1, 0) plus exact
    zeros, so it equals V.impulse_conv3d_same / _adjoint (np.pad and slicing, no convolution) bit for bit, in fp32 and in bf16."""
    ext = (4, 5, 7)
    # filter [tap][ca][cb], big-side and small-side channels; 8 -> 8 on the vector path, 3 -> 5 on the scalar one
    ca, cb = (8, 8) if path == "vector" else (5, 3) if entry == "tconv3d_fwd" else (3, 5)
    small = tuple(V.same_pads(ext[i], k[i], s[i])[0] for i in range(3))
    for dt in (F32, BF16):
        cr = {"gconv3d_fwd": ca, "gconv3d_dgrad": cb, "tconv3d_fwd": cb}[entry]
        assert _stage(_taps(k), cr, ca + cb - cr, dt)[1] == (path == "vector")
        if entry == "gconv3d_fwd":                                            # x [.., Cin = ca] -> y [.., Cout = cb]
            src = _np_storage(RNG.standard_normal((1,) + ext + (ca,)), dt)
            oshape = (1,) + small + (cb,)
        elif entry == "gconv3d_dgrad":                                        # dy [.., Cout = cb] -> dx [.., Cin = ca]
            src = _np_storage(RNG.standard_normal((1,) + small + (cb,)), dt)
            oshape = (1,) + ext + (ca,)
        else:                                                                 # x [.., Cin = cb] -> y [.., Cout = ca], extent in * s
            src = _np_storage(RNG.standard_normal((1,) + ext + (cb,)), dt)
            oshape = (1,) + tuple(ext[i] * s[i] for i in range(3)) + (ca,)
        sd = dev(src, dt)
        w = torch.zeros(tuple(k) + (ca, cb)).cuda()
        for t, tap in enumerate(np.ndindex(*k)):
            a, b = t % ca, (2 * t + 1) % cb
            w.zero_()
            w[tap][a, b] = 1.0
            out = torch.full(oshape, 7.0, dtype=tdt(dt)).cuda()
            if entry == "gconv3d_fwd":
                L.gconv3d_fwd(sd.data_ptr(), dt, w.data_ptr(), None, out.data_ptr(), dt, 1, *ext, ca, cb, *k, *s, 0, S())
                want = V.impulse_conv3d_same(src, k, s, tap, a, b, cb)
            elif entry == "gconv3d_dgrad":
                L.gconv3d_dgrad(sd.data_ptr(), dt, w.data_ptr(), out.data_ptr(), dt, 1, *ext, ca, cb, *k, *s, S())
                want = V.impulse_conv3d_same_adjoint(src, ext, k, s, tap, a, b, ca)
            else:
                L.tconv3d_fwd(sd.data_ptr(), dt, w.data_ptr(), None, out.data_ptr(), dt, 1, *ext, cb, ca, *k, *s, 0, S())
                want = V.impulse_conv3d_same_adjoint(src, oshape[1:4], k, s, tap, a, b, ca)
            got = out.float().cpu() + 0.0                                     # -0 -> +0
            assert torch.equal(got, torch.as_tensor(want) + 0.0), (entry, dt, tap, float((got - torch.as_tensor(want)).abs().max()))


# ---- E. transposed geometries with k < s --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [
    (2, 3, 2, 4, 8, 5, (1, 1, 1), (2, 2, 2), F32),                            # forward on the vector path, data gradient scalar
    (1, 2, 3, 3, 4, 8, (2, 1, 3), (3, 2, 2), F32),
    (1, 2, 3, 2, 8, 8, (1, 2, 1), (2, 3, 2), BF16),
])
def test_tconv3d_kernel_smaller_than_stride(L, case):
    B, D, H, W, Ci, Co, k, s, dt = case
    assert any(k[i] < s[i] for i in range(3))
    _conv_family(L, True, B, D, H, W, Ci, Co, k, s, dt)


# ---- F. epilogue branches and dtype pairs -----------------------------------------------------------------------------------------------
PATHS = [("vector", 8, 16), ("scalar", 5, 6)]


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("path,Ci,Co", PATHS)
def test_null_bias_forward(L, path, Ci, Co, transposed):
    k, s = ((4, 4, 4), (2, 2, 2)) if transposed else ((3, 3, 3), (1, 1, 1))
    assert _stage(_taps(k), Ci, Co, F32)[1] == (path == "vector")
    for act in (0, 1):
        _fwd_dgrad(L, transposed, 2, 3, 5, 6, Ci, Co, k, s, F32, dgrad=False, bias=False, act=act)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("path,Ci,Co", PATHS)
def test_softplus_and_identity_epilogue(L, path, Ci, Co, transposed):
    """act = 2 returns v itself above 20 and log1p(exp(v)) below: biases of +24, -24 and about 0 put whole channels on either side.
    Beside the file's metric over the whole tensor, the classes +24 and 0 meet it on their own.  The class -24 (values near exp(-24),
    invisible to a metric relative to 24) is held to a relative bound by reasoning: softplus(v) ~ exp(v) there, so its relative error
    is the absolute error of v -- at most one rounding of a value below 32, 2^-24 x 32 = 2^-19, per accumulated term and for the bias
    -- plus a few units of expf and log1pf (4 x 2^-19 covers them many times over)."""
    k, s = ((4, 4, 4), (2, 2, 2)) if transposed else ((3, 3, 3), (1, 1, 1))
    b = np.where(np.arange(Co) % 3 == 0, 24.0, np.where(np.arange(Co) % 3 == 1, -24.0, 0.0)) + 0.25 * RNG.standard_normal(Co)
    pre, y = _fwd_dgrad(L, transposed, 2, 3, 5, 6, Ci, Co, k, s, F32, dgrad=False, act=2, bias_values=b)
    assert (pre > 20.0).any() and (pre < -20.0).any() and (np.abs(pre) < 5.0).any()
    want = np.logaddexp(0.0, pre)                                             # softplus in float64 without a threshold
    for c in (0, 2):
        close(y[..., c::3], want[..., c::3], 4e-5, "softplus, bias class %d" % c)
    rel = np.abs(y[..., 1::3] / want[..., 1::3] - 1.0).max()
    print("softplus, bias class 1: relative %.3e (bound %.1e)" % (rel, (_taps(k) * Ci + 4) * 2.0 ** -19))
    assert rel < (_taps(k) * Ci + 4) * 2.0 ** -19
    _fwd_dgrad(L, transposed, 2, 3, 5, 6, Ci, Co, k, s, F32, dgrad=False, act=0, bias_values=b)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("path,Ci,Co", PATHS)
@pytest.mark.parametrize("dt,out_dt", [(BF16, F32), (F32, BF16)])
def test_mixed_dtype_pairs(L, dt, out_dt, path, Ci, Co, transposed):
    """bf16 in -> fp32 out and fp32 in -> bf16 out of phx_gconv3d_fwd / _dgrad and phx_tconv3d_fwd (and its _dgrad): the oracle sees the
    input rounded to its storage type, the bound follows the output type"""
    k, s = ((4, 4, 4), (2, 2, 2)) if transposed else ((3, 3, 3), (1, 2, 1))
    for (cr, cq) in ((Ci, Co), (Co, Ci)):                                       # 8 and 16 pass v3_vec_ok for either input type
        assert _stage(_taps(k), cr, cq, dt)[1] == (path == "vector")
    _fwd_dgrad(L, transposed, 2, 3, 5, 6, Ci, Co, k, s, dt, out_dt=out_dt)


# ---- G. phx_bn_moving_update_biased ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [0.01, 1.0])
@pytest.mark.parametrize("C", [1, 255, 256, 257, 600])
def test_bn_moving_update_biased(L, C, momentum):
    """moving_mean -= (moving_mean - mean) m, moving_var -= (moving_var - var) m with var = max(1 / rstd^2 - eps, 0), expected in float64
    from the fp32 inputs.  Bound, u = 2^-24 per fp32 operation: the mean takes a difference, a product and a difference of values no
    larger than |mm| + |mean| -> 2u (|mm| + |mean|); var is rstd^2, a reciprocal and a difference at the scale var + eps (3u), one more u
    for the difference to mv, all scaled by m -> 4u m (var + eps), plus the last difference at the scale of mv -> 2u |mv|.  (The mean's
    bound is a worst case.  The variance's is not quite one: at m = 1 and var >> mv, five roundings at the scale of var all falling the
    same way would give 5u var; it is kept as stated, and the inputs are a fixed stream.  Measured on the MI355X: the mean at most 0.70
    of its bound, the variance at most 0.48.)"""
    eps = np.float32(1e-3)
    var_in = np.array([0.0, 1e-8, 1e-3, 1.0, 1e4], dtype=np.float32)[(np.arange(C) + C) % 5]
    rstd = (np.float32(1.0) / np.sqrt(var_in + eps)).astype(np.float32)
    rng = np.random.default_rng(1000 + C)                                      # (its own stream: the same values whatever ran before)
    mean = rng.standard_normal(C).astype(np.float32)
    mm0 = rng.standard_normal(C).astype(np.float32)
    mv0 = np.abs(rng.standard_normal(C)).astype(np.float32)
    mv0[::7] = 0.0                                                             # starts AT zero too
    m32 = np.float32(momentum)
    var = np.maximum(1.0 / rstd.astype(np.float64) ** 2 - np.float64(eps), 0.0)
    want_mm = mm0.astype(np.float64) - (mm0.astype(np.float64) - mean.astype(np.float64)) * np.float64(m32)
    want_mv = mv0.astype(np.float64) - (mv0.astype(np.float64) - var) * np.float64(m32)
    mm, mv = dev(mm0), dev(mv0)
    meand, rstdd = dev(mean), dev(rstd)
    L.bn_moving_update_biased(meand.data_ptr(), rstdd.data_ptr(), float(eps), mm.data_ptr(), mv.data_ptr(), float(m32), C, S())
    u = 2.0 ** -24
    got_mm, got_mv = mm.cpu().numpy().astype(np.float64), mv.cpu().numpy().astype(np.float64)
    e_mm = np.abs(got_mm - want_mm) / (2 * u * (np.abs(mm0) + np.abs(mean)).astype(np.float64))
    e_mv = np.abs(got_mv - want_mv) / (float(m32) * 4 * u * (var + np.float64(eps)) + 2 * u * np.abs(mv0).astype(np.float64))
    print("moving mean: %.3f of its bound, moving variance: %.3f of its bound" % (e_mm.max(), e_mv.max()))
    assert e_mm.max() <= 1.0 and e_mv.max() <= 1.0, (e_mm.max(), e_mv.max(), int(e_mv.argmax()))
    assert (got_mv >= 0.0).all()


def test_bn_moving_update_biased_refusals(L):
    dll = L._dll
    C = 300
    bufs = [torch.full((C,), v, device="cuda") for v in (0.5, 2.0, 3.0, 4.0)]   # mean, rstd, moving mean, moving variance
    p = [ctypes.c_void_p(t.data_ptr()) for t in bufs]
    s = ctypes.c_void_p(S())
    assert dll.phx_bn_moving_update_biased(p[0], p[1], 1e-3, p[2], p[3], 0.0, C, s) == PHX_E_INVAL
    assert dll.phx_bn_moving_update_biased(p[0], p[1], 1e-3, p[2], p[3], 1.5, C, s) == PHX_E_INVAL
    assert dll.phx_bn_moving_update_biased(p[0], p[1], 1e-3, p[2], p[3], 0.5, 0, s) == PHX_E_INVAL
    for i in range(4):
        q = list(p)
        q[i] = None
        assert dll.phx_bn_moving_update_biased(q[0], q[1], 1e-3, q[2], q[3], 0.5, C, s) == PHX_E_INVAL
    torch.cuda.synchronize()
    for t, v in zip(bufs, (0.5, 2.0, 3.0, 4.0)):
        assert bool((t == v).all())
    with pytest.raises(Exception, match="bn_moving_update_biased"):
        L.bn_moving_update_biased(p[0].value, p[1].value, 1e-3, p[2].value, p[3].value, 0.0, C, S())


# ---- H. pools and up-sampling on axes of extent 1 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("shape", [(2, 1, 5, 1, 3), (1, 3, 1, 7, 16)])
def test_maxpool3d_every_window_on_unit_axes(L, shape, dt):
    B, D, H, W, C = shape
    for win in np.ndindex(2, 2, 2):
        win = tuple(int(v) + 1 for v in win)
        x = RNG.standard_normal(shape)
        x[0, :2, :2, :2, 0] = 0.0                                             # what exists of the first window ties at zero ...
        xr = rounded(x, dt).requires_grad_(True)
        yr = V.max_pool3d_same(xr, win)
        assert tuple(yr.shape) == (B, -(-D // win[0]), -(-H // win[1]), -(-W // win[2]), C)
        xd = dev(x, dt)
        y = torch.full(tuple(yr.shape), 7.0, dtype=tdt(dt)).cuda()
        L.maxpool3d_fwd(xd.data_ptr(), dt, y.data_ptr(), B, D, H, W, C, *win, S())
        assert np.array_equal(host(y), yr.detach().numpy()), win
        dy = RNG.standard_normal(tuple(yr.shape))
        (yr * rounded(dy, dt)).sum().backward()
        dyd = dev(dy, dt)
        dx = torch.full_like(xd, 7.0)
        L.maxpool3d_bwd(xd.data_ptr(), dyd.data_ptr(), dt, dx.data_ptr(), B, D, H, W, C, *win, S())
        g = host(dx)
        assert np.array_equal(g, xr.grad.numpy()), win
        first = g[0, :win[0], :win[1], :win[2], 0].reshape(-1)                 # ... and its first element alone takes the gradient
        assert first[0] == host(dyd)[0, 0, 0, 0, 0] and not first[1:].any(), win


@pytest.mark.parametrize("case", [(1, 1, 3, 4, 5, F32), (2, 3, 1, 1, 6, F32), (1, 1, 1, 1, 16, F32),
                                  (1, 1, 3, 4, 5, BF16), (2, 3, 1, 1, 6, BF16), (1, 1, 1, 1, 16, BF16)])
def test_bilinear_up3d_on_unit_axes(L, case):
    """forward, adjoint, its accumulating form and (fp32) the identity <up(x), dy> = <x, up^T(dy)>: the existing test's body at these shapes"""
    K.test_bilinear_up3d_fwd_bwd_and_adjoint(L, case)
