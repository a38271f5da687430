"""csrc/conv3d.hip through the C ABI against the float64 oracle (tests/volume_ref.py: torch-CPU restatements, independent of the
kernels): conv3D / transposed_conv3D forward and both gradients on the vector path and the scalar fallback, maxpool3D,
bilinear_upsample3D and its adjoint, the 5-D window, the refusals, and bit-identical repeats.  The metric is that of
tests/test_extra_layers_gpu.py -- max abs error over max abs reference -- with operands rounded to the storage type before the oracle
sees them.  Convolution bounds: the 2-D test's values times 2 (the reduction is up to 3x longer, the fp32 rounding error grows with its
square root): 4e-5 (fp32) / 1.6e-2 (bf16) forward and data gradient, 6e-5 filter gradient."""
import ctypes

import numpy as np
import pytest
import torch

from tests import volume_ref as V

pytestmark = pytest.mark.gpu
F32, BF16 = 0, 1
RNG = np.random.default_rng(23)
PHX_E_SHAPE = -2


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


def close(a, b, tol, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() / max(1e-12, np.abs(b).max())
    print("%s: %.3e (bound %.1e)" % (what, err, tol))
    assert err < tol, (what, err)


def host(t):
    return t.float().cpu().numpy()


def _conv_family(L, transposed, B, D, H, W, Ci, Co, k, s, dt):
    """forward (bias + ReLU epilogue), data gradient, filter gradient (accumulating into a pre-filled dw) of one layer"""
    x = RNG.standard_normal((B, D, H, W, Ci))
    fan = k[0] * k[1] * k[2] * Ci
    w = RNG.standard_normal(tuple(k) + ((Co, Ci) if transposed else (Ci, Co))) / np.sqrt(fan)
    b = RNG.standard_normal(Co) * 0.3
    xr = rounded(x, dt).requires_grad_(True)
    wr = torch.as_tensor(w, dtype=torch.float32).double().requires_grad_(True)
    conv = (lambda: V.conv3d_transpose_same(xr, wr, s)) if transposed else (lambda: V.conv3d_same(xr, wr, s))
    yr = torch.relu(V.bias_add(conv(), torch.as_tensor(b, dtype=torch.float32).double()))
    oshape = tuple(yr.shape)
    if not transposed:
        o = [ctypes.c_int() for _ in range(3)]
        L.gconv3d_out_size(D, H, W, *s, *[ctypes.byref(v) for v in o])
        assert tuple(v.value for v in o) == oshape[1:4]
    else:
        assert oshape[1:4] == (D * s[0], H * s[1], W * s[2])
    fwd, dgrad, wgrad = (L.tconv3d_fwd, L.tconv3d_dgrad, L.tconv3d_wgrad) if transposed else (L.gconv3d_fwd, L.gconv3d_dgrad, L.gconv3d_wgrad)
    xd, wd, bd = dev(x, dt), dev(w), dev(b)
    y = torch.empty(oshape, dtype=tdt(dt)).cuda()
    geo = (B, D, H, W, Ci, Co, *k, *s)
    fwd(xd.data_ptr(), dt, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), dt, *geo, 1, S())
    tol = 4e-5 if dt == F32 else 1.6e-2
    close(host(y), yr.detach().numpy(), tol, "fwd")
    dy = RNG.standard_normal(oshape)
    (conv() * rounded(dy, dt)).sum().backward()                                 # gradients of the un-activated convolution
    dyd = dev(dy, dt)
    dx = torch.full_like(xd, 7.0)
    dgrad(dyd.data_ptr(), dt, wd.data_ptr(), dx.data_ptr(), dt, *geo, S())
    close(host(dx), xr.grad.numpy(), tol, "dgrad")
    dwd = torch.full(tuple(w.shape), 0.25, dtype=torch.float32).cuda()
    wgrad(xd.data_ptr(), dt, dyd.data_ptr(), dt, dwd.data_ptr(), *geo, S())
    close(host(dwd) - 0.25, wr.grad.numpy(), 6e-5, "wgrad (accumulates)")


@pytest.mark.parametrize("case", [
    (2, 5, 7, 6, 5, 6, (3, 3, 3), (1, 1, 1), F32),         # scalar path
    (2, 6, 9, 7, 8, 16, (3, 3, 3), (2, 2, 2), F32),        # odd extent under stride, asymmetric pad
    (1, 4, 8, 8, 16, 8, (1, 1, 1), (1, 2, 2), F32),
    (2, 5, 6, 7, 16, 32, (3, 1, 2), (1, 2, 1), BF16),      # non-cubic kernel, even tap
    (2, 8, 8, 8, 32, 32, (3, 3, 3), (1, 1, 1), BF16),      # fast path
    (1, 3, 5, 4, 33, 7, (3, 3, 3), (1, 1, 1), BF16),       # fallback beside the fast path
])
def test_conv3d_fwd_dgrad_wgrad(L, case):
    B, D, H, W, Ci, Co, k, s, dt = case
    _conv_family(L, False, B, D, H, W, Ci, Co, k, s, dt)


@pytest.mark.parametrize("case", [
    (2, 3, 4, 5, 6, 4, (4, 4, 4), (2, 2, 2), F32),
    (2, 4, 4, 4, 16, 8, (4, 4, 4), (2, 2, 2), BF16),
    (1, 3, 5, 4, 5, 3, (3, 3, 3), (1, 2, 2), F32),
])
def test_tconv3d_fwd_dgrad_wgrad(L, case):
    B, D, H, W, Ci, Co, k, s, dt = case
    _conv_family(L, True, B, D, H, W, Ci, Co, k, s, dt)


@pytest.mark.parametrize("case", [(2, 5, 7, 6, 3, (2, 2, 2), F32), (2, 4, 6, 8, 16, (1, 2, 2), BF16)])
def test_maxpool3d_fwd_bwd(L, case):
    B, D, H, W, C, win, dt = case
    x = RNG.standard_normal((B, D, H, W, C))
    x[0, :2, :2, :2, 0] = 0.0                                                  # a window of ties (ReLU zeros): the first element wins
    x[1, 0, 0:2, 0:2, 1] = 0.0
    xr = rounded(x, dt).requires_grad_(True)
    yr = V.max_pool3d_same(xr, win)
    xd = dev(x, dt)
    y = torch.empty(tuple(yr.shape), dtype=tdt(dt)).cuda()
    L.maxpool3d_fwd(xd.data_ptr(), dt, y.data_ptr(), B, D, H, W, C, *win, S())
    close(host(y), yr.detach().numpy(), 1e-7, "maxpool3d fwd")
    dy = RNG.standard_normal(tuple(yr.shape))
    (yr * rounded(dy, dt)).sum().backward()
    dyd = dev(dy, dt)
    dx = torch.full_like(xd, 7.0)
    L.maxpool3d_bwd(xd.data_ptr(), dyd.data_ptr(), dt, dx.data_ptr(), B, D, H, W, C, *win, S())
    close(host(dx), xr.grad.numpy(), 1e-7, "maxpool3d bwd")
    g = host(dx)
    assert g[0, 0, 0, 0, 0] == host(dyd)[0, 0, 0, 0, 0] and not g[0, :win[0], :2, :2, 0].reshape(-1)[1:].any()   # tie -> first element only


@pytest.mark.parametrize("case", [(2, 3, 5, 4, 6, F32), (1, 4, 4, 4, 16, BF16)])
def test_bilinear_up3d_fwd_bwd_and_adjoint(L, case):
    B, D, H, W, C, dt = case
    x = RNG.standard_normal((B, D, H, W, C))
    xr = rounded(x, dt).requires_grad_(True)
    yr = V.bilinear_up2x_3d(xr)
    xd = dev(x, dt)
    y = torch.empty(B, 2 * D, 2 * H, 2 * W, C, dtype=tdt(dt)).cuda()
    L.bilinear_up2x_3d_fwd(xd.data_ptr(), dt, y.data_ptr(), B, D, H, W, C, S())
    tol = 1e-6 if dt == F32 else 2.0 ** -8                                     # one bf16 rounding: half a unit in the last of 8 bits
    close(host(y), yr.detach().numpy(), tol, "up3d fwd")
    dy = RNG.standard_normal(tuple(yr.shape))
    (yr * rounded(dy, dt)).sum().backward()
    dyd = dev(dy, dt)
    dx = torch.full_like(xd, 7.0)
    L.bilinear_up2x_3d_bwd(dyd.data_ptr(), dt, dx.data_ptr(), B, D, H, W, C, S())
    close(host(dx), xr.grad.numpy(), tol, "up3d bwd")
    if dt == F32:
        lhs = float((host(y).astype(np.float64) * host(dyd)).sum())
        rhs = float((host(xd).astype(np.float64) * host(dx)).sum())
        print("adjoint: <up(x), dy> = %.9g, <x, up^T(dy)> = %.9g" % (lhs, rhs))
        assert abs(lhs - rhs) < 1e-5 * max(abs(lhs), abs(rhs), float(np.abs(host(y)).max() * np.abs(host(dyd)).max()))
    # the accumulating form adds the same values
    acc = torch.full_like(xd, 0.5)
    L.bilinear_up2x_3d_bwd_acc(dyd.data_ptr(), dt, acc.data_ptr(), B, D, H, W, C, S())
    close(host(acc) - 0.5, xr.grad.numpy(), tol if dt == F32 else 2.0 ** -7, "up3d bwd (accumulates)")


def test_spatial_window3d_pad_and_crop(L):
    x = RNG.standard_normal((2, 4, 6, 5, 3)).astype(np.float32)
    xd = dev(x)
    for (od, oh, ow, oz, oy, ox) in [(6, 9, 8, -1, -1, -1), (2, 4, 3, 1, 1, 1), (4, 6, 5, 0, 0, 0), (5, 7, 4, -1, 0, 1), (3, 3, 3, 2, 4, 3)]:
        out = torch.full((2, od, oh, ow, 3), 9.0).cuda()
        L.spatial_window3d(xd.data_ptr(), out.data_ptr(), F32, 2, 4, 6, 5, od, oh, ow, 3, oz, oy, ox, S())
        want = np.zeros((2, od, oh, ow, 3), dtype=np.float32)
        for z in range(od):
            for y in range(oh):
                for xx in range(ow):
                    if 0 <= z + oz < 4 and 0 <= y + oy < 6 and 0 <= xx + ox < 5:
                        want[:, z, y, xx] = x[:, z + oz, y + oy, xx + ox]
        assert torch.equal(out.cpu(), torch.as_tensor(want)), (od, oh, ow, oz, oy, ox)


def test_refusals_return_the_shape_status_and_launch_nothing(L):
    dll = L._dll                                                               # the raw entry points: the status instead of an exception
    x = torch.ones(2 * 4 * 4 * 4 * 8, device="cuda")
    w = torch.ones(27 * 8 * 8, device="cuda")
    out = torch.full((2 * 8 * 8 * 8 * 8,), 5.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(S())
    for geo in [(0, 4, 4, 4, 8, 8, 3, 3, 3, 1, 1, 1), (2, 4, -1, 4, 8, 8, 3, 3, 3, 1, 1, 1), (2, 4, 4, 4, 8, 8, 3, 0, 3, 1, 1, 1),
                (2, 4, 4, 4, 8, 8, 3, 3, 3, 1, 0, 1), (2, 4, 4, 4, 0, 8, 3, 3, 3, 1, 1, 1)]:
        assert dll.phx_gconv3d_fwd(p(x), F32, p(w), None, p(out), F32, *geo, 0, s) == PHX_E_SHAPE
        assert dll.phx_gconv3d_dgrad(p(x), F32, p(w), p(out), F32, *geo, s) == PHX_E_SHAPE
        assert dll.phx_gconv3d_wgrad(p(x), F32, p(x), F32, p(out), *geo, s) == PHX_E_SHAPE
        assert dll.phx_tconv3d_fwd(p(x), F32, p(w), None, p(out), F32, *geo, 0, s) == PHX_E_SHAPE
        assert dll.phx_tconv3d_dgrad(p(x), F32, p(w), p(out), F32, *geo, s) == PHX_E_SHAPE
        assert dll.phx_tconv3d_wgrad(p(x), F32, p(x), F32, p(out), *geo, s) == PHX_E_SHAPE
    for win in [(3, 2, 2), (2, 2, 0), (2, 4, 2)]:
        assert dll.phx_maxpool3d_fwd(p(x), F32, p(out), 2, 4, 4, 4, 8, *win, s) == PHX_E_SHAPE
        assert dll.phx_maxpool3d_bwd(p(x), p(x), F32, p(out), 2, 4, 4, 4, 8, *win, s) == PHX_E_SHAPE
    assert dll.phx_maxpool3d_fwd(p(x), F32, p(out), 2, 0, 4, 4, 8, 2, 2, 2, s) == PHX_E_SHAPE
    assert dll.phx_bilinear_up2x_3d_fwd(p(x), F32, p(out), 2, 4, 0, 4, 8, s) == PHX_E_SHAPE
    assert dll.phx_bilinear_up2x_3d_bwd(p(x), F32, p(out), 2, 4, 4, -3, 8, s) == PHX_E_SHAPE
    assert dll.phx_spatial_window3d(p(x), p(out), F32, 2, 4, 4, 4, 0, 4, 4, 8, 0, 0, 0, s) == PHX_E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())                                            # the output buffer is untouched
    with pytest.raises(Exception, match="maxpool3d"):
        L.maxpool3d_fwd(x.data_ptr(), F32, out.data_ptr(), 2, 4, 4, 4, 8, 3, 3, 3, S())


@pytest.mark.parametrize("dt", [F32, BF16])
def test_repeats_are_bit_identical(L, dt):
    B, D, H, W, Ci, Co = 2, 6, 7, 9, 16, 24
    geo = (B, D, H, W, Ci, Co, 3, 3, 3, 1, 1, 1)
    xd, wd, bd = dev(RNG.standard_normal((B, D, H, W, Ci)), dt), dev(RNG.standard_normal((3, 3, 3, Ci, Co)) / 20), dev(RNG.standard_normal(Co))
    dyd = dev(RNG.standard_normal((B, D, H, W, Co)), dt)
    ys, dws, dxs = [], [], []
    for _ in range(2):
        y = torch.empty(B, D, H, W, Co, dtype=tdt(dt)).cuda()
        L.gconv3d_fwd(xd.data_ptr(), dt, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), dt, *geo, 1, S())
        dw = torch.zeros(3, 3, 3, Ci, Co).cuda()
        L.gconv3d_wgrad(xd.data_ptr(), dt, dyd.data_ptr(), dt, dw.data_ptr(), *geo, S())
        dx = torch.empty_like(xd)
        L.gconv3d_dgrad(dyd.data_ptr(), dt, wd.data_ptr(), dx.data_ptr(), dt, *geo, S())
        ys.append(y), dws.append(dw), dxs.append(dx)
    assert torch.equal(ys[0], ys[1]) and torch.equal(dws[0], dws[1]) and torch.equal(dxs[0], dxs[1])
    assert float(dws[0].abs().max()) > 0
