"""Float64 torch-CPU reference of the 2-D layers with explicit geometry (csrc/conv2d_pad.hip): convolution, transposed convolution and
max / average pooling under SAME and VALID padding, any stride, dilation and window.

There is no TensorFlow here: this is a RESTATEMENT of TF 1.12's documented rules, not a recording of its output.  With
ke = (k - 1) d + 1 per axis:
    SAME   out = ceil(in / s), total = max((out - 1) s + ke - in, 0), before = total // 2 (the extra row / column goes behind)
    VALID  out = (in - ke) // s + 1, no padding; in < ke is an error
    conv2d_transpose with output extent O: legal iff the forward convolution of O gives the input extent; it is the gradient of that
    convolution with respect to its input, so its padding is the forward convolution's on O
    max pool: padded taps never win, ties go to the first element of the window in row-major order
    avg pool: divides by the number of taps inside the map
The convolution is F.pad with the asymmetric padding followed by an unpadded F.conv2d; the transposed layer is written as the autograd
gradient of exactly that convolution; the pools work on explicitly unfolded windows.  tests/test_padded_layers_cpu.py ties the SAME
cases to oracle.tf1_ops, whose functions are pinned to fixtures the reference produced.  Independent of the kernels and of
phiseg_code_amd.graph.conv_geometry (which the CPU tests compare against `geometry` below)."""
import torch
import torch.nn.functional as F


def axis_geometry(n, k, s, d, padding):
    """-> (out, before, after) of one axis"""
    ke = (k - 1) * d + 1
    if padding == "VALID":
        if n < ke:
            raise ValueError("VALID: input extent %d smaller than the window extent %d" % (n, ke))
        return (n - ke) // s + 1, 0, 0
    assert padding == "SAME", padding
    out = -(-n // s)
    total = max((out - 1) * s + ke - n, 0)
    return out, total // 2, total - total // 2


def geometry(h, w, k, s, d, padding):
    """-> (Ho, Wo, pt, pl)"""
    ho, pt, _ = axis_geometry(h, k[0], s[0], d[0], padding)
    wo, pl, _ = axis_geometry(w, k[1], s[1], d[1], padding)
    return ho, wo, pt, pl


def conv2d(x, w_hwio, strides=(1, 1), dilations=(1, 1), padding="SAME"):
    """tf.nn.conv2d / tf.nn.atrous_conv2d: x [B, H, W, Cin], w [kh, kw, Cin, Cout] -> [B, Ho, Wo, Cout]"""
    kh, kw = int(w_hwio.shape[0]), int(w_hwio.shape[1])
    _, H, W, _ = x.shape
    _, pt, pb = axis_geometry(H, kh, strides[0], dilations[0], padding)
    _, pl, pr = axis_geometry(W, kw, strides[1], dilations[1], padding)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, w_hwio.permute(3, 2, 0, 1), stride=tuple(strides), dilation=tuple(dilations)).permute(0, 2, 3, 1)


def transpose_legal_range(n, k, s, padding):
    """output extents O of conv2d_transpose whose forward convolution gives n -> (lowest, highest)"""
    return ((n - 1) * s + 1, n * s) if padding == "SAME" else ((n - 1) * s + k, (n - 1) * s + k + s - 1)


def conv2d_transpose(x, w_hwoi, out_hw, strides=(2, 2), padding="SAME"):
    """tf.nn.conv2d_transpose(x [B, H, W, Cin], filter [kh, kw, Cout, Cin], output [B, Ho, Wo, Cout], strides, padding): the gradient
    with respect to its input of the convolution [B, Ho, Wo, Cout] -> [B, H, W, Cin] with the filter read as HWIO (I = Cout, O = Cin),
    taken by autograd of `conv2d` above (differentiable in x and w: create_graph)."""
    kh, kw, cout, cin = (int(v) for v in w_hwoi.shape)
    B, H, W, _ = x.shape
    for n, O, k, s in ((H, out_hw[0], kh, strides[0]), (W, out_hw[1], kw, strides[1])):
        lo, hi = transpose_legal_range(n, k, s, padding)
        if not lo <= O <= hi:
            raise ValueError("conv2d_transpose: output extent %d outside %d..%d" % (O, lo, hi))
    z = torch.zeros(B, int(out_hw[0]), int(out_hw[1]), cout, dtype=x.dtype, requires_grad=True)
    y = conv2d(z, w_hwoi, strides, (1, 1), padding)
    assert tuple(y.shape) == tuple(x.shape), (y.shape, x.shape)
    (g,) = torch.autograd.grad(y, z, grad_outputs=x, create_graph=True)
    return g


def _windows(x, k, s, padding, fill):
    """x [B, H, W, C] -> (windows [B, C, kh * kw, Ho, Wo] in row-major tap order with `fill` in the padding, mask of real taps)"""
    B, H, W, C = x.shape
    ho, pt, pb = axis_geometry(H, k[0], s[0], 1, padding)
    wo, pl, pr = axis_geometry(W, k[1], s[1], 1, padding)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb), value=fill)
    mp = F.pad(torch.ones(1, 1, H, W, dtype=x.dtype), (pl, pr, pt, pb))
    taps, mask = [], []
    for ky in range(k[0]):
        for kx in range(k[1]):
            sl = (slice(ky, ky + (ho - 1) * s[0] + 1, s[0]), slice(kx, kx + (wo - 1) * s[1] + 1, s[1]))
            taps.append(xp[:, :, sl[0], sl[1]])
            mask.append(mp[:, :, sl[0], sl[1]])
    return torch.stack(taps, dim=2), torch.stack(mask, dim=2)


def max_pool(x, k=(2, 2), s=(2, 2), padding="SAME"):
    """tf.nn.max_pool: the padding never wins; the gradient goes to the FIRST maximum of a window in row-major order (argmax of the
    unfolded taps with ties resolved to the lowest tap index, then a gather, so autograd routes the gradient to that tap alone)."""
    win, mask = _windows(x, k, s, padding, float("-inf"))
    m = win.detach().max(dim=2, keepdim=True).values
    ntap = win.shape[2]
    idx = torch.arange(ntap).reshape(1, 1, ntap, 1, 1).expand_as(win)
    first = torch.where(win.detach() == m, idx, torch.full_like(idx, ntap)).min(dim=2, keepdim=True).values
    return torch.gather(win, 2, first).squeeze(2).permute(0, 2, 3, 1)


def avg_pool(x, k=(2, 2), s=(2, 2), padding="SAME"):
    """tf.nn.avg_pool: the sum of the taps inside the map over their number"""
    win, mask = _windows(x, k, s, padding, 0.0)
    return (win.sum(dim=2) / mask.sum(dim=2)).permute(0, 2, 3, 1)


def bias_add(x, b):
    return x + b.reshape(1, 1, 1, -1)
