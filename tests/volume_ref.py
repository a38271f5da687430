"""Float64 oracle of the 3-D layer family (not a test file): torch-CPU restatements of the TF 1.12 semantics behind conv3D,
transposed_conv3D, maxpool3D, bilinear_upsample3D and batch norm on a rank-5 tensor -- independent of the kernels, differentiable by
torch autograd.  Tensors are NDHWC [B, D, H, W, C]; filters DHWIO (conv3d) / DHWOI (conv3d_transpose), as TF stores them."""
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
BN_DECAY = 0.99


def same_pads(size, k, s):
    """TF's SAME rule on one axis -> (out, before, after): out = ceil(in / s), total = max((out - 1) s + k - in, 0), before = total // 2."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2, total - total // 2


def conv3d_same(x, w_dhwio, strides=(1, 1, 1)):
    """tf.nn.conv3d(x, W, [1, sd, sh, sw, 1], 'SAME'): F.conv3d on an input padded explicitly by the SAME rule."""
    pads = [same_pads(x.shape[1 + i], int(w_dhwio.shape[i]), strides[i]) for i in range(3)]
    xp = F.pad(x.permute(0, 4, 1, 2, 3), (pads[2][1], pads[2][2], pads[1][1], pads[1][2], pads[0][1], pads[0][2]))
    return F.conv3d(xp, w_dhwio.permute(4, 3, 0, 1, 2), stride=tuple(strides)).permute(0, 2, 3, 4, 1)


def conv3d_transpose_same(x, w_dhwoi, strides=(2, 2, 2)):
    """tf.nn.conv3d_transpose(x, filter [kd, kh, kw, Cout, Cin], output in * s, 'SAME'): the input gradient of the stride-s SAME
    convolution.  F.conv_transpose3d gives the un-cropped (in - 1) s + k result, of which [before, before + in s) is kept per axis with
    before = max(k - s, 0) // 2 (the rule of oracle.tf1_ops.conv2d_transpose_same per axis); k < s leaves zeros at the far end."""
    full = F.conv_transpose3d(x.permute(0, 4, 1, 2, 3), w_dhwoi.permute(4, 3, 0, 1, 2), stride=tuple(strides))
    sl = [slice(None), slice(None)]
    padding = []
    for i in range(3):
        n, k, s = x.shape[1 + i], int(w_dhwoi.shape[i]), strides[i]
        before = max(k - s, 0) // 2
        padding = [0, max(0, before + n * s - full.shape[2 + i])] + padding
        sl.append(slice(before, before + n * s))
    full = F.pad(full, tuple(padding))
    return full[tuple(sl)].permute(0, 2, 3, 4, 1)


def impulse_conv3d_same(x, k, strides, tap, a, b, cout):
    """conv3D with the one-hot filter w[tap][a][b] = 1, no bias, no activation, WITHOUT a convolution (numpy, np.pad and slicing only):
    output channel b is input channel a zero-padded by the SAME rule, shifted by tap = (tz, ty, tx) and strided -- out[o] =
    padded[o s + tap] -- and every other output channel is zero.  x [B, D, H, W, Cin] -> [B, Do, Ho, Wo, cout], exact in any dtype."""
    import numpy as np
    pads = [same_pads(x.shape[1 + i], k[i], strides[i]) for i in range(3)]
    xp = np.pad(x[..., a], [(0, 0)] + [(p[1], p[2]) for p in pads])
    out = np.zeros((x.shape[0],) + tuple(p[0] for p in pads) + (cout,), dtype=x.dtype)
    sl = tuple(slice(tap[i], tap[i] + (pads[i][0] - 1) * strides[i] + 1, strides[i]) for i in range(3))
    out[..., b] = xp[(slice(None),) + sl]
    return out


def impulse_conv3d_same_adjoint(dy, big_dhw, k, strides, tap, a, b, ca):
    """The adjoint of impulse_conv3d_same, by slicing only: channel b of dy [B, Do, Ho, Wo, Cb] (Do = ceil(big / s)) is placed at
    o s + tap - before on channel a of a zero tensor [B, *big_dhw, ca]; what falls into the SAME padding is dropped.  This is the data
    gradient of conv3D under the one-hot filter w[tap][a][b] = 1, and -- conv3d_transpose being the input gradient of the stride-s SAME
    convolution on its own output extent in * s -- transposed_conv3D's forward pass under w_dhwoi[tap][a][b] = 1."""
    import numpy as np
    pads = [same_pads(big_dhw[i], k[i], strides[i]) for i in range(3)]
    assert tuple(dy.shape[1:4]) == tuple(p[0] for p in pads)
    xp = np.zeros((dy.shape[0],) + tuple(big_dhw[i] + pads[i][1] + pads[i][2] for i in range(3)), dtype=dy.dtype)
    sl = tuple(slice(tap[i], tap[i] + (pads[i][0] - 1) * strides[i] + 1, strides[i]) for i in range(3))
    xp[(slice(None),) + sl] = dy[..., b]
    out = np.zeros((dy.shape[0],) + tuple(big_dhw) + (ca,), dtype=dy.dtype)
    out[..., a] = xp[(slice(None),) + tuple(slice(pads[i][1], pads[i][1] + big_dhw[i]) for i in range(3))]
    return out


def bias_add(x, b):
    return x + b.reshape(1, 1, 1, 1, -1)


def max_pool3d_same(x, window=(2, 2, 2)):
    """tf.nn.max_pool3d, window = stride, SAME: the far-side padding never wins (-inf); the gradient goes to the first maximum of a
    window in row-major (d, h, w) order, as in TF's and torch's kernels."""
    pd, ph, pw = window
    d, h, w = x.shape[1:4]
    xp = F.pad(x.permute(0, 4, 1, 2, 3), (0, -w % pw, 0, -h % ph, 0, -d % pd), value=float("-inf"))
    return F.max_pool3d(xp, tuple(window), tuple(window)).permute(0, 2, 3, 4, 1)


def _up2_axis(x, axis):
    """legacy ResizeBilinear by 2 on one axis: up[2k] = x[k], up[2k + 1] = (x[k] + x[min(k + 1, n - 1)]) / 2"""
    n = x.shape[axis]
    nxt = torch.clamp(torch.arange(n) + 1, max=n - 1)
    odd = 0.5 * (x + x.index_select(axis, nxt))
    return torch.stack([x, odd], dim=axis + 1).reshape(x.shape[:axis] + (2 * n,) + x.shape[axis + 1:])


def bilinear_up2x_3d(x):
    """bilinear_upsample3D(factor=2): tf.image.resize_bilinear (legacy coordinates) on the (H, W) planes, then along D; the passes
    commute and the result is the separable form."""
    return _up2_axis(_up2_axis(_up2_axis(x, 3), 2), 1)


def crop_centre(t, out_dhw):
    """the 5-D branch of crop_and_concat: start = (larger - output) // 2 on three axes"""
    st = [(t.shape[1 + i] - out_dhw[i]) // 2 for i in range(3)]
    return t[:, st[0]:st[0] + out_dhw[0], st[1]:st[1] + out_dhw[1], st[2]:st[2] + out_dhw[2]]


def batch_norm_train_5d(x, gamma, beta):
    """tf.contrib.layers.batch_norm on a rank-5 tensor, training: the non-fused path -- the biased batch variance normalises AND feeds
    the moving average (no Bessel correction, unlike the fused rank-4 path).  -> (y, batch mean, BIASED batch variance)"""
    mean = x.mean(dim=(0, 1, 2, 3))
    var = ((x - mean) ** 2).mean(dim=(0, 1, 2, 3))
    return (x - mean) * torch.rsqrt(var + BN_EPS) * gamma + beta, mean, var


def dice_loss(logits, labels, epsilon=1e-10):
    """tfwrapper/losses.py dice_loss with its default flags (Dice per sample and label over all voxels, then the mean) on
    [B, ..., C] logits and integer labels [B, ...] -- the torch form of tests/seg_losses_ref.dice_loss"""
    C = logits.shape[-1]
    y = F.one_hot(labels.to(torch.long), C).to(logits.dtype).reshape(logits.shape[0], -1, C)
    sm = torch.softmax(logits, dim=-1).reshape(logits.shape[0], -1, C)
    dice = 2 * (sm * y).sum(dim=1) / (sm.sum(dim=1) + y.sum(dim=1) + epsilon)
    return 1.0 - dice.mean()


def weighted_cross_entropy(logits, labels, class_weights):
    """tfwrapper/losses.py pixel_wise_cross_entropy_loss_weighted: mean over all voxels of weight[label] * soft-max cross-entropy"""
    lab = labels.to(torch.long)
    ce = -torch.log_softmax(logits, dim=-1).gather(-1, lab.unsqueeze(-1)).squeeze(-1)
    w = torch.as_tensor(class_weights, dtype=torch.float32).to(logits.dtype)
    return (ce * w[lab]).mean()


def moving_update(moving, batch_value, decay=BN_DECAY):
    return moving - (moving - batch_value) * (1.0 - decay)


def batch_norm_infer(x, gamma, beta, moving_mean, moving_var):
    return (x - moving_mean) * torch.rsqrt(moving_var + BN_EPS) * gamma + beta
