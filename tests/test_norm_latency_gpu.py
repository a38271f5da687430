"""The batch-norm kernels whose loads are issued ahead of their prologues (csrc/norm.hip, csrc/norm_bwd.hip): phx_norm_apply_fused,
phx_norm_apply_pool, phx_norm_bwd_reduce, phx_norm_bwd_apply_fused and phx_bn_bwd_onepass, bf16, at the smallest shapes at which the
early loads can go wrong -- fewer pixels than one four-pixel trip (only the clamped early loads and the tail run), one trip plus a
tail, ragged last blocks, C / 8 = 3 (255 of 256 threads), the step's channel count -- against the defining formulas in float64
(torch autograd on the device, from the same bf16 tensors).

Tolerances are those of tests/test_kernels_gpu.py for the same kernels: 5e-5 of the maximum for mean / rstd, 1e-3 for dgamma / dbeta,
6e-3 for the activation and 8e-3 for dx, elements whose pre-activation lies within 1e-4 of the ReLU kink left out (fp32 and fp64 may
put them on different sides) -- at least 99.9 % of the elements stay in.  Every output buffer is pre-filled with NaN and carries four
pixels of slack behind it: an element not written, or one written past the end, shows."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = 1
ACT_ID, ACT_RELU = 0, 1
SLACK = 4                                            # pixels of NaN behind every streamed output

SHAPES = [(1, 1, 3, 8), (1, 1, 5, 8), (3, 5, 7, 8), (7, 12, 12, 96), (2, 4, 6, 24), (2, 16, 16, 192)]


@pytest.fixture(scope="module")
def L():
    from phiseg_code_amd import runtime as rt
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return rt.lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def close(got, ref, rel, what):
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), what + ": not finite"
    err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
    print("%s: rel-to-max err %.3e (bound %.1e)" % (what, err, rel))
    assert err <= rel, "%s: rel-to-max err %.3e > %.1e" % (what, err, rel)


def close_masked(got, ref, away, rel, what, scale=None):
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), what + ": an element was not written"
    err = float(((got - ref) * away).abs().max()) / max(float(ref.abs().max()) if scale is None else scale, 1e-30)
    print("%s: rel-to-max err %.3e (bound %.1e)" % (what, err, rel))
    assert err <= rel, "%s: rel-to-max err %.3e > %.1e" % (what, err, rel)


@functools.lru_cache(maxsize=None)
def reference(shape, act, G=0):
    """Inputs (drawn as tests/test_kernels_gpu.py draws them) and the float64 results of one layer; G == 0: batch norm (one statistic
    per channel over all B H W pixels, eps 1e-3), else group norm with G groups per sample (eps 1e-5).  Computed once per case and
    shared; nothing in it is written afterwards."""
    B, H, W, C = shape
    g = torch.Generator(device="cuda").manual_seed(1000 * C + 10 * B * H * W + act + 3 * G)
    x = (torch.randn(B * H * W, C, device="cuda", generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    dA = torch.randn(B * H * W, C, device="cuda", generator=g).to(torch.bfloat16)
    gamma = (1.0 + 0.2 * torch.randn(C, device="cuda", generator=g)).float()
    beta = (0.1 * torch.randn(C, device="cuda", generator=g)).float()
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    if G == 0:
        NS, P, GG, eps = 1, B * H * W, C, 1e-3
        mean = x64.mean(0)
        var = ((x64 - mean) ** 2).mean(0)
        rstd = 1.0 / torch.sqrt(var + eps)
        xhat = (x64 - mean) * rstd
    else:
        NS, P, GG, eps = B, H * W, G, 1e-5
        xg = x64.view(B, P, G, C // G)
        mean = xg.mean(dim=(1, 3), keepdim=True)
        var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        xhat = ((xg - mean) * rstd).reshape(B * P, C)
    pre = g64 * xhat + b64
    a = torch.relu(pre) if act == ACT_RELU else pre
    (a * dA.double()).sum().backward()
    away = (pre.detach().abs() > 1e-4) if act == ACT_RELU else torch.ones_like(pre, dtype=torch.bool)
    assert float(away.double().mean()) >= 0.999, "too many pre-activations at the ReLU kink"
    return dict(NS=NS, P=P, C=C, G=GG, eps=eps, act=act, x=x, dA=dA, gamma=gamma, beta=beta, mean=mean.detach().reshape(-1),
                rstd=rstd.detach().reshape(-1), a=a.detach(), away=away, dx=x64.grad, dgamma=g64.grad, dbeta=b64.grad)


def nan_buffer(P_total, C):
    """[P_total + SLACK][C] bf16 NaNs: the kernel writes the first P_total pixels."""
    return torch.full((P_total + SLACK, C), float("nan"), dtype=torch.bfloat16, device="cuda")


def slack_untouched(buf, P_total):
    return bool(torch.isnan(buf[P_total:].float()).all())


def nan_f32(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


def forward(L, r, pool_hw=None):
    """phx_norm_stats + the fused apply pass (pool_hw = (H, W): the pooling form) -> a (with slack), pooled, (mean, rstd, scale, shift)"""
    NS, P, C, G = r["NS"], r["P"], r["C"], r["G"]
    sums = torch.zeros(NS, C, 2, dtype=torch.float32, device="cuda")
    pivot = torch.zeros(NS, C, dtype=torch.float32, device="cuda")
    L.norm_stats(r["x"].data_ptr(), BF16, sums.data_ptr(), pivot.data_ptr(), NS, P, C, S())
    a = nan_buffer(NS * P, C)
    st = [nan_f32(NS * G), nan_f32(NS * G), nan_f32(NS * C), nan_f32(NS * C)]
    pooled = None
    if pool_hw is None:
        L.norm_apply_fused(r["x"].data_ptr(), BF16, sums.data_ptr(), pivot.data_ptr(), r["gamma"].data_ptr(), r["beta"].data_ptr(), r["eps"],
                           a.data_ptr(), BF16, *[t.data_ptr() for t in st], None, None, 0.0, NS, P, C, G, r["act"], S())
    else:
        pooled = nan_buffer(NS * P // 4, C)
        L.norm_apply_pool(r["x"].data_ptr(), sums.data_ptr(), pivot.data_ptr(), r["gamma"].data_ptr(), r["beta"].data_ptr(), r["eps"],
                          a.data_ptr(), pooled.data_ptr(), *[t.data_ptr() for t in st], None, None, 0.0, NS, P, C, G, pool_hw[0], pool_hw[1],
                          r["act"], S())
    torch.cuda.synchronize()
    return a, pooled, st


def check_forward(r, a, st, what):
    n = r["NS"] * r["P"]
    close(st[0], r["mean"], 5e-5, what + " mean")
    close(st[1], r["rstd"], 5e-5, what + " rstd")
    assert bool(torch.isfinite(st[2]).all()) and bool(torch.isfinite(st[3]).all()), what + ": scale / shift not published"
    close_masked(a[:n], r["a"], r["away"], 6e-3, what + " a")
    assert slack_untouched(a, n), what + ": a written past its end"


@pytest.mark.parametrize("act", [ACT_RELU, ACT_ID])
@pytest.mark.parametrize("shape", SHAPES)
def test_norm_apply_fused_early_loads(L, shape, act):
    r = reference(shape, act)
    a, _, st = forward(L, r)
    check_forward(r, a, st, "apply %s act %d" % (shape, act))


@pytest.mark.parametrize("act", [ACT_RELU, ACT_ID])
@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 4, 6, 24)])
def test_norm_apply_pool_one_stage_prologue(L, shape, act):
    B, H, W, C = shape
    r = reference(shape, act)
    a, pooled, st = forward(L, r, pool_hw=(H, W))
    what = "apply + pool %s act %d" % (shape, act)
    check_forward(r, a, st, what)
    quads = lambda t: t.view(B, H // 2, 2, W // 2, 2, C)
    pooled_ref = quads(r["a"]).mean(dim=(2, 4)).reshape(-1, C)
    away = quads(r["away"]).all(dim=4).all(dim=2).reshape(-1, C)
    nq = B * H * W // 4
    # the average is taken of the activations AS STORED: four values each within 2^-9 of max |a| of the float64 one, and the average
    # rounded to bf16 once more -- at most 2^-8 = 3.9e-3 of max |a|, so the activation's own bound and scale hold for it (with one quad
    # per channel the pooled value is the batch mean, about beta: its own maximum says nothing about its rounding error)
    close_masked(pooled[:nq], pooled_ref, away, 6e-3, what + " pooled", scale=float(r["a"].abs().max()))
    assert slack_untouched(pooled, nq), what + ": pooled written past its end"


def two_pass_backward(L, r, st, nrep):
    NS, P, C, G = r["NS"], r["P"], r["C"], r["G"]
    mean, rstd, scale, shift = st
    sums2 = torch.zeros(nrep, NS, C, 2, dtype=torch.float32, device="cuda")
    L.norm_bwd_reduce(r["dA"].data_ptr(), BF16, r["x"].data_ptr(), BF16, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                      sums2.data_ptr(), NS, P, C, G, r["act"], nrep, S())
    dx = nan_buffer(NS * P, C)
    dgamma, dbeta = torch.zeros(C, dtype=torch.float32, device="cuda"), torch.zeros(C, dtype=torch.float32, device="cuda")
    L.norm_bwd_apply_fused(r["dA"].data_ptr(), BF16, r["x"].data_ptr(), BF16, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                           r["gamma"].data_ptr(), sums2.data_ptr(), dx.data_ptr(), BF16, dgamma.data_ptr(), dbeta.data_ptr(), NS, P, C, G,
                           r["act"], nrep, S())
    torch.cuda.synchronize()
    return dx, dgamma, dbeta


def check_backward(r, dx, dgamma, dbeta, what):
    n = r["NS"] * r["P"]
    close(dbeta, r["dbeta"], 1e-3, what + " dbeta")
    close(dgamma, r["dgamma"], 1e-3, what + " dgamma")
    close_masked(dx[:n], r["dx"], r["away"], 8e-3, what + " dx")
    assert slack_untouched(dx, n), what + ": dx written past its end"


@pytest.mark.parametrize("nrep", [1, 4])
@pytest.mark.parametrize("act", [ACT_RELU, ACT_ID])
@pytest.mark.parametrize("shape", SHAPES)
def test_norm_bwd_reduce_and_apply_early_loads(L, shape, act, nrep):
    r = reference(shape, act)
    _, _, st = forward(L, r)
    dx, dgamma, dbeta = two_pass_backward(L, r, st, nrep)
    check_backward(r, dx, dgamma, dbeta, "two-pass backward %s act %d nrep %d" % (shape, act, nrep))


@pytest.mark.parametrize("nrep", [1, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_bn_bwd_onepass_early_loads(L, shape, nrep):
    r = reference(shape, ACT_RELU)
    P, C = r["P"], r["C"]
    assert L.bn_bwd_onepass_supported(P, C, ACT_RELU) == 1
    _, _, (mean, rstd, scale, shift) = forward(L, r)
    nbar = int(L.bn_bwd_onepass_barrier_words())
    for rep in range(2):                             # (a second launch on re-zeroed state: every launch leaves the time-out word clear)
        sums2 = torch.zeros(nrep, C, 2, dtype=torch.float32, device="cuda")
        bar = torch.zeros(nbar, dtype=torch.int32, device="cuda")
        dx = nan_buffer(P, C)
        dgamma, dbeta = torch.zeros(C, dtype=torch.float32, device="cuda"), torch.zeros(C, dtype=torch.float32, device="cuda")
        L.bn_bwd_onepass(r["dA"].data_ptr(), r["x"].data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                         r["gamma"].data_ptr(), sums2.data_ptr(), bar.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), P, C,
                         ACT_RELU, nrep, S())
        torch.cuda.synchronize()
        assert int(bar[288]) == 0, "grid barrier timed out"
        check_backward(r, dx, dgamma, dbeta, "one-pass backward %s nrep %d launch %d" % (shape, nrep, rep))


@pytest.mark.parametrize("nrep", [1, 4])
@pytest.mark.parametrize("act", [ACT_RELU, ACT_ID])
def test_group_norm_keeps_its_staged_prologues(L, act, nrep):
    """Group norm (G = 2 per sample): the statistic crosses channels, so the forward pass keeps two LDS stages and the backward apply
    three; only the data loads and the first channel's gamma / beta moved."""
    r = reference((2, 4, 4, 32), act, G=2)
    a, _, st = forward(L, r)
    check_forward(r, a, st, "group norm act %d" % act)
    dx, dgamma, dbeta = two_pass_backward(L, r, st, nrep)
    check_backward(r, dx, dgamma, dbeta, "group norm backward act %d nrep %d" % (act, nrep))
