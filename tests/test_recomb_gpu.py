"""phx_recomb_samples (csrc/recomb.hip) against a float64 numpy restatement with the rounding points of include/phx.h.

Tolerance: derived, not tuned.  An elementwise a-priori bound is carried through the same layers in float64:
    E_l = |s_l| (|W_l|^T E_{l-1} + (K_in + Z + 3) 2^-24 |W_l|^T |a_{l-1}|)      (fp32 accumulation of K_in + Z products, scale, shift)
    E_l += 2^-8 |a_l|   where the PHX_BF16 form rounds a_l to bf16  (one ulp: the two roundings may fall on different sides)
ReLU is 1-Lipschitz.  Asserted: |device - restatement| <= 2 E on the logits, <= 2 max_c E on the soft-max.
The exact case (small integers, every intermediate representable in bf16) must agree bit for bit in both forms: a permuted k order or
a transposed store changes almost every element there.
Shapes: B = 2, n = 3, P = 80 (not a multiple of the 32-pixel tile), Z in {1, 6}, C in {2, 3}; KF = 32 and 64 (the width of the feature
map; the chain itself is 32 wide); both feat dtypes; scales of both signs and NULL; logits only / soft-max only / both."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
K = 32
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def L():
    from phiseg_code_amd import runtime as rt
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return rt.lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def bf16(a):
    """float64 array -> nearest-even bf16 value, as float64"""
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(torch.bfloat16).double().numpy()


def restate(feat, z, W, b3, s, t, n, dt):
    """feat [B, P, KF] (already representable in dt), z [B * n, Z], W = [W0, W1, W2, W3], s / t lists of [K] (s[l] None = 1)
    -> (logits, soft-max, E) in float64, E the a-priori bound on the logits."""
    B, P, KF = feat.shape
    Z = z.shape[1]
    r = bf16 if dt == BF16 else (lambda a: np.asarray(a, dtype=np.float64))
    x = np.concatenate([np.repeat(feat, n, axis=0), np.repeat(z[:, None, :], P, axis=1)], axis=-1)     # [B n, P, KF + Z]
    W0 = np.concatenate([r(W[0][:KF]), W[0][KF:]], axis=0)                                               # the z rows stay fp32
    a, E = x, np.zeros_like(x)
    for l, Wl in enumerate((W0, r(W[1]), r(W[2]))):
        sl = np.ones(K) if s[l] is None else s[l]
        pre = a @ Wl
        fan = (KF if l == 0 else K) + Z + 3
        E = np.abs(sl) * (E @ np.abs(Wl) + fan * U24 * (np.abs(a) @ np.abs(Wl)))
        a = np.maximum(sl * pre + t[l], 0.0)
        if dt == BF16 and l < 2:
            E = E + 2.0 ** -8 * np.abs(a)
            a = bf16(a)
    logits = a @ W[3] + b3
    E = E @ np.abs(W[3]) + (K + Z + 3) * U24 * (np.abs(a) @ np.abs(W[3]) + np.abs(b3))
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    return logits, e / e.sum(axis=-1, keepdims=True), E


def launch(L, feat, z, W, b3, s, t, n, dt, want=("logits", "sm"), KF=None, Kc=K, Z=None, C=None):
    B, P, kf = feat.shape
    f = torch.as_tensor(feat, dtype=torch.float32).cuda()
    f = (f.to(torch.bfloat16) if dt == BF16 else f).contiguous()
    d = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()
    zd, Wd, bd, sd, td = d(z), [d(w) for w in W], d(b3), [d(v) for v in s], [d(v) for v in t]
    Cn = W[3].shape[1]
    # sentinel-filled outputs with a guard row behind them: a store past the end or a missing store shows
    outs = {k: torch.full((B * n * P * Cn + 64,), -777.0, dtype=torch.float32, device="cuda") for k in want}
    p = lambda v: None if v is None else v.data_ptr()
    L.recomb_samples(f.data_ptr(), dt, zd.data_ptr(), Wd[0].data_ptr(), Wd[1].data_ptr(), Wd[2].data_ptr(), Wd[3].data_ptr(), bd.data_ptr(),
                     p(sd[0]), p(td[0]), p(sd[1]), p(td[1]), p(sd[2]), p(td[2]), p(outs.get("logits")), p(outs.get("sm")),
                     B, n, P, kf if KF is None else KF, Kc, z.shape[1] if Z is None else Z, Cn if C is None else C, S())
    torch.cuda.synchronize()
    res = {}
    for k, v in outs.items():
        h = v.cpu().double().numpy()
        assert (h[-64:] == -777.0).all(), "%s: stored past the end" % k
        res[k] = h[:-64].reshape(B * n, P, Cn)
        assert (res[k] != -777.0).all(), "%s: elements never stored" % k
    return res


def random_case(rng, B, n, P, KF, Z, C, dt, scales):
    feat = rng.standard_normal((B, P, KF))
    feat = bf16(feat) if dt == BF16 else feat.astype(np.float32).astype(np.float64)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    z = f32(rng.standard_normal((B * n, Z)) * 1.5)
    W = [f32(rng.standard_normal((KF + Z, K)) * 0.25 + 0.02), f32(rng.standard_normal((K, K)) * 0.3 - 0.01),
         f32(rng.standard_normal((K, K)) * 0.3 + 0.03), f32(rng.standard_normal((K, C)) * 0.4)]
    b3 = f32(rng.standard_normal(C))
    s = [None if not scales else f32(rng.uniform(0.5, 1.5, K) * rng.choice([-1.0, 1.0], K)) for _ in range(3)]
    t = [f32(rng.standard_normal(K) * 0.3 + 0.2) for _ in range(3)]
    return feat, z, W, b3, s, t


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("KF,Z,C,scales,want", [(32, 6, 2, True, ("logits", "sm")), (32, 1, 3, False, ("logits",)), (64, 6, 2, True, ("sm",)),
                                                (64, 1, 3, True, ("logits", "sm")), (32, 6, 3, True, ("sm",)), (64, 6, 2, False, ("logits",))])
def test_recomb_samples_vs_float64_restatement(L, dt, KF, Z, C, scales, want):
    B, n, P = 2, 3, 80
    rng = np.random.default_rng(100 * KF + 10 * Z + C + dt)
    feat, z, W, b3, s, t = random_case(rng, B, n, P, KF, Z, C, dt, scales)
    lg, sm, E = restate(feat, z, W, b3, s, t, n, dt)
    got = launch(L, feat, z, W, b3, s, t, n, dt, want)
    if "logits" in got:
        err = np.abs(got["logits"] - lg)
        print("logits: max err %.3e, max bound 2E %.3e, max err / (2E) %.3f, max |logit| %.2f" % (err.max(), 2 * E.max(), (err / (2 * E)).max(), np.abs(lg).max()))
        assert (err <= 2 * E).all()
        assert lg.std() > 0.1 and np.abs(lg[0] - lg[1]).max() > 1e-3          # the samples of an image differ
    if "sm" in got:
        err = np.abs(got["sm"] - sm)
        bound = 2 * E.max(axis=-1, keepdims=True)
        print("soft-max: max err %.3e, max err / bound %.3f" % (err.max(), (err / bound).max()))
        assert (err <= bound).all()
        assert np.abs(got["sm"].sum(axis=-1) - 1.0).max() < 1e-5


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("KF,Z,C", [(32, 6, 2), (64, 1, 3)])
def test_recomb_samples_exact_integer_case(L, dt, KF, Z, C):
    """Small integers, s = 1: every intermediate is an integer of magnitude <= 256 (exact in bf16), the logits are exact in fp32 in
    any summation order -> bit-for-bit equality with the restatement."""
    B, n, P = 2, 3, 80
    rng = np.random.default_rng(7 + KF + Z)

    def sparse(rows, cols, nnz, values):
        w = np.zeros((rows, cols))
        for c in range(cols):
            w[rng.choice(rows, nnz, replace=False), c] = rng.choice(values, nnz)
        return w
    feat = rng.integers(0, 3, (B, P, KF)).astype(np.float64)                                  # 0 .. 2
    z = rng.integers(-2, 3, (B * n, Z)).astype(np.float64)
    W0 = np.concatenate([sparse(KF, K, 3, [-1.0, 1.0]), sparse(Z, K, 1, [-1.0, 1.0])])        # |pre0| <= 3 * 2 + 2, + t <= 10
    W1 = sparse(K, K, 3, [-1.0, 1.0, 2.0])                                                    # <= 3 * 2 * 10 + 2 = 62
    W2 = sparse(K, K, 3, [-1.0, 1.0])                                                         # <= 3 * 62 + 2 = 188 <= 256
    W3 = rng.integers(-2, 3, (K, C)).astype(np.float64)
    b3 = rng.integers(-3, 4, C).astype(np.float64)
    s = [None, np.ones(K), None]
    t = [rng.integers(0, 3, K).astype(np.float64) for _ in range(3)]
    lg, sm, _ = restate(feat, z, [W0, W1, W2, W3], b3, s, t, n, dt)
    assert np.abs(lg).max() <= 2 * 32 * 188 + 3 and len(np.unique(lg)) > 50 and np.abs(lg[0] - lg[1]).max() > 0
    got = launch(L, feat, z, [W0, W1, W2, W3], b3, s, t, n, dt, ("logits", "sm"))
    np.testing.assert_array_equal(got["logits"], lg)
    assert np.abs(got["sm"] - sm).max() <= 2.0 ** -21


def test_recomb_samples_rejects_what_it_does_not_take(L):
    from phiseg_code_amd.runtime import PhxError
    rng = np.random.default_rng(3)
    B, n, P, Z, C = 1, 2, 40, 6, 2
    feat, z, W, b3, s, t = random_case(rng, B, n, P, 32, Z, C, F32, True)
    launch(L, feat, z, W, b3, s, t, n, F32)                                                   # the accepted call
    with pytest.raises(PhxError):
        launch(L, feat, z, W, b3, s, t, n, F32, Kc=16)                                        # K != 32
    with pytest.raises(PhxError):
        launch(L, feat, z, W, b3, s, t, n, F32, KF=48)                                        # a feature width the kernel has no form for
    with pytest.raises(PhxError):
        launch(L, feat, z, W, b3, s, t, n, F32, C=9)
    with pytest.raises(PhxError):
        launch(L, feat, z, W, b3, s, t, n, F32, Z=33)
    with pytest.raises(PhxError):
        launch(L, feat, z, W, b3, s, t, n, F32, Z=0)
    with pytest.raises(PhxError):
        launch(L, feat, z, W, b3, s, t, n, F32, want=())                                      # both outputs NULL
    with pytest.raises(PhxError):
        launch(L, feat, z, W, b3, s, t, n, 7)                                                 # not a dtype code
