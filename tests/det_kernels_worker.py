"""Worker of tests/test_kernels_deterministic_gpu.py: kernel parity against the float64 oracle INSIDE a PHX_DETERMINISTIC=1 process.

libphx reads PHX_DETERMINISTIC once per process and then plans other launches at a dozen sites (one block per reduction, partial filters
plus an ordered fold, fixed-point loss partials, block b -> accumulator replica b).  tests/test_kernels_gpu.py runs with the variable
unset, so this worker -- started with it set, one process, one GPU context -- calls the same parity functions (imported, not copied) on
their small cases, plus the checks that only make sense in this mode (section "mode only" below).

Output: one line per check, `CHECK <name> PASS` or `CHECK <name> FAIL <message>`, then `DONE <count> <seconds>`.  An AssertionError is a
FAIL and the next check runs; anything else (a HIP error, an unexpected PhxError, a RuntimeError of torch) prints `ABORT <name>` and
ends the process with a non-zero status at once: nothing more is started on the GPU.  Nothing is retried.

Which check reaches which deterministic branch:
  losses_opt.hip  k_residual_ce fixed point / k_reduce_loss_parts   residual_ce[...], residual_ce_contract[...]
                  phx_kl_diag_gauss (one block)                      kl_and_adam, kl_multi[...] (its per-level launches)
                  phx_kl_diag_gauss_multi (one block per level)      kl_multi[...]
  norm.hip        phx_norm_stats chunk = P                           norm_stats_one_block[...], norm_fwd_bwd[...], bn_small[...]
  norm_bwd.hip    norm_bwd_reduce_launch chunk = ceil(P / nrep)      norm_bwd_nrep64[...]
                  phx_bn_bwd_onepass_supported == 0                  mode_is_on
  norm_onelaunch  norm_wave_plan want = 1                            norm_small[...] (64 samples: several passes of one block)
  heads.hip       head_wgrad_geometry ch = npix, g = 1               mode_is_on, head1x1[...], head1x1_wgrad_multi[...], latent_heads[...]
  elementwise.hip phx_channel_sum_accumulate in one block            concat_split_add_cast_misc
  conv_direct.hip tiny-map kernel off, tpb = ntiles                  conv2d_direct[...], direct_wgrad_single_add[...]
  conv_wgrad.hip  wgrad_atomic_tiles() == 0, reduce gy = 1           mode_is_on, mfma[...], wgrad_small_tiles_ws[...], wgrad_deferred_*
  conv_mfma.hip   fwd_stats_atomic_ok false                          mode_is_on
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32, BF16 = 0, 1

# phx_residual_ce's contract beyond shift = 0 .. L-1 and all-or-no ds (tests/test_glue_kernel_edges_gpu.py runs the same list in the default
# mode): (C, H, W, shifts, ds levels handed over) as digit strings -- L = 3 with every way of leaving levels NULL that the all-or-none
# callers never take, then repeated shifts, no full-resolution level, the 16x level alone, eight levels of eight classes
RESIDUAL_CE_CONTRACT = [(3, H, W, "012", m) for (H, W) in ((16, 16), (32, 48)) for m in ("100", "010", "001", "101")] + \
                       [(C, H, W, sh, "1" * len(sh)) for (H, W) in ((16, 16), (32, 48))
                        for (C, sh) in ((2, "00"), (4, "13"), (3, "024"), (5, "4"), (2, "04"), (8, "00112344"))]

# ---- the table: (name prefix, function, cases).  A function named "K.<name>" lives in tests/test_kernels_gpu.py and is called as
# f(L, case) (case_star: f(L, *case)); the others are defined below.  Names carry no blanks (the pytest side splits the lines).
_RERUN = [
    # the small CONV_DIRECT_CASES.  (64,2,2,192,2,3), (2,4,4,24,2,3), (3,8,8,24,2,1), (7,3,5,70,3,3): the tiny-map filter-gradient kernel is
    # switched off here, they reach the generic k_conv_direct_wgrad.  ((1,6,6,38,32,1) is one pixel tile: the launch of the default mode.)
    ("conv2d_direct", "K.test_conv2d_direct_fwd_dgrad_wgrad", False, [
        (2, 16, 16, 3, 32, 3, "relu", False, F32, F32), (2, 64, 64, 1, 4, 3, "identity", True, F32, F32),
        (3, 8, 8, 24, 2, 1, "softplus", True, F32, F32), (2, 4, 4, 24, 2, 3, "identity", True, F32, F32),
        (5, 2, 2, 24, 24, 3, "relu", False, F32, F32), (2, 32, 32, 2, 64, 3, "identity", False, F32, BF16),
        (2, 16, 16, 128, 2, 1, "identity", True, BF16, F32), (2, 3, 3, 20, 17, 3, "identity", True, F32, F32),
        (1, 128, 128, 32, 32, 3, "identity", False, F32, F32), (64, 2, 2, 192, 2, 3, "identity", True, BF16, F32),
        (7, 3, 5, 70, 3, 3, "softplus", True, BF16, F32), (9, 4, 4, 2, 130, 3, "relu", True, F32, BF16)]),
    ("mfma", "K._mfma_case", False, [(2, 16, 16, 32, 32), (3, 8, 8, 64, 128), (5, 4, 4, 192, 64), (40, 2, 2, 32, 96), (3, 3, 3, 64, 32),
                                     (2, 12, 12, 32, 64), (1, 48, 48, 96, 32)]),
    ("norm_fwd_bwd", "K.test_norm_fwd_bwd", False, [
        ("batch", 3, 8, 8, 32, None, F32), ("batch", 2, 16, 16, 6, None, F32), ("batch", 2, 16, 16, 192, None, BF16),
        ("group", 3, 8, 8, 32, 2, F32), ("group", 2, 4, 4, 24, 2, F32), ("group", 2, 8, 8, 192, 12, BF16), ("instance", 3, 8, 8, 12, None, F32)]),
    ("bn_small", "K.test_bn_small_one_launch_layer", False, [(64, 2, 2, 192, 1), (64, 4, 4, 192, 1), (37, 3, 3, 48, 1), (64, 8, 8, 192, 1)]),
    ("bn_wide", "K.test_bn_wide_one_launch_layer_from_split_k_slices", False, [(64, 2, 2, 192, 1, 6), (64, 4, 4, 192, 1, 3), (12, 4, 4, 64, 1, 1),
                                                                             (37, 3, 3, 36, 0, 5)]),
    # ("group", 64, 2, 2, 192, ...) and (70, 4, 4, 32, ...): more samples than one pass of the single block holds
    ("norm_small", "K.test_norm_small_one_launch_layer", False, [("group", 3, 8, 8, 32, 2, 1), ("group", 2, 4, 4, 192, 12, 1),
                                                                 ("group", 64, 2, 2, 192, 12, 1), ("group", 70, 4, 4, 32, 2, 0)]),
    ("norm_fused_head", "K.test_norm_layer_with_fused_head", False, [("batch", 2, 16, 16, 128, 2), ("batch", 3, 8, 24, 32, 4), ("group", 2, 16, 16, 64, 2)]),
    ("head1x1", "K.test_head1x1_kernels", False, [(3, 16, 16, 128, 2, BF16, "identity"), (2, 8, 8, 192, 2, BF16, "softplus"),
                                                  (2, 4, 4, 32, 6, F32, "identity"), (2, 8, 8, 24, 4, F32, "softplus"),
                                                  (1, 128, 128, 128, 2, BF16, "identity"), (2, 2, 2, 32, 8, BF16, "identity")]),
    ("head1x1_wgrad_multi", "K.test_head1x1_wgrad_multi_matches_per_head_launches", False, [2, 4]),
    ("latent_heads", "K.test_latent_heads_fused", False, [(3, 16, 16, 32, 2, BF16), (2, 8, 8, 192, 2, BF16), (5, 2, 2, 192, 2, BF16), (2, 4, 4, 64, 6, BF16),
                                                          (1, 32, 32, 64, 4, F32)]),
    ("concat_split_add_cast_misc", "K.test_concat_split_add_cast_misc", None, [()]),
    ("kl_and_adam", "K.test_kl_and_adam", None, [()]),
    ("wgrad_deferred_multi_layer_reduction", "K.test_wgrad_deferred_multi_layer_reduction", None, [()]),
    ("wgrad_deferred_small_map_launches", "K.test_wgrad_deferred_small_map_launches", None, [()]),
    # both modes (tests/test_kernels_gpu.py runs them too); here a second launch must also give the same bits
    ("residual_ce_contract", "residual_ce_contract", True, RESIDUAL_CE_CONTRACT),
    ("kl_multi", "kl_multi", True, [(1, True), (3, True), (6, True), (1, False), (3, False), (6, False)]),
]
_MODE_ONLY = [
    ("mode_is_on", "mode_is_on", None, [()]),
    # kind, B, H, W, C, G, storage, act: batch norm at the engine's threshold P = 4096, at a P that 64 does not divide, group norm with
    # NS > 1 and G < C
    ("norm_bwd_nrep64", "norm_bwd_nrep64", True, [(kind, B, H, W, C, G, dt, act)
                                                  for (kind, B, H, W, C, G) in [("batch", 1, 64, 64, 32, 32), ("batch", 3, 40, 37, 64, 64),
                                                                                 ("group", 2, 72, 72, 32, 4)]
                                                  for dt in (BF16, F32) for act in (1, 0)]),
    ("norm_stats_one_block", "norm_stats_one_block", True, [(1, 128 * 128, 32, BF16), (1, 2 * 64 * 64, 192, BF16), (2, 64 * 64, 192, F32)]),
    ("wgrad_small_tiles_ws", "wgrad_small_tiles_ws", True, [(2, 16, 16, 32, 32), (3, 8, 8, 64, 128), (5, 4, 4, 192, 64), (40, 2, 2, 32, 96),
                                                            (3, 3, 3, 64, 32)]),
    ("direct_wgrad_single_add", "direct_wgrad_single_add", True, [(64, 2, 2, 192, 2, 3, BF16), (2, 4, 4, 24, 2, 3, F32), (7, 3, 5, 70, 3, 3, BF16)]),
    # C, H, W, Ls, B: the cases of test_residual_ce (48 blocks on 32 slots at 64 x 64) and 128 blocks: four to a slot
    ("residual_ce", "residual_ce_fixed_point", True, [(2, 64, 64, 5, 3), (4, 48, 48, 5, 3), (2, 32, 32, 1, 3), (3, 16, 16, 3, 3), (2, 24, 40, 4, 3),
                                                      (3, 32, 48, 5, 3), (8, 32, 16, 3, 3), (2, 64, 64, 5, 8)]),
]


def _name(prefix, case):
    if case == ():
        return prefix
    parts = case if isinstance(case, tuple) else (case,)
    return "%s[%s]" % (prefix, "-".join(str(p) for p in parts))


TABLE = [(_name(prefix, case), fn, star, case) for (prefix, fn, star, cases) in _MODE_ONLY + _RERUN for case in cases]
CHECKS = [t[0] for t in TABLE]                      # what the pytest side parametrises over: no GPU, no library load to get here
assert len(set(CHECKS)) == len(CHECKS) and not any(" " in n for n in CHECKS)


# ---- mode only ------------------------------------------------------------------------------------------------------------------
def mode_is_on(L):
    """Without these every other check could pass while the library plans the default mode's launches."""
    import ctypes
    assert os.environ.get("PHX_DETERMINISTIC") == "1"
    assert L.conv3x3_mfma_stats_atomic_supported(64, 8, 8, 192, 192) == 0
    assert L.bn_bwd_onepass_supported(64 * 32 * 32, 128, 1) == 0
    plan4 = (ctypes.c_int * 4)()
    L.head1x1_wgrad_plan(64 * 16 * 16, 192, 2, plan4)
    assert plan4[2] == 1 and plan4[1] == 64 * 16 * 16, list(plan4)             # one block that walks every pixel
    plan6 = (ctypes.c_int * 6)()
    for shape in [(2, 16, 16, 32, 32), (40, 2, 2, 32, 96), (3, 3, 3, 64, 32)]:  # at most 4 pixel tiles: atomics in the default mode
        L.conv3x3_wgrad_reduce_plan(*shape, plan6)
        assert plan6[0] == 1, (shape, list(plan6))
    L.conv3x3_wgrad_reduce_plan(40, 16, 16, 32, 32, plan6)                      # 40 slices: two reduction rows in the default mode
    assert plan6[1] >= 32 and plan6[5] == 1, list(plan6)


def norm_bwd_nrep64(L, kind, B, H, W, C, G, dt, act):
    """phx_norm_bwd_reduce + phx_norm_bwd_apply_fused with the 64 accumulator replicas the engine passes in this mode (no kernel test of
    the default mode goes above 4): dx, dgamma, dbeta against float64 autograd of the oracle, the reference and tolerances of
    test_norm_fwd_bwd (group norm: also phx_norm_bwd_apply_fused_bias, the same dx and the convolution bias gradient in closed form);
    everything computed twice, bit for bit.  With the identity activation also the partition itself: block b owns
    replica b, i.e. replica r holds the sums over pixels [r * ceil(P / 64), (r + 1) * ceil(P / 64)) and nothing else."""
    import numpy as np
    import torch
    from oracle import tf1_ops as T
    from tests import test_kernels_gpu as K
    nrep, S = 64, K.S
    rng = np.random.default_rng([11, B, H, W, C, dt, act])
    x = rng.standard_normal((B, H, W, C)) * 1.5 + 0.3
    gamma, beta = 1.0 + 0.2 * rng.standard_normal(C), 0.1 * rng.standard_normal(C)
    xr = K.rounded(x, dt).requires_grad_(True)
    gr = torch.as_tensor(gamma, dtype=torch.float32).double().requires_grad_(True)
    br = torch.as_tensor(beta, dtype=torch.float32).double().requires_grad_(True)
    if kind == "batch":
        NS, P, eps = 1, B * H * W, 1e-3
        yr = T.batch_norm_train(xr, gr, br)[0]
    else:
        NS, P, eps = B, H * W, 1e-5
        yr = T.group_norm(xr, gr, br, G)
    ar = T.relu(yr) if act else yr
    dA = rng.standard_normal((B, H, W, C))
    if act:        # where fp32 and float64 may put the pre-activation on different sides of the ReLU kink, no gradient arrives
        dA[np.abs(yr.detach().numpy()) < 1e-4] = 0.0
    dAr = K.rounded(dA, dt)
    (ar * dAr).sum().backward()
    xd, dAd, gd, bd = K.dev(x, dt), K.dev(dA, dt), K.dev(gamma), K.dev(beta)
    sums, pivot = torch.zeros(NS, C, 2).cuda(), torch.zeros(NS, C).cuda()
    L.norm_stats(xd.data_ptr(), dt, sums.data_ptr(), pivot.data_ptr(), NS, P, C, S())
    a = torch.empty(B, H, W, C, dtype=K.tdt(dt)).cuda()
    mean, rstd = torch.empty(NS * G).cuda(), torch.empty(NS * G).cuda()
    scale, shift = torch.empty(NS * C).cuda(), torch.empty(NS * C).cuda()
    L.norm_apply_fused(xd.data_ptr(), dt, sums.data_ptr(), pivot.data_ptr(), gd.data_ptr(), bd.data_ptr(), eps, a.data_ptr(), dt,
                       mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, None, 0.0, NS, P, C, G, act, S())
    K.close(K.host(a), ar.detach().numpy(), 2e-5 if dt == F32 else 6e-3, kind + " fwd")
    runs = []
    for _ in range(2):
        acc = torch.zeros(nrep, NS, C, 2).cuda()                    # (the header: zeroed by the caller)
        L.norm_bwd_reduce(dAd.data_ptr(), dt, xd.data_ptr(), dt, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                          acc.data_ptr(), NS, P, C, G, act, nrep, S())
        dx = torch.full((B, H, W, C), float("nan"), dtype=K.tdt(dt)).cuda()
        dgamma, dbeta = torch.zeros(C).cuda(), torch.zeros(C).cuda()
        L.norm_bwd_apply_fused(dAd.data_ptr(), dt, xd.data_ptr(), dt, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                               gd.data_ptr(), acc.data_ptr(), dx.data_ptr(), dt, dgamma.data_ptr(), dbeta.data_ptr(), NS, P, C, G, act,
                               nrep, S())
        dbias = torch.zeros(C).cuda()
        if kind == "group":     # the form the engine launches for group norm: the convolution bias gradient in closed form beside the same dx
            dx3 = torch.full_like(dx, float("nan"))
            dg3, dbe3 = torch.zeros(C).cuda(), torch.zeros(C).cuda()
            L.norm_bwd_apply_fused_bias(dAd.data_ptr(), dt, xd.data_ptr(), dt, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                                        rstd.data_ptr(), gd.data_ptr(), acc.data_ptr(), dx3.data_ptr(), dt, dg3.data_ptr(), dbe3.data_ptr(),
                                        sums.data_ptr(), pivot.data_ptr(), dbias.data_ptr(), NS, P, C, G, act, nrep, S())
            assert torch.equal(dx3, dx) and torch.equal(dg3, dgamma) and torch.equal(dbe3, dbeta)
        runs.append((acc, dx, dgamma, dbeta, dbias))
    acc, dx, dgamma, dbeta, dbias = runs[0]
    if kind == "group":         # (bound and scale of test_norm_fwd_bwd's bias gradient)
        ref_db = xr.grad.numpy().sum(axis=(0, 1, 2))
        scale_db = max(1.0, float(np.abs(xr.grad.numpy()).sum(axis=(0, 1, 2)).max()))
        err = float(np.abs(K.host(dbias) - ref_db).max()) / scale_db
        assert err < (2e-5 if dt == F32 else 2e-3), (kind, "bias gradient", err)
    K.close(K.host(dx), xr.grad.numpy(), 5e-5 if dt == F32 else 8e-3, kind + " fused dx")
    K.close(K.host(dgamma), gr.grad.numpy(), 5e-5 if dt == F32 else 2e-3, kind + " fused dgamma")
    K.close(K.host(dbeta), br.grad.numpy(), 5e-5 if dt == F32 else 2e-3, kind + " fused dbeta")
    for u, v in zip(*runs):
        assert torch.equal(u, v), "norm backward with 64 replicas: two runs differ in bits"
    if act == 0:
        # g = dA here.  Tolerance: a slice is at most 81 pixels, its fp32 sum is good to ~81 * 2^-24 and mean / rstd to ~1e-6 relative, so
        # 1e-4 of the largest sum is far above the arithmetic -- and a single pixel in the wrong slice moves a sum by ~1 / sqrt(81) of it
        x64, d64 = xr.detach().reshape(NS, P, G, C // G), dAr.reshape(NS, P, C)
        mu = x64.mean(dim=(1, 3), keepdim=True)
        xhat = ((x64 - mu) / torch.sqrt(((x64 - mu) ** 2).mean(dim=(1, 3), keepdim=True) + eps)).reshape(NS, P, C)
        chunk = (P + nrep - 1) // nrep
        ref = torch.zeros(nrep, NS, C, 2, dtype=torch.float64)
        for r in range(nrep):
            sl = slice(r * chunk, min(P, (r + 1) * chunk))
            ref[r, :, :, 0] = d64[:, sl].sum(dim=1)
            ref[r, :, :, 1] = (d64[:, sl] * xhat[:, sl]).sum(dim=1)
        K.close(K.host(acc), ref.numpy(), 1e-4, kind + " replica r = pixel slice r")


def norm_stats_one_block(L, NS, P, C, dt):
    """phx_norm_stats with chunk = P (one block per sample group walks all P pixels): the sums about the pivot against float64.
    Bound per channel: the longest chain of fp32 additions a sum goes through is P / PL per thread + PL partial sums in LDS (PL = pixel
    lanes of the block) + the term's own roundings, so |error| <= (P / PL + PL + 8) * 2^-24 * sum |term|; mean and rstd, finalised from
    the sums, to the 1e-5 the one-launch batch-norm tests ask of theirs."""
    import numpy as np
    import torch
    from tests import test_kernels_gpu as K
    S = K.S
    rng = np.random.default_rng([12, NS, P, C, dt])
    x = rng.standard_normal((NS, P, C)) * 1.5 + 0.3
    xd = K.dev(x, dt)
    x64 = K.rounded(x, dt).numpy()
    piv = x64[:, :1, :]
    t1, t2 = x64 - piv, (x64 - piv) ** 2
    PL = 256 // (C // 8)
    bound = (P / PL + PL + 8) * 2.0 ** -24
    runs = []
    for _ in range(2):
        sums = torch.zeros(NS, C, 2).cuda()                          # accumulated: the header asks for zeros
        pivot = torch.full((NS, C), float("nan")).cuda()             # written
        L.norm_stats(xd.data_ptr(), dt, sums.data_ptr(), pivot.data_ptr(), NS, P, C, S())
        runs.append((sums, pivot))
    sums, pivot = runs[0]
    assert np.array_equal(K.host(pivot), piv[:, 0, :])
    got = K.host(sums)
    for j, t in enumerate((t1, t2)):
        err, lim = np.abs(got[:, :, j] - t.sum(axis=1)), bound * np.abs(t).sum(axis=1)
        assert np.all(err <= lim), "norm_stats sum %d: error is %.3g times the bound" % (j, float((err / lim).max()))
    gd, bd = torch.ones(C).cuda(), torch.zeros(C).cuda()
    mean, rstd, scale, shift = (torch.empty(NS * C).cuda() for _ in range(4))
    L.norm_finalize(sums.data_ptr(), pivot.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-3, NS, P, C, C, mean.data_ptr(), rstd.data_ptr(),
                    scale.data_ptr(), shift.data_ptr(), None, None, 0.0, S())
    K.close(K.host(mean).reshape(NS, C), x64.mean(axis=1), 1e-5, "mean")
    K.close(K.host(rstd).reshape(NS, C), 1.0 / np.sqrt(x64.var(axis=1) + 1e-3), 1e-5, "rstd")
    for u, v in zip(*runs):
        assert torch.equal(u, v), "norm_stats: two runs differ in bits"


def wgrad_small_tiles_ws(L, B, H, W, Cin, Cout):
    """phx_conv3x3_wgrad_mfma_bf16 with a workspace on maps of 1 to 4 pixel tiles: the default mode adds those straight into dw with
    atomics, this mode writes partial filters and folds them in order.  Accumulated onto what dw holds, against float64 autograd (the
    tolerance of _mfma_case's workspace launch); the workspace need not be initialised (NaN before each launch); twice, bit for bit."""
    import ctypes
    import numpy as np
    import torch
    from oracle import tf1_ops as T
    from tests import test_kernels_gpu as K
    S = K.S
    plan6 = (ctypes.c_int * 6)()
    L.conv3x3_wgrad_reduce_plan(B, H, W, Cin, Cout, plan6)
    assert plan6[0] == 1 and plan6[5] == 1, list(plan6)
    rng = np.random.default_rng([13, B, H, W, Cin, Cout])
    x, dy = rng.standard_normal((B, H, W, Cin)), rng.standard_normal((B, H, W, Cout))
    xr = K.rounded(x, BF16)
    wr = torch.zeros(3, 3, Cin, Cout, dtype=torch.float64, requires_grad=True)
    (T.conv2d_same(xr, wr) * K.rounded(dy, BF16)).sum().backward()
    xd, dyd = K.dev(x, BF16), K.dev(dy, BF16)
    wsb = int(L.conv3x3_wgrad_ws_bytes(B, H, W, Cin, Cout))
    assert wsb >= 4
    ws = torch.empty(wsb // 4, dtype=torch.float32).cuda()
    runs = []
    for _ in range(2):
        ws.fill_(float("nan"))
        dw = torch.full((3, 3, Cin, Cout), 0.25, dtype=torch.float32).cuda()
        L.conv3x3_wgrad_mfma_bf16(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb, B, H, W, Cin, Cout, S())
        runs.append(dw)
    K.close(K.host(runs[0]) - 0.25, wr.grad.numpy(), 1e-4, "mfma wgrad (workspace, small tiles)")
    assert torch.equal(runs[0], runs[1]), "small-tile filter gradient: two runs differ in bits"


def direct_wgrad_single_add(L, B, H, W, Cin, Cout, k, xdt):
    """phx_conv2d_direct_wgrad on tiny maps with Cout <= 4 (the mu / sigma convolutions): the tiny-map kernel's pixel groups meet in
    atomics, so this mode launches the generic kernel with ONE block along the pixel axis -- a single add per filter element.  Hence
    dw(c) == c + dw(0) in fp32, bit for bit, for any start value c (two blocks adding a and b give (c + a) + b instead, which rounds
    differently on a good part of the elements); also against float64 autograd and twice."""
    import numpy as np
    import torch
    from oracle import tf1_ops as T
    from tests import test_kernels_gpu as K
    S = K.S
    rng = np.random.default_rng([14, B, H, W, Cin, Cout, k])
    x, dy = rng.standard_normal((B, H, W, Cin)), rng.standard_normal((B, H, W, Cout))
    xr = K.rounded(x, xdt)
    wr = torch.zeros(k, k, Cin, Cout, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    ((T.conv2d_same(xr, wr) + br.reshape(1, 1, 1, -1)) * K.rounded(dy, F32)).sum().backward()
    xd, dyd = K.dev(x, xdt), K.dev(dy)
    out = {}
    for c in (0.0, 0.0, 0.37):
        dw = torch.full((k, k, Cin, Cout), c, dtype=torch.float32).cuda()
        db = torch.full((Cout,), c, dtype=torch.float32).cuda()
        L.conv2d_direct_wgrad(xd.data_ptr(), xdt, dyd.data_ptr(), F32, dw.data_ptr(), db.data_ptr(), B, H, W, Cin, Cout, k, S())
        torch.cuda.synchronize()
        if c in out:
            assert torch.equal(out[c][0], dw) and torch.equal(out[c][1], db), "direct filter gradient: two runs differ in bits"
        out[c] = (dw, db)
    K.close(K.host(out[0.0][0]), wr.grad.numpy(), 2e-5, "wgrad")
    K.close(K.host(out[0.0][1]), br.grad.numpy(), 2e-5, "dbias")
    c32 = torch.tensor(0.37, dtype=torch.float32).cuda()
    assert torch.equal(out[0.37][0], c32 + out[0.0][0]), "dw: more than one add per filter element"
    assert torch.equal(out[0.37][1], c32 + out[0.0][1]), "dbias: more than one add per element"


def residual_ce_fixed_point(L, C, H, W, Ls, B):
    from tests import test_kernels_gpu as K
    K._residual_ce_case(L, C, H, W, Ls, B=B, bitwise=True)


def residual_ce_contract(L, C, H, W, shifts, ds_levels):
    from tests import test_kernels_gpu as K
    K._residual_ce_case(L, C, H, W, len(shifts), bitwise=True, shifts=[int(c) for c in shifts], ds_mask=[c == "1" for c in ds_levels])


def kl_multi(L, nlev, grads):
    from tests import test_kernels_gpu as K
    K._kl_multi_case(L, nlev, grads, bitwise=True)


# ---------------------------------------------------------------------------------------------------------------------------------
def main():
    only = set(sys.argv[1:])                        # (a development aid: names of the checks to run; none = all)
    t0 = time.time()
    import torch
    from phiseg_code_amd import runtime as rt
    from tests import test_kernels_gpu as K
    assert torch.cuda.is_available(), "the worker needs a GPU"
    L = rt.lib()
    done = 0
    for name, fn, star, case in TABLE:
        if only and name not in only:
            continue
        f = getattr(K, fn[2:]) if fn.startswith("K.") else globals()[fn]
        try:
            if star is None:
                f(L)
            elif star:
                f(L, *case)
            else:
                f(L, case)
            torch.cuda.synchronize()
        except AssertionError as e:
            print("CHECK %s FAIL %s" % (name, " ".join(str(e).split())[:600] or "assertion"), flush=True)
        except BaseException as e:                  # a HIP error, an unexpected PhxError, a RuntimeError of torch: stop here
            print("ABORT %s %s: %s" % (name, type(e).__name__, " ".join(str(e).split())[:600]), flush=True)
            sys.exit(3)
        else:
            print("CHECK %s PASS" % name, flush=True)
        done += 1
    print("DONE %d %.1f" % (done, time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
