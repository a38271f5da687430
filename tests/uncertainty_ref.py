"""Seeded inputs and a numpy restatement of the eight per-pixel Monte-Carlo maps (include/phx.h, PHX_MC_*), shared by
tools/make_goldens_uncertainty.py (which stores what the REFERENCE's own code gives on these inputs) and the uncertainty tests.

The restatement follows the reference's arithmetic step by step (phiseg/phiseg_model.py:378-475 of the reference,
phiseg_generate_samples.py:46-82) and takes the working precision as an argument: float64 is the yardstick, float32 is the
precision the reference itself works in -- its error against the float64 golden sets the band the device must stay in."""
import numpy as np

from tests.helpers import METRICS_CASES, metrics_case

CASES = METRICS_CASES[:4]                # (seed, N, M, X, Y, C, mode): (6, 4, 2), (16, 4, 4), (5, 3, 3), (4, 2, 2 "identical")
assert all(c[1] >= c[2] for c in CASES), "E_YY reads the first M samples"
MAPS = ("std_mean", "xent_mean", "cov_trace", "cov_det", "cov_det_drop_last", "e_ss", "e_sy", "e_yy")


def logits_of(sm):
    """Logits with the given soft-max, shifted so that both sides of the reference's clip(., 1e-5, 1 - 1e-5) are active:
    log(sm) - mean_c log(sm) + 0.3 (1e-30 keeps an underflowed soft-max finite)."""
    lg = np.log(sm.astype(np.float64) + 1e-30)
    return (lg - lg.mean(axis=-1, keepdims=True) + 0.3).astype(np.float32)


def uncertainty_case(k, unnormalised=False):
    """-> (logits [N, X, Y, C] f32, sm [N, X, Y, C] f32, gts [M, X, Y] u8, s_ref [X, Y] u8) of case k.  unnormalised: every soft-max
    element times U(0.5, 1.5) -- rows no longer sum to one, so the C x C sample covariance is well conditioned (the COV_DET pin)."""
    seed = CASES[k][0]
    sm, gts = metrics_case(*CASES[k])
    logits = logits_of(sm)
    if unnormalised:
        rng = np.random.default_rng(1000 + seed)
        sm = (sm.astype(np.float64) * rng.uniform(0.5, 1.5, size=sm.shape)).astype(np.float32)
    return logits, sm, gts, gts[0].copy()


def lidc_case():
    """I = 3 images of N = 100 samples, M = 4 annotations, 128 x 128, C = 2: the inputs of test_device_metrics_batch_of_images_lidc_shape
    -> (logits [3, 100, 128, 128, 2], sm, gts [3, 4, 128, 128], s_ref [3, 128, 128])."""
    sms, gts, refs = [], [], []
    for seed in (21, 22, 23):
        sm, gt = metrics_case(seed, 100, 4, 128, 128, 2, "plain" if seed != 22 else "empty_fg")
        sms.append(sm); gts.append(gt); refs.append(gt[seed % 4])
    sm = np.stack(sms)
    return logits_of(sm), sm, np.stack(gts), np.stack(refs)


def reference_maps(logits, sm, gts, s_ref, dtype=np.float64):
    """The eight planes of one image in `dtype` arithmetic -> dict name -> [X, Y] (+ "var1": the ddof-1 variances [X, Y, C] of sm, the
    factors of Hadamard's bound on COV_DET; "mean_sm", "argmax")."""
    logits, sm = np.asarray(logits).astype(dtype), np.asarray(sm).astype(dtype)
    N, X, Y, C = sm.shape
    M = gts.shape[0]
    out = {}
    # predict_mean_variance_and_error_maps
    out["std_mean"] = np.mean(np.std(sm, axis=0), axis=-1)
    out["mean_sm"] = np.mean(sm, axis=0)
    out["argmax"] = np.argmax(out["mean_sm"], axis=-1)
    mx = logits.max(axis=-1, keepdims=True)
    lse = mx[..., 0] + np.log(np.exp(logits - mx).sum(axis=-1))
    picked = np.take_along_axis(logits, np.broadcast_to(np.asarray(s_ref).astype(np.int64)[None, ..., None], (N, X, Y, 1)), axis=-1)[..., 0]
    out["xent_mean"] = np.mean(lse - picked, axis=0)
    # predict_segmentation_sample_variance_sm_cov: sum of the eigenvalues = trace
    a = np.clip(logits[..., :-1].transpose((1, 2, 3, 0)), dtype(1e-5), dtype(1 - 1e-5))
    corr = np.einsum('ghij,ghkj->ghik', a, a) / dtype(N)
    mu = np.mean(a, axis=-1)
    cov = corr - np.einsum('ghi,ghj->ghij', mu, mu)
    out["cov_trace"] = np.trace(cov, axis1=-2, axis2=-1)
    # predict_segmentation_sample_variance_sm_cov_bf (and the same without the last class)
    s = sm.transpose((1, 2, 3, 0))
    d = s - s.mean(axis=-1, keepdims=True)
    cov1 = np.einsum('ghik,ghjk->ghij', d, d) / dtype(N - 1)
    out["cov_det"] = np.linalg.det(cov1)
    out["cov_det_drop_last"] = np.linalg.det(cov1[:, :, :-1, :-1])
    out["var1"] = np.einsum('ghii->ghi', cov1)
    # generate_error_maps
    eps = dtype(1e-8)
    lg = np.log(sm + eps)
    oh = np.eye(C, dtype=dtype)[np.asarray(gts).astype(np.int64)]                    # [M, X, Y, C]
    out["e_ss"] = np.mean(-np.sum(out["mean_sm"][None] * lg, axis=-1), axis=0)
    out["e_sy"] = np.mean(np.mean(-np.sum(oh[:, None] * lg[None], axis=-1), axis=1), axis=0)
    out["e_yy"] = np.mean(np.mean(-np.sum(oh[:, None] * lg[None, :M], axis=-1), axis=1), axis=0)
    return out


def band(golden, ref32):
    """The acceptance band of one plane: 4 x max(error of the float32 restatement against the golden, 2^-23 max|golden|): the factor
    allows for device expf / logf being a couple of ulp where numpy's are one and for another summation order."""
    err_ref32 = float(np.abs(np.asarray(ref32, dtype=np.float64) - golden).max())
    return 4.0 * max(err_ref32, 2.0 ** -23 * float(np.abs(golden).max())), err_ref32
