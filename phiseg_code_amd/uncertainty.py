"""Per-pixel uncertainty and error maps of N Monte-Carlo segmentation samples, formed on the device in one pass (phx_mc_stats,
csrc/mc_stats.hip): what the reference's inference API computes in numpy from samples pulled to the host one sess.run at a time
(phiseg/phiseg_model.py:378-475) and what its sample script calls generate_error_maps (phiseg_generate_samples.py:46-82).

Plane definitions: include/phx.h, "per-pixel Monte-Carlo sample statistics".  There is no host fallback."""
import numpy as np

MAPS = ("std_mean", "xent_mean", "cov_trace", "cov_det", "cov_det_drop_last", "e_ss", "e_sy", "e_yy")     # plane k = PHX_MC_<NAME>
PLANE = {name: k for k, name in enumerate(MAPS)}
_NEED_SM = ("std_mean", "cov_det", "cov_det_drop_last", "e_ss", "e_sy", "e_yy")
_NEED_LOGITS = ("xent_mean", "cov_trace")
MAX_CLASSES = 8            # MC_MAXC of csrc/mc_stats.hip: this one stays capped (the many-class entries are in many_class.py)


def _available(has_logits, has_sm, has_gt, has_ref):
    out = []
    for name in MAPS:
        if name in _NEED_SM and not has_sm:
            continue
        if name in _NEED_LOGITS and not has_logits:
            continue
        if name in ("e_sy", "e_yy") and not has_gt:
            continue
        if name == "xent_mean" and not has_ref:
            continue
        out.append(name)
    return out


def check_classes(C):
    """phx_mc_stats keeps a pixel's C x C covariance in registers: 2 <= C <= 8, said here before anything is uploaded or launched."""
    if not 2 <= int(C) <= MAX_CLASSES:
        raise ValueError("mc_statistics: 2 <= C <= %d classes (phx_mc_stats keeps a pixel's C x C covariance in registers), got C = %d"
                         % (MAX_CLASSES, int(C)))


def mc_stats_device(logits_ptr, sm_ptr, gt_ptr, sref_ptr, I, N, M, P, C, maps, stream, mean=False, amax=False):
    """Launch phx_mc_stats on `stream` over device memory: -> (maps tensor [I, 8, P] f32 or None, mean_sm tensor [I, P, C] or None,
    arg-max tensor [I, P] u8 or None), all on the device and NOT synchronised."""
    import torch
    from . import runtime as rt
    check_classes(C)
    L = rt.lib()
    for name in maps:
        if name not in PLANE:
            raise ValueError("unknown map %r (one of %s)" % (name, ", ".join(MAPS)))
    if "e_yy" in maps and N < M:
        raise ValueError("e_yy reads the first M = %d samples: it needs N >= M (N = %d)" % (M, N))
    mask = 0
    for name in maps:
        mask |= 1 << PLANE[name]
    dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(I, len(MAPS), P, dtype=torch.float32, device=dev) if mask else None       # (planes not asked for stay unwritten)
    mean_t = torch.empty(I, P, C, dtype=torch.float32, device=dev) if mean else None
    amax_t = torch.empty(I, P, dtype=torch.uint8, device=dev) if amax else None
    wsb = int(L.mc_stats_ws_bytes(I, N, M, P, C))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev) if wsb else None
    L.mc_stats(logits_ptr or None, sm_ptr or None, gt_ptr or None, sref_ptr or None, I, N, M, P, C, mask,
               mean_t.data_ptr() if mean else None, amax_t.data_ptr() if amax else None, out.data_ptr() if mask else None,
               ws.data_ptr() if ws is not None else None, wsb, stream)
    return out, mean_t, amax_t


def mc_statistics(logits=None, sm=None, gts=None, s_ref=None, maps=None, mean=True, num_samples=None, stream=None):
    """Per-pixel statistics of Monte-Carlo samples.

    logits, sm: [N, X, Y, C] (one image) or [I, N, X, Y, C] float32 host arrays, or the engine's device buffers of a sampling plan
                ([I * N, X, Y, C], rows i * N + k; pass num_samples = N and the plan's stream) -- either may be None;
    gts:        [M, X, Y] / [I, M, X, Y] label maps (for e_sy / e_yy), s_ref: [X, Y] / [I, X, Y] one annotation (for xent_mean);
    maps:       names out of MAPS (default: every map the given inputs allow).
    -> dict name -> [X, Y] / [I, X, Y] float32, plus "mean_sm" [.., X, Y, C] and "argmax" [.., X, Y] when sm is given and mean=True.
    Only the requested maps are copied back to the host."""
    import torch
    from . import runtime as rt
    L = rt.lib()
    first = logits if logits is not None else sm
    if first is None:
        raise ValueError("mc_statistics needs logits or sm")
    check_classes(tuple(first.shape if hasattr(first, "ptr") else np.shape(first))[-1])
    on_device = hasattr(first, "ptr")
    dev = torch.device("cuda", torch.cuda.current_device())
    keep = []

    def up(a, dt):
        t = torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
        keep.append(t)
        return t.data_ptr()

    if on_device:
        if num_samples is None or stream is None:
            raise ValueError("device buffers need num_samples and the stream their producer ran on")
        shp = tuple(first.shape)
        N = int(num_samples)
        I, X, Y, C = shp[0] // N, shp[1], shp[2], shp[3]
        if I * N != shp[0]:
            raise ValueError("buffer of %d rows does not hold %d samples per image" % (shp[0], N))
        batched = I > 1
        lp = logits.ptr if logits is not None else None
        sp = sm.ptr if sm is not None else None
    else:
        arr = np.asarray(first)
        batched = arr.ndim == 5
        if arr.ndim not in (4, 5):
            raise ValueError("samples are [N, X, Y, C] or [I, N, X, Y, C]")
        I, N, X, Y, C = ((1,) + arr.shape) if not batched else arr.shape
        for other in (logits, sm):
            if other is not None and tuple(np.shape(other)) != arr.shape:
                raise ValueError("logits and sm differ in shape")
        lp = up(logits, np.float32) if logits is not None else None
        sp = up(sm, np.float32) if sm is not None else None
        stream = torch.cuda.current_stream().cuda_stream
    P = X * Y
    M = 0
    gp = rp = None
    if gts is not None:
        g = np.asarray(gts).reshape((I, -1, X, Y))
        M = g.shape[1]
        gp = up(g, np.uint8)
    if s_ref is not None:
        rp = up(np.asarray(s_ref).reshape((I, X, Y)), np.uint8)
    if maps is None:
        maps = _available(logits is not None, sm is not None, gts is not None, s_ref is not None)
        if N < M:
            maps = [m for m in maps if m != "e_yy"]
    maps = list(maps)
    want_mean = bool(mean and sm is not None)
    if on_device and keep:
        torch.cuda.current_stream().synchronize()           # the uploads ran on torch's stream, the kernel runs on the plan's
    out, mean_t, amax_t = mc_stats_device(lp, sp, gp, rp, I, N, M, P, C, maps, stream, mean=want_mean, amax=want_mean)
    if on_device:
        L.stream_sync(stream)
    else:
        torch.cuda.current_stream().synchronize()
    res = {}
    shape = (I, X, Y) if batched else (X, Y)
    for name in maps:
        res[name] = out[:, PLANE[name]].cpu().numpy().reshape(shape)
    if want_mean:
        res["mean_sm"] = mean_t.cpu().numpy().reshape(shape + (C,))
        res["argmax"] = amax_t.cpu().numpy().reshape(shape)
    return res


def generate_error_maps(sample_arr, gt_arr):
    """The reference's generate_error_maps (phiseg_generate_samples.py:46-82): sample_arr [N, X, Y, C] soft-max samples, gt_arr
    [M, X, Y, C] one-hot annotations -> (E_ss, E_sy_avg, E_yy_avg), each [X, Y].  E_yy_avg reproduces the reference's formula, which
    pairs the first M SAMPLES (not the annotations) with the annotations; it needs N >= M (ValueError, where the reference raises
    IndexError)."""
    gts = np.asarray(gt_arr).argmax(axis=-1).astype(np.uint8)
    sample_arr = np.asarray(sample_arr)
    if sample_arr.shape[0] < gts.shape[0]:
        raise ValueError("generate_error_maps: E_yy reads the first M = %d samples, only N = %d given" % (gts.shape[0], sample_arr.shape[0]))
    r = mc_statistics(sm=sample_arr, gts=gts, maps=("e_ss", "e_sy", "e_yy"), mean=False)
    return r["e_ss"], r["e_sy"], r["e_yy"]
