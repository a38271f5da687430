"""dev (GPU box): the norm + 1x1 head fusion at the likelihood's top layer (64 x 128 x 128 x 128 -> 2): separate launches vs fused."""
import sys
import torch
sys.path.insert(0, ".")
from phiseg_code_amd import runtime as rt
L = rt.lib()
st = torch.cuda.current_stream().cuda_stream
BF = rt.BF16
def timeit(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
B, H, W, C, NO = 64, 128, 128, 128, 2
P = B * H * W
y = (torch.randn(P, C, device="cuda") * 1.5).to(torch.bfloat16)
a = torch.empty_like(y); dA = torch.empty_like(y); dx = torch.empty_like(y)
sums = torch.stack([y.float().sum(0), (y.float() ** 2).sum(0)], -1).contiguous()
g, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
wh, bh = torch.randn(C, NO, device="cuda") * 0.1, torch.zeros(NO, device="cuda")
mean, rstd, scale, shift = (torch.empty(C, device="cuda") for _ in range(4))
yh, dyh = torch.empty(P, NO, device="cuda"), torch.randn(P, NO, device="cuda")
s2 = torch.zeros(4, C, 2, device="cuda"); dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
ap = lambda: L.norm_apply_fused(y.data_ptr(), BF, sums.data_ptr(), None, g.data_ptr(), b.data_ptr(), 1e-3, a.data_ptr(), BF, mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, None, 0.0, 1, P, C, C, 1, st)
hf = lambda: L.head1x1_fwd(a.data_ptr(), BF, wh.data_ptr(), bh.data_ptr(), yh.data_ptr(), P, C, NO, 0, st)
aph = lambda: L.norm_apply_fused_head(y.data_ptr(), BF, sums.data_ptr(), None, g.data_ptr(), b.data_ptr(), 1e-3, a.data_ptr(), BF, mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, None, 0.0, 1, P, C, C, 1, wh.data_ptr(), bh.data_ptr(), NO, yh.data_ptr(), st)
hd = lambda: L.head1x1_dgrad(dyh.data_ptr(), wh.data_ptr(), dA.data_ptr(), BF, P, C, NO, st)
br = lambda: L.norm_bwd_reduce(dA.data_ptr(), BF, y.data_ptr(), BF, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(), s2.data_ptr(), 1, P, C, C, 1, 4, st)
brh = lambda: L.norm_bwd_reduce_head(dyh.data_ptr(), wh.data_ptr(), NO, y.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(), s2.data_ptr(), 1, P, C, C, 1, 4, st)
ba = lambda: L.norm_bwd_apply_fused_bias(dA.data_ptr(), BF, y.data_ptr(), BF, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g.data_ptr(), s2.data_ptr(), dx.data_ptr(), BF, dg.data_ptr(), db.data_ptr(), None, None, None, 1, P, C, C, 1, 4, st)
bah = lambda: L.norm_bwd_apply_fused_head(dyh.data_ptr(), wh.data_ptr(), NO, y.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g.data_ptr(), s2.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), None, None, None, 1, P, C, C, 1, 4, st)
for name, fn in (("apply", ap), ("head fwd", hf), ("apply+head", aph), ("head dgrad", hd), ("bwd reduce", br), ("bwd reduce (head)", brh), ("bwd apply", ba), ("bwd apply (head)", bah)):
    print("%-20s %7.1f us" % (name, timeit(fn)), flush=True)


# ---- the head's filter / bias gradient as a rider of the backward pair, against the stand-alone job it replaces --------------------------
# per shape: trio = reduce + apply + ONE-job phx_head1x1_wgrad_multi (xscale form: it reads y again); rider = reduce_rider + apply_rider.
# Each arm is timed REP times (sequences of N) -- the spread of an arm is what a difference has to clear.
import ctypes
import numpy as np
HEADW_DT = [("x", "<u8"), ("dy", "<u8"), ("dw", "<u8"), ("db", "<u8"), ("npix", "<u8"), ("C", "<i4"), ("PL", "<i4"), ("chunk", "<i4"),
            ("blk0", "<i4"), ("xscale", "<u8"), ("xshift", "<u8"), ("xact", "<i4"), ("pad", "<i4")]
REP = 5


def rider_case(B, H, W, C, NO, head_form):
    P = B * H * W
    y = (torch.randn(P, C, device="cuda") * 1.5).to(torch.bfloat16)
    dA, dx = torch.randn(P, C, device="cuda").to(torch.bfloat16), torch.empty(P, C, device="cuda", dtype=torch.bfloat16)
    dyh, wh = torch.randn(P, NO, device="cuda"), torch.randn(C, NO, device="cuda") * 0.1
    g = torch.ones(C, device="cuda")
    scale, shift, mean = 1 + 0.3 * torch.randn(C, device="cuda"), 0.2 * torch.randn(C, device="cuda"), 0.1 * torch.randn(C, device="cuda")
    rstd = 1 + 0.1 * torch.rand(C, device="cuda")
    s2, hacc = torch.zeros(4, C, 2, device="cuda"), torch.zeros(4, C + 1, NO, device="cuda")
    dg, db, dw, dbh = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, NO, device="cuda"), torch.zeros(NO, device="cuda")
    p = lambda t: t.data_ptr()
    stat = (p(scale), p(shift), p(mean), p(rstd))
    if head_form:
        red = lambda: L.norm_bwd_reduce_head(p(dyh), p(wh), NO, p(y), *stat, p(s2), 1, P, C, C, 1, 4, st)
        app = lambda: L.norm_bwd_apply_fused_head(p(dyh), p(wh), NO, p(y), *stat, p(g), p(s2), p(dx), p(dg), p(db), None, None, None, 1, P, C, C, 1, 4, st)
    else:
        red = lambda: L.norm_bwd_reduce(p(dA), BF, p(y), BF, *stat, p(s2), 1, P, C, C, 1, 4, st)
        app = lambda: L.norm_bwd_apply_fused(p(dA), BF, p(y), BF, *stat, p(g), p(s2), p(dx), BF, p(dg), p(db), 1, P, C, C, 1, 4, st)
    lead = (None if head_form else p(dA), p(dyh), p(wh) if head_form else None, NO, p(y), *stat)
    red_r = lambda: L.norm_bwd_reduce_rider(*lead, p(s2), p(hacc), P, C, 1, 4, st)
    app_r = lambda: L.norm_bwd_apply_fused_rider(*lead, p(g), p(s2), p(dx), p(dg), p(db), p(hacc), p(dw), p(dbh), P, C, 1, 4, st)
    plan = (ctypes.c_int * 4)()
    L.head1x1_wgrad_plan(P, C, NO, plan)
    rec = np.zeros(1, dtype=HEADW_DT)
    rec[0] = (p(y), p(dyh), p(dw), p(dbh), P, C, plan[0], plan[1], 0, p(scale), p(shift), 1, 0)
    desc = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    job = lambda: L.head1x1_wgrad_multi(p(desc), 1, plan[2], BF, NO, plan[3], st)

    def trio():
        red(); app(); job()

    def pair():
        red_r(); app_r()
    rows = {}
    for name, fn in (("reduce", red), ("apply", app), ("head job", job), ("reduce+rider", red_r), ("apply+fold", app_r), ("TRIO", trio), ("RIDER PAIR", pair)):
        t = [timeit(fn) for _ in range(REP)]
        rows[name] = t
        print("  %-14s %s  mean %7.1f us  spread %5.1f" % (name, " ".join("%7.1f" % v for v in t), sum(t) / REP, max(t) - min(t)), flush=True)
    gain = sum(rows["TRIO"]) / REP - sum(rows["RIDER PAIR"]) / REP
    spread = max(max(rows[k]) - min(rows[k]) for k in ("TRIO", "RIDER PAIR"))
    print("  -> rider saves %.1f us per step (largest same-arm spread %.1f us): %s" % (gain, spread, "KEEP" if gain > spread else "DROP"), flush=True)


for shape in ((64, 128, 128, 128, 2, True), (64, 64, 64, 192, 2, False), (64, 32, 32, 192, 2, False), (64, 128, 128, 128, 4, True), (64, 64, 64, 128, 4, False)):
    print("rider %s" % (shape,), flush=True)
    try:
        rider_case(*shape)
    except rt.PhxError as e:          # (C = 192: C / 8 = 24 is outside the riders' domain -- the stand-alone job stays)
        print("  not in the riders' domain: %s" % e, flush=True)
