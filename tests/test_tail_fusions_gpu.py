"""The two fusions of the training step's serial tail (MI355X): the filter / bias gradient of a 1x1 head as a rider of its producer's
batch-norm backward (phx_norm_bwd_reduce_rider + phx_norm_bwd_apply_fused_rider) and the padded-filter folds of all deferred layers
in one launch (phx_unpad_filter_grad_multi) -- each against the launches it replaces, and in the plan (PHX_HEAD_RIDER=0 / 1)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_kernels_gpu import BF16, L, S, close, dev, host  # noqa: F401  (L: the module-scoped library fixture)

pytestmark = pytest.mark.gpu

RNG = np.random.default_rng(11)
HEADW_DT = [("x", "<u8"), ("dy", "<u8"), ("dw", "<u8"), ("db", "<u8"), ("npix", "<u8"), ("C", "<i4"), ("PL", "<i4"), ("chunk", "<i4"),
            ("blk0", "<i4"), ("xscale", "<u8"), ("xshift", "<u8"), ("xact", "<i4"), ("pad", "<i4")]
# dw_head / db_head: the bound tests/test_kernels_gpu.py::test_head1x1_wgrad_multi_matches_per_head_launches holds the same quantity to
# (fp32 partial sums per thread, per block and across blocks; relative to the largest element).  The longest chain here has 2 048 terms:
# eps_fp32 * sqrt(2048) = 2.7e-6 of a random-walk error against float64, inside the same bound.
HEAD_TOL = 1e-5

RIDER_SHAPES = [(1, 2, 4, 32, 2),        # one block (P = 8 pixels): sums2 bit for bit
                (2, 8, 8, 32, 2), (3, 6, 10, 64, 2), (2, 16, 16, 128, 4),
                (2, 32, 32, 128, 2)]     # many blocks


def _rider_inputs(B, H, W, C, HR):
    P = B * H * W
    x = dev(1.5 * RNG.standard_normal((P, C)), BF16)
    dy = dev(RNG.standard_normal((P, HR)))
    wh = dev(0.3 * RNG.standard_normal((C, HR)))
    dA = dev(RNG.standard_normal((P, C)), BF16)
    scale, shift = dev(1.0 + 0.3 * RNG.standard_normal(C)), dev(0.2 * RNG.standard_normal(C))
    mean, rstd = dev(0.1 * RNG.standard_normal(C)), dev(1.0 + 0.1 * RNG.random(C))
    gamma = dev(1.0 + 0.2 * RNG.standard_normal(C))
    return P, x, dy, wh, dA, scale, shift, mean, rstd, gamma


@pytest.mark.parametrize("form", ["head", "tensor"])
@pytest.mark.parametrize("shape", RIDER_SHAPES)
def test_norm_bwd_head_rider_equals_the_launches_it_replaces(L, shape, form):
    """reduce + apply with the rider against (a) the entry points without it on the same inputs -- sums2 within the fp32 summation order
    (bit for bit where one block covers the tensor), dx bit for bit given the same sums2 -- and (b) the head's filter / bias gradient
    against a float64 restatement on the device (a rounded to bf16 by the library's own phx_affine_act, products and sums in float64) and
    against phx_head1x1_wgrad_multi's xscale form, accumulating onto a non-zero (dw, db).  form "head": dA = dy_head w_head^T formed on the
    fly (HN > 0); "tensor": dA is a tensor of its own (HN = 0).  nrep 1 and 4, ReLU and identity."""
    B, H, W, C, HR = shape
    P, x, dy, wh, dA, scale, shift, mean, rstd, gamma = _rider_inputs(*shape)
    p = lambda t: t.data_ptr()
    for nrep in (1, 4):
        for act in (1, 0):
            # ---- the pair without the rider
            s2_ref = torch.zeros(nrep, C, 2, device="cuda")
            dx_ref, dg_ref, db_ref = torch.empty_like(x), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
            if form == "head":
                L.norm_bwd_reduce_head(p(dy), p(wh), HR, p(x), p(scale), p(shift), p(mean), p(rstd), p(s2_ref), 1, P, C, C, act, nrep, S())
                L.norm_bwd_apply_fused_head(p(dy), p(wh), HR, p(x), p(scale), p(shift), p(mean), p(rstd), p(gamma), p(s2_ref), p(dx_ref),
                                            p(dg_ref), p(db_ref), None, None, None, 1, P, C, C, act, nrep, S())
            else:
                L.norm_bwd_reduce(p(dA), BF16, p(x), BF16, p(scale), p(shift), p(mean), p(rstd), p(s2_ref), 1, P, C, C, act, nrep, S())
                L.norm_bwd_apply_fused(p(dA), BF16, p(x), BF16, p(scale), p(shift), p(mean), p(rstd), p(gamma), p(s2_ref), p(dx_ref), BF16,
                                       p(dg_ref), p(db_ref), 1, P, C, C, act, nrep, S())
            # ---- with the rider
            lead = (None if form == "head" else p(dA), p(dy), p(wh) if form == "head" else None, HR, p(x), p(scale), p(shift), p(mean), p(rstd))
            s2 = torch.zeros(nrep, C, 2, device="cuda")
            hacc = torch.zeros(nrep, C + 1, HR, device="cuda")
            dw, dbh = torch.full((C, HR), 0.5, device="cuda"), torch.full((HR,), -1.0, device="cuda")
            dx, dg, db = torch.empty_like(x), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
            L.norm_bwd_reduce_rider(*lead, p(s2), p(hacc), P, C, act, nrep, S())
            # (the apply launch on the REFERENCE sums: dx then has to be the same bits)
            L.norm_bwd_apply_fused_rider(*lead, p(gamma), p(s2_ref), p(dx), p(dg), p(db), p(hacc), p(dw), p(dbh), P, C, act, nrep, S())
            torch.cuda.synchronize()
            what = "%s nrep %d act %d %s" % (shape, nrep, act, form)
            if P <= 256 // (C // 8):
                assert torch.equal(s2, s2_ref), "sums2 (one block) " + what
            close(host(s2.sum(0)), host(s2_ref.sum(0)), 1e-5, "sums2 " + what)
            assert torch.equal(dx.view(torch.int16), dx_ref.view(torch.int16)), "dx " + what
            assert torch.equal(dg, dg_ref) and torch.equal(db, db_ref), "dgamma / dbeta " + what
            # ---- the head's gradients: float64 restatement
            a = torch.empty_like(x)
            L.affine_act(p(x), BF16, p(scale), p(shift), p(a), BF16, 1, P, C, act, S())
            torch.cuda.synchronize()
            dw64 = 0.5 + a.double().t() @ dy.double()
            db64 = -1.0 + dy.double().sum(0)
            print("%s: dw_head err %.2e, db_head err %.2e (rel. to max)" % (
                what, float((dw.double() - dw64).abs().max() / dw64.abs().max()), float((dbh.double() - db64).abs().max() / db64.abs().max())))
            close(host(dw), dw64.cpu().numpy(), HEAD_TOL, "dw_head vs float64 " + what)
            close(host(dbh), db64.cpu().numpy(), HEAD_TOL, "db_head vs float64 " + what)
            # ---- ... and the job of phx_head1x1_wgrad_multi they replace (x = the pre-normalisation tensor, xscale form)
            dw_m, db_m = torch.full((C, HR), 0.5, device="cuda"), torch.full((HR,), -1.0, device="cuda")
            plan = (ctypes.c_int * 4)()
            L.head1x1_wgrad_plan(P, C, HR, plan)
            rec = np.zeros(1, dtype=HEADW_DT)
            rec[0] = (p(x), p(dy), p(dw_m), p(db_m), P, C, plan[0], plan[1], 0, p(scale), p(shift), act, 0)
            desc = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
            L.head1x1_wgrad_multi(p(desc), 1, plan[2], BF16, HR, plan[3], S())
            close(host(dw), host(dw_m), HEAD_TOL, "dw_head vs head1x1_wgrad_multi " + what)
            close(host(dbh), host(db_m), HEAD_TOL, "db_head vs head1x1_wgrad_multi " + what)


def test_norm_bwd_head_rider_refuses_a_channel_count_outside_its_domain(L):
    """C = 192: C / 8 = 24 is no power of two -- both entry points return the invalid-argument status (-1) and launch nothing."""
    from phiseg_code_amd import runtime as rt
    P, x, dy, wh, dA, scale, shift, mean, rstd, gamma = _rider_inputs(2, 32, 32, 192, 2)
    p = lambda t: t.data_ptr()
    s2, hacc = torch.zeros(1, 192, 2, device="cuda"), torch.zeros(1, 193, 2, device="cuda")
    dw, dbh, dx = torch.zeros(192, 2, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros_like(x)
    dg, db = torch.zeros(192, device="cuda"), torch.zeros(192, device="cuda")
    for dA_p, wh_p in ((p(dA), None), (None, p(wh))):
        lead = (dA_p, p(dy), wh_p, 2, p(x), p(scale), p(shift), p(mean), p(rstd))
        with pytest.raises(rt.PhxError, match=r"\(-1\)"):
            L.norm_bwd_reduce_rider(*lead, p(s2), p(hacc), P, 192, 1, 1, S())
        with pytest.raises(rt.PhxError, match=r"\(-1\)"):
            L.norm_bwd_apply_fused_rider(*lead, p(gamma), p(s2), p(dx), p(dg), p(db), p(hacc), p(dw), p(dbh), P, 192, 1, 1, S())
    torch.cuda.synchronize()
    assert float(hacc.abs().max()) == 0.0 and float(dw.abs().max()) == 0.0 and float(dx.float().abs().max()) == 0.0


UNPAD_DT = [("dw_pad", "<u8"), ("dw", "<u8"), ("cin", "<i4"), ("cin_pad", "<i4"), ("cout", "<i4"), ("ntap", "<i4"), ("blk0", "<i4"),
            ("reserved", "<i4")]


@pytest.mark.parametrize("grids", ["per_element", [1, 3, 2, 5], [7, 1, 4, 1]])
def test_unpad_filter_grad_multi_equals_the_per_layer_launches(L, grids):
    """One phx_unpad_filter_grad_multi launch == phx_unpad_filter_grad_accumulate / _center per layer, bit for bit, onto a non-zero dw;
    job grids of one thread per element (what the plan emits) and grids that are no multiples of each other (a job strides over its
    elements with the blocks it has)."""
    assert np.dtype(UNPAD_DT).itemsize == 40
    jobs = [(1, 32, 32, 9), (3, 32, 32, 9), (2, 32, 64, 9), (2, 32, 192, 1)]
    rec, keep, blk = np.zeros(len(jobs), dtype=UNPAD_DT), [], 0
    for i, (cin, cpad, cout, ntap) in enumerate(jobs):
        dwp = dev(RNG.standard_normal((9, cpad, cout)))
        start = dev(RNG.standard_normal((ntap, cin, cout)))
        ref, got = start.clone(), start.clone()
        (L.unpad_filter_grad_center if ntap == 1 else L.unpad_filter_grad_accumulate)(dwp.data_ptr(), ref.data_ptr(), cin, cpad, cout, S())
        rec[i] = (dwp.data_ptr(), got.data_ptr(), cin, cpad, cout, ntap, blk, 0)
        blk += (ntap * cin * cout + 255) // 256 if grids == "per_element" else grids[i]
        keep.append((dwp, start, ref, got))
    desc = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    L.unpad_filter_grad_multi(desc.data_ptr(), len(jobs), blk, S())
    torch.cuda.synchronize()
    for (cin, cpad, cout, ntap), (dwp, start, ref, got) in zip(jobs, keep):
        want = start + (dwp[4:5] if ntap == 1 else dwp)[:, :cin, :]
        assert torch.equal(ref, want), "per-layer launch %s" % ((cin, cpad, cout, ntap),)
        assert torch.equal(got, ref), "multi launch %s" % ((cin, cpad, cout, ntap),)


def test_unpad_filter_grad_multi_refuses_an_empty_job_list(L):
    from phiseg_code_amd import runtime as rt
    with pytest.raises(rt.PhxError, match=r"\(-1\)"):
        L.unpad_filter_grad_multi(None, 0, 0, S())


# ---- in the plan ----------------------------------------------------------------------------------------------------------------
def _plan_arm(monkeypatch, rider):
    from tests.test_model_gpu import _lidc_setup
    monkeypatch.setenv("PHX_ONEPASS", "0")       # batch 2: the reduce + apply pair (and with it the rider) on every generic layer
    monkeypatch.setenv("PHX_HEAD_RIDER", rider)
    cfg, model, params, x_np, s_np = _lidc_setup("bf16", perturbed=True)      # fixture lidc_phiseg_bn, batch 2
    plan = model.sess.plan_for([model.loss_tot], True, cfg["B"], True)
    plan.set_input("x_input", x_np)
    plan.set_input("s_input", s_np)
    model.sess.store.set_lr(0.0)
    plan.run()
    plan.sync()
    launches = [(getattr(fn, "__name__", ""), args) for fn, args in plan.launches]
    return float(plan.fetch(model.loss_tot)), model.sess.store.export(grads=True), launches


def test_training_plan_with_head_riders_and_one_fold_launch_equals_the_plan_without(monkeypatch):
    """phiseg_7_5 (n0 = 32, 128 x 128, batch 2, bf16, batch norm), PHX_HEAD_RIDER=1 against 0, PHX_ONEPASS=0 in both: the rider launches
    are in the plan, phx_head1x1_wgrad_multi carries fewer jobs, the deferred padded-filter folds are ONE launch; loss and gradients
    within the bounds tests/test_plan_variants_gpu.py holds same-arithmetic rewrites of the batch-norm plan to (loss 2e-2, mean relative
    gradient distance 0.5), and every likelihood head's filter and bias within that file's per-variable bound for a re-ordered sum (0.1)."""
    l0, g0, n0 = _plan_arm(monkeypatch, "0")
    l1, g1, n1 = _plan_arm(monkeypatch, "1")
    cnt = lambda ls, name: sum(n == name for n, _ in ls)
    hjobs = lambda ls: sum(a[1] for n, a in ls if n == "phx_head1x1_wgrad_multi")
    assert cnt(n0, "phx_norm_bwd_reduce_rider") == 0 and cnt(n0, "phx_norm_bwd_apply_fused_rider") == 0
    assert cnt(n1, "phx_norm_bwd_reduce_rider") >= 1 and cnt(n1, "phx_norm_bwd_apply_fused_rider") == cnt(n1, "phx_norm_bwd_reduce_rider")
    assert hjobs(n1) == hjobs(n0) - cnt(n1, "phx_norm_bwd_reduce_rider"), (hjobs(n0), hjobs(n1))
    for ls in (n0, n1):
        assert cnt(ls, "phx_unpad_filter_grad_multi") == 1
        assert [a[1] for n, a in ls if n == "phx_unpad_filter_grad_multi"][0] >= 2
    assert abs(l1 - l0) <= 2e-2 * abs(l0), (l0, l1)
    errs, heads = [], []
    for name, ga in g0.items():
        nrm = np.linalg.norm(ga)
        if nrm < 1e-8 * max(1.0, np.sqrt(ga.size)):
            continue
        e = np.linalg.norm(g1[name] - ga) / nrm
        errs.append(e)
        if "likelihood/y_lvl" in name:
            heads.append((name, e))
    print("head riders on / off: loss %.6g / %.6g, mean relative gradient distance %.4f over %d variables; heads %s" % (
        l1, l0, np.mean(errs), len(errs), ", ".join("%s %.2e" % h for h in heads)))
    assert len(errs) >= 360 and np.mean(errs) <= 0.5, (len(errs), np.mean(errs))
    assert len(heads) == 10, heads
    for name, e in heads:
        assert e <= 0.1, (name, e)
