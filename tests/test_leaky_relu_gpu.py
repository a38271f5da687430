"""leaky_relu end to end on the GPU.

Kernels, through the C ABI (phx_leaky_relu_fwd / _bwd, csrc/leaky_relu.hip): every dtype pair, sizes around the vector width V and the
grid cap, special values, guard rows around every output, in place, pointers off a 16-byte boundary, the refusals.  EQUALITY IS
BITWISE: the forward is one correctly rounded fp32 multiply and a selection, then one round-to-nearest-even to the storage type; the
backward one multiply by alpha or none -- numpy's float32 arithmetic and torch's .to(torch.bfloat16) do the same, no tolerance is needed.

Engine: the two toy nets of tests/leaky_net.py -- every layer function with leaky_relu and / or normalise_post_activation -- as fp32
training and inference plans against float64 autograd (bounds of tests/test_extra_layers_gpu.py), the bf16 plan against the fp32 plan,
and a worker process for hipGraph capture under PHX_DETERMINISTIC=1."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from phiseg_code_amd import runtime as rt
from tests import leaky_net as N
from tests import leaky_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
TDT = {F32: torch.float32, BF16: torch.bfloat16}
IDT = {F32: torch.int32, BF16: torch.int16}
ESIZE = {F32: 4, BF16: 2}
ALPHAS = (0.01, 0.2)
GUARD = 64                      # elements of guard row before and after every buffer (a multiple of 16 bytes in both types)
SENTINEL = 96.0                 # exact in bf16
# csrc/leaky_relu.hip as written: LR_MAX_BLOCKS = 2048 blocks of LR_BLOCK = 256 threads, one item of V elements per thread and trip
GRID_CAP, BLOCK = 2048, 256
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, 2.0 ** -126, -2.0 ** -126, 2.0 ** -130, -2.0 ** -130, 1e30, -1e30], dtype=np.float32)
#                   +-0, +-inf, the smallest normal, a denormal (one of bf16 too), +-1e30


def _header_constants():
    src = re.sub(r"/\*.*?\*/", "", open(rt.HEADER).read(), flags=re.S)
    return {k: int(v) for k, v in re.findall(r"\b(PHX_[A-Z0-9_]+)\s*=\s*(-?\d+)", src)}


H = _header_constants()
assert (H["PHX_F32"], H["PHX_BF16"]) == (F32, BF16)


@pytest.fixture(scope="module")
def L():
    return rt.lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def vec(*dts):
    """V of the kernel as written: 4 elements per item when every tensor is fp32, 8 as soon as one is bf16"""
    return 8 if BF16 in dts else 4


def sizes(*dts):
    V = vec(*dts)
    # ... the last one: GRID_CAP * BLOCK items fill one trip of the capped grid, five more take the grid-stride loop's second trip,
    # and three elements are left for the scalar tail
    return [1, V - 1, V, V + 1, 255 * V + 3, (GRID_CAP * BLOCK + 5) * V + 3]


def data(n, dt, seed, special_at=0):
    """random fp32 data with the special values at known positions (at the start -- wrapped for tiny n -- and, for n >= 64, in the
    scalar tail at the end), rounded to the storage type -> (device tensor in that type, its values as float32 numpy)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(np.float32)
    k = min(n, SPECIAL.size)
    a[:k] = np.roll(SPECIAL, -special_at)[:k]
    if n >= 64:
        a[n - SPECIAL.size:] = SPECIAL[::-1]
    t = torch.from_numpy(a).to(TDT[dt])
    return t.cuda(), t.float().numpy()


class Guarded:
    """n elements between two guard rows, everything SENTINEL; `off` more elements shift the payload off the 16-byte boundary"""

    def __init__(self, n, dt, off=0, init=None):
        self.n, self.dt, self.lo = n, dt, GUARD + off
        self.t = torch.full((self.lo + n + GUARD,), SENTINEL, dtype=TDT[dt], device="cuda")
        if init is not None:
            self.t[self.lo:self.lo + n] = init
        self.ptr = self.t.data_ptr() + self.lo * ESIZE[dt]
        assert self.t.data_ptr() % 16 == 0 and self.ptr % 16 == (off * ESIZE[dt]) % 16

    def payload(self):
        return self.t[self.lo:self.lo + self.n]

    def check_guards(self, what):
        torch.cuda.synchronize()
        s = torch.tensor(SENTINEL, dtype=TDT[self.dt]).view(IDT[self.dt]).item()
        bits = self.t.view(IDT[self.dt])
        assert bool((bits[:self.lo] == s).all()) and bool((bits[self.lo + self.n:] == s).all()), "%s: a guard row changed" % what


def bits_equal(got, ref, dt, what):
    """got: device tensor of type dt; ref: float32 numpy, rounded to dt the way torch rounds"""
    want = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32)).to(TDT[dt]).view(IDT[dt])
    have = got.detach().cpu().contiguous().view(IDT[dt])
    bad = torch.nonzero(want != have).flatten()
    assert bad.numel() == 0, "%s: %d of %d elements differ in their bits, first at %d" % (what, bad.numel(), want.numel(), int(bad[0]))


def refused(fn, *args):
    with pytest.raises(rt.PhxError, match=r"\(%d\)" % H["PHX_E_INVAL"]):
        fn(*args)


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y_dt", [F32, BF16])
@pytest.mark.parametrize("x_dt", [F32, BF16])
def test_forward_bitwise_every_dtype_pair(L, x_dt, y_dt):
    for alpha in ALPHAS:
        for n in sizes(x_dt, y_dt):
            x, x32 = data(n, x_dt, 1000 + n % 97)
            keep = x.clone()
            y = Guarded(n, y_dt)
            L.leaky_relu_fwd(x.data_ptr(), x_dt, y.ptr, y_dt, n, alpha, S())
            y.check_guards("fwd n=%d" % n)
            what = "fwd x=%d y=%d alpha=%g n=%d" % (x_dt, y_dt, alpha, n)
            bits_equal(y.payload(), leaky_ref.forward_f32(x32, alpha), y_dt, what)
            assert torch.equal(x.view(IDT[x_dt]), keep.view(IDT[x_dt])), what + ": the input changed"
            if x_dt == y_dt:                               # in place: the same bits
                z = Guarded(n, x_dt, init=x)
                L.leaky_relu_fwd(z.ptr, x_dt, z.ptr, x_dt, n, alpha, S())
                z.check_guards("fwd in place n=%d" % n)
                assert torch.equal(z.payload().view(IDT[x_dt]), y.payload().view(IDT[x_dt])), what + ": in place differs"


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y_dt", [F32, BF16])
@pytest.mark.parametrize("d_dt", [F32, BF16])
def test_backward_bitwise_every_dtype_pair(L, d_dt, y_dt):
    for alpha in ALPHAS:
        for n in sizes(d_dt, y_dt):
            y, y32 = data(n, y_dt, 2000 + n % 97)          # the stored OUTPUT: +-0 pass the whole gradient, -inf / -1e30 scale it
            dy, dy32 = data(n, d_dt, 3000 + n % 97, special_at=3)
            keep_y, keep_dy = y.clone(), dy.clone()
            dx = Guarded(n, d_dt)
            L.leaky_relu_bwd(dy.data_ptr(), d_dt, y.data_ptr(), y_dt, dx.ptr, d_dt, n, alpha, S())
            dx.check_guards("bwd n=%d" % n)
            what = "bwd dy=%d y=%d alpha=%g n=%d" % (d_dt, y_dt, alpha, n)
            bits_equal(dx.payload(), leaky_ref.backward_f32(dy32, y32, alpha), d_dt, what)
            assert torch.equal(y.view(IDT[y_dt]), keep_y.view(IDT[y_dt])) and torch.equal(dy.view(IDT[d_dt]), keep_dy.view(IDT[d_dt])), what
            z = Guarded(n, d_dt, init=dy)                  # in place: dpre == dy
            L.leaky_relu_bwd(z.ptr, d_dt, y.data_ptr(), y_dt, z.ptr, d_dt, n, alpha, S())
            z.check_guards("bwd in place n=%d" % n)
            assert torch.equal(z.payload().view(IDT[d_dt]), dx.payload().view(IDT[d_dt])), what + ": in place differs"


def test_the_tie_passes_the_whole_gradient(L):
    y = torch.tensor([0.0, -0.0, 1.0, -1.0], device="cuda")
    dy = torch.tensor([3.0, 5.0, 7.0, 11.0], device="cuda")
    dx = torch.zeros(4, device="cuda")
    L.leaky_relu_bwd(dy.data_ptr(), F32, y.data_ptr(), F32, dx.data_ptr(), F32, 4, 0.25, S())
    torch.cuda.synchronize()
    assert dx.tolist() == [3.0, 5.0, 7.0, 2.75]            # 1 at +-0: not alpha, not (1 + alpha) / 2


# ---- pointers off a 16-byte boundary: include/phx.h promises the right bits, not a refusal -----------------------------------------
@pytest.mark.parametrize("case", [(F32, F32, 1, 1), (BF16, BF16, 1, 1), (F32, BF16, 1, 1), (BF16, F32, 1, 0), (F32, F32, 0, 3), (BF16, BF16, 5, 2)])
def test_pointers_one_element_off_a_16_byte_boundary(L, case):
    """both tensors one element off (one scalar head aligns them), and offsets no common head aligns (every element on its own)"""
    a_dt, b_dt, off_a, off_b = case
    alpha = 0.2
    for n in (1, vec(a_dt, b_dt) + 1, 255 * vec(a_dt, b_dt) + 3):
        src, src32 = data(n, a_dt, 4000 + n % 97)
        x = Guarded(n, a_dt, off=off_a, init=src)
        y = Guarded(n, b_dt, off=off_b)
        L.leaky_relu_fwd(x.ptr, a_dt, y.ptr, b_dt, n, alpha, S())
        y.check_guards("fwd")
        x.check_guards("fwd input")
        y_ref = leaky_ref.forward_f32(src32, alpha)
        bits_equal(y.payload(), y_ref, b_dt, "misaligned fwd %s n=%d" % (case, n))
        assert torch.equal(x.payload().view(IDT[a_dt]), src.view(IDT[a_dt]))
        # backward: dy / dpre in a_dt at off_a, the stored output in b_dt at off_b
        dy, dy32 = data(n, a_dt, 5000 + n % 97, special_at=5)
        d_in = Guarded(n, a_dt, off=off_a, init=dy)
        d_out = Guarded(n, a_dt, off=off_a)
        y32 = y.payload().float().cpu().numpy()
        L.leaky_relu_bwd(d_in.ptr, a_dt, y.ptr, b_dt, d_out.ptr, a_dt, n, alpha, S())
        d_out.check_guards("bwd")
        d_in.check_guards("bwd input")
        bits_equal(d_out.payload(), leaky_ref.backward_f32(dy32, y32, alpha), a_dt, "misaligned bwd %s n=%d" % (case, n))


# ---- the contract's edges ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_call(L):
    n = 40
    x, _ = data(n, F32, 7)
    y = Guarded(n, F32)
    d = Guarded(n, F32)
    for alpha in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        refused(L.leaky_relu_fwd, x.data_ptr(), F32, y.ptr, F32, n, alpha, S())
        refused(L.leaky_relu_bwd, x.data_ptr(), F32, x.data_ptr(), F32, d.ptr, F32, n, alpha, S())
    for bad in (2, -1, 7):
        refused(L.leaky_relu_fwd, x.data_ptr(), bad, y.ptr, F32, n, 0.1, S())
        refused(L.leaky_relu_fwd, x.data_ptr(), F32, y.ptr, bad, n, 0.1, S())
        refused(L.leaky_relu_bwd, x.data_ptr(), F32, x.data_ptr(), bad, d.ptr, F32, n, 0.1, S())
        refused(L.leaky_relu_bwd, x.data_ptr(), bad, x.data_ptr(), F32, d.ptr, bad, n, 0.1, S())
    refused(L.leaky_relu_bwd, x.data_ptr(), F32, x.data_ptr(), F32, d.ptr, BF16, n, 0.1, S())      # dy_dt != dpre_dt, as phx_act_bwd
    refused(L.leaky_relu_bwd, x.data_ptr(), BF16, x.data_ptr(), F32, d.ptr, F32, n, 0.1, S())
    refused(L.leaky_relu_fwd, None, F32, y.ptr, F32, n, 0.1, S())                                   # a null tensor with n > 0
    refused(L.leaky_relu_fwd, x.data_ptr() + 2, F32, y.ptr, F32, n - 1, 0.1, S())                   # not even aligned to its element
    # n == 0: what phx_act_bwd does today -- PHX_OK, nothing touched
    L.act_bwd(x.data_ptr(), F32, x.data_ptr(), F32, d.ptr, F32, 0, H["PHX_ACT_RELU"], S())
    L.leaky_relu_fwd(x.data_ptr(), F32, y.ptr, F32, 0, 0.1, S())
    L.leaky_relu_bwd(x.data_ptr(), F32, x.data_ptr(), F32, d.ptr, F32, 0, 0.1, S())
    for g in (y, d):                                        # nothing was launched by a refusal, nothing written by an empty call
        g.check_guards("refusals")
        assert bool((g.payload() == SENTINEL).all())


# ---- through the engine ----------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _trained(net):
    """the fp32 training plan (optimize=False, no hipGraph) of a toy net and the float64 oracle on the same values, computed once and
    shared by the tests"""
    if net not in _CACHE:
        g, t = N.build(net)
        vals = N.values(g)
        x, lab = N.inputs(g, t)
        loss, logits, grads, _ = N.run_plan(g, t, vals, x, lab)
        _CACHE[net] = dict(g=g, t=t, vals=vals, x=x, lab=lab, got=(loss, logits, grads), ref=N.oracle(g, vals, x, lab, net))
    return _CACHE[net]


def _check_against(got, ref, min_checked, logits_tol=3e-4, loss_rtol=3e-5, grad_tol=3e-3):
    """the bounds of tests/test_extra_layers_gpu.py::test_extra_layers_in_a_graph"""
    loss, logits, grads = got
    print("logits err / max %.3e, loss rel %.3e" % (np.abs(logits - ref["logits"]).max() / np.abs(ref["logits"]).max(),
                                                     abs(loss - ref["loss"]) / abs(ref["loss"])))
    np.testing.assert_allclose(logits, ref["logits"], rtol=0, atol=logits_tol * float(np.abs(ref["logits"]).max()))
    np.testing.assert_allclose(loss, ref["loss"], rtol=loss_rtol)
    checked = 0
    for n, r in ref["grads"].items():
        if np.abs(r).max() < 1e-9:                          # a bias in front of batch norm
            assert np.abs(grads[n]).max() < 1e-4, n
            continue
        print("%s err / max %.3e" % (n, np.abs(grads[n] - r).max() / np.abs(r).max()))
        np.testing.assert_allclose(grads[n], r, rtol=0, atol=grad_tol * max(np.abs(r).max(), 1e-6), err_msg=n)
        checked += 1
    assert checked >= min_checked, checked


def test_fp32_training_plan_matches_autograd():
    tr = _trained("2d")
    names = set(tr["g"].variables)
    assert "net/c1/b" not in names and {"net/dil/b", "net/up/b", "net/r/projection/W", "net/i/bn_projection/BatchNorm/gamma", "net/fc/W"} <= names
    kinds = [op.type for op in tr["g"].ops]
    assert kinds.count("leaky_relu") == 9 and kinds.count("dropout") == 1
    _check_against(tr["got"], tr["ref"], min_checked=12)


def test_inference_plan_and_the_node_as_a_fetch():
    """dropout is the identity, batch norm reads the moving pair; a leaky_relu node's output is fetched beside its producer's"""
    tr = _trained("2d")
    g, t = tr["g"], tr["t"]
    c1 = t["c1"]
    assert c1.op.type == "leaky_relu"
    _, logits, _, (a, pre) = N.run_plan(g, t, tr["vals"], tr["x"], tr["lab"], training=False, fetch=[c1, c1.op.inputs[0]])
    ref = N.oracle(g, tr["vals"], tr["x"], tr["lab"], "2d", training=False)
    print("inference logits err / max %.3e" % (np.abs(logits - ref["logits"]).max() / np.abs(ref["logits"]).max()))
    np.testing.assert_allclose(logits, ref["logits"], rtol=0, atol=3e-4 * float(np.abs(ref["logits"]).max()))
    assert np.array_equal(a, leaky_ref.forward_f32(pre, 0.01)) and (pre < 0).any()      # out of place: the producer's output is intact


def test_volume_net_with_global_averagepool3d():
    tr = _trained("3d")
    assert tr["t"]["pooled"].shape == (None, 6)
    _check_against(tr["got"], tr["ref"], min_checked=5)      # (W, gamma, beta, head W, head b; the bias in front of batch norm has none)
    _, logits, _, (pooled, c) = N.run_plan(tr["g"], tr["t"], tr["vals"], tr["x"], tr["lab"], training=False, fetch=[tr["t"]["pooled"], tr["t"]["c"]])
    np.testing.assert_allclose(pooled, c.astype(np.float64).mean(axis=(1, 2, 3)), rtol=1e-5, atol=1e-6)
    ref = N.oracle(tr["g"], tr["vals"], tr["x"], tr["lab"], "3d", training=False)
    np.testing.assert_allclose(logits, ref["logits"], rtol=0, atol=3e-4 * float(np.abs(ref["logits"]).max()))


def test_bf16_plan_against_the_fp32_plan():
    """Every fetch finite, and the bf16 plan agrees with the fp32 plan within the band of
    tests/test_volume_graph_gpu.py::test_bf16_plan_within_the_storage_policy_band (its lines 121 and 136: `e <= 2 * d`): d is the
    float64 oracle's own sensitivity to the storage policy -- the oracle with every stored tensor rounded to bf16 against the exact one,
    max abs over the logits, per gradient tensor over its max -- and the factor is that file's 2.  A gradient that is zero in exact
    arithmetic (a bias in front of batch norm) has no scale: |db| <= 2 * 2^-9 sum |dy|, that file's line 127."""
    tr = _trained("2d")
    g, t, vals, x, lab = (tr[k] for k in ("g", "t", "vals", "x", "lab"))
    fetch = [t[k] for k in ("c1", "c2", "dil", "up", "r", "i", "fc")]
    loss, logits, grads, extra = N.run_plan(g, t, vals, x, lab, compute_dtype="bf16", fetch=fetch)
    assert np.isfinite(loss) and np.isfinite(logits).all() and all(np.isfinite(a).all() for a in extra)
    assert all(np.isfinite(v).all() for v in grads.values())
    f_loss, f_logits, f_grads = tr["got"]
    exact, rnd = tr["ref"], N.oracle(g, vals, x, lab, "2d", stored=N.bf16_round)
    d_logits = float(np.abs(rnd["logits"] - exact["logits"]).max())
    e_logits = float(np.abs(logits - f_logits).max())
    print("bf16 logits: oracle distance %.3e, bf16 plan - fp32 plan %.3e" % (d_logits, e_logits))
    fails = []
    if not e_logits <= 2 * d_logits:
        fails.append(("logits", e_logits, d_logits))
    for n, r in exact["grads"].items():
        if np.abs(r).max() < 1e-9:
            bound = 2 * 2.0 ** -9 * rnd["dy_abs"][n]
            print("bf16 %s: structurally zero, |db| max %.3e, bound %.3e" % (n, np.abs(grads[n]).max(), bound.min()))
            if not (np.abs(grads[n]) <= bound).all():
                fails.append((n, float(np.abs(grads[n]).max()), float(bound.min())))
            continue
        scale = max(float(np.abs(r).max()), 1e-12)
        d = float(np.abs(rnd["grads"][n] - r).max()) / scale
        e = float(np.abs(grads[n] - f_grads[n]).max()) / scale
        print("bf16 %s: oracle distance %.3e, bf16 plan - fp32 plan %.3e" % (n, d, e))
        if not e <= 2 * d:
            fails.append((n, e, d))
    assert not fails, fails


def test_hip_graph_and_deterministic_mode():
    """use_hip_graph=True with PHX_DETERMINISTIC=1 (read once per process: a worker): the plan's eager first run, the capture's first
    launch, a replay and a plan that is never captured give bit-identical loss, logits and gradients."""
    env = dict(os.environ, PYTHONPATH=ROOT, PHX_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "leaky_graph_worker.py")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    row = json.loads(r.stdout.strip().splitlines()[-1])
    assert row["deterministic"] is True and row["captured"] is True, row
    assert row["repeat_equal"] and row["eager_equal"], row
    assert row["ngrads"] >= 12 and np.isfinite(row["loss"]) and row["leaky_launches"] == 18, row
