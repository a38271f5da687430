"""Launch-list dump: build the plan of a named case (no kernel runs) and print `launches` / `opt_launches` with every argument
normalised, the allocation sequence and the uploaded job tables -- two engines that lower a case identically print identical text.
    python tools/dump_launches.py CASE [> file]        (PHX_* switches come from the environment: one process per setting)
Uses only Plan.launches / opt_launches / tags / _keep / _lanes, the ParamStore arenas and fn.__name__."""
import bisect
import ctypes
import os
import sys

import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (behind PYTHONPATH: another engine tree may be put in front)
from phiseg_code_amd import engine, graph as G, optimizers  # noqa: E402
from phiseg_code_amd.phiseg import phiseg_model  # noqa: E402
from phiseg_code_amd.tfwrapper import activations as act, layers, normalisation as tfnorm  # noqa: E402
from tests.helpers import load_golden  # noqa: E402
from tests.test_graph_cpu import make_config  # noqa: E402


def model_plan(golden, dt, B=None, norm=None, what="train", momentum=False, norm_fn=None):
    _, cfg, _ = load_golden(golden)
    cfg = dict(cfg, B=B or cfg["B"], **({"norm": norm} if norm else {}))
    c = make_config(cfg, dt)
    if norm_fn is not None:             # a normaliser the fixtures' config table does not name
        c.layer_norm = norm_fn
    if momentum:
        c.optimizer = optimizers.MomentumOptimizer
    m = phiseg_model.phiseg(c, rng_seed=cfg["eps_seed"])
    if what == "train":                 # sess.run([train_step, loss_tot], training)
        return m.sess.plan_for([m.loss_tot], True, cfg["B"], True)
    if what == "sample":                # four samples per image in one pass
        return m.sess.plan_for([m.sampling_graph(4)[1]], False, cfg["B"], False)
    return m.sess.plan_for([m.s_out_eval_sm], False, cfg["B"], False)


def layer_plan(kind, norm):
    """The graphs of tests/test_extra_layers_gpu.py (general units, stand-alone norm_act, residual units) plus a transposed unit."""
    g = G.reset_default_graph()
    nfn = getattr(tfnorm, norm)
    if kind == "extra":
        B, x_inp, s_inp = 3, G.placeholder(G.KIND_F32, [None, 12, 12, 3], name="x_input"), G.placeholder(G.KIND_U8, [None, 6, 6], name="s_input")
        with g.variable_scope("net"):
            a = layers.conv2D(x_inp, "c1", num_filters=8, kernel_size=(5, 5), strides=(2, 2), normalisation=nfn, training=True)
            d = layers.dilated_conv2D(x_inp, "dil", num_filters=4, rate=2, normalisation=nfn, training=True)
            cat = layers.crop_and_concat([a, layers.pad_to_size(layers.maxpool2D(d), [None, 9, 8, 4])])
            dr = layers.dropout(cat, keep_prob=0.8, training=True)
            fc = layers.dense_layer(dr, "fc", hidden_units=5, normalisation=nfn, training=True)
            gate = layers.conv2D(G.tile_pixels(G.global_average_pool(fc), 6, 6), "mix", num_filters=12, kernel_size=(1, 1),
                                 normalisation=tfnorm.identity, training=True)
            up = layers.transposed_conv2D(gate, "up", num_filters=12, normalisation=nfn, training=True)     # (not in the test: the transposed unit)
            s = layers.conv2D(G.concat([dr, layers.maxpool2D(up)], axis=-1), "head", num_filters=2, kernel_size=(1, 1), activation=act.identity)
    else:
        B, x_inp, s_inp = 2, G.placeholder(G.KIND_F32, [None, 8, 8, 4], name="x_input"), G.placeholder(G.KIND_U8, [None, 2, 2], name="s_input")
        kw = dict(normalisation=nfn, training=True, num_groups=2)
        with g.variable_scope("net"):
            r = layers.residual_unit2D(x_inp, "r1", num_filters=4, **kw)
            r = layers.residual_unit2D(r, "r2", num_filters=8, down_sample=True, **kw)
            r = layers.residual_unit2D(r, "r3", num_filters=6, projection=True, **kw)
            r = layers.identity_residual_unit2D(r, "i1", num_filters=6, **kw)
            r = layers.identity_residual_unit2D(r, "i2", num_filters=12, down_sample=True, projection=False, **kw)
            r = layers.identity_residual_unit2D(r, "i3", num_filters=8, projection=True, **kw)
            s = layers.conv2D(r, "head", num_filters=2, kernel_size=(1, 1), activation=act.identity)
    loss = G.weighted_sum([G.residual_multinoulli([s], s_inp, 1.0)[0][0]], [1.0])
    return engine.Plan(engine.ParamStore(g, seed=3), [loss, s], loss=loss, batch=B, training=True, compute_dtype="f32", optimize=False,
                       use_hip_graph=False)


CASES = {"lidc_bf16_b2": lambda: model_plan("lidc_phiseg_bn", "bf16", 2), "lidc_bf16_b24": lambda: model_plan("lidc_phiseg_bn", "bf16", 24),
         "lidc_bf16_b64": lambda: model_plan("lidc_phiseg_bn", "bf16", 64), "lidc_bf16_gn": lambda: model_plan("lidc_phiseg_bn", "bf16", 2, "group_norm"),
         "lidc_bf16_in": lambda: model_plan("lidc_phiseg_bn", "bf16", 2, "instance_norm"), "lidc_f32": lambda: model_plan("lidc_phiseg_bn", "f32"),
         "tiny_f32": lambda: model_plan("tiny_phiseg_bn", "f32"), "lidc_f32_infer": lambda: model_plan("lidc_phiseg_bn", "f32", what="infer"), "lidc_bf16_infer": lambda: model_plan("lidc_phiseg_bn", "bf16", 2, what="infer"),
         "lidc_bf16_sample": lambda: model_plan("lidc_phiseg_bn", "bf16", 2, what="sample"), "probunet_bf16": lambda: model_plan("tiny_probunet_bn", "bf16"),
         "detunet_bf16": lambda: model_plan("tiny_detunet_bn", "bf16"), "lidc_bf16_momentum": lambda: model_plan("lidc_phiseg_bn", "bf16", 2, momentum=True),
         "tiny_f32_momentum": lambda: model_plan("tiny_phiseg_bn", "f32", momentum=True),
         "lidc_bf16_ln": lambda: model_plan("lidc_phiseg_bn", "bf16", 2, norm_fn=tfnorm.layer_norm),
         "lidc_f32_ln": lambda: model_plan("lidc_phiseg_bn", "f32", norm_fn=tfnorm.layer_norm)}
for _n in ("identity", "batch_norm", "group_norm2D", "layer_norm"):
    CASES["extra_" + _n] = lambda n=_n: layer_plan("extra", n)
    CASES["residual_" + _n] = lambda n=_n: layer_plan("residual", n)


def span(o):
    """(address, bytes) of a kept allocation: Buf, torch tensor or ctypes array."""
    t = o.t if hasattr(o, "dt") else o
    return (t.data_ptr(), t.numel() * t.element_size()) if torch.is_tensor(t) else (ctypes.addressof(o), ctypes.sizeof(o))


def dump(plan, out=sys.stdout):
    owners = [(v.data_ptr(), v.numel() * v.element_size(), k) for k, v in sorted(vars(plan.store).items()) if torch.is_tensor(v)]
    owners.append((plan.launches[0][1][0], 32 << 20, "zero"))
    for i, o in enumerate(plan._keep):          # views (zero-arena accumulators, slices of a kept buffer) keep their owner's label
        a, n = span(o)
        if not any(b <= a < b + m for b, m, _ in owners):
            owners.append((a, max(n, 1), i))
    owners.sort(key=lambda r: r[0])
    starts = [r[0] for r in owners]
    lanes, events = [ln.value for ln in plan._lanes], {}

    def addr(v):
        j = bisect.bisect_right(starts, v) - 1
        return "%s+%d" % (owners[j][2], v - owners[j][0]) if j >= 0 and v < owners[j][0] + owners[j][1] else None

    def words(raw):                             # aligned 8-byte words that point into an allocation are relabelled
        w = [int.from_bytes(raw[i:i + 8], "little") for i in range(0, len(raw) - len(raw) % 8, 8)]
        return ",".join((addr(x) if x >= 4096 else None) or "%x" % x for x in w) + "|" + raw[len(w) * 8:].hex()

    def arg(v):
        if isinstance(v, ctypes.c_void_p):
            v = v.value
            if v in lanes:
                return "lane%d" % lanes.index(v)
            return (addr(v) if v else "None") or "ev%d" % events.setdefault(v, len(events))
        if isinstance(v, (ctypes.Array, ctypes.Structure, bytes)):
            return words(bytes(v))
        if isinstance(v, (tuple, list)):
            return "(" + " ".join(arg(x) for x in v) + ")"
        if isinstance(v, int) and not isinstance(v, bool) and v >= 4096:
            return addr(v) or str(v)
        return repr(v)
    for name in ("launches", "opt_launches"):
        lst = getattr(plan, name)
        for i, (fn, args) in enumerate(lst):
            tag = plan.tags.get((id(lst), i))
            print(name, i, getattr(fn, "__name__", repr(fn)), "tag=%r" % (tag,), *[arg(a) for a in args], file=out)
    for i, o in enumerate(plan._keep):
        a, n = span(o)
        t = o.t if hasattr(o, "dt") else o
        if hasattr(o, "dt"):
            print("keep", i, "Buf", o.shape, o.dt, addr(a), file=out)
        elif torch.is_tensor(t):
            print("keep", i, "tensor", tuple(t.shape), t.dtype, words(t.cpu().numpy().tobytes()) if t.dtype == torch.uint8 else "", file=out)
        else:
            print("keep", i, type(o).__name__, words(bytes(o)), file=out)
    print("zero_bytes", plan.launches[0][1][2], file=out)


if __name__ == "__main__":
    dump(CASES[sys.argv[1]]())
