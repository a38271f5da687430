"""Forward lowering of the symbolic graph (engine.Plan mixin): one `_fw_<op type>` method per operator type emits the libphx launches
of that operator into the plan's launch list and records what the backward pass needs (`self.saved`).  Replaces the forward half of
what TensorFlow builds for `sess.run` in the reference (phiseg/phiseg_model.py:20-157, tfwrapper/layers.py, model_zoo/*.py)."""
import ctypes
import types

import numpy as np
import torch

from phiseg_code_amd import graph as G
from phiseg_code_amd import many_class
from phiseg_code_amd import multichannel
from phiseg_code_amd import runtime as rt
from phiseg_code_amd import upconv
from phiseg_code_amd.tfwrapper import normalisation as tfnorm
from phiseg_code_amd.engine_common import *  # noqa: F401,F403
from phiseg_code_amd.engine_common import _BN_SMALL, _BN_SMALL_F32, _BN_WIDE, _BN_WIDE_MAXLINES, _SKIP_HEAD_A, _DETERMINISTIC, _NREP, _NREP_MINP, _fgn_mode, _dual_enabled, _recomb_enabled, _noop, _device, _TORCH_DT, _NP_DT, _ESIZE, _LIK_SIDE_MAXLVL, _WGRAD_DEFER_BLOCKS, _STAMPS  # noqa: F401


def conv_norm_route(Lb, norm, training, bw, act_dt, x_dt, y_dt, out_dt, B, H, Wd, cin_eff, cout, Gn, mfma, head1x1, concat_free, upsampled,
                    deterministic=_DETERMINISTIC, fgn=None):
    """Which lowering the normalisation of a plain conv unit takes -> (NormRoute, StatsSource or None).  Pure: the library handle
    answers capability queries, everything else is a plain value (concat_free / upsampled: the input is a DualBuf / an UpBuf;
    fgn: the PHX_FGN mode, read from the environment when None).  DESIGN.md section 1 lists the routes."""
    fgn = _fgn_mode() if fgn is None else fgn
    if norm is None:
        return NormRoute.NONE, None
    if norm == "layer":
        # whole-sample statistics, no variables: always the plain materialised form on the flat kernels of csrc/layer_norm.hip (no pool /
        # head / depth-to-space / xf / conv-epilogue form)
        return NormRoute.LAYER, None
    per_batch = norm in ("batch", "renorm")        # statistics over the whole batch (NS = 1)
    NS, P = (1, B * H * Wd) if per_batch else (B, H * Wd)
    if norm == "batch" and not training:
        return (NormRoute.INFER_FOLDED if (mfma and not head1x1 and not bw) else NormRoute.INFER), None
    both_bf16 = y_dt == BF16 and out_dt == BF16
    if norm == "renorm" and both_bf16 and P <= _BN_SMALL and Lb.renorm_small_supported(P, cout, y_dt, out_dt):
        # training-mode batch renormalisation (an inference-mode layer arrives here as batch norm): one launch on the H <= 8 levels of a
        # bf16 plan -- where batch norm has its one-launch forms -- else the generic route with batch norm's statistics source (an fp32
        # plan with a fresh state then computes what the batch-norm plan computes, bit for bit); no pool / head / depth-to-space / wide / xf form
        return NormRoute.RENORM_SMALL, None
    if norm == "batch" and both_bf16 and P <= _BN_SMALL and Lb.bn_small_supported(P, cout, BF16):
        if mfma and not head1x1 and _BN_SMALL_F32 and Lb.conv3x3_mfma_f32out_supported(B, H, Wd, cin_eff, cout):
            nz = int(Lb.conv3x3_mfma_ksplit(B, H, Wd, cin_eff, cout))
            wide = bool(_BN_WIDE and Lb.bn_wide_supported(P, cout) and P * nz <= _BN_WIDE_MAXLINES)
            return (NormRoute.BN_WIDE if wide else NormRoute.BN_SMALL_F32Y), None
        return NormRoute.BN_SMALL, None
    if (not per_batch and mfma and not head1x1 and not concat_free and not deterministic and (fgn >= 2 or (fgn == 1 and Gn != cout))
            and both_bf16 and x_dt == BF16 and Lb.conv3x3_fgn_supported(B, H, Wd, cin_eff, cout, Gn)
            and Lb.norm_small_supported(NS, P, cout, Gn, BF16)):
        return NormRoute.FGN, None
    if not per_batch and both_bf16 and Lb.norm_small_supported(NS, P, cout, Gn, BF16):
        return NormRoute.NORM_SMALL, None
    small = P <= 16384 or act_dt == F32
    tiles = Lb.conv3x3_mfma_bf16_tiles_dual if concat_free else Lb.conv3x3_mfma_bf16_tiles
    if upsampled:
        stats = StatsSource.PIVOT_PASS
    elif per_batch and mfma and not small:
        stats = StatsSource.PARTIALS
    elif (per_batch and mfma and small and not deterministic and not head1x1 and act_dt == BF16
          and Lb.conv3x3_mfma_stats_atomic_supported(B, H, Wd, cin_eff, cout)):
        stats = StatsSource.ATOMIC
    elif (not per_batch and mfma and not head1x1 and act_dt == BF16 and H % 16 == 0 and Wd % 16 == 0
          and int(tiles(B, H, Wd, cin_eff, cout)) % B == 0):
        stats = StatsSource.PARTIALS_NS
    elif per_batch and not small and not deterministic:
        stats = StatsSource.DIRECT
    else:
        stats = StatsSource.PIVOT_PASS
    return NormRoute.GENERIC, stats


class ForwardLowering:
    # ---- forward emitters -----------------------------------------------------------------------
    def _fw_placeholder(self, op, bw):
        t = op.outputs[0]
        b = self._alloc_like(t, zero=True)
        self.val[t] = b
        self.feeds[op.name.rsplit("/", 1)[-1]] = b

    def _fw_constant(self, op, bw):
        b = self._alloc((), F32, zero=True)
        if op.attrs["value"] != 0.0:
            b.t.fill_(op.attrs["value"])
        self.val[op.outputs[0]] = b

    def _fw_l2_weights(self, op, bw):
        st = self.store
        if not hasattr(st, "decay_mask"):
            m = torch.zeros_like(st.params)
            for v in op.attrs["vars"]:
                off = st.offset[v.name]
                m[off:off + v.size] = 1.0
            st.decay_mask = m
            device_sync()
        out = self._alloc((), F32)
        work = self._alloc((256,), F32)
        self.val[op.outputs[0]] = out
        # data parallel (loss_inv_batch = 1 / (B * world)): every rank evaluates the term on the full parameter set, the scalar fetches
        # and the gradient arena are SUMMED over the ranks -> each rank carries a 1 / world share of the term and of its gradient
        share = self.inv_batch * self.B
        self._emit(self.L.l2_masked, st.params.data_ptr(), st.decay_mask.data_ptr(), st.n_train, op.attrs["scale"] * share, work.ptr, out.ptr,
                   self.stream)
        if bw:
            self._l2_weight = self.loss_weight.get(op.outputs[0], 0.0) * op.attrs["scale"] * share

    def _fw_one_hot(self, op, bw):
        pass            # virtual: consumed by the fused posterior-input kernel / the loss kernel

    def _fw_sub_const(self, op, bw):
        pass

    def _fw_nn_resize(self, op, bw):
        src = self.val[op.inputs[0]]
        v = Buf(src.shape, src.dt, like=src.t)
        v.shift = op.attrs["shift"]
        self.val[op.outputs[0]] = v

    def _fw_random_normal(self, op, bw):
        pass

    def _fw_mul(self, op, bw):
        pass

    def _fw_concat(self, op, bw):
        a, b = op.inputs
        ot = op.outputs[0]
        va, vb = self.val.get(a), self.val.get(b)
        cons = self._real_consumers(ot, self._opset)
        if (_dual_enabled() and self.act_dt == BF16 and self._dt_of(ot) == BF16 and isinstance(va, Buf) and isinstance(vb, Buf) and va.dt == BF16 and vb.dt == BF16
                and len(va.shape) == 4 and va.shape[-1] % 32 == 0 and vb.shape[-1] % 32 == 0 and len(cons) == 1 and ot not in self.fetches):
            c = cons[0]
            ca = c.attrs if c.type == "conv_unit" else None
            if (ca is not None and ca["ksize"] == 3 and ca.get("transposed") is None and ca.get("general") is None and ca.get("volume") is None and ca.get("explicit") is None
                    and ca["W"].shape[-1] % 32 == 0 and self.op_lane.get(c) == self.op_lane.get(op) and c not in self._lat):
                # concat-free: the one reader, a 3x3 convolution on the MFMA path, takes the two tensors as they are (no launch here)
                self.val[ot] = DualBuf(va, vb)
                return
        out = self._alloc_like(ot)
        self.val[ot] = out
        npix = int(np.prod(out.shape[:-1]))
        if b.op.type == "sub_const" and b.op.inputs[0].op.type == "one_hot":
            # concat[x, one_hot(s) - 0.5] (posteriors.py:87) in one kernel
            oh = b.op.inputs[0].op
            xb, sb = self.val[a], self.val[oh.inputs[0]]
            if a.shape[-1] > 1:                # a multi-channel image (multichannel.py): the entry of its own, Cx = 1 keeps the one below
                assert abs(b.op.attrs["c"] - 0.5) < 1e-12 and multichannel.posterior_input_entry(a.shape[-1]) == "posterior_input_mc"
                self._emit(self.L.posterior_input_mc, xb.ptr, sb.ptr, out.ptr, out.dt, npix, a.shape[-1], oh.attrs["depth"], self.stream)
                return
            assert abs(b.op.attrs["c"] - 0.5) < 1e-12 and a.shape[-1] == 1
            self._emit(self.L.posterior_input, xb.ptr, sb.ptr, out.ptr, out.dt, npix, oh.attrs["depth"], self.stream)
            return
        ab, bb = self._as_dt(self.val[a], out.dt), self._as_dt(self.val[b], out.dt)
        self._emit(self.L.concat2, ab.ptr, ab.shape[-1], bb.ptr, bb.shape[-1], out.ptr, npix, out.dt, self.stream)

    def _as_dt(self, buf, dt):
        if buf.dt == dt:
            return buf
        c = self._alloc(buf.shape, dt)
        self._emit(self.L.cast, buf.ptr, buf.dt, c.ptr, dt, buf.n, self.stream)
        return c

    def _packed(self, W):
        """bf16 packed copies of a 3x3 filter, refreshed at the head of every run (after the optimiser moved W)."""
        if W.name not in self._wpk:
            kh, kw, cin, cout = W.shape
            wf, wd = self._alloc((9 * cin * cout,), BF16), self._alloc((9 * cin * cout,), BF16)
            self._wpk[W.name] = (wf, wd)
            self._pack_jobs.append((self.store.ptr(W), wf.ptr, wd.ptr, cin, cin, cout))
        return self._wpk[W.name]

    def _packed_f32(self, W, need_dgrad):
        """fp32 packed copies of a 3x3 filter for the fp32 matrix kernels (csrc/conv_f32_mfma.hip: [K8 / 8][9][N][8]), refreshed at the
        head of every run; the data-gradient copy only where a data gradient is taken."""
        kh, kw, cin, cout = W.shape
        rec = self._wpk32.get(W.name)
        if rec is None:
            wf = self._alloc((int(self.L.conv3x3_f32_mfma_packed_floats(cin, cout)),), F32)
            rec = self._wpk32[W.name] = [wf, None, len(self._pack32_jobs)]
            self._pack32_jobs.append([self.store.ptr(W), wf.ptr, 0, cin, cout])
        if need_dgrad and rec[1] is None:
            rec[1] = self._alloc((int(self.L.conv3x3_f32_mfma_packed_floats(cout, cin)),), F32)
            self._pack32_jobs[rec[2]][2] = rec[1].ptr
        return rec[0], rec[1]

    # ---- the generic normalisation lowering, shared by the conv units, the transposed / general units and norm_act --------------
    def _norm_vectors(self, sv, B, HW, C, num_groups):
        """Statistics geometry of sv.norm on a [B, HW, C] tensor -- NS statistics sets of P values per channel, G groups -- and the
        four per-layer vectors, all recorded on `sv`.  Layer norm: one statistics set per sample over all HW * C values, no scale / shift."""
        if sv.norm == "layer":
            sv.NS, sv.P, sv.G = B, HW, 1
            sv.mean, sv.rstd = self._alloc((B,), F32), self._alloc((B,), F32)
            return
        if sv.norm in ("batch", "renorm"):
            sv.NS, sv.P, sv.G = 1, B * HW, C
        else:
            sv.G = C if sv.norm == "instance" else (num_groups or max(2, C // 16))
            sv.NS, sv.P = B, HW
        sv.scale, sv.shift = self._alloc((sv.NS * C,), F32), self._alloc((sv.NS * C,), F32)
        sv.mean, sv.rstd = self._alloc((sv.NS * sv.G,), F32), self._alloc((sv.NS * sv.G,), F32)

    @staticmethod
    def _lowered_norm(a, training):
        """The normalisation kind a unit is lowered as: batch renormalisation in inference mode IS inference-mode batch norm (r = 1, d = 0,
        the moving statistics) and takes its routes and kernels; only a training-mode layer is "renorm"."""
        return "batch" if (a["norm"] == "renorm" and not training) else a["norm"]

    def _renorm_setup(self, sv, nv, C):
        """A training-mode batch-renorm layer: the vectors its forward launch publishes beside mean / rstd / scale / shift and, in a plan
        with a loss, the gradient scratch and the layer's record of the step's tail launch (Plan._emit_renorm_tail)."""
        rn = sv.renorm = RenormSaved(self._alloc((C,), F32), self._alloc((C,), F32), self._alloc((C,), F32))
        if self.loss is not None:
            if any(j[1]["renorm_mean"] is nv["renorm_mean"] for j in self._renorm_jobs):
                raise NotImplementedError("batch_renorm: two training-mode instances of the layer %s in one plan would read and update the "
                                          "same renorm state within one step" % nv["renorm_mean"].name.rsplit("/", 1)[0])
            rn.dgs, rn.dbs = self._alloc_zeroed(C), self._alloc_zeroed(C)
            self._renorm_jobs.append((sv, nv, C))

    def _renorm_args(self, sv, nv):
        """(r, d, gamma_eff, the four renorm variables, the step counter): the arguments the renorm forward entry points add.  The clip
        bounds follow the optimiser step, read on the device: a captured graph walks the schedule with no host value baked in."""
        rn, st = sv.renorm, self.store
        return (rn.r.ptr, rn.d.ptr, rn.gamma_eff.ptr, *[st.ptr(nv[k]) for k in tfnorm.RENORM_STATE], st.step.data_ptr())

    def _renorm_apply(self, sv, nv, y, sums, pivot, out, C, act):
        self._emit(self.L.renorm_apply_fused, y.ptr, y.dt, sums.ptr, pivot.ptr if pivot is not None else None, self.store.ptr(nv["gamma"]),
                   self.store.ptr(nv["beta"]), tfnorm.EPS["renorm"], out.ptr, out.dt, sv.mean.ptr, sv.rstd.ptr, sv.scale.ptr, sv.shift.ptr,
                   *self._renorm_args(sv, nv), sv.P, C, act, self.stream, tag="bytes_norm_apply", flops=float(y.nbytes + out.nbytes))

    def _moving_args(self, nv, upd):
        """(moving mean, moving variance, momentum) arguments: the moving statistics move only in a training plan's batch norm."""
        if not upd:
            return None, None, 0.0
        return self.store.ptr(nv["moving_mean"]), self.store.ptr(nv["moving_variance"]), 1.0 - tfnorm.BN_DECAY

    def _norm_apply_args(self, sv, a, y, sums, pivot, out, C, act, training):
        """Arguments of phx_norm_apply_fused (and its _d2s / _head forms) up to the stream."""
        nv = a["norm_vars"]
        return (y.ptr, y.dt, sums.ptr, pivot.ptr if pivot is not None else None, self.store.ptr(nv["gamma"]), self.store.ptr(nv["beta"]),
                tfnorm.EPS[sv.norm], out.ptr, out.dt, sv.mean.ptr, sv.rstd.ptr, sv.scale.ptr, sv.shift.ptr,
                *self._moving_args(nv, sv.norm == "batch" and training and self.loss is not None and sv.volume is None), sv.NS, sv.P, C, sv.G, act)

    def _norm_stats_pass(self, sv, y, sums, C, conv=_noop):
        """Shifted (pivot) sums of y in a stand-alone pass, behind the launch `conv` that writes y (if any); -> the pivot vector."""
        pivot = self._alloc((sv.NS * C,), F32)
        conv()
        self._emit(self.L.norm_stats, y.ptr, y.dt, sums.ptr, pivot.ptr, sv.NS, sv.P, C, self.stream)
        return pivot

    def _norm_fwd(self, sv, a, y, out, C, act, training, conv=_noop):
        """out = act(norm(y)) the generic way: inference-mode batch norm as scale / shift + phx_affine_act, anything else as a
        statistics pass + the fused apply.  `conv`: the launch that writes y, where the caller has not emitted it yet."""
        S, Lb, nv = self.stream, self.L, a["norm_vars"]
        if sv.norm == "layer":
            conv()
            return self._layer_norm_fwd(sv, y, out, act)
        if sv.norm == "batch" and not training:
            self._emit(Lb.bn_infer_scale_shift, self.store.ptr(nv["gamma"]), self.store.ptr(nv["beta"]), self.store.ptr(nv["moving_mean"]),
                       self.store.ptr(nv["moving_variance"]), tfnorm.EPS[sv.norm], C, sv.scale.ptr, sv.shift.ptr, S)
            conv()
            self._emit(Lb.affine_act, y.ptr, y.dt, sv.scale.ptr, sv.shift.ptr, out.ptr, out.dt, sv.NS, sv.P, C, act, S)
            return
        sums = self._alloc_zeroed(sv.NS * C * 2)
        pivot = self._norm_stats_pass(sv, y, sums, C, conv)
        if sv.norm == "renorm":
            self._renorm_setup(sv, nv, C)
            return self._renorm_apply(sv, nv, y, sums, pivot, out, C, act)
        self._emit(Lb.norm_apply_fused, *self._norm_apply_args(sv, a, y, sums, pivot, out, C, act, training), S)

    def _layer_norm_phases(self, B, N):
        """-> (workspace or None, phases): a one-launch layer is ONE entry of the launch list (phase 0), a split one two (phases 1, 2),
        so that an entry is a kernel launch and carries its own bytes."""
        n = int(self.L.layer_norm_ws_floats(B, N))
        return (self._alloc((n,), F32), (1, 2)) if n else (None, (0,))

    def _layer_norm_fwd(self, sv, y, out, act):
        """out = act(layer_norm(y)) on the flat per-sample kernels (phx_layer_norm_fwd); mean / rstd [B] stay on sv for the backward pass."""
        B, N = sv.NS, y.n // sv.NS
        ws, phases = self._layer_norm_phases(B, N)
        for ph in phases:
            self._emit(self.L.layer_norm_fwd, y.ptr, y.dt, tfnorm.EPS["layer"], out.ptr, out.dt, sv.mean.ptr, sv.rstd.ptr,
                       ws.ptr if ws is not None else None, B, N, act, ph, self.stream, tag="bytes_norm_apply",
                       flops=float(y.nbytes + (0 if ph == 1 else out.nbytes)))

    def _fw_tconv_unit(self, op, bw):
        """tf.nn.conv2d_transpose -> [bias] -> [norm] -> act (tfwrapper/layers.py:197-258) on the direct kernels of tconv.hip;
        the normalisation runs as statistics pass + fused apply on the up-sampled tensor.  The general 2-D units (gconv.hip) and the 3-D
        units (conv3d.hip) take the same form."""
        a = op.attrs
        x = self.val[op.inputs[0]]
        W, b = a["W"], a["b"]
        B, H, Wd = x.shape[0], x.shape[1], x.shape[2]
        S, Lb = self.stream, self.L
        vol, exp = a.get("volume"), a.get("explicit")
        if exp is not None:
            # a 2-D unit with its whole geometry on the kernels of csrc/conv2d_pad.hip (VALID padding, a free output_shape of the
            # transposed layer): filter HWIO (form "conv") / HWOI ("tconv"), geo = (B, H, W, Cin, Cout, kh, kw, sh, sw, dh, dw, Ho, Wo, pt, pl)
            cin, cout = (W.shape[2], W.shape[3]) if exp[0] == "conv" else (W.shape[3], W.shape[2])
            geo = (B, H, Wd, cin, cout) + tuple(exp[1:])
            conv_fwd = Lb.conv2d_pad_fwd if exp[0] == "conv" else Lb.tconv2d_pad_fwd
        elif vol is not None:
            # conv3D / transposed_conv3D on the kernels of csrc/conv3d.hip: x is [B, D, H, W, C], filter DHWIO / DHWOI
            form = vol[0]
            cin, cout = (W.shape[3], W.shape[4]) if form == "conv" else (W.shape[4], W.shape[3])
            geo = tuple(x.shape[:4]) + (cin, cout) + tuple(vol[1:])
            conv_fwd = Lb.gconv3d_fwd if form == "conv" else Lb.tconv3d_fwd
        elif a.get("general") is not None:
            # strided / dilated SAME convolution on the direct kernels of gconv.hip (conv2D with strides, dilated_conv2D,
            # dense_layer as a 1x1 convolution of the flattened input); filter HWIO (a dense layer's [F, U] is [1][1][F][U])
            geo = (B, H, Wd, W.shape[-2], W.shape[-1]) + tuple(a["general"])
            cin, cout = W.shape[-2], W.shape[-1]
            conv_fwd = Lb.gconv2d_fwd
        else:
            kh, kw, sh, sw = a["transposed"]
            cout, cin = W.shape[2], W.shape[3]
            geo = (B, H, Wd, cin, cout, kh, kw, sh, sw)
            conv_fwd = Lb.tconv2d_fwd
        out = self._alloc_like(op.outputs[0])
        self.val[op.outputs[0]] = out
        act = rt.ACT_CODES[a["act"]]
        training = a["training"] if isinstance(a["training"], bool) else self.training
        norm = self._lowered_norm(a, training)
        wptr, bptr = self.store.ptr(W), (self.store.ptr(b) if b is not None else None)
        sv = self.saved[op] = ConvSaved.plain(x, out, norm, cin, transposed=a.get("transposed"), general=a.get("general"), volume=vol, geo=geo,
                                              explicit=exp[0] if exp is not None else None)
        if norm is None:
            self._emit(conv_fwd, x.ptr, x.dt, wptr, bptr, out.ptr, out.dt, *geo, act, S)
            return
        # (a volume's pre-normalisation tensor is kept in the folded shape [B, D H, W, C]: the normalisation passes see [B, pixels, C])
        y = sv.y = self._alloc(self._folded(out.shape), out.dt)
        self._emit(conv_fwd, x.ptr, x.dt, wptr, bptr, y.ptr, y.dt, *geo, 0, S)
        self._norm_vectors(sv, B, int(np.prod(out.shape[1:-1])), cout, a["num_groups"])
        sv.route = NormRoute.INFER if (norm == "batch" and not training) else (NormRoute.LAYER if norm == "layer" else NormRoute.GENERIC)
        self._norm_fwd(sv, a, y, out, cout, act, training)
        self._moving_biased(sv, a, cout, training)

    @staticmethod
    def _folded(shape):
        """[B, D, H, W, C] -> [B, D H, W, C] (the same memory); a 4-D shape as it is."""
        return tuple(shape) if len(shape) != 5 else (shape[0], shape[1] * shape[2], shape[3], shape[4])

    def _moving_biased(self, sv, a, C, training):
        """Batch norm on a rank-5 tensor moves its moving pair with the BIASED batch variance (tf.contrib.layers.batch_norm's non-fused
        path): the apply launch got no moving pointers (_norm_apply_args), this launch updates the pair from the
        statistics it published."""
        if sv.volume is not None and sv.norm == "batch" and training and self.loss is not None:
            nv = a["norm_vars"]
            self._emit(self.L.bn_moving_update_biased, sv.mean.ptr, sv.rstd.ptr, tfnorm.EPS["batch"], self.store.ptr(nv["moving_mean"]),
                       self.store.ptr(nv["moving_variance"]), 1.0 - tfnorm.BN_DECAY, C, self.stream)

    # ---- fused latent heads: mu = conv1x1(x), sigma = softplus(conv1x1(x)), z = mu + sigma * eps (posteriors.py:125-128,
    # priors.py:117-120) as one launch forward (phx_latent_heads_fwd) and one backward (phx_latent_heads_bwd) ----------------------
    def _find_latent_heads(self, ops):
        pos = {op: i for i, op in enumerate(ops)}
        opset = set(ops)
        out = {}

        def is_head(op, act):
            a = op.attrs
            if op.type != "conv_unit" or a.get("transposed") is not None or a.get("general") is not None or a.get("volume") is not None or a.get("explicit") is not None:
                return False
            W = a["W"]
            return (a["ksize"] == 1 and a["norm"] is None and a["b"] is not None and a["act"] == act and W.shape[-1] in (2, 4, 6)
                    and W.shape[-2] % 8 == 0 and op.outputs[0].kind == G.KIND_F32)
        for mu in ops:
            if mu in out or not is_head(mu, "identity"):
                continue
            x = mu.inputs[0]
            sib = [c for c in x.consumers if c in opset and c is not mu and is_head(c, "softplus")
                   and c.attrs["W"].shape == mu.attrs["W"].shape and c not in out]
            if len(sib) != 1:
                continue
            sig = sib[0]
            add = None
            for c in mu.outputs[0].consumers:
                if (c in opset and c.type == "add" and c.outputs[0] not in self.fed and c.inputs[0] is mu.outputs[0] and c.inputs[1].op.type == "mul"
                        and c.inputs[1].op.inputs[0] is sig.outputs[0] and c.inputs[1].op.inputs[1].op.type == "random_normal"):
                    add = c
            members = [o for o in (mu, sig, add) if o is not None]
            last = max(members, key=lambda o: pos[o])
            virt = {add.inputs[1].op, add.inputs[1].op.inputs[1].op} if add is not None else set()
            # nothing may read mu / sigma before the group's launch, the heads must sit on one lane, and neither may be a fetch
            ok = all(pos.get(c, 1 << 30) > pos[last] or c in members or c in virt
                     for t in (mu.outputs[0], sig.outputs[0]) for c in t.consumers if c in opset)
            ok = ok and len({self.op_lane[o] for o in members}) == 1
            if not ok:
                continue
            rec = dict(mu=mu, sig=sig, add=add, last=last, x=x)
            for o in members:
                out[o] = rec
        return out

    def _fw_latent_group(self, rec):
        mu_op, sig_op, add_op = rec["mu"], rec["sig"], rec["add"]
        x = self.val[rec["x"]]
        mu, sigma = self.val[mu_op.outputs[0]], self.val[sig_op.outputs[0]]
        z = self.val[add_op.outputs[0]] if add_op is not None else None
        cin, zd = mu_op.attrs["W"].shape[-2], mu_op.attrs["W"].shape[-1]
        npix = int(np.prod(x.shape[:-1]))
        hw = npix // x.shape[0]
        sid = add_op.inputs[1].op.inputs[1].op.attrs["stream"] if add_op is not None else 0
        st = self.store
        self._emit(self.L.latent_heads_fwd, x.ptr, x.dt, st.ptr(mu_op.attrs["W"]), st.ptr(mu_op.attrs["b"]), st.ptr(sig_op.attrs["W"]),
                   st.ptr(sig_op.attrs["b"]), mu.ptr, sigma.ptr, z.ptr if z is not None else None, npix, cin, zd, hw, self.rng_seed,
                   self._noise_step_ptr(), sid, self.sample_offset, self.stream)
        rec.update(npix=npix, hw=hw, sid=sid, cin=cin, zd=zd)

    # ---- prob_unet2D's recombination chain at n samples per image (likelihoods.py:147-157 behind sampling_graph) as ONE launch:
    # tile_batch(feat) -> concat with tile_pixels(z) -> three 1x1 conv units -> 1x1 head [-> soft-max aggregate] = phx_recomb_samples.
    # Neither the tiled feature map nor the broadcast z nor any activation of the chain is materialised ---------
    def _find_recomb_chains(self, ops):
        """-> {member op: record} for every chain of an INFERENCE plan the kernel takes (K = 32, KF = 32 / 64, Z <= 32, 2 <= C <= 8, inference-mode
        batch norm or identity norm, no intermediate fetched or read from outside); every other configuration keeps the unit-by-unit
        lowering."""
        out = {}
        if self.loss is not None or not _recomb_enabled():
            return out
        opset = set(ops)

        def sole_reader(t):
            """the one op of the plan that reads t, provided nobody fetches t"""
            cons = [c for c in t.consumers if c in opset]
            return cons[0] if (len(cons) == 1 and t not in self.fetches and t not in self.fed) else None

        def plain_1x1(op):
            a = op.attrs
            return (op.type == "conv_unit" and a.get("transposed") is None and a.get("general") is None and a.get("volume") is None and a.get("explicit") is None and a["ksize"] == 1
                    and op not in self._lat)
        for tb in ops:
            if tb.type != "tile_batch" or len(tb.inputs[0].shape) != 4:
                continue
            KF = tb.inputs[0].shape[-1]            # (the decoder's last level is 2 n0 wide: 64 channels into the 32-wide chain at n0 = 32)
            if KF not in (32, 64):
                continue
            cat = sole_reader(tb.outputs[0])
            if cat is None or cat.type != "concat" or cat.inputs[0] is not tb.outputs[0] or cat.inputs[1].op.type != "tile_pixels":
                continue
            tp = cat.inputs[1].op
            if tp not in opset or sole_reader(tp.outputs[0]) is not cat or tp.inputs[0].kind != G.KIND_F32:
                continue
            Z = tp.inputs[0].shape[-1]
            units, t = [], cat.outputs[0]
            for _ in range(3):
                u = sole_reader(t)
                if u is None or not plain_1x1(u) or u.inputs[0] is not t:
                    break
                a = u.attrs
                training = a["training"] if isinstance(a["training"], bool) else self.training
                norm_ok = (a["norm"] in ("batch", "renorm") and not training and a["b"] is None) or (a["norm"] is None and a["b"] is not None)
                if not norm_ok or a["act"] != "relu" or tuple(a["W"].shape[2:]) != (KF + Z if not units else 32, 32):
                    break
                units.append(u)
                t = u.outputs[0]
            if len(units) != 3:
                continue
            head = sole_reader(t)
            if head is None or not plain_1x1(head) or head.inputs[0] is not t:
                continue
            ha = head.attrs
            C = ha["W"].shape[-1]
            if (ha["norm"] is not None or ha["b"] is None or ha["act"] != "identity" or head.outputs[0].kind != G.KIND_F32
                    or ha["W"].shape[-2] != 32 or not (1 <= Z <= 32) or not (2 <= C <= 8)):
                continue
            members = [tb, tp, cat] + units + [head]
            agg = sole_reader(head.outputs[0])
            if agg is not None and agg.type == "aggregate" and agg.attrs["L"] == 1:
                members.append(agg)            # the soft-max (and the one-level "sum") ride on the same launch
            else:
                agg = None
            if len({self.op_lane[o] for o in members}) != 1:
                continue
            rec = dict(tb=tb, tp=tp, units=units, head=head, agg=agg, last=members[-1], KF=KF, Z=Z, C=C, n=tb.attrs["tile"])
            for o in members:
                out[o] = rec
        return out

    def _fw_recomb_member(self, op):
        """A member of a fused recombination chain: its values are never made; the chain's last operator emits the launch."""
        rec = self._recomb[op]
        if op is not rec["last"]:
            return
        st, head, agg = self.store, rec["head"], rec["agg"]
        feat, z = self.val[rec["tb"].inputs[0]], self.val[rec["tp"].inputs[0]]
        assert isinstance(feat, Buf) and feat.dt in (F32, BF16) and z.dt == F32
        B, P, n = feat.shape[0], feat.shape[1] * feat.shape[2], rec["n"]
        assert z.shape[0] == B * n, "recombination chain: z has %d rows, %d images x %d samples expected" % (z.shape[0], B, n)
        st_ptrs = []
        for u in rec["units"]:
            a = u.attrs
            if a["norm"] in ("batch", "renorm"):
                nv = a["norm_vars"]
                scale, shift = self._alloc((32,), F32), self._alloc((32,), F32)
                self._bninfer_jobs.append((st.ptr(nv["gamma"]), st.ptr(nv["beta"]), st.ptr(nv["moving_mean"]), st.ptr(nv["moving_variance"]),
                                           scale.ptr, shift.ptr, 32, tfnorm.EPS["batch"]))
                st_ptrs += [scale.ptr, shift.ptr]
            else:
                st_ptrs += [None, st.ptr(a["b"])]
        lg = sm = None
        if agg is not None:
            used = [t in self.fetches or any(c in self._opset for c in t.consumers) for t in agg.outputs]
            if used[0] or not used[1]:
                lg = self._alloc_like(agg.outputs[0])
            if used[1]:
                sm = self._alloc_like(agg.outputs[1])
            self.val[agg.outputs[0]], self.val[agg.outputs[1]] = lg, sm
            self.val[head.outputs[0]] = lg
        else:
            lg = self.val[head.outputs[0]] = self._alloc_like(head.outputs[0])
        W = [st.ptr(u.attrs["W"]) for u in rec["units"]]
        self._emit(self.L.recomb_samples, feat.ptr, feat.dt, z.ptr, W[0], W[1], W[2], st.ptr(head.attrs["W"]), st.ptr(head.attrs["b"]),
                   *st_ptrs, lg.ptr if lg is not None else None, sm.ptr if sm is not None else None, B, n, P, rec["KF"], 32, rec["Z"], rec["C"],
                   self.stream)

    def _norm_head_consumer(self, op):
        """The 1x1 head (bias, no norm, identity, fp32 out, 2 / 4 outputs) that is the ONLY reader of this unit's output, or None."""
        if self.act_dt != BF16:
            return None
        out = op.outputs[0]
        if out in self.fetches:
            return None
        cons = self._real_consumers(out, self._opset)
        if len(cons) != 1 or cons[0].type != "conv_unit" or cons[0] in self._lat:
            return None
        c, ca = cons[0], cons[0].attrs
        if (ca.get("transposed") is not None or ca.get("general") is not None or ca.get("volume") is not None or ca.get("explicit") is not None or ca["ksize"] != 1 or ca["norm"] is not None
                or ca["b"] is None or ca["act"] != "identity" or c.inputs[0] is not out or c.outputs[0].kind != G.KIND_F32
                or c.outputs[0] in self.fetches or self.op_lane.get(c) != self.op_lane.get(op)):
            return None
        return c

    def _xf_edge_ok(self, op, B, H, Wd, C):
        """May conv unit `op` leave its activation a = relu(bn(y)) unwritten?  -- every real reader is a 3x3 conv unit with batch norm
        (no bias, statistics epilogue) that reads it directly (not through a concat), trains, and whose forward and filter-gradient
        kernels take the input transform at this shape (phx_conv3x3_xf_supported / phx_conv3x3_wgrad_xf_supported: the HBM-bound 32 -> 32
        layers of the 128 x 128 level -- on the matrix-bound shapes the transform costs more than the apply pass it deletes,
        DESIGN.md section 5); nobody fetches it."""
        out = op.outputs[0]
        if out in self.fetches:
            return False
        cons = self._real_consumers(out, self._opset)
        if not cons:
            return False
        for c in cons:
            ca = c.attrs
            if (c.type != "conv_unit" or c in self._lat or ca.get("transposed") is not None or ca.get("general") is not None or ca.get("volume") is not None or ca.get("explicit") is not None
                    or ca["ksize"] != 3 or ca["norm"] != "batch" or ca["b"] is not None or c.inputs[0] is not out):
                return False
            tr = ca["training"] if isinstance(ca["training"], bool) else self.training
            cin, cout = ca["W"].shape[-2], ca["W"].shape[-1]
            if (not tr or cin != C or not self.L.conv3x3_xf_supported(B, H, Wd, cin, cout)
                    or not self.L.conv3x3_wgrad_xf_supported(B, H, Wd, cin, cout)):
                return False
        return True

    def _fw_conv_unit(self, op, bw):
        """conv -> [bias] -> [norm] -> act: prepare the operands, choose the normalisation route (conv_norm_route), emit that route."""
        a = op.attrs
        if a.get("transposed") is not None or a.get("general") is not None or a.get("volume") is not None or a.get("explicit") is not None:
            return self._fw_tconv_unit(op, bw)
        if op in self._norm_head:                # its forward ran inside the producer's apply pass
            self.saved[op] = ConvSaved.plain(self.val[op.inputs[0]], self.val[op.outputs[0]], None, a["W"].shape[-2], head1x1=True, norm_head=True)
            return
        rec = self._lat.get(op)
        if rec is not None:                      # a latent head: its arithmetic runs in the group's one launch
            self.val[op.outputs[0]] = self._alloc_like(op.outputs[0])
            self.saved[op] = ConvSaved.plain(None, self.val[op.outputs[0]], None, a["W"].shape[-2], latent=True)
            if rec["last"] is op:
                self._fw_latent_group(rec)
            return
        o = self._conv_operands(op, bw)
        sv = self.saved[op] = o.sv
        if sv.norm is None:
            self._conv_into(o, o.out, o.act)
            return
        o.y = self._alloc(o.out.shape, o.out.dt)
        self._norm_vectors(sv, o.B, o.H * o.Wd, o.cout, a["num_groups"])
        nv = a["norm_vars"]
        if sv.norm != "layer":                   # (layer norm has no variables)
            o.params = (self.store.ptr(nv["gamma"]), self.store.ptr(nv["beta"]), tfnorm.EPS[sv.norm])
            o.moving = self._moving_args(nv, sv.norm == "batch" and o.training and self.loss is not None)
        if sv.norm == "renorm":
            self._renorm_setup(sv, nv, o.cout)
        sv.route, o.stats = conv_norm_route(self.L, sv.norm, o.training, bw, self.act_dt, o.x.dt, o.y.dt, o.out.dt, o.B, o.H, o.Wd, sv.cin_eff,
                                            o.cout, sv.G, sv.mfma, sv.head1x1, o.dual is not None, o.up is not None)
        getattr(self, "_fw_unit_" + sv.route.name.lower())(o, sv)
        if sv.route is not NormRoute.INFER_FOLDED:
            sv.y = o.y

    def _conv_operands(self, op, bw):
        """Classify a plain conv unit's convolution (bf16 MFMA as it is / channel-padded / 1x1 head / fp32 MFMA / direct; concat-free,
        phase-form or unmaterialised input), pad its input where needed and look up its packed filter -> the operand record the
        launch methods take (_fw_conv_unit and the normalisation route add y, params, moving, stats, sums, pivot, apply_args)."""
        a = op.attrs
        x = self.val[op.inputs[0]]
        W, b = a["W"], a["b"]
        k, (_, _, cin, cout) = a["ksize"], W.shape
        B, H, Wd = x.shape[0], x.shape[1], x.shape[2]
        out = self._alloc_like(op.outputs[0])
        self.val[op.outputs[0]] = out
        mfma = (self.act_dt == BF16 and x.dt == BF16 and out.dt == BF16 and k == 3 and cin % 32 == 0
                and cout % 32 == 0)
        dual = x if isinstance(x, DualBuf) else None
        assert dual is None or mfma, "concat-free input reached a convolution off the MFMA path"
        up = x if isinstance(x, UpBuf) else None      # bilinear_upsample2D of up.src, never written: this unit runs in the phase form (upconv.py)
        xf = x if isinstance(x, XfBuf) else None      # the producer's activation was never written: this launch re-forms it (see _xf_edge_ok)
        assert xf is None or (mfma and a["norm"] == "batch" and b is None), "unmaterialised activation reached a convolution that cannot re-form it"
        cin_eff = cin
        # Convolutions the 3x3 MFMA kernels do not take as they are: input channels not a multiple of 32 (image Cin = 1 / 3,
        # latent Cin = 2, prob_unet2D's feature + z concat) are zero-padded, and 1x1 filters (prob_unet2D's recombination
        # layers, likelihoods.py) run as the centre tap of a 3x3 -- 9x the FLOPs on the matrix cores still beats the fp32
        # direct kernel by 30x.  Both get their own packed filter copies ("padded" path).
        k1 = k == 1 and cout % 32 == 0
        padded = (self.act_dt == BF16 and out.dt == BF16 and cout % 32 == 0 and
                  ((k == 3 and (cin % 32 != 0 or x.dt != BF16)) or k1))
        if padded:
            cin_eff = (cin + 31) // 32 * 32
            if cin_eff != cin or x.dt != BF16:        # (with cin_eff == cin the pad kernel is just the cast to bf16)
                xp = self._alloc((B, H, Wd, cin_eff), BF16)
                self._emit(self.L.pad_channels_bf16, x.ptr, x.dt, cin, xp.ptr, cin_eff, B * H * Wd, self.stream)
                x = xp
            mfma = True
        head1x1 = (k == 1 and out.dt == F32 and cout in (2, 4, 6, 8) and a["norm"] is None and b is not None)
        # fp32 plans: the 3x3 convolution on the fp32 matrix instruction (same arithmetic class as the direct kernel: an fp32 FMA chain)
        f32m = bool(not mfma and self.act_dt == F32 and x.dt == F32 and out.dt == F32 and k == 3 and cout % 32 == 0 and _f32_mfma_enabled()
                    and isinstance(x, Buf) and self.L.conv3x3_f32_mfma_supported(B, H, Wd, cin, cout))
        training = a["training"] if isinstance(a["training"], bool) else self.training
        sv = ConvSaved(x, out, self._lowered_norm(a, training), mfma, padded, cin_eff, bool(padded and k1), head1x1, f32m=f32m)
        wptr, wf = self.store.ptr(W), None
        if padded:
            wf = self._alloc((9 * cin_eff * cout,), BF16)
            sv.wd_pad = self._alloc((9 * cin_eff * cout,), BF16) if (bw and self.req.get(op.inputs[0], False)) else None
            self._pack_jobs.append((wptr, wf.ptr, sv.wd_pad.ptr if sv.wd_pad else 0, cin, cin_eff, cout, 1 if k1 else 0))
        elif mfma:
            wf, _ = self._packed(W)
        return types.SimpleNamespace(op=op, a=a, bw=bw, sv=sv, x=x, out=out, W=W, k=k, cin=cin, cout=cout, B=B, H=H, Wd=Wd, dual=dual, up=up, xf=xf,
                                     wf=wf, wptr=wptr, bptr=self.store.ptr(b) if b is not None else None, act=rt.ACT_CODES[a["act"]],
                                     training=training,
                                     y=None, sums=None, pivot=None, stats=None, apply_args=None)

    def _mfma_conv(self, o, y, bias_p, oscale_p, act_code, stats, stats_mode, ws, wsb):
        """One forward launch on the bf16 MFMA path (plain or concat-free input): phx_conv3x3_mfma_bf16_dual takes every option"""
        Lb, x, xf, dual = self.L, o.x, o.xf, o.dual
        geo = (o.B, o.H, o.Wd, o.sv.cin_eff, o.cout, self.stream)
        flops = 18.0 * o.cin * o.cout * o.B * o.H * o.Wd
        if xf is not None:
            assert bias_p is None and oscale_p is None and act_code == 0 and stats_mode in (0, 1) and ws is None
            self._emit(Lb.conv3x3_mfma_bf16_xf, xf.y.ptr, xf.scale.ptr, xf.shift.ptr, o.wf.ptr, y.ptr,
                       stats.ptr if stats is not None else None, *geo, tag="conv3x3_mfma_fwd", flops=flops)
            return
        self._emit(Lb.conv3x3_mfma_bf16_dual, x.ptr, dual.b.ptr if dual is not None else None, dual.k1 if dual is not None else 0,
                   o.wf.ptr, y.ptr if y is not None else None, None, 0, bias_p, oscale_p, act_code,
                   stats.ptr if stats is not None else None, stats_mode, ws.ptr if ws is not None else None, wsb,
                   *geo, tag="conv3x3_mfma_fwd", flops=flops)

    def _conv_tiles(self, o):
        tiles = self.L.conv3x3_mfma_bf16_tiles_dual if o.dual is not None else self.L.conv3x3_mfma_bf16_tiles
        return int(tiles(o.B, o.H, o.Wd, o.sv.cin_eff, o.cout))

    def _conv_into(self, o, y, act_code, stats_direct=None, stats_part=None, stats_atomic=None):
        """The unit's convolution (+ bias, + activation `act_code`) into y on whichever kernel its operands select."""
        S, Lb, x, sv, op = self.stream, self.L, o.x, o.sv, o.op
        B, H, Wd, cin, cout = o.B, o.H, o.Wd, o.cin, o.cout
        if o.up is not None:
            # y <- the hi-res pre-normalisation map in PACKED pixel order [B, h, w, (a, b, cout)]: the per-channel norm kernels do not
            # care about the order of the pixels; the apply pass's output is permuted to hi-res below
            assert act_code == 0 and stats_direct is None and stats_part is None and stats_atomic is None
            sv.upconv = upconv.forward(self._emit, self._alloc, Lb, S, o.up.src, o.wptr, o.wf, y, B, H // 2, Wd // 2, cin, cout,
                                       need_dgrad=bool(o.bw and self.req.get(op.inputs[0].op.inputs[0], False)), bias_ptr=o.bptr)
        elif stats_atomic is not None:
            self._mfma_conv(o, y, o.bptr, None, act_code, stats_atomic, 2, None, 0)
        elif sv.head1x1:
            self._emit(Lb.head1x1_fwd, x.ptr, x.dt, o.wptr, o.bptr, y.ptr, B * H * Wd, cin, cout, act_code, S)
        elif sv.mfma:
            wsb = int(Lb.conv3x3_mfma_ws_bytes(B, H, Wd, sv.cin_eff, cout)) if stats_part is None else 0
            ws = self._alloc((wsb // 4,), F32) if wsb else None          # split-K slices (small maps)
            self._mfma_conv(o, y, o.bptr, None, act_code, stats_part, 1 if stats_part is not None else 0, ws, wsb)
        elif sv.f32m and stats_direct is None and y.dt == F32:
            need_dgrad = bool(o.bw and self.req.get(op.inputs[0], False) and cin % 32 == 0)
            w32, _ = self._packed_f32(o.W, need_dgrad)
            self._emit(Lb.conv3x3_f32_mfma, x.ptr, w32.ptr, o.bptr, y.ptr, B, H, Wd, cin, cout, act_code, S,
                       tag="conv3x3_f32_mfma_fwd", flops=18.0 * cin * cout * B * H * Wd)
        else:
            self._emit(Lb.conv2d_direct, x.ptr, x.dt, o.wptr, o.bptr, y.ptr, y.dt, B, H, Wd, cin, cout, o.k, act_code,
                       0, stats_direct.ptr if stats_direct is not None else None, S)

    # ---- one emitter per normalisation route (NormRoute; the table is in DESIGN.md section 1) ------------------------------------
    def _fw_unit_infer_folded(self, o, sv):
        # inference-mode batch norm + activation folded into the convolution's epilogue (phx_conv3x3_mfma_bf16_affine):
        # one launch where the reference runs conv2d, batch_norm and relu; the scale / shift vectors of all layers come
        # from one launch at the head of the run
        nv = o.a["norm_vars"]
        gptr, beptr, eps = o.params
        self._bninfer_jobs.append((gptr, beptr, self.store.ptr(nv["moving_mean"]), self.store.ptr(nv["moving_variance"]),
                                   sv.scale.ptr, sv.shift.ptr, o.cout, eps))
        wsb = int(self.L.conv3x3_mfma_ws_bytes(o.B, o.H, o.Wd, sv.cin_eff, o.cout))
        ws = self._alloc((wsb // 4,), F32) if wsb else None
        self._mfma_conv(o, o.out, sv.shift.ptr, sv.scale.ptr, o.act, None, 0, ws, wsb)

    def _fw_unit_infer(self, o, sv):
        self._norm_fwd(sv, o.a, o.y, o.out, o.cout, o.act, o.training, conv=lambda: self._conv_into(o, o.y, 0))

    def _conv_f32out(self, o, sum_slices):
        """The 2 x 2 / 4 x 4 levels: the pre-normalisation tensor stays in fp32 (the split-K kernel's accumulators, summed) --
        a channel is normalised from a few dozen to a few hundred values here, and the bf16 rounding of y (2^-9 of the
        channel mean) is blown up with their spread: the two coarsest KL terms trained 40 % high.
        -> (workspace of slices, slice count)"""
        Lb, dual, geo = self.L, o.dual, (o.B, o.H, o.Wd, o.sv.cin_eff, o.cout)
        o.y = self._alloc(o.out.shape, F32)
        wsb = int(Lb.conv3x3_mfma_ws_bytes(*geo))
        ws = self._alloc((wsb // 4,), F32) if wsb else None
        self._emit(Lb.conv3x3_mfma_bf16_f32out, o.x.ptr, dual.b.ptr if dual is not None else None,
                   dual.k1 if dual is not None else 0, o.wf.ptr, o.y.ptr, sum_slices, ws.ptr if ws is not None else None, wsb,
                   *geo, self.stream, tag="conv3x3_mfma_fwd", flops=18.0 * o.cin * o.cout * o.B * o.H * o.Wd)
        return ws, int(Lb.conv3x3_mfma_ksplit(*geo))

    def _fw_unit_bn_wide(self, o, sv):
        # the batch-norm launch is the split-K finishing pass as well (phx_bn_wide_fwd: four channels per block,
        # sums the slices in slice order): one launch fewer per layer, 48 blocks instead of 12 on a 192-channel layer
        # (a block of that launch pulls P x nz 128-byte lines through ONE CU whatever its channel count: measured + 5 us per
        # layer at 2 x 2 (P = 256, six slices), - 8 us at 4 x 4 (P = 1 024, three slices) against finishing pass + phx_bn_small_fwd)
        ws, nz = self._conv_f32out(o, 0)
        y, out = o.y, o.out
        self._emit(self.L.bn_wide_fwd, ws.ptr if nz > 1 else y.ptr, nz, y.ptr, *o.params, out.ptr, sv.mean.ptr, sv.rstd.ptr,
                   sv.scale.ptr, sv.shift.ptr, *o.moving, sv.P, o.cout, o.act,
                   self.stream, tag="bytes_norm_apply", flops=float(y.nbytes + out.nbytes))

    def _fw_unit_bn_small(self, o, sv):
        # H <= 8 levels: the whole batch-norm layer in one launch (phx_bn_small_fwd / _bwd; csrc/norm_onelaunch.hip)
        # (policy P <= 1024, the H <= 4 levels: at P = 4096 the single launch measured no faster than the chain)
        if sv.route is NormRoute.BN_SMALL_F32Y:
            self._conv_f32out(o, 1)
        else:
            self._conv_into(o, o.y, 0)
        y, out = o.y, o.out
        self._emit(self.L.bn_small_fwd, y.ptr, y.dt, *o.params, out.ptr, sv.mean.ptr, sv.rstd.ptr, sv.scale.ptr, sv.shift.ptr,
                   *o.moving, sv.P, o.cout, o.act, self.stream,
                   tag="bytes_norm_apply", flops=float(y.nbytes + out.nbytes))

    _fw_unit_bn_small_f32y = _fw_unit_bn_small

    def _fw_unit_renorm_small(self, o, sv):
        # H <= 8 levels, training-mode batch renormalisation: the whole forward in one launch (phx_renorm_small_fwd); like batch norm the
        # 2 x 2 / 4 x 4 levels of a bf16 plan keep the pre-normalisation tensor in fp32.  The backward pass is phx_bn_small_bwd's.
        if (sv.mfma and not sv.head1x1 and _BN_SMALL_F32 and o.y.dt == BF16
                and self.L.conv3x3_mfma_f32out_supported(o.B, o.H, o.Wd, sv.cin_eff, o.cout)):
            self._conv_f32out(o, 1)
        else:
            self._conv_into(o, o.y, 0)
        y, out, nv = o.y, o.out, o.a["norm_vars"]
        self._emit(self.L.renorm_small_fwd, y.ptr, y.dt, *o.params, out.ptr, out.dt, sv.mean.ptr, sv.rstd.ptr, sv.scale.ptr, sv.shift.ptr,
                   *self._renorm_args(sv, nv), sv.P, o.cout, o.act, self.stream, tag="bytes_norm_apply", flops=float(y.nbytes + out.nbytes))

    def _fw_unit_layer(self, o, sv):
        # layer norm: the convolution writes y (bias in, activation off, no statistics epilogue), then the flat per-sample kernels
        self._conv_into(o, o.y, 0)
        self._layer_norm_fwd(sv, o.y, o.out, o.act)

    def _fw_unit_fgn(self, o, sv):
        # maps of at most 16 x 16: convolution, bias, group / instance norm and activation in ONE launch (a block holds whole
        # samples and whole groups: no cross-block step); the backward pass is phx_norm_small_bwd's
        self._emit(self.L.conv3x3_mfma_bf16_fgn, o.x.ptr, o.wf.ptr, o.y.ptr, o.out.ptr, o.bptr, *o.params, sv.G, o.act,
                   sv.mean.ptr, sv.rstd.ptr, sv.scale.ptr, sv.shift.ptr, o.B, o.H, o.Wd, sv.cin_eff, o.cout, self.stream,
                   tag="conv3x3_mfma_fwd", flops=18.0 * o.cin * o.cout * o.B * o.H * o.Wd, shape=("fgn", o.B, o.H, o.Wd, sv.cin_eff, o.cout))

    def _fw_unit_norm_small(self, o, sv):
        # group / instance norm on maps of up to 256 pixels: the whole layer in one launch as well (phx_norm_small_fwd / _bwd: a
        # wave per (sample, 16-channel slice)); a split-K convolution hands over its slices and its bias
        self._conv_into(o, o.y, 0)
        y, out = o.y, o.out
        self._emit(self.L.norm_small_fwd, y.ptr, None, 0, None, *o.params, out.ptr, sv.mean.ptr, sv.rstd.ptr,
                   sv.scale.ptr, sv.shift.ptr, sv.NS, sv.P, o.cout, sv.G, o.act, self.stream,
                   tag="bytes_norm_apply", flops=float(y.nbytes + out.nbytes))

    def _fw_unit_generic(self, o, sv):
        """Statistics from o.stats (StatsSource), then the first apply-pass variant that takes the unit."""
        o.sums = self._alloc_zeroed(sv.NS * o.cout * 2)
        self._conv_with_stats(o, sv)
        if sv.norm == "renorm":          # (no pool / head / depth-to-space / xf form: the plain renorm apply pass)
            return self._renorm_apply(sv, o.a["norm_vars"], o.y, o.sums, o.pivot, o.out, o.cout, o.act)
        o.apply_args = self._norm_apply_args(sv, o.a, o.y, o.sums, o.pivot, o.out, o.cout, o.act, o.training)
        for apply in (self._apply_xf, self._apply_d2s, self._apply_head, self._apply_pool, self._apply_plain):
            if apply(o, sv):
                break
        if sv.norm != "batch":
            sv.fsums, sv.fpivot = o.sums, o.pivot         # forward per-channel sums: the bias gradient is closed-form from them

    def _conv_with_stats(self, o, sv):
        """The convolution into o.y with the per-channel sums in o.sums: shifted (pivot) sums in a stand-alone pass -- always on the
        fp32 parity path, and on the bf16 path when a statistic has few samples (cheap there) -- otherwise from the conv epilogue."""
        Lb, S, y, src = self.L, self.stream, o.y, o.stats
        if src is StatsSource.PIVOT_PASS:
            # (phase form: the frame of the packed map is written after the phase convolution: its statistics epilogue cannot be used)
            o.pivot = self._norm_stats_pass(sv, y, o.sums, o.cout, conv=lambda: self._conv_into(o, y, 0))
        elif src is StatsSource.ATOMIC:
            # few pixel tiles (the H <= 16 levels): the convolution adds its statistics straight into `sums` -- no pass over y
            self._conv_into(o, y, 0, stats_atomic=o.sums)
        elif src is StatsSource.DIRECT:
            self._conv_into(o, y, 0, stats_direct=o.sums)        # (direct kernels add their tiles' sums atomically)
        else:
            ntile = self._conv_tiles(o)
            part = self._alloc((ntile * 2 * o.cout,), F32)
            self._conv_into(o, y, 0, stats_part=part)
            if src is StatsSource.PARTIALS:
                self._emit(Lb.norm_reduce_partials, part.ptr, ntile, o.cout, o.sums.ptr, S)
            else:
                # group / instance norm on maps of at least 16 x 16: a pixel tile lies inside one sample, so the convolution's per-tile
                # sums reduce to per-sample sums without another pass over y (phx_norm_reduce_partials_ns)
                self._emit(Lb.norm_reduce_partials_ns, part.ptr, ntile // o.B, o.B, o.cout, o.sums.ptr, S)

    def _apply_xf(self, o, sv):
        """Every reader of a = relu(bn(y)) is a large-map 3x3 convolution (and its filter gradient): no apply pass, no tensor a --
        the statistics are finalised by a one-block launch and the readers transform y in their loaders (XfBuf)."""
        y, out = o.y, o.out
        if not (o.bw and o.stats is StatsSource.PARTIALS and o.training and o.act == rt.ACT_RELU and y.dt == BF16 and out.dt == BF16
                and not sv.head1x1 and _xf_enabled() and self._xf_edge_ok(o.op, o.B, o.H, o.Wd, o.cout)):
            return False
        self._emit(self.L.norm_finalize, o.sums.ptr, None, *o.params, sv.NS, sv.P, o.cout, sv.G, sv.mean.ptr, sv.rstd.ptr,
                   sv.scale.ptr, sv.shift.ptr, *o.moving, self.stream)
        self.val[o.op.outputs[0]] = XfBuf(out, y, sv.scale, sv.shift)
        sv.out = None
        return True

    def _apply_d2s(self, o, sv):
        """Phase form: y is in the packed pixel order, the readers of a want hi-res rows: the apply pass writes them (depth-to-space
        on the fly)."""
        if o.up is None:
            return False
        self._emit(self.L.norm_apply_fused_d2s, *o.apply_args, o.H // 2, o.Wd // 2, self.stream, tag="bytes_norm_apply",
                   flops=float(o.y.nbytes + o.out.nbytes))
        return True

    def _apply_head(self, o, sv):
        """The unit's only reader is a 1x1 head: it rides on the apply pass (phx_norm_apply_fused_head), no pass of its own over a."""
        y, out, op = o.y, o.out, o.op
        hop = self._norm_head_consumer(op) if (y.dt == BF16 and out.dt == BF16) else None
        if hop is None or not self.L.norm_head_supported(o.cout, hop.attrs["W"].shape[-1], y.dt, out.dt):
            return False
        hW, hb = hop.attrs["W"], hop.attrs["b"]
        yh = self._alloc_like(hop.outputs[0])
        self.val[hop.outputs[0]] = yh
        # training plan, batch norm: a itself is never written -- its one other reader, the head's filter gradient (a leaf of the
        # backward graph), re-forms it from y with this layer's scale / shift (phx_head1x1_wgrad_multi, xscale): for the
        # likelihood's top layer (128 channels @ 128 x 128) 268 MB less to write on the critical lane
        skip_a = bool(o.bw and sv.norm == "batch" and sv.NS == 1 and _SKIP_HEAD_A)
        args = o.apply_args
        if skip_a:
            args = args[:7] + (None,) + args[8:]
            sv.a_unwritten = dict(y=y, scale=sv.scale, shift=sv.shift, act=o.act)
        self._emit(self.L.norm_apply_fused_head, *args, self.store.ptr(hW), self.store.ptr(hb), hW.shape[-1], yh.ptr, self.stream,
                   tag="bytes_norm_apply", flops=float(y.nbytes + (0 if skip_a else out.nbytes)))
        self._norm_head[hop] = op
        return True

    def _apply_pool(self, o, sv):
        """One of the readers is averagepool2D (the next encoder level): the apply pass writes the pooled tensor too."""
        y, out = o.y, o.out
        pop = self._pool_consumer(o.op, o.H, o.Wd, o.cout) if (y.dt == BF16 and out.dt == BF16) else None
        if pop is None:
            return False
        pooled = self._alloc(self._cshape(pop.outputs[0]), out.dt)
        self.val[pop.outputs[0]] = pooled
        self._pool_done.add(pop)
        self._emit(self.L.norm_apply_pool, y.ptr, o.sums.ptr, o.pivot.ptr if o.pivot is not None else None, *o.params, out.ptr,
                   pooled.ptr, sv.mean.ptr, sv.rstd.ptr, sv.scale.ptr, sv.shift.ptr, *o.moving, sv.NS, sv.P, o.cout, sv.G, o.H, o.Wd, o.act,
                   self.stream, tag="bytes_norm_apply", flops=float(y.nbytes + out.nbytes + pooled.nbytes))
        return True

    def _apply_plain(self, o, sv):
        self._emit(self.L.norm_apply_fused, *o.apply_args, self.stream, tag="bytes_norm_apply", flops=float(o.y.nbytes + o.out.nbytes))
        return True

    def _fw_maxpool(self, op, bw):
        x = self.val[op.inputs[0]]
        out = self._alloc(self._cshape(op.outputs[0]), x.dt)
        self.val[op.outputs[0]] = out
        self._emit(self.L.maxpool2x2_fwd, x.ptr, x.dt, out.ptr, x.shape[0], x.shape[1], x.shape[2], x.shape[3], self.stream)

    @staticmethod
    def _pool2d_args(op, x):
        """(mode, B, H, W, C, kh, kw, sh, sw, pt, pl, Ho, Wo) of a pool2d node on its input buffer"""
        a, o = op.attrs, op.outputs[0].shape
        return ({"max": 0, "avg": 1}[a["mode"]], *x.shape, *a["window"], *a["strides"], *a["pad"], o[1], o[2])

    def _fw_pool2d(self, op, bw):
        x = self.val[op.inputs[0]]
        out = self._alloc(self._cshape(op.outputs[0]), x.dt)
        self.val[op.outputs[0]] = out
        self._emit(self.L.pool2d_fwd, x.ptr, x.dt, out.ptr, *self._pool2d_args(op, x), self.stream)

    def _fw_max_pool3d(self, op, bw):
        x = self.val[op.inputs[0]]
        out = self._alloc(self._cshape(op.outputs[0]), x.dt)
        self.val[op.outputs[0]] = out
        self._emit(self.L.maxpool3d_fwd, x.ptr, x.dt, out.ptr, *x.shape, *op.attrs["window"], self.stream)

    def _fw_bilinear_up3d(self, op, bw):
        x = self.val[op.inputs[0]]
        out = self._alloc(self._cshape(op.outputs[0]), x.dt)
        self.val[op.outputs[0]] = out
        self._emit(self.L.bilinear_up2x_3d_fwd, x.ptr, x.dt, out.ptr, *x.shape, self.stream)

    def _fw_spatial_window3d(self, op, bw):
        x = self.val[op.inputs[0]]
        out = self._alloc(self._cshape(op.outputs[0]), x.dt)
        self.val[op.outputs[0]] = out
        self._emit(self.L.spatial_window3d, x.ptr, out.ptr, x.dt, *x.shape[:4], *out.shape[1:4], x.shape[4], *op.attrs["off"], self.stream)

    def _fw_fold_depth(self, op, bw):
        x = self.val[op.inputs[0]]
        self.val[op.outputs[0]] = Buf(self._cshape(op.outputs[0]), x.dt, like=x.t)      # same memory, new shape

    def _fw_spatial_window(self, op, bw):
        x = self.val[op.inputs[0]]
        out = self._alloc(self._cshape(op.outputs[0]), x.dt)
        self.val[op.outputs[0]] = out
        oy, ox = op.attrs["off"]
        self._emit(self.L.spatial_window, x.ptr, out.ptr, x.dt, x.shape[0], x.shape[1], x.shape[2], out.shape[1], out.shape[2],
                   x.shape[3], oy, ox, self.stream)

    def _dropout_on(self, op):
        tr = op.attrs["training"]
        return (tr if isinstance(tr, bool) else self.training) and op.attrs["keep_prob"] < 1.0

    def _fw_dropout(self, op, bw):
        x = self.val[op.inputs[0]]
        if not self._dropout_on(op):
            self.val[op.outputs[0]] = x                      # inference: identity (layers.py:659-661)
            return
        out = self._alloc(x.shape, x.dt)
        self.val[op.outputs[0]] = out
        self._emit(self.L.dropout, x.ptr, out.ptr, x.dt, x.n // x.shape[0], x.shape[0], op.attrs["keep_prob"], self.rng_seed,
                   self._noise_step_ptr(), op.attrs["stream"], self.sample_offset, self.stream)

    def _fw_window4(self, op, bw):
        x = self.val[op.inputs[0]]
        out = self._alloc(self._cshape(op.outputs[0]), x.dt)
        self.val[op.outputs[0]] = out
        (sy, sx), (oy, ox, oc) = op.attrs["stride"], op.attrs["off"]
        self._emit(self.L.window4_fwd, x.ptr, out.ptr, x.dt, x.shape[0], x.shape[1], x.shape[2], x.shape[3], out.shape[1],
                   out.shape[2], out.shape[3], sy, sx, oy, ox, oc, self.stream)

    def _fw_add_act(self, op, bw):
        a, b = self.val[op.inputs[0]], self.val[op.inputs[1]]
        out = self._alloc(a.shape, a.dt)
        self.val[op.outputs[0]] = out
        b = self._as_dt(b, a.dt)
        self._emit(self.L.add_act, a.ptr, b.ptr, out.ptr, a.dt, a.n, rt.ACT_CODES[op.attrs["act"]], self.stream)

    def _fw_leaky_relu(self, op, bw):
        """max(x, alpha x) into a buffer of the node's own: the producer's output stays as it is for its other readers, a fetch and the
        producer's own backward."""
        x = self.val[op.inputs[0]]
        if not isinstance(x, Buf) or x.shift:
            raise NotImplementedError("leaky_relu %s: its input is not a stored tensor (%s)" % (op.name, type(x).__name__))
        out = self._alloc(x.shape, x.dt)
        self.val[op.outputs[0]] = out
        self._emit(self.L.leaky_relu_fwd, x.ptr, x.dt, out.ptr, out.dt, x.n, op.attrs["alpha"], self.stream)

    def _fw_norm_act(self, op, bw):
        """Stand-alone act(normalisation(x)): statistics pass + fused apply (the generic path of the convolution units)."""
        a = op.attrs
        x = self.val[op.inputs[0]]
        out = self._alloc(x.shape, x.dt)
        self.val[op.outputs[0]] = out
        vol = ("norm",) if len(x.shape) == 5 else None
        if vol is not None:                      # a volume: the same memory as [B, D H, W, C]
            x = Buf(self._folded(x.shape), x.dt, like=x.t)
        B, C = x.shape[0], x.shape[3]
        HW = x.shape[1] * x.shape[2]
        act = rt.ACT_CODES[a["act"]]
        training = a["training"] if isinstance(a["training"], bool) else self.training
        norm = self._lowered_norm(a, training)
        sv = self.saved[op] = ConvSaved.plain(x, out, norm, C, volume=vol)
        if norm is None:
            ones = Buf((C,), F32, like=torch.ones(C, dtype=torch.float32, device=_device()))
            zeros = Buf((C,), F32, like=torch.zeros(C, dtype=torch.float32, device=_device()))
            self._keep += [ones, zeros]
            self._emit(self.L.affine_act, x.ptr, x.dt, ones.ptr, zeros.ptr, out.ptr, out.dt, 1, B * HW, C, act, self.stream)
            return
        sv.y = x
        self._norm_vectors(sv, B, HW, C, a["num_groups"])
        sv.route = NormRoute.INFER if (norm == "batch" and not training) else (NormRoute.LAYER if norm == "layer" else NormRoute.GENERIC)
        self._norm_fwd(sv, a, x, out, C, act, training)
        self._moving_biased(sv, a, C, training)

    def _fw_flatten(self, op, bw):
        x = self.val[op.inputs[0]]
        self.val[op.outputs[0]] = Buf(self._cshape(op.outputs[0]), x.dt, like=x.t)      # same memory, new shape

    def _pool_consumer(self, op, H, Wd, C):
        """The averagepool2D op that reads this conv unit's output directly, on the same lane, on an even map -- or None."""
        if not _POOL_FUSE or not self.L.norm_apply_pool_supported(H, Wd, C):
            return None
        out = op.outputs[0]
        ln = self.op_lane.get(op)
        for c in self._real_consumers(out, self._opset):
            if c.type == "avgpool" and c.inputs[0] is out and self.op_lane.get(c) == ln and c not in self._pool_done:
                # the pool then emits no launch of its own and records no forward event: every reader of the pooled tensor has to sit
                # on the producer's lane too (stream order is its only ordering), and the pooled tensor may not be a fetch
                if c.outputs[0] in self.fetches or any(self.op_lane.get(r) != ln for r in self._real_consumers(c.outputs[0], self._opset)):
                    continue
                return c
        return None

    def _fw_avgpool(self, op, bw):
        if op in self._pool_done:                # the producer's apply pass wrote it (phx_norm_apply_pool)
            return
        x = self.val[op.inputs[0]]
        out = self._alloc(self._cshape(op.outputs[0]), x.dt)
        self.val[op.outputs[0]] = out
        self._emit(self.L.avgpool2x2_fwd, x.ptr, x.dt, out.ptr, x.shape[0], x.shape[1], x.shape[2], x.shape[3],
                   self.stream)

    def _upconv_consumer(self, op, x, bw):
        """The 3x3 conv unit (batch norm, training plan) that is the ONLY reader of this resize and runs in the phase form -- or None."""
        mh = _upconv_min_h()
        if not (mh > 0 and bw and self.loss is not None and self.act_dt == BF16 and isinstance(x, Buf) and x.dt == BF16 and len(x.shape) == 4):
            return None
        ot = op.outputs[0]
        cons = self._real_consumers(ot, self._opset)
        # (the small-map forms of _fw_conv_unit -- one-launch batch norm, fused group norm, wave-per-sample norm: maps up to 16 x 16 --
        # read x.ptr and an UpBuf has none: the phase form starts at 32 x 32 low-resolution maps whatever PHX_UPCONV says)
        if len(cons) != 1 or ot in self.fetches or x.shape[1] < max(mh, 32) or x.shape[2] < max(mh, 32):
            return None
        c = cons[0]
        a = c.attrs if c.type == "conv_unit" else None
        if (a is None or c.inputs[0] is not ot or a["ksize"] != 3 or a.get("transposed") is not None or a.get("general") is not None or a.get("volume") is not None or a.get("explicit") is not None
                or a["norm"] not in ("batch", "group", "instance") or (a["norm"] == "batch") != (a["b"] is None)
                or self.op_lane.get(c) != self.op_lane.get(op) or c in self._lat):
            return None
        training = a["training"] if isinstance(a["training"], bool) else self.training
        cin, cout = a["W"].shape[-2], a["W"].shape[-1]
        if not training or cin != x.shape[3] or not self.L.upconv_supported(x.shape[0], x.shape[1], x.shape[2], cin, cout):
            return None
        # Measured per edge at batch 64 (profiles/r05_ab_upconv.txt): 192 -> 32 from 64 x 64 + 1.0 % of the step; 192 -> 64 from 32 x 32 - 1.3 %,
        # 32 -> 32 from 64 x 64 - 1 % (the form trades the 4 Cin-channel hi-res tensor for ten more launches and a 4 Cout-column filter
        # gradient: it pays where the up-sampled tensor dominates the layer's bytes)
        if cin < 4 * cout:
            return None
        return c

    def _fw_bilinear_up(self, op, bw):
        x = self.val[op.inputs[0]]
        if self._upconv_consumer(op, x, bw) is not None:
            # no launch, no hi-res tensor: the reader convolves the low-resolution map with the phase filters (_fw_conv_unit, upconv.py)
            self.val[op.outputs[0]] = UpBuf(x, self._cshape(op.outputs[0]))
            return
        out = self._alloc(self._cshape(op.outputs[0]), x.dt)
        self.val[op.outputs[0]] = out
        self._emit(self.L.bilinear_up2x_fwd, x.ptr, x.dt, out.ptr, x.shape[0], x.shape[1], x.shape[2], x.shape[3],
                   self.stream)

    def _fw_add(self, op, bw):
        if op.outputs[0] in self.fed:
            # a fed latent: an F32 feed buffer stands for z, its readers (bilinear up-sampling, the likelihood's first convolutions) read
            # it like a computed one; mu / sigma / the noise above it are not part of this plan unless something else needs them
            t = op.outputs[0]
            z = self._alloc(self._cshape(t), F32, zero=True)
            self.val[t] = z
            self.feeds[t] = z
            return
        mu_t, m = op.inputs
        if m.op.type != "mul" or m.op.inputs[1].op.type != "random_normal":
            raise NotImplementedError("only z = mu + sigma * random_normal(...) is on the hot path")
        rec = self._lat.get(op)
        if rec is not None:
            self.val[op.outputs[0]] = self._alloc(self.val[mu_t].shape, F32)
            self.saved[op] = dict(latent=True)
            if rec["last"] is op:
                self._fw_latent_group(rec)
            return
        sigma_t, eps_t = m.op.inputs
        mu, sigma = self.val[mu_t], self.val[sigma_t]
        z = self._alloc(mu.shape, F32)
        self.val[op.outputs[0]] = z
        per = mu.n // mu.shape[0]
        stream_id = eps_t.op.attrs["stream"]
        self._emit(self.L.reparam_fwd, mu.ptr, sigma.ptr, z.ptr, mu.shape[0], per, self.rng_seed,
                   self._noise_step_ptr(), stream_id, self.sample_offset, self.stream)
        self.saved[op] = dict(mu_t=mu_t, sigma_t=sigma_t, per=per, stream_id=stream_id)

    def _fw_tile_batch(self, op, bw):
        x = self.val[op.inputs[0]]
        out = self._alloc(self._cshape(op.outputs[0]), x.dt)
        self.val[op.outputs[0]] = out
        n = op.attrs["tile"]
        assert out.shape[0] == x.shape[0] * n
        per = x.n // x.shape[0]
        if (per * _ESIZE[x.dt]) % 16 and x.dt == F32:
            # rows that are no multiple of 16 bytes (prob_unet2D's mu / sigma: [B, zdim]): out[b][k][:] = x[b][:] is the pixel broadcast with
            # n "pixels" per row
            self._emit(self.L.broadcast_pixels_fwd, x.ptr, out.ptr, F32, x.shape[0], n, per, self.stream)
            return
        self._emit(self.L.repeat_batch, x.ptr, out.ptr, x.shape[0], (x.n // x.shape[0]) * _ESIZE[x.dt], n, self.stream)

    def _fw_global_avgpool(self, op, bw):
        x = self._as_dt(self.val[op.inputs[0]], F32)
        out = self._alloc_like(op.outputs[0])
        self.val[op.outputs[0]] = out
        self._emit(self.L.global_avgpool_fwd, x.ptr, out.ptr, x.shape[0], x.shape[1] * x.shape[2], x.shape[3],
                   self.stream)

    def _fw_tile_pixels(self, op, bw):
        z = self.val[op.inputs[0]]
        out = self._alloc_like(op.outputs[0])
        self.val[op.outputs[0]] = out
        self._emit(self.L.broadcast_pixels_fwd, z.ptr, out.ptr, out.dt, out.shape[0], out.shape[1] * out.shape[2],
                   out.shape[3], self.stream)

    def _level_args(self, tensors):
        bufs = [self.val[t] for t in tensors]
        for b in bufs:
            assert b.dt == F32, "logit levels are fp32 heads"
        return bufs, rt.ptr_array([b.ptr for b in bufs]), rt.int_array([b.shift for b in bufs])

    def _fw_residual_ce(self, op, bw):
        Ls = op.attrs["L"]
        s_t, lab_t = op.inputs[:Ls], op.inputs[Ls]
        bufs, sp, shp = self._level_args(s_t)
        lab = self.val[lab_t]
        B, H, W = lab.shape
        C = bufs[0].shape[3]
        losses = self._alloc((8 + 512,), F32)
        s_out = self._alloc_like(op.outputs[Ls])
        self.val[op.outputs[Ls]] = s_out
        for l in range(Ls):
            v = Buf((), F32, like=losses.t[l:l + 1])
            self._keep.append(v)
            self.val[op.outputs[l]] = v
        dsp, dbufs, w = None, None, 0.0
        if bw:
            ws = [self.loss_weight.get(op.outputs[l], 0.0) for l in range(Ls)]
            assert all(abs(x - ws[0]) < 1e-12 for x in ws), "one weight for all residual-CE levels"
            w = ws[0]
            dbufs = []
            for b in bufs:
                if b.shape[1] != H:        # coarse levels are accumulated atomically -> zero every run
                    zb = self._alloc_zeroed(b.n)
                    zb.shape = b.shape
                    dbufs.append(zb)
                else:
                    dbufs.append(self._alloc(b.shape, F32))
            dsp = rt.ptr_array([b.ptr for b in dbufs])
            self.saved[op] = dict(dbufs=dbufs, src=[t.op.inputs[0] if t.op.type == "nn_resize" else t for t in s_t])
        if many_class.residual_ce_entry(C) == "residual_ce":
            self._emit(self.L.residual_ce, sp, dsp, shp, Ls, lab.ptr, B, H, W, C, w, self.inv_batch, losses.ptr,
                       s_out.ptr, None, self.stream)
        else:
            wsb = int(self.L.residual_ce_wide_ws_bytes(B, H, W))
            work = self._alloc((wsb // 4,), F32)
            self._emit(self.L.residual_ce_wide, sp, dsp, shp, Ls, lab.ptr, B, H, W, C, w, self.inv_batch, losses.ptr,
                       s_out.ptr, None, work.ptr, wsb, self.stream)

    def _fw_aggregate(self, op, bw):
        Ls = op.attrs["L"]
        bufs, sp, shp = self._level_args(op.inputs)
        s_out, sm = self._alloc_like(op.outputs[0]), self._alloc_like(op.outputs[1])
        self.val[op.outputs[0]], self.val[op.outputs[1]] = s_out, sm
        B, H, W, C = s_out.shape
        if many_class.residual_ce_entry(C) == "residual_ce":
            self._emit(self.L.residual_ce, sp, None, shp, Ls, None, B, H, W, C, 0.0, 1.0, None, s_out.ptr, sm.ptr,
                       self.stream)
        else:
            self._emit(self.L.residual_ce_wide, sp, None, shp, Ls, None, B, H, W, C, 0.0, 1.0, None, s_out.ptr, sm.ptr,
                       None, 0, self.stream)

    def _fw_xent_map(self, op, bw):
        lg, lab = self.val[op.inputs[0]], self.val[op.inputs[1]]
        assert lg.dt == F32 and lg.shift == 0, "eval_xent reads the summed full-resolution logits"
        out = self._alloc_like(op.outputs[0])
        self.val[op.outputs[0]] = out
        self._emit(getattr(self.L, many_class.xent_map_entry(lg.shape[-1])), lg.ptr, lab.ptr, out.ptr, out.n, lg.shape[-1], self.stream)

    # ---- tfwrapper/losses.py (csrc/seg_losses.hip) ------------------------------------------------------------------------------
    def _seg_loss_args(self, op):
        lg, lab = self.val[op.inputs[0]], self.val[op.inputs[1]]
        assert lg.dt == F32 and lg.shift == 0 and lab.dt == U8, "segmentation losses read full-resolution fp32 logits and u8 labels"
        return lg, lab, lg.shape

    def _dice_launches(self, op, table, loss, coef):
        """The sums pass and the finishing launch of one Dice operator."""
        a = op.attrs
        if a["sum_over_batches"] and self.dist_active:
            raise NotImplementedError("%s: a batch-summed Dice (macro_robust / sum_over_batches=True) needs a collective over the ranks' "
                                      "sums, which data-parallel plans do not have" % op.name)
        lg, lab, (B, H, W, C) = self._seg_loss_args(op)
        wsb = int(self.L.dice_ws_bytes(B, H, W, C))
        ws = self._alloc((wsb // 4,), F32)
        self._emit(self.L.dice_sums, lg.ptr, lab.ptr, ws.ptr, wsb, B, H, W, C, self.stream)
        self._emit(self.L.dice_finish, ws.ptr, wsb, B, H, W, C, int(a.get("use_hard_pred", False)), int(a["sum_over_labels"]),
                   int(a["sum_over_batches"]), int(a.get("only_foreground", False)), a["epsilon"], self.inv_batch,
                   table.ptr if table is not None else None, loss.ptr if loss is not None else None,
                   coef.ptr if coef is not None else None, self.stream)

    def _fw_dice_loss(self, op, bw):
        out = self._alloc((), F32)
        self.val[op.outputs[0]] = out
        B, _, _, C = self.val[op.inputs[0]].shape
        w = self.loss_weight.get(op.outputs[0], 0.0) if bw else 0.0
        coef = self._alloc((B * C * 2,), F32) if (w != 0.0 and self.req.get(op.inputs[0], False)) else None
        self._dice_launches(op, None, out, coef)
        if coef is not None:
            self.saved[op] = dict(coef=coef, gscale=w)

    def _fw_dice_table(self, op, bw):
        if op.outputs[0] in self.loss_weight:
            raise ValueError("%s: get_dice is a fetch-only table without a gradient; use dice_loss as a loss term" % op.name)
        out = self._alloc_like(op.outputs[0])
        self.val[op.outputs[0]] = out
        self._dice_launches(op, out, None, None)

    def _fw_seg_xent(self, op, bw):
        lg, lab, (B, H, W, C) = self._seg_loss_args(op)
        out = self._alloc((), F32)
        self.val[op.outputs[0]] = out
        cw = None
        if op.attrs["class_weights"] is not None:
            cw = self._alloc((C,), F32)
            cw.t.copy_(torch.tensor(op.attrs["class_weights"], dtype=torch.float32))
            device_sync()
        w = self.loss_weight.get(op.outputs[0], 0.0) if bw else 0.0
        d = self._alloc(lg.shape, F32) if (w != 0.0 and self.req.get(op.inputs[0], False)) else None
        wsb = int(self.L.seg_xent_ws_bytes(B, H, W, C))
        ws = self._alloc((wsb // 4,), F32)
        self._emit(self.L.seg_xent, lg.ptr, lab.ptr, cw.ptr if cw is not None else None, int(op.attrs["use_sigmoid"]), self.inv_batch,
                   w, 0, out.ptr, d.ptr if d is not None else None, ws.ptr, wsb, B, H, W, C, self.stream)
        if d is not None:
            self.saved[op] = dict(d=d)

    def _fw_kl(self, op, bw):
        mu0, s0, mu1, s1 = [self.val[t] for t in op.inputs]
        grp = self._kl_group
        if grp is not None and op in grp["ops"]:
            # every level of the hierarchical KL term in ONE launch, emitted at the last level's operator (phx_kl_diag_gauss_multi);
            # the loss scalars live in the per-step zero arena (accumulated atomically: no memset node per level)
            loss = self._alloc_zeroed(1)
            loss.shape = ()
            self.val[op.outputs[0]] = loss
            gs = [self._alloc(mu0.shape, F32) for _ in range(4)] if bw else [None] * 4
            if bw:
                self.saved[op] = dict(gs=gs)
            grp["recs"].append((mu0, s0, mu1, s1, gs, loss, op.attrs["level_weight"]))
            if op is grp["ops"][-1]:
                recs = grp["recs"]
                ptrs = rt.ptr_array([p for r in recs for p in ([r[0].ptr, r[1].ptr, r[2].ptr, r[3].ptr] +
                                                               [g.ptr if g is not None else None for g in r[4]] + [r[5].ptr])])
                ns = (ctypes.c_size_t * len(recs))(*[r[0].n for r in recs])
                lws = (ctypes.c_float * len(recs))(*[r[6] for r in recs])
                self._keep += [ptrs, ns, lws]
                self._emit(self.L.kl_diag_gauss_multi, ptrs, ctypes.cast(ns, ctypes.c_void_p), ctypes.cast(lws, ctypes.c_void_p), len(recs),
                           self.inv_batch, grp["gscale"] if bw else 0.0, self.stream)
            return
        loss = self._alloc((), F32)
        self.val[op.outputs[0]] = loss
        gs = [None] * 4
        gscale = 0.0
        if bw:
            gscale = self.loss_weight.get(op.outputs[0], 0.0)
            gs = [self._alloc(mu0.shape, F32) for _ in range(4)]
            self.saved[op] = dict(gs=gs)
        self._emit(self.L.kl_diag_gauss, mu0.ptr, s0.ptr, mu1.ptr, s1.ptr, mu0.n, op.attrs["level_weight"],
                   self.inv_batch, gscale, loss.ptr, *[g.ptr if g is not None else None for g in gs], self.stream)

    def _fw_weighted_sum(self, op, bw):
        out = self._alloc((), F32)
        self.val[op.outputs[0]] = out
        ptrs = rt.ptr_array([self.val[t].ptr for t in op.inputs])
        ws = (ctypes.c_float * len(op.inputs))(*op.attrs["weights"])
        self._keep.append(ws)
        self._emit(self.L.weighted_sum, ptrs, ctypes.cast(ws, ctypes.c_void_p), len(op.inputs), out.ptr, self.stream)
