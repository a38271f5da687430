"""Reverse-mode backward pass of the plan (engine.Plan mixin): one `_bw_<op type>` method per operator type emits the launches that
turn the gradient of the operator's outputs into gradients of its inputs and variables -- what `optimizer.minimize` derives in the
reference (phiseg/phiseg_model.py:135-141) -- plus the gradient bookkeeping (`_add_grad`, `_finalize_grad`)."""
import ctypes

import numpy as np

from phiseg_code_amd import runtime as rt
from phiseg_code_amd import upconv
from phiseg_code_amd.engine_common import *  # noqa: F401,F403
from phiseg_code_amd.engine_common import _HEAD_RIDER_NOUT, _BN_SMALL, _BN_SMALL_F32, _BN_WIDE, _BN_WIDE_MAXLINES, _DETERMINISTIC, _NREP, _NREP_MINP, _fgn_mode, _dual_enabled, _noop, _device, _TORCH_DT, _NP_DT, _ESIZE, _LIK_SIDE_MAXLVL, _WGRAD_DEFER_BLOCKS, _STAMPS  # noqa: F401


class BackwardLowering:
    def _bw_l2_weights(self, op):
        st = self.store
        self._emit(self.L.axpy_masked, st.grads.data_ptr(), st.params.data_ptr(), st.decay_mask.data_ptr(), st.n_train,
                   float(self._l2_weight), self.stream)

    def _bw_latent_group(self, rec):
        """Called at the group's LAST operator (the first one the backward sweep meets): every contribution to the gradients of mu,
        sigma and z has been registered by then (their readers come later in the forward order)."""
        mu_op, sig_op, add_op = rec["mu"], rec["sig"], rec["add"]
        mu_t, sig_t = mu_op.outputs[0], sig_op.outputs[0]
        for t in (mu_t, sig_t):
            if t in self.grad:
                self._finalize_grad(t)
        dz = self.grad.get(add_op.outputs[0]) if add_op is not None else None
        dmu, dsg = self.grad.get(mu_t), self.grad.get(sig_t)
        for o in (mu_op, sig_op, add_op):
            if o is not None:
                self._bw_skip.add(o)
        if dz is None and dmu is None and dsg is None:
            return
        x_t = rec["x"]
        x, sigma = self.val[x_t], self.val[sig_t]
        npix, cin, zd = rec["npix"], rec["cin"], rec["zd"]
        gmu, gsig = self._alloc((npix, zd), F32), self._alloc((npix, zd), F32)
        st, Lb = self.store, self.L
        wmu, wsg = mu_op.attrs["W"], sig_op.attrs["W"]
        if not self.req.get(x_t, False):
            raise NotImplementedError("latent heads on a tensor without gradient")

        def wr(g):
            self._emit(Lb.latent_heads_bwd, dz.ptr if dz is not None else None, dmu.ptr if dmu is not None else None,
                       dsg.ptr if dsg is not None else None, sigma.ptr, st.ptr(wmu), st.ptr(wsg), g.ptr, g.dt, gmu.ptr, gsig.ptr, npix,
                       cin, zd, rec["hw"], self.rng_seed, self._noise_step_ptr(), rec["sid"], self.sample_offset, self.stream)
        self._add_grad(x_t, write_fn=wr)
        for hop, gy in ((mu_op, gmu), (sig_op, gsig)):      # the two filter / bias gradients: leaves, one launch for all heads later
            W, b = hop.attrs["W"], hop.attrs["b"]
            if cin % 8 == 0:
                plan4 = (ctypes.c_int * 4)()
                Lb.head1x1_wgrad_plan(npix, cin, zd, plan4)
                self._headw_jobs.setdefault((x.dt, zd), []).append((x.ptr, gy.ptr, st.grad_ptr(W), st.grad_ptr(b), npix, cin, plan4[0],
                                                                    plan4[1], plan4[2], plan4[3]))
            else:
                self._emit(Lb.head1x1_wgrad, x.ptr, x.dt, gy.ptr, st.grad_ptr(W), st.grad_ptr(b), npix, cin, zd, self.stream)

    def _bw_tile_batch(self, op):
        raise NotImplementedError("tile_batch is part of the sampling path only")

    # ---- backward -------------------------------------------------------------------------------
    def _add_grad(self, t, write_fn=None, buf=None, accum_fn=None):
        """Accumulate a gradient contribution for tensor t: either `buf` (already complete) or produced by
        write_fn(target).  The first contribution owns the buffer; later ones are added in place -- by accum_fn(owner buffer) when
        the contributing kernel has an accumulating form (no buffer of its own, no add pass), else by phx_add_inplace."""
        if not self.req.get(t, False):
            return
        if accum_fn is not None and t in self.grad:
            g = self.grad[t]
            own = [evl for b, evl in self.pending.get(t, []) if b is g]
            # (only behind contributions of THIS lane: waiting here for another lane's write would tie the two backward chains
            # together early -- measured 3 % slower than leaving that contribution in a buffer of its own for the finaliser)
            if g.dt == self.val[t].dt and own and all(evl is None or evl[1] == self._lane for evl in own):
                accum_fn(g)
                evl = self._record(self._lane) if len(self._lanes) > 1 else None
                self.pending[t].append((g, evl))             # (same buffer: the finaliser only waits for it)
                return
        if buf is None:
            buf = self._alloc(self.val[t].shape, self.val[t].dt)
            write_fn(buf)
        if t not in self.grad:
            self.grad[t] = buf
        # the producer's backward (possibly on another lane) folds this contribution in: _finalize_grad
        evl = self._record(self._lane) if len(self._lanes) > 1 else None
        self.pending.setdefault(t, []).append((buf, evl))

    def _slice_grad_ok(self, op, xin, B, H, Wd, K, N):
        """May the data gradient of convolution `op` (reduction channels K = its Cout, N = its Cin) hand its split-K slices to the
        producer of its input?  -- that producer is a one-launch wide batch-norm layer, this convolution is the input's ONLY
        reader (so the slices are the whole gradient), on the same lane, nobody fetches the gradient, and the launch does run split-K."""
        if _BN_WIDE < 2 or xin in self.fetches or self.act_dt != BF16:
            return False
        prod = self._real_producer(xin)
        if prod is None or prod.type != "conv_unit" or getattr(self.saved.get(prod), "route", None) is not NormRoute.BN_WIDE or prod.outputs[0] is not xin:
            return False
        if self.op_lane.get(prod) != self.op_lane.get(op):
            return False
        cons = self._real_consumers(xin, self._opset)
        if len(cons) != 1 or cons[0] is not op or xin in self.grad or self.pending.get(xin):
            return False
        nzd = int(self.L.conv3x3_mfma_ksplit(B, H, Wd, K, N))
        return nzd > 1 and B * H * Wd * nzd <= _BN_WIDE_MAXLINES

    def _real_producer(self, t):
        """Producer op whose launches create the data behind tensor t (looks through launch-less view ops)."""
        op = t.op
        while op is not None and op.type in self._VIRTUAL and op.inputs:
            op = op.inputs[0].op
        return op

    def _real_consumers(self, t, opset):
        out = []
        for c in t.consumers:
            if c not in opset:
                continue
            if c.type in self._VIRTUAL:
                for o in c.outputs:
                    out.extend(self._real_consumers(o, opset))
            else:
                out.append(c)
        return out

    def _finalize_grad(self, t):
        """Called on the producer's lane before its backward: wait for every contribution to grad[t] (they were
        written on the consumers' lanes) and fold the late ones into the primary buffer."""
        for buf, evl in self.pending.pop(t, []):
            self._wait(evl)
            g = self.grad[t]
            if buf is not g:
                assert g.dt == buf.dt and g.n == buf.n
                self._emit(self.L.add_inplace, g.ptr, buf.ptr, g.n, g.dt, self.stream)

    def _bw_placeholder(self, op):
        pass


    _bw_one_hot = _bw_sub_const = _bw_random_normal = _bw_mul = _bw_weighted_sum = _bw_constant = _bw_dice_table = _bw_placeholder

    def _resize_adjoint(self, dfine, dst, add):
        """dst (a coarse level's gradient, [B, h, w, C] fp32) = / += the 2^s x 2^s block sums of the full-resolution dfine."""
        B, h, w, C = dst.shape
        assert dfine.dt == F32 and dst.dt == F32 and dfine.shape[1] % h == 0
        self._emit(self.L.nn_resize_adjoint, dfine.ptr, dst.ptr, B, h, w, C, (dfine.shape[1] // h).bit_length() - 1, int(add), self.stream)

    def _bw_nn_resize(self, op):
        """Adjoint of the nearest-neighbour view: a FULL-resolution gradient on the resized tensor -> block sums on the stored one
        (a factor-1 view -- the finest level of likelihoods.phiseg -- hands the buffer on)."""
        d, src = self.grad[op.outputs[0]], self.val[op.inputs[0]]
        if op.attrs["shift"] == 0:
            return self._add_grad(op.inputs[0], buf=d)
        assert d.shape[1] == src.shape[1] << op.attrs["shift"], "the gradient of a resized tensor is taken at full resolution"
        self._add_grad(op.inputs[0], write_fn=lambda g: self._resize_adjoint(d, g, False), accum_fn=lambda g: self._resize_adjoint(d, g, True))

    def _bw_residual_ce(self, op):
        sv = self.saved.get(op)
        if sv:
            g = self.grad.get(op.outputs[op.attrs["L"]])
            if g is not None:
                # a third-party term (dice_loss, seg_xent) on the summed output s_out = sum_l resize(s_l): its gradient reaches every
                # level -- added into the buffers this operator's own gradient sits in, before they are passed on
                for d in sv["dbufs"]:
                    if d.shape[1] == g.shape[1]:
                        self._emit(self.L.add_inplace, d.ptr, g.ptr, d.n, F32, self.stream)
                    else:
                        self._resize_adjoint(g, d, True)
            for t, d in zip(sv["src"], sv["dbufs"]):
                self._add_grad(t, buf=d)

    def _bw_aggregate(self, op):
        """s_out = sum_l resize(s_l): a gradient on the summed logits goes to level 0 as it is and to the coarser levels through the
        resize adjoint.  (The coarse levels first: the level-0 contribution shares g's buffer, which later contributions may add to.)"""
        if op.outputs[1] in self.grad:
            raise NotImplementedError("no backward through the soft-max output of aggregate_logits: take the loss on the logits")
        g = self.grad.get(op.outputs[0])
        if g is None:
            return
        src = [t.op.inputs[0] if t.op.type == "nn_resize" else t for t in op.inputs]
        order = sorted(range(len(src)), key=lambda l: self.val[op.inputs[l]].shift == 0)
        for l in order:
            if self.val[op.inputs[l]].shift == 0:
                self._add_grad(src[l], buf=g)
            else:
                self._add_grad(src[l], write_fn=lambda d: self._resize_adjoint(g, d, False), accum_fn=lambda d: self._resize_adjoint(g, d, True))

    def _bw_dice_loss(self, op):
        sv = self.saved.get(op)
        if sv:
            lg, lab = self.val[op.inputs[0]], self.val[op.inputs[1]]
            B, H, W, C = lg.shape

            def emit(g, add):
                self._emit(self.L.dice_grad, lg.ptr, lab.ptr, sv["coef"].ptr, sv["gscale"], add, g.ptr, B, H, W, C, self.stream)
            self._add_grad(op.inputs[0], write_fn=lambda g: emit(g, 0), accum_fn=lambda g: emit(g, 1))

    def _bw_seg_xent(self, op):
        sv = self.saved.get(op)
        if sv:
            self._add_grad(op.inputs[0], buf=sv["d"])

    def _bw_kl(self, op):
        sv = self.saved.get(op)
        if sv:
            for t, g in zip(op.inputs, sv["gs"]):
                self._add_grad(t, buf=g)

    def _bw_add(self, op):
        if op in self._lat:
            return self._bw_latent_group(self._lat[op])
        sv, dz = self.saved[op], self.grad[op.outputs[0]]
        self._add_grad(sv["mu_t"], buf=dz)
        B = dz.shape[0]

        def wr(target):
            self._emit(self.L.reparam_bwd, dz.ptr, target.ptr, B, sv["per"], self.rng_seed,
                       self._noise_step_ptr(), sv["stream_id"], self.sample_offset, self.stream)
        self._add_grad(sv["sigma_t"], write_fn=wr)

    def _bw_concat(self, op):
        a, b = op.inputs
        d = self.grad[op.outputs[0]]
        if b.op.type == "sub_const":
            return                       # posterior input: x and s are data
        npix = int(np.prod(d.shape[:-1]))
        ca, cb = self.val[a].shape[-1], self.val[b].shape[-1]
        da = self._alloc(self.val[a].shape, d.dt) if self.req.get(a) else None
        db = self._alloc(self.val[b].shape, d.dt) if self.req.get(b) else None
        self._emit(self.L.split2, d.ptr, da.ptr if da else None, ca, db.ptr if db else None, cb, npix, d.dt,
                   self.stream)
        for t, g in ((a, da), (b, db)):
            if g is not None:
                self._add_grad(t, buf=self._as_dt(g, self.val[t].dt))

    def _bw_maxpool(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(
            self.L.maxpool2x2_bwd, x.ptr, d.ptr, d.dt, g.ptr, x.shape[0], x.shape[1], x.shape[2], x.shape[3], self.stream))

    def _bw_max_pool3d(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(
            self.L.maxpool3d_bwd, x.ptr, d.ptr, d.dt, g.ptr, *x.shape, *op.attrs["window"], self.stream))

    def _bw_bilinear_up3d(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(self.L.bilinear_up2x_3d_bwd, d.ptr, d.dt, g.ptr, *x.shape, self.stream),
                       accum_fn=(lambda g: self._emit(self.L.bilinear_up2x_3d_bwd_acc, d.ptr, d.dt, g.ptr, *x.shape, self.stream))
                       if d.dt == x.dt else None)

    def _bw_spatial_window3d(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        oz, oy, ox = op.attrs["off"]
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(
            self.L.spatial_window3d, d.ptr, g.ptr, d.dt, x.shape[0], *d.shape[1:4], *x.shape[1:4], x.shape[4], -oz, -oy, -ox, self.stream))

    def _bw_fold_depth(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        self._add_grad(op.inputs[0], buf=Buf(x.shape, d.dt, like=d.t))

    def _bw_spatial_window(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        oy, ox = op.attrs["off"]
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(
            self.L.spatial_window, d.ptr, g.ptr, d.dt, x.shape[0], d.shape[1], d.shape[2], x.shape[1], x.shape[2], x.shape[3],
            -oy, -ox, self.stream))

    def _bw_dropout(self, op):
        d = self.grad[op.outputs[0]]
        if not self._dropout_on(op):
            self._add_grad(op.inputs[0], buf=d)
            return
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(
            self.L.dropout, d.ptr, g.ptr, d.dt, d.n // d.shape[0], d.shape[0], op.attrs["keep_prob"], self.rng_seed,
            self._noise_step_ptr(), op.attrs["stream"], self.sample_offset, self.stream))

    def _bw_window4(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        (sy, sx), (oy, ox, oc) = op.attrs["stride"], op.attrs["off"]
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(
            self.L.window4_bwd, d.ptr, g.ptr, d.dt, x.shape[0], x.shape[1], x.shape[2], x.shape[3], d.shape[1], d.shape[2],
            d.shape[3], sy, sx, oy, ox, oc, self.stream))

    def _bw_add_act(self, op):
        d, out = self.grad[op.outputs[0]], self.val[op.outputs[0]]
        act = rt.ACT_CODES[op.attrs["act"]]
        for t in op.inputs:                                   # (one buffer per input: later contributions are added in place)
            if act != rt.ACT_ID:
                self._add_grad(t, write_fn=lambda g: self._emit(self.L.act_bwd, d.ptr, d.dt, out.ptr, out.dt, g.ptr, g.dt, d.n, act,
                                                                self.stream))
            else:
                self._add_grad(t, write_fn=lambda g: self._emit(self.L.memcpy_d2d, g.ptr, d.ptr, d.nbytes, self.stream))

    def _bw_leaky_relu(self, op):
        """dx = dy * (y >= 0 ? 1 : alpha) from the node's own output (its input is not read again); an input with further readers gets
        the contribution through _add_grad, as with dropout and add_act."""
        d, out = self.grad[op.outputs[0]], self.val[op.outputs[0]]

        def wr(g):
            dd = self._as_dt(d, g.dt)
            self._emit(self.L.leaky_relu_bwd, dd.ptr, dd.dt, out.ptr, out.dt, g.ptr, g.dt, out.n, op.attrs["alpha"], self.stream)
        self._add_grad(op.inputs[0], write_fn=wr)

    def _norm_grad_ptrs(self, sv, nv):
        """(gamma, dgamma, dbeta) pointers the norm backward kernels take.  A batch-renorm layer hands them gamma_eff = gamma * r and its
        per-layer scratch: with r and d constant the layer is batch norm with gamma_eff, and the step's tail launch forms the parameter
        gradients dgamma = r dgamma' + d dbeta', dbeta = dbeta' from the scratch (Plan._emit_renorm_tail)."""
        rn = sv.renorm
        if rn is not None:
            return rn.gamma_eff.ptr, rn.dgs.ptr, rn.dbs.ptr
        return self.store.ptr(nv["gamma"]), self.store.grad_ptr(nv["gamma"]), self.store.grad_ptr(nv["beta"])

    def _norm_bwd(self, sv, nv, dA, dY, C, act, nrep, sums2, bias=None, tagged=False, s2d=(), rider=None):
        """Generic normalisation backward: the reduction over (dA, y), then the fused apply that writes dY and adds dgamma / dbeta.
        bias: (forward sums, forward pivot, db) pointers of the closed-form conv-bias gradient (phx_norm_bwd_apply_fused_bias and the
        _s2d / _head forms), None without.  s2d: (h, w) of a phase-form unit, whose hi-res dA is read through the space-to-depth
        permutation.  A HeadGrad dA is formed on the fly (dy_head w_head^T).  rider: the filter / bias gradient of that head
        (_head_rider_for) rides on the pair; where the pair cannot carry it, its job goes back to the heads' own launch."""
        Lb, y = self.L, sv.y
        if sv.norm == "layer":
            return self._layer_norm_bwd(sv, dA, dY, act)
        gamma_p, dgamma_p, dbeta_p = self._norm_grad_ptrs(sv, nv)
        if rider is not None:
            ok = (isinstance(dA, HeadGrad) and dA.dy.ptr == rider["dy"] and dA.nout == rider["nout"] and not s2d
                  and (bias is None or bias[2] is None) and sv.NS == 1 and sv.G == C and y.dt == BF16 and dY.dt == BF16)
            if not ok:
                self._headw_jobs.setdefault(rider["key"], []).append(rider["job"])
            else:
                hacc = self._alloc_zeroed(nrep * (C + 1) * rider["nout"])
                lead = (None, rider["dy"], dA.w_ptr, rider["nout"], y.ptr, sv.scale.ptr, sv.shift.ptr, sv.mean.ptr, sv.rstd.ptr)
                self._emit(Lb.norm_bwd_reduce_rider, *lead, sums2.ptr, hacc.ptr, sv.P, C, act, nrep, self.stream,
                           tag="bytes_norm_bwd_reduce" if tagged else None, flops=float(y.nbytes))
                self._emit(Lb.norm_bwd_apply_fused_rider, *lead, gamma_p, sums2.ptr, dY.ptr, dgamma_p,
                           dbeta_p, hacc.ptr, rider["dw"], rider["db"], sv.P, C, act, nrep, self.stream,
                           tag="bytes_norm_bwd_apply" if tagged else None, flops=float(y.nbytes + dY.nbytes))
                return
        if isinstance(dA, HeadGrad):
            lead, nb, ydt = (dA.dy.ptr, dA.w_ptr, dA.nout, y.ptr), 0, ()
            reduce, apply = Lb.norm_bwd_reduce_head, Lb.norm_bwd_apply_fused_head
        else:
            lead, nb, ydt = (dA.ptr, dA.dt, y.ptr, y.dt), dA.nbytes, (dY.dt,)
            reduce, apply = (Lb.norm_bwd_reduce_s2d, Lb.norm_bwd_apply_fused_s2d) if s2d else \
                (Lb.norm_bwd_reduce, Lb.norm_bwd_apply_fused if bias is None else Lb.norm_bwd_apply_fused_bias)
        lead += (sv.scale.ptr, sv.shift.ptr, sv.mean.ptr, sv.rstd.ptr)
        dims = (sv.NS, sv.P, C, sv.G, act, nrep, *s2d, self.stream)
        self._emit(reduce, *lead, sums2.ptr, *dims, tag="bytes_norm_bwd_reduce" if tagged else None, flops=float(nb + y.nbytes))
        self._emit(apply, *lead, gamma_p, sums2.ptr, dY.ptr, *ydt, dgamma_p,
                   dbeta_p, *(bias or ()), *dims,
                   tag="bytes_norm_bwd_apply" if tagged else None, flops=float(nb + y.nbytes + dY.nbytes))

    def _layer_norm_bwd(self, sv, dA, dY, act):
        """dY from dA through act and layer norm (phx_layer_norm_bwd): no variables, so no gradient but dY; a conv unit's bias gradient is
        the per-channel sum of dY, taken by the filter stage as for a unit without normalisation."""
        y, B = sv.y, sv.NS
        N = y.n // B
        ws, phases = self._layer_norm_phases(B, N)
        for ph in phases:
            self._emit(self.L.layer_norm_bwd, dA.ptr, dA.dt, y.ptr, y.dt, sv.mean.ptr, sv.rstd.ptr, dY.ptr, dY.dt,
                       ws.ptr if ws is not None else None, B, N, act, ph, self.stream,
                       tag="bytes_norm_bwd_reduce" if ph == 1 else "bytes_norm_bwd_apply",
                       flops=float(dA.nbytes + y.nbytes + (0 if ph == 1 else dY.nbytes)))

    def _bw_norm_layer(self, op, sv, dA, act):
        dY = self._alloc(sv.y.shape, sv.y.dt)
        self._layer_norm_bwd(sv, dA, dY, act)
        return dY, False

    def _bw_norm_act(self, op):
        a, sv = op.attrs, self.saved[op]
        dA = self.grad[op.outputs[0]]
        act = rt.ACT_CODES[a["act"]]
        if sv.norm is None:
            out = sv.out
            self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(self.L.act_bwd, dA.ptr, dA.dt, out.ptr, out.dt, g.ptr, g.dt, dA.n,
                                                                       act, self.stream))
            return
        if sv.route is NormRoute.INFER:
            raise NotImplementedError("backward through inference-mode batch norm is not on the hot path")
        C = sv.y.shape[3]
        if sv.route is NormRoute.LAYER:
            self._add_grad(op.inputs[0], write_fn=lambda g: self._layer_norm_bwd(sv, dA, g, act))
            return
        nrep = _NREP if sv.P >= _NREP_MINP else 1
        sums2 = self._alloc_zeroed(nrep * sv.NS * C * 2)
        self._add_grad(op.inputs[0], write_fn=lambda g: self._norm_bwd(sv, a["norm_vars"], dA, g, C, act, nrep, sums2))

    def _bw_flatten(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        self._add_grad(op.inputs[0], buf=Buf(x.shape, d.dt, like=d.t))

    def _bw_avgpool(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(
            self.L.avgpool2x2_bwd, d.ptr, d.dt, g.ptr, x.shape[0], x.shape[1], x.shape[2], x.shape[3], self.stream),
            accum_fn=(lambda g: self._emit(self.L.avgpool2x2_bwd_acc, d.ptr, d.dt, g.ptr, x.shape[0], x.shape[1], x.shape[2], x.shape[3],
                                           self.stream)) if d.dt == x.dt else None)

    def _bw_bilinear_up(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(
            self.L.bilinear_up2x_bwd, d.ptr, d.dt, g.ptr, x.shape[0], x.shape[1], x.shape[2], x.shape[3], self.stream),
            accum_fn=(lambda g: self._emit(self.L.bilinear_up2x_bwd_acc, d.ptr, d.dt, g.ptr, x.shape[0], x.shape[1], x.shape[2],
                                           x.shape[3], self.stream)) if d.dt == x.dt else None)

    def _bw_global_avgpool(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]

        def wr(g):
            # the kernel writes fp32: a pooled bf16 tensor (a hidden layer's output; the zoo pools fp32 heads only) takes its gradient
            # through an fp32 buffer and a cast -- writing fp32 into the bf16 buffer would run past its end
            t = g if g.dt == F32 else self._alloc(g.shape, F32)
            self._emit(self.L.global_avgpool_bwd, d.ptr, t.ptr, x.shape[0], x.shape[1] * x.shape[2], x.shape[3], self.stream)
            if t is not g:
                self._emit(self.L.cast, t.ptr, F32, g.ptr, g.dt, g.n, self.stream)
        self._add_grad(op.inputs[0], write_fn=wr)

    def _bw_tile_pixels(self, op):
        d = self.grad[op.outputs[0]]
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(
            self.L.broadcast_pixels_bwd, d.ptr, d.dt, g.ptr, d.shape[0], d.shape[1] * d.shape[2], d.shape[3],
            self.stream))

    def _bw_conv_unit(self, op):
        """Norm backward (by the saved route) -> dY, then the filter gradient, then the data gradient; the phase-form, general and
        transposed units have their own gradient methods."""
        if op in self._lat:
            return self._bw_latent_group(self._lat[op])
        sv, b = self.saved[op], op.attrs["b"]
        dY, db_done = self._bw_unit_norm(op, sv, self.grad[op.outputs[0]])
        db = self.store.grad_ptr(b) if (b is not None and not db_done) else None
        if sv.upconv is not None:
            return self._bw_unit_upconv(op, sv, dY, db)
        if sv.explicit is not None:
            return self._bw_unit_explicit(op, sv, dY, db)
        if sv.volume is not None:
            return self._bw_unit_volume(op, sv, dY, db)
        if sv.general is not None:
            return self._bw_unit_general(op, sv, dY, db)
        if sv.transposed is not None:
            return self._bw_unit_transposed(op, sv, dY, db)
        self._bw_unit_filter(op, sv, dY, db)
        self._bw_unit_data(op, sv, dY)

    @staticmethod
    def _unit_dims(op, sv):
        """(B, H, W, Cin, Cout) of a unit's convolution, from its saved input and its filter."""
        W = op.attrs["W"]
        cin, cout = (W.shape[3], W.shape[2]) if sv.transposed is not None else (W.shape[-2], W.shape[-1])
        return sv.x.shape[0], sv.x.shape[1], sv.x.shape[2], cin, cout

    # ---- stage 1: the normalisation / activation backward, dA -> (dY, bias gradient already formed?) ------------------------------
    def _bw_unit_norm(self, op, sv, dA):
        act = rt.ACT_CODES[op.attrs["act"]]
        if sv.upconv is not None:
            # phase form (upconv.py): y and everything downstream of it live in the PACKED pixel order; dA is a hi-res map -- the two
            # norm-backward passes read it through the space-to-depth permutation
            assert isinstance(dA, Buf) and dA.dt == BF16 and sv.route is NormRoute.GENERIC
        if sv.norm is None:
            if act == rt.ACT_ID:
                return dA, False
            dY = self._alloc(sv.out.shape, dA.dt)
            self._emit(self.L.act_bwd, dA.ptr, dA.dt, sv.out.ptr, sv.out.dt, dY.ptr, dY.dt, dA.n, act, self.stream)
            return dY, False
        if sv.y is None or sv.mean is None or (sv.norm == "batch" and not self.training):
            raise NotImplementedError("backward through inference-mode batch norm is not on the hot path")
        R = NormRoute
        if sv.route is R.LAYER:
            return self._bw_norm_layer(op, sv, dA, act)
        one_launch = {R.BN_WIDE: self._bw_norm_bn_wide, R.BN_SMALL_F32Y: self._bw_norm_bn_small, R.BN_SMALL: self._bw_norm_bn_small,
                      R.FGN: self._bw_norm_small, R.NORM_SMALL: self._bw_norm_small, R.RENORM_SMALL: self._bw_norm_bn_small}.get(sv.route) if dA.dt == BF16 else None
        if sv.route is R.RENORM_SMALL and not self.L.bn_small_supported(sv.P, sv.y.shape[3], BF16):
            one_launch = None            # (phx_bn_small_bwd owns 16 channels per block, phx_renorm_small_fwd eight: C % 16 != 0 goes the generic way)
        return (one_launch or self._bw_norm_generic)(op, sv, dA, act)

    def _bw_one_launch_args(self, op, sv, dY):
        """(saved statistics..., gamma, dY, dgamma, dbeta): the argument run the one-launch norm backward kernels share."""
        gamma_p, dgamma_p, dbeta_p = self._norm_grad_ptrs(sv, op.attrs["norm_vars"])
        return (sv.scale.ptr, sv.shift.ptr, sv.mean.ptr, sv.rstd.ptr, gamma_p, dY.ptr, dgamma_p, dbeta_p)

    def _bw_norm_bn_wide(self, op, sv, dA, act):
        y, dY = sv.y, self._alloc(sv.y.shape, BF16)
        sg = dA if isinstance(dA, SliceGrad) else None      # the consumer's split-K data gradient left its slices: summed here
        self._emit(self.L.bn_wide_bwd, None if sg is not None else dA.ptr, sg.ws.ptr if sg is not None else None,
                   sg.nz if sg is not None else 0, y.ptr, *self._bw_one_launch_args(op, sv, dY), sv.P, y.shape[3], act, self.stream,
                   tag="bytes_norm_bwd_apply", flops=float(dY.nbytes + y.nbytes + dY.nbytes))
        return dY, False

    def _bw_norm_bn_small(self, op, sv, dA, act):
        y, dY = sv.y, self._alloc(sv.y.shape, BF16)
        self._emit(self.L.bn_small_bwd, dA.ptr, y.ptr, y.dt, *self._bw_one_launch_args(op, sv, dY), sv.P, y.shape[3], act, self.stream,
                   tag="bytes_norm_bwd_apply", flops=float(dA.nbytes + y.nbytes + dY.nbytes))
        return dY, False

    def _bw_norm_small(self, op, sv, dA, act):
        y, b, dY = sv.y, op.attrs["b"], self._alloc(sv.y.shape, sv.y.dt)
        self._emit(self.L.norm_small_bwd, dA.ptr, y.ptr, *self._bw_one_launch_args(op, sv, dY),
                   self.store.grad_ptr(b) if b is not None else None, sv.NS, sv.P, y.shape[3], sv.G, act, self.stream,
                   tag="bytes_norm_bwd_apply", flops=float(dA.nbytes + y.nbytes + dY.nbytes))
        return dY, True

    def _bw_norm_generic(self, op, sv, dA, act):
        """The shared reduce + fused apply (_norm_bwd), or ONE launch on the mid-size batch-norm layers (phx_bn_bwd_onepass)."""
        S, Lb, nv, b = self.stream, self.L, op.attrs["norm_vars"], op.attrs["b"]
        y, NS, P, Gn, cout = sv.y, sv.NS, sv.P, sv.G, sv.y.shape[3]
        nrep = _NREP if P >= _NREP_MINP else 1   # replicated accumulators: see k_norm_bwd_reduce
        if _DETERMINISTIC and P >= _NREP_MINP:
            nrep = 64                             # one block per replica there: more replicas = more blocks
        sums2 = self._alloc_zeroed(nrep * NS * cout * 2)
        self._alloc((NS * Gn * 2,), F32)         # (read by nothing; it keeps the plan's allocation sequence as it has always been)
        dY = self._alloc(y.shape, y.dt)
        # group / instance norm keep the convolution bias: its gradient (the per-channel sum of dY) comes out of the apply
        # launch in closed form instead of a pass over dY (phx_norm_bwd_apply_fused_bias)
        fs = sv.fsums if b is not None else None
        bias = (fs.ptr if fs is not None else None, sv.fpivot.ptr if (fs is not None and sv.fpivot is not None) else None,
                self.store.grad_ptr(b) if fs is not None else None)
        if (sv.upconv is None and fs is None and sv.norm == "batch" and NS == 1 and Gn == cout and isinstance(dA, Buf)
                and dA.dt == BF16 and y.dt == BF16 and _onepass_enabled() and Lb.bn_bwd_onepass_supported(P, cout, act)):
            # mid-size batch-norm layers: ONE launch, (dA, y) read once and held in registers across a grid barrier
            bar = self._alloc_zeroed(int(Lb.bn_bwd_onepass_barrier_words()))
            self._barriers.append(bar)
            self._emit(Lb.bn_bwd_onepass, dA.ptr, y.ptr, sv.scale.ptr, sv.shift.ptr, sv.mean.ptr, sv.rstd.ptr, self.store.ptr(nv["gamma"]),
                       sums2.ptr, bar.ptr, dY.ptr, self.store.grad_ptr(nv["gamma"]), self.store.grad_ptr(nv["beta"]), P, cout, act, nrep, S,
                       tag="bytes_norm_bwd_onepass", flops=float(dA.nbytes + y.nbytes + dY.nbytes))
        else:
            s2d = (sv.x.shape[1] // 2, sv.x.shape[2] // 2) if sv.upconv is not None else ()
            self._norm_bwd(sv, nv, dA, dY, cout, act, nrep, sums2, bias=bias, tagged=True, s2d=s2d, rider=self._head_riders.pop(op, None))
        return dY, fs is not None

    # ---- the units off the common path: stages 2 and 3 in one method each ------------------------------------------------------
    def _bw_unit_upconv(self, op, sv, dY, db):
        """Phase form (upconv.py): the gradient goes straight to the resize's input (its adjoint is part of the form)."""
        S, Lb, W, upc = self.stream, self.L, op.attrs["W"], sv.upconv
        B, H, Wd, cin, cout = self._unit_dims(op, sv)
        h, w = H // 2, Wd // 2
        if db is not None:                           # (not reached with the closed-form bias gradient of the norm backward; kept exact)
            self._emit(Lb.channel_sum_accumulate, dY.ptr, dY.dt, db, B * H * Wd, cout, S)
        upconv.backward_prepare(self._emit, self._alloc, Lb, S, upc, dY, B, h, w, cout)
        # (filter gradients before or after the data gradients: same step time, measured three alternating pairs)
        upconv.backward_filters(self._emit, self._alloc, self._alloc_zeroed, Lb, S, upc, sv.x.src, dY, self.store.grad_ptr(W), B, h, w, cin, cout)
        xin = op.inputs[0].op.inputs[0]              # the low-resolution tensor bilinear_upsample2D read
        if self.req.get(xin, False):
            _, wd_w = self._packed(W)
            self._add_grad(xin, write_fn=lambda g: upconv.backward_data(self._emit, self._alloc, Lb, S, upc, dY, wd_w, g, B, h, w, cin, cout))

    def _bw_unit_direct(self, op, sv, dY, db, wgrad, dgrad, cout=None, ws=()):
        """Filter, bias and data gradient of a unit on the direct kernels (gconv.hip / tconv.hip / conv3d.hip / conv2d_pad.hip) with the
        geometry saved forward.  ws: the workspace argument of a filter-gradient entry that takes one, behind dw."""
        S, x, W = self.stream, sv.x, op.attrs["W"]
        cout = cout or self._unit_dims(op, sv)[4]
        self._emit(wgrad, x.ptr, x.dt, dY.ptr, dY.dt, self.store.grad_ptr(W), *ws, *sv.geo, S)
        if db is not None:
            self._emit(self.L.channel_sum_accumulate, dY.ptr, dY.dt, db, dY.n // cout, cout, S)
        if self.req.get(op.inputs[0], False):
            self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(dgrad, dY.ptr, dY.dt, self.store.ptr(W), g.ptr, g.dt, *sv.geo, S))

    def _bw_unit_general(self, op, sv, dY, db):
        self._bw_unit_direct(op, sv, dY, db, self.L.gconv2d_wgrad, self.L.gconv2d_dgrad)

    def _bw_unit_volume(self, op, sv, dY, db):
        Lb = self.L
        wgrad, dgrad = (Lb.gconv3d_wgrad, Lb.gconv3d_dgrad) if sv.volume[0] == "conv" else (Lb.tconv3d_wgrad, Lb.tconv3d_dgrad)
        self._bw_unit_direct(op, sv, dY, db, wgrad, dgrad, cout=sv.geo[5])

    def _bw_unit_explicit(self, op, sv, dY, db):
        """conv2d_pad.hip: the filter gradient sums the pixels of the smaller tensor (the convolution's output, the transposed
        convolution's input) per block and adds the blocks' sums in a second launch, through a workspace of the plan's."""
        Lb, conv = self.L, sv.explicit == "conv"
        B, H, Wd, cin, cout, kh, kw = sv.geo[:7]
        Ho, Wo = sv.geo[11:13]
        small = (B, Ho, Wo, cin, cout) if conv else (B, H, Wd, cout, cin)
        n = int(Lb.conv2d_pad_wgrad_ws_floats(*small, kh, kw))
        ws = self._alloc((n,), F32).ptr if n else None
        wgrad, dgrad = (Lb.conv2d_pad_wgrad, Lb.conv2d_pad_dgrad) if conv else (Lb.tconv2d_pad_wgrad, Lb.tconv2d_pad_dgrad)
        self._bw_unit_direct(op, sv, dY, db, wgrad, dgrad, cout=cout, ws=(ws,))

    def _bw_pool2d(self, op):
        x, d = self.val[op.inputs[0]], self.grad[op.outputs[0]]
        args = self._pool2d_args(op, x)
        self._add_grad(op.inputs[0], write_fn=lambda g: self._emit(self.L.pool2d_bwd, x.ptr, d.ptr, d.dt, g.ptr, *args, self.stream),
                       accum_fn=(lambda g: self._emit(self.L.pool2d_bwd_acc, x.ptr, d.ptr, d.dt, g.ptr, *args, self.stream))
                       if d.dt == x.dt else None)

    def _bw_unit_transposed(self, op, sv, dY, db):
        self._bw_unit_direct(op, sv, dY, db, self.L.tconv2d_wgrad, self.L.tconv2d_dgrad)

    # ---- stage 2: the filter (and bias) gradient --------------------------------------------------------------------------------
    def _bw_unit_filter(self, op, sv, dY, db):
        # (The filter gradient is a leaf of the backward graph; moving these launches to another lane, beside the data-
        # gradient chain, was measured 20 % SLOWER: both are bound by the same global->LDS path, so the kernel on the
        # critical path just gets half of it.)
        S, Lb, x, W, k = self.stream, self.L, sv.x, op.attrs["W"], op.attrs["ksize"]
        B, H, Wd, cin, cout = self._unit_dims(op, sv)
        dw = self.store.grad_ptr(W)
        if sv.head1x1 and cin % 8 == 0 and db is not None:
            # a leaf of the backward graph: all heads share one launch after the lanes have joined (phx_head1x1_wgrad_multi)
            plan4 = (ctypes.c_int * 4)()
            Lb.head1x1_wgrad_plan(B * H * Wd, cin, cout, plan4)
            prod = self._norm_head.get(op)
            au = self.saved[prod].a_unwritten if prod is not None else None
            src, extra = (x, ()) if au is None else (au["y"], ((au["scale"].ptr, au["shift"].ptr, au["act"]),))
            # (au: the producer never wrote a = act(bn(y)) -- the job re-forms it from y: phx_head1x1_wgrad_multi, xscale)
            key, job = (src.dt, cout), (src.ptr, dY.ptr, dw, db, B * H * Wd, cin, *plan4) + extra
            rprod = self._head_rider_for(op, B * H * Wd, cin, cout)
            if rprod is not None:
                # the producer's norm backward (later in the backward order, same lane) streams the very tensor this job would read
                # again: the head's filter / bias gradient rides on its reduction (phx_norm_bwd_reduce_rider)
                self._head_riders[rprod] = dict(dy=dY.ptr, dw=dw, db=db, nout=cout, key=key, job=job)
            else:
                self._headw_jobs.setdefault(key, []).append(job)
        elif sv.head1x1:
            self._emit(Lb.head1x1_wgrad, x.ptr, x.dt, dY.ptr, dw, db, B * H * Wd, cin, cout, S)
        elif sv.padded or sv.mfma:
            self._bw_filter_mfma(op, sv, dY, dw, db)
        elif (sv.f32m and k == 3 and x.dt == F32 and dY.dt == F32 and isinstance(x, Buf)
              and Lb.conv3x3_f32_mfma_wgrad_supported(B, H, Wd, cin, cout)):
            # fp32 plans: the filter gradient on the fp32 matrix instruction; partial filters in a workspace, summed in slice order
            # (a fixed order in every mode)
            wsb = int(Lb.conv3x3_f32_mfma_wgrad_ws_bytes(B, H, Wd, cin, cout, 1 if db is not None else 0))
            ws = self._alloc((wsb // 4,), F32)
            self._emit(Lb.conv3x3_f32_mfma_wgrad, x.ptr, dY.ptr, dw, db, ws.ptr, wsb, B, H, Wd, cin, cout, S,
                       tag="conv3x3_f32_mfma_wgrad", flops=18.0 * cin * cout * B * H * Wd)
        elif _DETERMINISTIC:
            # ordered partial filters: the fixed summation order at full parallelism (the plain entry point's deterministic
            # launch is one block per channel block -- 0.47 s instead of 0.1 s per fp32 training step at n0 = 32, batch 12)
            wsb = int(Lb.conv2d_direct_wgrad_ordered_ws_bytes(B, H, Wd, cin, cout, k))
            ws = self._alloc((wsb // 4,), F32) if wsb else None
            self._emit(Lb.conv2d_direct_wgrad_ordered, x.ptr, x.dt, dY.ptr, dY.dt, dw, db, ws.ptr if ws is not None else None, wsb,
                       B, H, Wd, cin, cout, k, S)
        else:
            self._emit(Lb.conv2d_direct_wgrad, x.ptr, x.dt, dY.ptr, dY.dt, dw, db, B, H, Wd, cin, cout, k, S)

    def _head_rider_for(self, op, npix, cin, nout):
        """The conv unit whose norm backward carries the filter gradient of 1x1 head `op` as a rider, or None: the batch-norm unit on
        the head's lane whose ONLY reader the head is (its gradient is the HeadGrad placeholder, so its backward is the reduce + apply
        pair of _norm_bwd -- never the one-launch forms or the phase form), in the kernels' domain (phx_norm_head_supported).  The
        form for a unit with further readers (dA a tensor) is in the library but lost to the stand-alone job where it was measured
        (LABBOOK), so such heads keep their job.  Deterministic mode keeps the heads' own launch."""
        if not _head_rider_enabled() or _DETERMINISTIC or self.act_dt != BF16 or nout not in _HEAD_RIDER_NOUT:
            return None
        prod = self._norm_head.get(op)
        psv = self.saved.get(prod) if prod is not None else None
        if (not isinstance(psv, ConvSaved) or prod.outputs[0] is not op.inputs[0] or self.op_lane.get(prod) != self.op_lane.get(op)
                or psv.route is not NormRoute.GENERIC or psv.norm != "batch" or psv.upconv is not None or prod.attrs["b"] is not None
                or psv.y is None or psv.y.dt != BF16 or psv.NS != 1 or psv.P != npix or psv.y.shape[3] != cin or psv.G != cin
                or prod in self._head_riders or not self.L.norm_head_supported(cin, nout, BF16, BF16)):
            return None
        return prod

    def _bw_filter_mfma(self, op, sv, dY, dw, db):
        """bf16 MFMA filter gradient.  Padded layers (zero-padded input channels / 1x1 as centre tap): the gradient goes to a padded
        filter buffer first and a small kernel folds it into dw afterwards."""
        S, Lb, x = self.stream, self.L, sv.x
        B, H, Wd, cin, cout = self._unit_dims(op, sv)
        ce = sv.cin_eff if sv.padded else cin
        tgt = self._alloc_zeroed(9 * ce * cout).ptr if sv.padded else dw
        dual = x if isinstance(x, DualBuf) else None       # concat-free input: the filter gradient reads the two tensors in place
        xf = x if isinstance(x, XfBuf) else None           # unmaterialised input activation: re-formed from y by the kernel's loader
        k1d = dual.k1 if dual is not None else 0
        wsb = int(Lb.conv3x3_wgrad_ws_bytes_dual(B, H, Wd, ce, cout, k1d))
        wsp = self._alloc((wsb // 4,), F32)      # per-layer workspace of partial filters (no cross-lane sharing)
        plan6 = (ctypes.c_int * 6)()
        Lb.conv3x3_wgrad_reduce_plan_dual(B, H, Wd, ce, cout, k1d, plan6)
        if xf is None:
            wargs = (x.ptr, dY.ptr, tgt, wsp.ptr, wsb, B, H, Wd, ce, cout)
            dargs = (x.ptr, dual.b.ptr if dual is not None else None, k1d) + wargs[1:]      # (x, x2, K1, dy, ...)
        tag = dict(tag="conv3x3_mfma_wgrad", flops=18.0 * cin * cout * B * H * Wd)
        # The filter gradients are leaves of the backward graph.  Small and mid-size maps: the launch itself is
        # deferred -- one launch per kernel variant runs all such layers side by side after the lanes have joined
        # (phx_conv3x3_wgrad_multi); their latency leaves the posterior / prior / likelihood chains.
        # (an unmaterialised input only exists on maps too large for the deferred launches: _xf_edge_ok)
        deferred = xf is None and self._defer_filter_gradient(dargs, wsp, tgt, ce, cout)
        if deferred:
            pass
        elif plan6[0]:
            # large maps: the launch stays here, only the sum over its partial filters is deferred to ONE launch for all
            # layers (phx_wgrad_reduce_multi)
            if xf is not None:
                self._emit(Lb.conv3x3_wgrad_mfma_bf16_partial_xf, xf.y.ptr, xf.scale.ptr, xf.shift.ptr, dY.ptr, tgt, wsp.ptr, wsb,
                           B, H, Wd, ce, cout, S, **tag)
            elif dual is not None:
                self._emit(Lb.conv3x3_wgrad_mfma_bf16_dual, *dargs, 0, S, **tag)
            else:
                self._emit(Lb.conv3x3_wgrad_mfma_bf16_partial, *wargs, S, **tag)
            self._wgr_jobs.append((wsp.ptr, tgt, plan6[1], ce, cout, plan6[2], plan6[3], plan6[4], plan6[5]))
            deferred = True
        elif xf is not None:
            raise rt.PhxError("filter gradient of an unmaterialised input activation without a workspace plan (see _xf_edge_ok)")
        elif dual is not None:
            self._emit(Lb.conv3x3_wgrad_mfma_bf16_dual, *dargs, 1, S, **tag)
        else:
            self._emit(Lb.conv3x3_wgrad_mfma_bf16, *wargs, S, **tag)
        if sv.padded:
            if deferred:
                # after the deferred launches, on lane 0: ONE launch folds them all (phx_unpad_filter_grad_multi)
                self._tail_jobs.append((tgt, dw, cin, ce, cout, 1 if sv.k1 else 9))
            else:
                self._emit(Lb.unpad_filter_grad_center if sv.k1 else Lb.unpad_filter_grad_accumulate, tgt, dw, cin, ce, cout, S)
        if db is not None:
            self._emit(Lb.channel_sum_accumulate, dY.ptr, dY.dt, db, B * H * Wd, cout, S)

    def _defer_filter_gradient(self, dargs, wsp, tgt, ce, cout):
        """Queue the layer's job record for its kernel variant's deferred launch, if the library defers this shape -> deferred?"""
        Lb = self.L
        jb, info = ctypes.create_string_buffer(int(Lb.conv3x3_wgrad_multi_job_bytes())), (ctypes.c_int * 9)()
        Lb.conv3x3_wgrad_multi_job_dual(*dargs, _WGRAD_DEFER_BLOCKS, 0, jb, info)
        if not info[0]:
            return False
        grp = self._wgm_jobs.setdefault(int(info[0]), dict(recs=[], blocks=0, lds=0))
        Lb.conv3x3_wgrad_multi_job_dual(*dargs, _WGRAD_DEFER_BLOCKS, grp["blocks"], jb, info)
        grp["recs"].append(jb.raw)
        grp["blocks"] += int(info[1])
        grp["lds"] = max(grp["lds"], int(info[2]))
        if info[3]:
            self._wgr_jobs.append((wsp.ptr, tgt, info[4], ce, cout, info[5], info[6], info[7], info[8]))
        return True

    # ---- stage 3: the data gradient ---------------------------------------------------------------------------------------------
    def _bw_unit_data(self, op, sv, dY):
        S, Lb, x, W, k = self.stream, self.L, sv.x, op.attrs["W"], op.attrs["ksize"]
        B, H, Wd, cin, cout = self._unit_dims(op, sv)
        xin = op.inputs[0]
        if not self.req.get(xin, False):
            return
        dtag = dict(tag="conv3x3_mfma_dgrad", flops=18.0 * cin * cout * B * H * Wd)

        def mfma_dgrad(g):
            """The 3x3 data gradient on the MFMA path into g (None: the split-K slices stay in the workspace) -> the workspace"""
            wsb = int(Lb.conv3x3_mfma_ws_bytes(B, H, Wd, cout, cin))
            ws = self._alloc((wsb // 4,), F32) if wsb else None      # split-K slices (small maps)
            self._emit(Lb.conv3x3_mfma_bf16_ws, dY.ptr, wd.ptr, g.ptr if g is not None else None, None, 0, None, ws.ptr if ws else None, wsb,
                       B, H, Wd, cout, cin, S, **dtag)
            return ws
        if isinstance(x, DualBuf):
            # concat-free: the two halves of d(concat) are written straight to the gradients of the concatenated tensors
            ta, tb = xin.op.inputs
            _, wd = self._packed(W)
            g1, g2 = self._alloc(x.a.shape, BF16), self._alloc(x.b.shape, BF16)
            wsb = int(Lb.conv3x3_mfma_ws_bytes(B, H, Wd, cout, cin))
            ws = self._alloc((wsb // 4,), F32) if wsb else None      # split-K slices (small maps)
            self._emit(Lb.conv3x3_mfma_bf16_dual, dY.ptr, None, 0, wd.ptr, g1.ptr, g2.ptr, x.k1, None, None, 0, None, 0,
                       ws.ptr if ws else None, wsb, B, H, Wd, cout, cin, S, **dtag)
            for t, gb in ((ta, g1), (tb, g2)):
                if self.req.get(t, False):
                    self._add_grad(t, buf=gb)
        elif sv.norm_head:              # no data-gradient launch: the producer's norm backward forms dA = dY W^T itself
            self._add_grad(xin, buf=HeadGrad(self.val[xin], dY, self.store.ptr(W), cout))
        elif sv.head1x1:
            self._add_grad(xin, write_fn=lambda g: self._emit(
                Lb.head1x1_dgrad, dY.ptr, self.store.ptr(W), g.ptr, g.dt, B * H * Wd, cin, cout, S))
        elif sv.padded:
            ce, wdp = sv.cin_eff, sv.wd_pad

            def wr(g):
                inplace = ce == cin and g.dt == BF16        # nothing to strip / cast: the data gradient is written in place
                gp = g if inplace else self._alloc((B, H, Wd, ce), BF16)
                self._emit(Lb.conv3x3_mfma_bf16, dY.ptr, wdp.ptr, gp.ptr, None, 0, None, B, H, Wd, cout, ce, S, **dtag)
                if not inplace:
                    self._emit(Lb.unpad_channels_bf16, gp.ptr, g.ptr, g.dt, cin, ce, B * H * Wd, S)
            self._add_grad(xin, write_fn=wr)
        elif sv.mfma and self._slice_grad_ok(op, xin, B, H, Wd, cout, cin):
            # 2 x 2 / 4 x 4 levels: the split-K data gradient leaves its fp32 slices for the producer's one-launch batch-norm
            # backward (phx_bn_wide_bwd sums them): no finishing launch, no bf16 gradient tensor
            _, wd = self._packed(W)
            ws = mfma_dgrad(None)
            self._add_grad(xin, buf=SliceGrad(self.val[xin], ws, int(Lb.conv3x3_mfma_ksplit(B, H, Wd, cout, cin))))
        elif sv.mfma:
            _, wd = self._packed(W)
            self._add_grad(xin, write_fn=mfma_dgrad)
        elif sv.f32m and cin % 32 == 0 and dY.dt == F32 and self._wpk32.get(W.name, (None, None))[1] is not None:
            wd32 = self._wpk32[W.name][1]

            def wr_f32m(g):
                assert g.dt == F32
                self._emit(Lb.conv3x3_f32_mfma, dY.ptr, wd32.ptr, None, g.ptr, B, H, Wd, cout, cin, 0, S,
                           tag="conv3x3_f32_mfma_dgrad", flops=18.0 * cin * cout * B * H * Wd)
            self._add_grad(xin, write_fn=wr_f32m)
        else:
            self._add_grad(xin, write_fn=lambda g: self._emit(
                Lb.conv2d_direct, dY.ptr, dY.dt, self.store.ptr(W), None, g.ptr, g.dt, B, H, Wd, cin, cout, k, 0,
                1, None, S))
