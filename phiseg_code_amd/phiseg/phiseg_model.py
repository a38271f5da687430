"""The PHiSeg model: graph wiring, ELBO, train loop, sampling API.

Counterpart of the reference's phiseg/phiseg_model.py with the same public surface
(``phiseg(exp_config)``, ``.train(data)``, ``.predict*``, ``.generate_prior_samples``, ``.load_weights``,
attributes ``x_inp``, ``s_inp``, ``training_pl``, ``lr_pl``, ``z_list``, ``s_out_list``, ``s_out_eval``,
``s_out_eval_sm``, ``loss_dict``, ``loss_tot``, ``train_step``, ``sess``) -- but ``sess.run`` lowers the
requested fetches to hand-written HIP kernels replayed from a hipGraph (phiseg_code_amd.engine) instead of
dispatching TensorFlow ops.

Deliberate, documented differences from the TF1 graph:
* Q1/Q4: only the live graph is executed per training step (the reference also runs the generation-mode
  prior, the evaluation likelihood and the never-consumed up-sampling branches because their batch-norm
  update ops sit in UPDATE_OPS); batch-norm moving statistics are updated once per step from the training
  graph instance.
* Q10: noise is a seeded Philox4x32-10 stream keyed by (seed, step, net, level, global sample index).
"""
import logging
import os
import time

import numpy as np

from phiseg_code_amd import engine
from phiseg_code_amd import graph as G
from phiseg_code_amd import many_class
from phiseg_code_amd import multichannel
from phiseg_code_amd import optimizers
from phiseg_code_amd import utils
from phiseg_code_amd.tfwrapper import normalisation as tfnorm

logging.basicConfig(level=logging.INFO, format='%(asctime)s %(message)s')


class _Flag:
    """Scalar placeholder fed through feed_dict (training_pl, lr_pl)."""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "<placeholder %s>" % self.name


class TrainStep:
    """Handle returned as ``model.train_step``: fetching it runs backward + the optimiser's update (optimizer.minimize)."""

    def __init__(self, loss):
        self.loss = loss


class Session:
    """``sess.run(fetches, feed_dict)`` over compiled plans (one per fetch set / batch size / training flag)."""

    def __init__(self, model, compute_dtype, rng_seed=42, dist=None):
        self.model = model
        self.compute_dtype = compute_dtype
        self.rng_seed = rng_seed
        self.dist = dist
        self.store = None
        self.plans = {}
        self._lr = None

    def _ensure_store(self):
        if self.store is None:
            self.store = engine.ParamStore(self.model.graph, seed=self.model.init_seed,
                                           live=engine.live_variables(self.model.loss_tot), optimizer=self.model.optimizer)
            if self.dist is not None and self.dist.active:
                # identical replicas (the Philox initialiser already gives every rank the same values; this also covers
                # weights loaded on one rank only)
                self.dist.broadcast_(self.store.params)
                self.dist.broadcast_(self.store.state)
                engine.device_sync()
        return self.store

    def plan_for(self, fetch_tensors, train, batch, training, stamp_tagged=False, fed=()):
        key = (tuple(id(t) for t in fetch_tensors), bool(train), int(batch), bool(training)) + (("stamped",) if stamp_tagged else ())
        if fed:
            key += ("fed",) + tuple(id(t) for t in fed)
        if key not in self.plans:
            store = self._ensure_store()
            world, rank = (self.dist.world, self.dist.rank) if self.dist else (1, 0)
            self.plans[key] = engine.Plan(
                store, fetch_tensors, loss=self.model.loss_tot if train else None, batch=batch, training=training,
                compute_dtype=self.compute_dtype, rng_seed=self.rng_seed, sample_offset=rank * batch,
                loss_inv_batch=1.0 / (batch * world), split_optimizer=bool(self.dist and self.dist.active), stamp_tagged=stamp_tagged,
                fed=fed, optimizer=self.model.optimizer, dist_active=bool(self.dist and self.dist.active))
        return self.plans[key]

    def latent_feeds(self, feed_dict):
        """The latent feeds of a feed_dict: keys that are members of model.z_list, in level order (phiseg_model.py:315 of the
        reference: sess.run(s_out_list, {z_list[i]: ...}) decodes chosen latents).  Any other tensor key that is not a placeholder
        cannot be fed."""
        m = self.model
        fed = []
        for k in feed_dict:
            if isinstance(k, G.Tensor) and k is not m.x_inp and k is not m.s_inp:
                lv = [i for i, z in enumerate(m.z_list) if z is k]
                if not lv:
                    raise ValueError("feed_dict: %r is neither a placeholder nor a member of z_list -- only latents can be fed" % (k,))
                fed.append((lv[0], k))
        return [k for _, k in sorted(fed, key=lambda e: e[0])]

    def _launch(self, tensors, feed_dict, train=False):
        """Compile (once) and run the plan of these fetches with these feeds -> the plan; nothing is copied back."""
        m = self.model
        fed = self.latent_feeds(feed_dict)
        if fed and train:
            raise ValueError("latent feeds are for inference: a training step computes its own posterior samples")
        x = feed_dict.get(m.x_inp)
        if x is None:
            raise ValueError("feed_dict must provide x_inp")
        x = np.asarray(x)
        training = bool(feed_dict.get(m.training_pl, False))
        if train and training and m.bn_double_update:
            tensors = tensors + [m.s_out_eval]         # Q4: the second graph instances run (and update moving statistics) too
        plan = self.plan_for(tensors, train, x.shape[0], training, fed=fed)
        if "x_input" in plan.feeds:                    # (a fully fed decode of a likelihood that does not read x has no use for it)
            plan.set_input("x_input", x)
        if "s_input" in plan.feeds:
            if m.s_inp not in feed_dict:
                raise ValueError("these fetches need s_inp")
            plan.set_input("s_input", feed_dict[m.s_inp])
        for t in fed:
            want = plan.feeds[t].shape
            v = np.asarray(feed_dict[t], dtype=np.float32)
            if tuple(v.shape) != tuple(want):
                raise ValueError("latent feed %s: got shape %s, the plan expects %s" % (t.name, v.shape, want))
            plan.set_input(t, v)
        if m.lr_pl in feed_dict and float(feed_dict[m.lr_pl]) != self._lr:
            self._lr = float(feed_dict[m.lr_pl])
            self.store.set_lr(self._lr)               # (synchronises: the plans replay on their own HIP streams)
        dp = self.dist is not None and self.dist.active
        if train and dp:
            plan.run_main()
            self.dist.allreduce_sum(self.store.grads[:self.store.n_live], plan)
            plan.run_opt()
        else:
            plan.run()
        return plan

    def run_buffers(self, tensors, feed_dict):
        """Run the plan of `tensors` and hand back its device buffers instead of host copies: -> (plan, [plan.val[t] ...]).  The
        buffers belong to the plan and are overwritten by its next run; work on them is enqueued on plan.stream (nothing here
        synchronises or copies)."""
        tensors = list(tensors)
        plan = self._launch(tensors, feed_dict or {})
        return plan, [plan.val[t] for t in tensors]

    def run(self, fetches, feed_dict=None):
        feed_dict = feed_dict or {}
        m = self.model
        single = not isinstance(fetches, (list, tuple))
        flat, spec = [], []

        def walk(f):
            if isinstance(f, (list, tuple)):
                return [walk(x) for x in f]
            flat.append(f)
            return len(flat) - 1
        spec = walk([fetches] if single else list(fetches))
        train = any(isinstance(f, TrainStep) for f in flat)
        tensors = [f for f in flat if isinstance(f, G.Tensor)]
        plan = self._launch(tensors, feed_dict, train)
        dp = self.dist is not None and self.dist.active
        vals = [plan.fetch(f) if isinstance(f, G.Tensor) else None for f in flat]
        if dp and "s_input" in plan.feeds:
            # the loss kernels scale every term by 1 / (B_local * world): a rank's scalar is its SHARE of the global-batch mean
            # (phiseg_model.py:221,236 take the mean over the whole batch) -- sum the shares
            for i, f in enumerate(flat):
                if isinstance(f, G.Tensor) and f.shape == () and vals[i] is not None:
                    vals[i] = np.float32(self.dist.sum_float(float(vals[i])))

        def build(s):
            return [build(x) for x in s] if isinstance(s, list) else vals[s]
        out = build(spec)
        return out[0] if single else out


class phiseg():

    def __init__(self, exp_config, dist=None, init_seed=0, rng_seed=42, bn_double_update=None):
        """bn_double_update (default: $PHX_BN_DOUBLE_UPDATE == 1): reproduce the TF graph's UPDATE_OPS behaviour (SURVEY.md Q4,
        phiseg_model.py:135-141): every training step also runs the generation-mode prior and the evaluation likelihood in
        training mode, so the batch-norm moving statistics of the layers they share with the training instances are updated
        TWICE per step.  Off by default: only the live graph runs (1.9x less forward work)."""
        self.exp_config = exp_config
        self.bn_double_update = (os.environ.get("PHX_BN_DOUBLE_UPDATE", "0") == "1") if bn_double_update is None else bool(bn_double_update)
        self.init_seed = init_seed
        if self.bn_double_update and exp_config.layer_norm is tfnorm.batch_renorm:
            raise NotImplementedError("bn_double_update=True with layer_norm=batch_renorm: the two training-mode instances of a layer would "
                                      "read and update the same renorm state within one step")
        self.checks()
        self.graph = G.reset_default_graph()
        L = exp_config.latent_levels

        # placeholders (phiseg_model.py:26-32)
        self.x_inp = G.placeholder(G.KIND_F32, [None] + list(exp_config.image_size), name='x_input')
        self.s_inp = G.placeholder(G.KIND_U8, [None] + list(exp_config.image_size[0:2]), name='s_input')
        self.s_inp_oh = G.one_hot(self.s_inp, depth=exp_config.nlabels)
        self.training_pl = _Flag('training_time')
        self.lr_pl = _Flag('learning_rate')

        # networks (phiseg_model.py:37-98)
        net_kw = dict(n0=exp_config.n0, resolution_levels=exp_config.resolution_levels, latent_levels=L,
                      norm=exp_config.layer_norm)
        self.z_list, self.mu_list, self.sigma_list = exp_config.posterior(
            self.x_inp, self.s_inp_oh, exp_config.zdim0, training=self.training_pl, **net_kw)
        self.prior_z_list, self.prior_mu_list, self.prior_sigma_list = exp_config.prior(
            self.z_list, self.x_inp, zdim_0=exp_config.zdim0, n_classes=exp_config.nlabels,
            training=self.training_pl, generation_mode=False, **net_kw)
        self.prior_z_list_gen, self.prior_mu_list_gen, self.prior_sigma_list_gen = exp_config.prior(
            self.z_list, self.x_inp, zdim_0=exp_config.zdim0, n_classes=exp_config.nlabels,
            training=self.training_pl, generation_mode=True, scope_reuse=True, **net_kw)
        self.s_out_list = exp_config.likelihood(self.z_list, self.training_pl, n_classes=exp_config.nlabels,
                                                image_size=exp_config.image_size, x=self.x_inp, **net_kw)
        self.s_out_eval_list = exp_config.likelihood(self.prior_z_list_gen, self.training_pl, scope_reuse=True,
                                                     n_classes=exp_config.nlabels, image_size=exp_config.image_size,
                                                     x=self.x_inp, **net_kw)
        # aggregated outputs (phiseg_model.py:106-109)
        self.s_out_eval, self.s_out_eval_sm = G.aggregate_logits(self.s_out_eval_list)

        # losses (phiseg_model.py:113-130)
        self.loss_dict = {}
        terms, weights = [], []
        self.s_out = None
        if getattr(exp_config, 'residual_multinoulli_loss_weight', None) is not None:
            logging.info(' - Adding residual multinoulli loss')
            w = exp_config.residual_multinoulli_loss_weight
            ce, self.s_out = G.residual_multinoulli(self.s_out_list, self.s_inp, w)
            for ii in reversed(range(L)):
                self.loss_dict['residual_multinoulli_loss_lvl%d' % ii] = ce[ii]
                terms.append(ce[ii])
                weights.append(w)
        if getattr(exp_config, 'KL_divergence_loss_weight', None) is not None:
            logging.info(' - Adding hierarchical KL loss')
            w = exp_config.KL_divergence_loss_weight
            lw = [4 ** i for i in range(L)] if exp_config.exponential_weighting else [1] * L
            for ii in reversed(range(L)):
                kl = G.kl_two_gauss(self.mu_list[ii], self.sigma_list[ii], self.prior_mu_list[ii],
                                    self.prior_sigma_list[ii], lw[ii], w)
                self.loss_dict['KL_divergence_loss_lvl%d' % ii] = kl
                terms.append(kl)
                weights.append(w)
        if getattr(exp_config, 'weight_decay_weight', None) is not None:
            logging.info(' - Adding weight decay')                      # add_weight_decay (phiseg_model.py:126-128, 290-299)
            wd = G.l2_of_collection(float(exp_config.weight_decay_weight), 'weight_variables')
            self.loss_dict['weight_decay'] = wd
            terms.append(wd)
            weights.append(1.0)
        self._loss_terms, self._loss_weights = terms, weights       # add_loss_term() rebuilds loss_tot from these
        self.loss_tot = G.weighted_sum(terms, weights)
        self.loss_dict['total_loss'] = self.loss_tot
        self.optimizer = self._make_optimizer(exp_config)
        self.train_step = TrainStep(self.loss_tot)

        self._multi = {}
        self._lazy = {}                                   # graph nodes added after construction (eval_xent, ...): see _lazy_node
        self.keep_checkpoint_every_n_hours = 3.0          # tf.train.Saver(max_to_keep=1, keep_checkpoint_every_n_hours=3) (phiseg_model.py:144)
        self._ckpt_permanent, self._ckpt_last_permanent = {}, time.time()
        self._ckpt_written, self._ckpt_order = {}, {}      # per saver prefix: the steps this instance wrote (set / in write order)
        self.sess = Session(self, getattr(exp_config, 'compute_dtype', 'f32'), rng_seed=rng_seed, dist=dist)
        self.dist = dist

    def checks(self):
        # the label maps are uint8 and the class-aware kernels stop at 256 classes: say so here, not from inside the first launch
        many_class.check_nlabels(self.exp_config.nlabels)
        # likewise the image channels: 1 .. 16 (multichannel.py)
        multichannel.check_image_size(self.exp_config.image_size)

    def add_loss_term(self, name, scalar, weight=1.0):
        """Add a scalar of the caller's making (tfwrapper.losses.dice_loss, cross_entropy_loss, ... on a tensor of this model) to the
        objective: loss_dict[name] = scalar, and loss_tot, loss_dict['total_loss'] and train_step are rebuilt as the weighted sum of the
        old terms plus weight * scalar -- so optimizer.minimize (train_step) follows the new objective.  Legal only before the session
        has compiled a plan or created its ParamStore: the live-variable set and the plans are keyed on the old loss."""
        if self.sess.store is not None or self.sess.plans:
            raise RuntimeError("add_loss_term(%r): the session has already created its parameter store or compiled a plan for the "
                               "old loss -- add loss terms before the first sess.run / set_weights" % (name,))
        if not isinstance(scalar, G.Tensor) or scalar.shape != ():
            raise ValueError("add_loss_term(%r): the term must be a scalar graph tensor, got %r" % (name, scalar))
        if scalar.op.type == "dice_table":
            raise ValueError("add_loss_term(%r): get_dice is a fetch-only table without a gradient; use dice_loss" % (name,))
        if name in self.loss_dict:
            raise ValueError("add_loss_term: loss_dict already has an entry %r" % (name,))
        if self.dist is not None and self.dist.active and scalar.op.attrs.get("sum_over_batches", False):
            raise NotImplementedError("add_loss_term(%r): a batch-summed Dice (macro_robust / sum_over_batches=True) needs a collective "
                                      "over the ranks' sums, which data-parallel training does not have" % (name,))
        G.set_default_graph(self.graph)
        self._loss_terms = self._loss_terms + [scalar]
        self._loss_weights = self._loss_weights + [float(weight)]
        self.loss_dict[name] = scalar
        self.loss_tot = G.weighted_sum(self._loss_terms, self._loss_weights)
        self.loss_dict['total_loss'] = self.loss_tot
        self.train_step = TrainStep(self.loss_tot)
        return scalar

    def _make_optimizer(self, exp_config):
        """phiseg_model.py:135-141: Momentum is instantiated with momentum 0.9 and Nesterov's form, anything else with the learning
        rate alone.  A config without `optimizer` trains with Adam.  The instance only carries hyper-parameters (engine.Plan lowers
        it to phx_adam_tf1 / phx_momentum_tf1), so it has to be an AdamOptimizer or a MomentumOptimizer (or a subclass of one)."""
        opt = getattr(exp_config, 'optimizer', optimizers.AdamOptimizer)
        known = (optimizers.AdamOptimizer, optimizers.MomentumOptimizer)
        if not callable(opt) or (isinstance(opt, type) and not issubclass(opt, known)):
            raise ValueError("exp_config.optimizer must be optimizers.AdamOptimizer or optimizers.MomentumOptimizer (or a subclass), got %r" % (opt,))
        if opt == optimizers.MomentumOptimizer:
            optimizer = opt(learning_rate=self.lr_pl, momentum=0.9, use_nesterov=True)
        else:
            optimizer = opt(learning_rate=self.lr_pl)
        if not isinstance(optimizer, known):
            raise ValueError("exp_config.optimizer produced %r: neither an AdamOptimizer nor a MomentumOptimizer" % (optimizer,))
        return optimizer

    # ---- training loop (phiseg_model.py:166-207) -------------------------------------------------
    def _is_writer(self):
        return self.dist is None or not self.dist.active or self.dist.rank == 0

    def _setup_log_dir_and_continue_mode(self, log_dir=None):
        """phiseg_model.py:821-845: log dir = <log_root>/<log_dir_name>/<experiment_name>; when it already holds a
        model.ckpt-N checkpoint the run continues from the highest N and logs into <log_dir>_cont."""
        from phiseg_code_amd.config import system as sys_config
        from phiseg_code_amd.tfwrapper import utils as tfutils
        cfg = self.exp_config
        self.log_dir = log_dir or os.path.join(sys_config.log_root, cfg.log_dir_name, cfg.experiment_name)
        self.init_checkpoint_path = None
        self.continue_run = False
        self.init_step = 0
        if os.path.isdir(self.log_dir):
            ckpt = tfutils.get_latest_model_checkpoint_path(self.log_dir, 'model.ckpt')
            if ckpt is not False:
                self.init_checkpoint_path = ckpt
                self.continue_run = True
                self.init_step = int(os.path.basename(ckpt).split('-')[-1])
                self.log_dir += '_cont'
                logging.info('--------------------------- Continuing previous run --------------------------------')
                logging.info('Checkpoint path: %s' % self.init_checkpoint_path)
                logging.info('Latest step was: %d' % self.init_step)
        if self._is_writer():
            os.makedirs(self.log_dir, exist_ok=True)

    def train(self, data, num_iter=None, log_every=100, log_dir=None, summaries=False):
        """The reference's train(data) (phiseg_model.py:166-207): continue mode, lr schedule, one ELBO step per iteration,
        `_do_validation` (checkpoint + metrics + best-of checkpoints) every `validation_frequency` steps.  `log_dir=None` keeps
        everything in memory (no checkpoints, no validation); pass a directory to get the reference's on-disk behaviour.
        summaries=True (with a log_dir): the reference's TensorBoard summaries (199-203, 662-701, 704-818) go to ONE event file
        events.out.tfevents.<time>.<host> in the log dir (phiseg_code_amd/summary.py) -- every `tensorboard_update_frequency` steps the
        loss, the learning rate, the mean of every mu / sigma, a histogram of every filter, bias and conv unit's activations and (with
        `do_image_summaries`) the image grids, from one inference-mode run on the batch just trained on; at every validation the
        train / validation loss terms, Dice, GED, NCC and the val_* / generated_* grids.  The summary run reads the parameters and
        writes nothing the training step reads: losses are the same with and without it.  Off (the default): no event file, no extra plan.
        Data-parallel: `data` should draw rank-dependent batches (SyntheticLIDC(cfg, seed=1234 + rank)); the returned /
        logged loss is the global-batch mean; only rank 0 writes files."""
        cfg = self.exp_config
        num_iter = cfg.num_iter if num_iter is None else num_iter
        on_disk = log_dir is not None
        self.init_step, self.continue_run = 0, False
        if on_disk:
            self._setup_log_dir_and_continue_mode(log_dir)
            if self.continue_run:
                self.load_weights(self.init_checkpoint_path)
        self.best_dice, self.best_loss, self.best_ged, self.best_ncc = -1, np.inf, np.inf, -1
        self._summary_writer = None
        if summaries and on_disk and self._is_writer():
            from phiseg_code_amd import summary
            self._summary_writer = summary.EventFileWriter(self.log_dir)
        try:
            return self._train_loop(data, num_iter, log_every, on_disk)
        finally:
            if self._summary_writer is not None:
                self._summary_writer.close()
                self._summary_writer = None

    def _train_loop(self, data, num_iter, log_every, on_disk):
        cfg = self.exp_config
        losses = []
        t0 = time.time()
        for step in range(self.init_step, num_iter):
            lr_key, _ = utils.find_floor_in_list(cfg.lr_schedule_dict.keys(), step)
            lr = cfg.lr_schedule_dict[lr_key]
            x_b, s_b = data.train.next_batch(cfg.batch_size)
            _, loss_tot_eval = self.sess.run([self.train_step, self.loss_tot],
                                             feed_dict={self.x_inp: x_b, self.s_inp: s_b, self.training_pl: True,
                                                        self.lr_pl: lr})
            losses.append(float(loss_tot_eval))
            if log_every and step % log_every == 0:
                world = self.dist.world if (self.dist is not None and self.dist.active) else 1
                logging.info('step %d  loss %.4f  (%.1f img/s)', step, losses[-1],
                             (step - self.init_step + 1) * cfg.batch_size * world / max(time.time() - t0, 1e-9))
            if self._summary_writer is not None and step % cfg.tensorboard_update_frequency == 0:
                self._write_training_summary(step, x_b, s_b, lr)
            vf = getattr(cfg, 'validation_frequency', None)
            if on_disk and vf and step % vf == 0:
                self._do_validation(data)
        return losses

    # ---- TensorBoard summaries (phiseg_model.py:199-203, 662-701, 704-818) -----------------------------------
    def _summary_spec(self):
        """What one summary run fetches, built once: the loss, every mu / sigma, the output levels, s_accum, and the output of every
        conv unit the loss depends on (the never-consumed up-sampling branches, SURVEY.md Q1, and the generation-mode prior / the
        evaluation likelihood are not reachable from loss_tot: the reference histograms their activations too, we do not)."""
        if getattr(self, '_summary_spec_cache', None) is None:
            L = self.exp_config.latent_levels
            seen, stack = set(), [self.loss_tot.op]
            while stack:
                op = stack.pop()
                if op not in seen:
                    seen.add(op)
                    stack.extend(i.op for i in op.inputs)
            units, used = [], {}
            for op in self.graph.ops:
                if op in seen and op.type == 'conv_unit':
                    w = op.attrs['W'].name
                    scope = w[:-2] if w.endswith('/W') else op.name          # the unit's variable scope (tf: the layer's name scope)
                    k = used.get(scope, 0)
                    used[scope] = k + 1
                    units.append(((scope if k == 0 else '%s_%d' % (scope, k)) + '/activations', op.outputs[0]))
            scalars = []
            for ii in range(L):
                scalars += [('average_mu_lvl%d' % ii, self.mu_list[ii]), ('average_sigma_lvl%d' % ii, self.sigma_list[ii]),
                            ('average_prior_mu_lvl%d' % ii, self.prior_mu_list[ii]), ('average_prior_sigma_lvl%d' % ii, self.prior_sigma_list[ii])]
            scalars = [(tag, t) for tag, t in scalars if isinstance(t, G.Tensor) and len(t.shape) > 0]
            # s_accum[ii] = s_out_list[L-1] + ... + s_out_list[ii] (phiseg_model.py:245-258): level L-1 is the last output level itself,
            # level 0 is self.s_out, the levels between are added to the graph here
            s_out = self.s_out if self.s_out is not None else self._s_out_sum()
            accum = []
            for ii in range(L):
                if ii == L - 1:
                    accum.append(self.s_out_list[ii])
                elif ii == 0:
                    accum.append(s_out)
                else:
                    accum.append(self._lazy_node('s_accum_%d' % ii, lambda ii=ii: G.aggregate_logits(self.s_out_list[ii:])[0]))
            images = [('s_out', s_out)] + [e for ii in range(L) for e in (('s_out_list_%d' % ii, self.s_out_list[ii]), ('s_accum_list_%d' % ii, accum[ii]))]
            fetches = []
            for t in [self.loss_tot] + [t for _, t in scalars] + [t for _, t in images] + [t for _, t in units]:
                if not any(t is f for f in fetches):
                    fetches.append(t)
            self._summary_spec_cache = dict(units=units, scalars=scalars, images=images, fetches=fetches, hist={})
        return self._summary_spec_cache

    def _summary_run(self, x_b, s_b, lr, histograms):
        """One inference-mode run of the summary plan on (x_b, s_b); behind the replay, on the plan's stream: one histogram call over the
        activations and one over the parameter arena's filters and biases (histograms=True), and one grid launch per image summary.
        -> (loss, {tag: (count row, stats row)} or None, [(name, uint8 grid)]).  Advances the sampling noise step, which no training
        step reads (training plans key their noise by the optimiser step)."""
        from phiseg_code_amd import runtime as rt
        from phiseg_code_amd import summary
        cfg = self.exp_config
        spec = self._summary_spec()
        fd = {self.x_inp: x_b, self.s_inp: s_b, self.training_pl: False}
        if lr is not None:
            fd[self.lr_pl] = lr
        plan, _ = self.sess.run_buffers(spec['fetches'], fd)
        stream = plan.stream
        hist = None
        if histograms:
            if id(plan) not in spec['hist']:
                store = self.sess._ensure_store()
                # the activations, then any mu / sigma that is not itself a conv unit's output (its mean comes from the same call)
                segs = list(spec['units']) + [(tag, t) for tag, t in spec['scalars'] if not any(t is u for _, u in spec['units'])]
                seg_t, seg_tags = [t for _, t in segs], [tag for tag, _ in segs]
                bufs = [plan.val[t] for t in seg_t]
                act = summary.Histogrammer([(b.ptr, b.n, b.dt) for b in bufs])
                pvars = [v for name, v in self.graph.variables.items() if v.trainable and (name.endswith('/W') or name.endswith('/b'))]
                par = summary.Histogrammer([(store.ptr(v), v.size, rt.F32) for v in pvars])
                spec['hist'][id(plan)] = (act, seg_t, seg_tags, par, [v.name + '_0' for v in pvars])       # (tf: '<name>:0' -> '<name>_0')
            act, seg_t, seg_tags, par, par_tags = spec['hist'][id(plan)]
            act.run(stream)
            par.run(stream)
        grids = []
        if getattr(cfg, 'do_image_summaries', False):
            B = int(np.asarray(x_b).shape[0])
            xb, sb = plan.feeds['x_input'], plan.feeds['s_input']
            H, W = xb.shape[1], xb.shape[2]
            grids.append(('x_inp', summary.grid_image_device(xb.ptr, B, H, W, xb.shape[3], stream)))
            grids.append(('s_inp', summary.grid_u8_device(sb.ptr, summary.GRID_LABELS_U8, B, H, W, 1, stream)))
            for name, t in spec['images']:
                b = plan.val[t]
                grids.append((name, summary.grid_u8_device(b.ptr, summary.GRID_LOGITS_F32, B, H, W, b.shape[-1], stream, shift=b.shift)))
        plan.sync()
        world = self.dist.world if (self.dist is not None and self.dist.active) else 1
        loss = float(plan.fetch(self.loss_tot)) * world        # (data parallel: the writer rank's share of the global mean -> its batch's loss)
        if histograms:
            a_counts, a_stats = act.result(stream)
            p_counts, p_stats = par.result(stream)
            summary.check_finite(par_tags, p_stats)
            summary.check_finite(seg_tags, a_stats)
            hist = dict(par=(par_tags, p_counts, p_stats), act=([tag for tag, _ in spec['units']], a_counts, a_stats), seg_t=seg_t)
        grids = [(name, g.cpu().numpy()) for name, g in grids]
        self._advance_noise()
        return loss, hist, grids

    def _write_training_summary(self, step, x_b, s_b, lr):
        """phiseg_model.py:199-203: sess.run(self.summary, {x_inp, s_inp, training_pl: False, lr_pl}) + add_summary + flush"""
        from phiseg_code_amd import summary as S
        loss, hist, grids = self._summary_run(x_b, s_b, lr, histograms=True)
        spec = self._summary_spec()
        values = [S.scalar_value('batch_total_loss', loss), S.scalar_value('learning_rate', lr)]
        if any(name.endswith('/renorm_mean') for name in self.graph.variables):
            # normalisation.py:128-129: the clipping bounds of the batch-renorm layers -- the ones the training step `step` ran with
            rmax, dmax = tfnorm.renorm_clip(step)
            values += [S.scalar_value('rmax_clip', rmax), S.scalar_value('dmax_clip', dmax)]
        _, a_counts, a_stats = hist['act']
        for tag, t in spec['scalars']:
            st = a_stats[[i for i, u in enumerate(hist['seg_t']) if u is t][0]]
            values.append(S.scalar_value(tag, st[S.STAT_SUM] / max(st[S.STAT_NUM], 1.0)))
        for tags, counts, stats in (hist['par'], hist['act']):
            for i, tag in enumerate(tags):
                st = stats[i]
                values.append(S.histogram_value(tag, st[S.STAT_MIN], st[S.STAT_MAX], st[S.STAT_NUM], st[S.STAT_SUM], st[S.STAT_SUM_SQUARES], counts[i]))
        values += [S.image_value('train_%s/image/0' % name, g) for name, g in grids]
        self._summary_writer.add_summary(values, step)
        self._summary_writer.flush()

    def _write_validation_summary(self, global_step, names, val_out, train_out, out, val_batch):
        """phiseg_model.py:662-701: the validation summary (loss terms of the validation batch, Dice / ELBO / GED / NCC, the val_* and
        generated_* grids) and the train summary (loss terms of a training batch), both at global_step."""
        from phiseg_code_amd import summary as S
        cfg = self.exp_config
        values = [S.scalar_value('val_batch_%s' % n, v) for n, v in zip(names, val_out)]
        if val_batch is not None and getattr(cfg, 'do_image_summaries', False):
            val_x, val_s = val_batch
            _, _, grids = self._summary_run(val_x, val_s, None, histograms=False)
            values += [S.image_value('val_%s/image/0' % name, g) for name, g in grids]
            B = int(np.asarray(val_x).shape[0])
            plan, (lg,) = self.sess.run_buffers([self.s_out_eval], {self.training_pl: False, self.x_inp: val_x})
            xb = plan.feeds['x_input']
            H, W = xb.shape[1], xb.shape[2]
            seg = S.grid_u8_device(lg.ptr, S.GRID_LOGITS_F32, B, H, W, lg.shape[-1], plan.stream, shift=lg.shift)
            xin = S.grid_image_device(xb.ptr, B, H, W, xb.shape[3], plan.stream)
            plan.sync()
            values += [S.image_value('generated_seg/image/0', seg.cpu().numpy()), S.image_value('generated_x_in/image/0', xin.cpu().numpy())]
            self._advance_noise()
        psd = np.asarray(out['per_structure_dice']).reshape(-1)
        values += [S.scalar_value('validation_dice_tot_score', out['dice']), S.scalar_value('validation_dice_mean_score', float(np.mean(psd)))]
        values += [S.scalar_value('validation_dice_lbl_%d' % ii, psd[ii]) for ii in range(psd.size)]
        values += [S.scalar_value('validation_neg_elbo', out['loss']), S.scalar_value('validation_GED', out['ged']),
                   S.scalar_value('validation_NCC', out['ncc'])]
        self._summary_writer.add_summary(values, global_step)
        self._summary_writer.add_summary([S.scalar_value('train_batch_%s' % n, v) for n, v in zip(names, train_out)], global_step)
        self._summary_writer.flush()

    # ---- validation (phiseg_model.py:530-660): N Monte-Carlo samples per image, metrics on the device ---------------
    def _do_validation(self, data):
        """For every validation image: `validation_samples` segmentation samples + the ELBO against one randomly chosen
        annotation (phiseg_model.py:570-586), then GED over the foreground labels, variance-NCC and the Dice of the mean
        prediction (586-613).  The reference scores these in Python loops on the host (N*M + N^2 + M^2 IoU evaluations per
        image); here they are one libphx call per image (utils.validation_metrics -> phx_validation_metrics).
        -> dict(loss, dice, per_structure_dice, ged, ncc), the averages the reference logs (615-634)."""
        cfg = self.exp_config
        store = self.sess._ensure_store()
        global_step = int(store.step.cpu().item()) - 1               # tf global_step - 1 (phiseg_model.py:532)
        dp = self.dist is not None and self.dist.active
        # Data parallel: every decision below that leads to a collective (save_weights averages the batch-norm moving statistics
        # over the replicas) must be the same on all ranks -- the per-rank metrics differ (noise offsets, random annotators).  Rank 0
        # decides; its flags are broadcast.  The replicas' moving statistics are averaged ONCE, here, so that the best-of saves
        # further down run no collective at all.
        save = getattr(self, 'log_dir', None) is not None and os.path.isdir(getattr(self, 'log_dir', '') or '')
        if dp:
            save = bool(self.dist.broadcast_flags([1 if save else 0])[0])
            self._average_replica_state()
        if save:
            self.save_weights(os.path.join(self.log_dir, 'model.ckpt-%d' % global_step), format=self._ckpt_format(),
                              keep_prefix='model.ckpt', max_to_keep=1, average_state=False)
        names, val_out, train_out, val_batch = [], [], [], None
        if hasattr(data.validation, 'next_batch'):                   # BATCH VALIDATION of every loss term (537-556)
            names = list(self.loss_dict.keys())
            val_x, val_s = data.validation.next_batch(cfg.batch_size)
            val_batch = (val_x, val_s)
            val_out = self.sess.run(list(self.loss_dict.values()),
                                    feed_dict={self.x_inp: val_x, self.s_inp: val_s, self.training_pl: False})
            train_x, train_s = data.train.next_batch(cfg.batch_size)
            train_out = self.sess.run(list(self.loss_dict.values()),
                                      feed_dict={self.x_inp: train_x, self.s_inp: train_s, self.training_pl: False})
            logging.info('----- Step: %d ------' % global_step)
            logging.info('BATCH VALIDATION:')
            for ii, loss_name in enumerate(names):
                logging.info('%s | training: %f | validation: %f' % (loss_name, train_out[ii], val_out[ii]))
        imgs, labs = data.validation.images, data.validation.labels
        n_img = imgs.shape[0] if cfg.num_validation_images == 'all' else min(cfg.num_validation_images, imgs.shape[0])
        ns = cfg.validation_samples
        dice_list, elbo_list, ged_list, ncc_list = [], [], [], []
        for ii in range(n_img):
            x = imgs[ii, ...].reshape([1] + list(cfg.image_size))
            s_gt_arr = labs[ii, ...]                                   # [X, Y, num annotators]
            s = s_gt_arr[:, :, np.random.choice(cfg.annotator_range)]
            x_b, s_b = np.tile(x, [ns, 1, 1, 1]), np.tile(s, [ns, 1, 1])
            fd = {self.training_pl: False, self.x_inp: x_b, self.s_inp: s_b}
            sm_arr, elbo = self.sess.run([self.s_out_eval_sm, self.loss_tot], feed_dict=fd)
            self._advance_noise()
            gts = np.ascontiguousarray(s_gt_arr.transpose((2, 0, 1)))  # num annotators x X x Y
            ged, ncc, dice = utils.validation_metrics(sm_arr[None], gts[None], s[None], cfg.nlabels)
            dice_list.append(dice[0])
            elbo_list.append(float(elbo))
            ged_list.append(float(ged[0]))
            ncc_list.append(float(ncc[0]))
        dice_arr = np.asarray(dice_list)
        out = dict(loss=utils.list_mean(elbo_list), dice=float(np.mean(dice_arr)), per_structure_dice=dice_arr.mean(axis=0),
                   ged=utils.list_mean(ged_list), ncc=utils.list_mean(ncc_list))
        logging.info('FULL VALIDATION (%d images):' % n_img)
        logging.info(' - Mean foreground dice: %.4f' % np.mean(out['per_structure_dice']))
        logging.info(' - Mean (neg.) ELBO: %.4f' % out['loss'])
        logging.info(' - Mean GED: %.4f' % out['ged'])
        logging.info(' - Mean NCC: %.4f' % out['ncc'])
        # best-of checkpoints (phiseg_model.py:638-660)
        if not hasattr(self, 'best_dice'):
            self.best_dice, self.best_loss, self.best_ged, self.best_ncc = -1, np.inf, np.inf, -1
        mean_dice = float(np.mean(out['per_structure_dice']))
        cands = (('dice', mean_dice, mean_dice >= self.best_dice, 'New best validation Dice! (%.3f)'),
                 ('loss', out['loss'], out['loss'] <= self.best_loss, 'New best validation loss! (%.3f)'),
                 ('ged', out['ged'], out['ged'] <= self.best_ged, 'New best GED score! (%.3f)'),
                 ('ncc', out['ncc'], out['ncc'] >= self.best_ncc, 'New best NCC score! (%.3f)'))
        flags = [1 if c[2] else 0 for c in cands]
        if dp:
            flags = self.dist.broadcast_flags(flags)                   # rank 0's metrics decide on every rank
        for (key, value, _, fmt), better in zip(cands, flags):
            if better:
                setattr(self, 'best_' + key, value)
                logging.info(fmt % value)
                if save:                                               # (the reference: Saver(max_to_keep=2) per best-of saver)
                    self.save_weights(os.path.join(self.log_dir, 'model_best_%s.ckpt-%d' % (key, global_step)), format=self._ckpt_format(),
                                      keep_prefix='model_best_%s.ckpt' % key, max_to_keep=2, average_state=False)
        if getattr(self, '_summary_writer', None) is not None:
            self._write_validation_summary(global_step, names, val_out, train_out, out, val_batch)
        return out

    def _average_replica_state(self):
        """Data parallel: batch-norm moving statistics are per replica; average them over the ranks.  The whole
        state arena is averaged: a batch-renorm layer's renorm_mean / renorm_stddev with it (its two weights are equal on all ranks)."""
        store = self.sess._ensure_store()
        if self.dist is not None and self.dist.active and store.n_state:
            avg = store.state.clone()
            self.dist.allreduce_sum(avg)
            avg /= self.dist.world
            store.state.copy_(avg)
            engine.device_sync()

    def _note_checkpoint(self, keep_prefix, path):
        import re
        m = re.search(re.escape(keep_prefix) + r'-(\d+)(?:\.npz)?$', os.path.basename(path))
        if m:
            st = int(m.group(1))
            self._ckpt_written.setdefault(keep_prefix, set()).add(st)
            order = self._ckpt_order.setdefault(keep_prefix, [])
            if st in order:
                order.remove(st)
            order.append(st)

    def _prune_checkpoints(self, directory, keep_prefix, max_to_keep):
        """tf.train.Saver(max_to_keep=...) (phiseg_model.py:144-148): delete all but the newest `max_to_keep` checkpoints named
        <keep_prefix>-<step>(.npz | .index + .data-*); -> the retained prefixes, oldest first."""
        import glob
        import re
        found = {}
        # like Saver._last_checkpoints: only checkpoints THIS instance has written are rotated -- files an earlier run left in the
        # directory (a fresh run into an old log_dir writes model.ckpt-0 while model.ckpt-5000 is still there) are never touched
        mine = self._ckpt_written.setdefault(keep_prefix, set())
        for f in glob.glob(os.path.join(directory, keep_prefix + '-*')):
            m = re.match(re.escape(keep_prefix) + r'-(\d+)(\.npz|\.index|\.data-\d+-of-\d+)$', os.path.basename(f))
            if m and int(m.group(1)) in mine:
                found.setdefault(int(m.group(1)), []).append(f)
        steps = [st for st in self._ckpt_order.get(keep_prefix, []) if st in found]      # write order, as tf.train.Saver keeps it
        # keep_checkpoint_every_n_hours (3 for the training saver): a checkpoint that falls out of the max_to_keep window is kept for
        # good when that many hours of training have passed since the last one kept this way
        keep_h = self.keep_checkpoint_every_n_hours if keep_prefix == 'model.ckpt' else None
        perm = self._ckpt_permanent.setdefault(keep_prefix, set())
        for s in steps[:-max_to_keep] if max_to_keep > 0 else []:
            if s in perm:
                continue
            if keep_h is not None and time.time() - self._ckpt_last_permanent >= keep_h * 3600.0:
                perm.add(s)
                self._ckpt_last_permanent = time.time()
                continue
            for f in found[s]:
                try:
                    os.remove(f)
                except OSError:
                    pass
        kept = [s for s in steps if s in perm or s in steps[-max_to_keep:]]
        return [os.path.join(directory, '%s-%d' % (keep_prefix, s)) for s in kept]

    # ---- checkpoints (npz keyed by the TF variable names of SURVEY.md Appendix B) -------------------
    def _ckpt_format(self):
        """exp_config.checkpoint_format: 'npz' (default) or 'tf' (TensorFlow tensor bundles, as the reference's Saver writes)"""
        return getattr(self.exp_config, 'checkpoint_format', 'npz')

    def save_weights(self, path, format='npz', keep_prefix=None, max_to_keep=0, average_state=True):
        """What tf.train.Saver writes for this graph (phiseg_model.py:144-148, 534-535): every variable, the optimiser's slots under
        TF's names -- '<var>/Adam' (m) and '<var>/Adam_1' (v) for Adam, '<var>/Momentum' (the accumulator) for Momentum -- and the
        step (TF keeps beta1_power / beta2_power and global_step; one integer carries the same information).  File: <path>.npz, or
        with format='tf' a TensorFlow tensor-bundle checkpoint <path>.index + <path>.data-00000-of-00001
        (tfwrapper/tf_checkpoint.py) that tf.train.Saver.restore of the reference graph accepts: same variable names and
        global_step, with beta1_power / beta2_power for Adam (TF's MomentumOptimizer has no non-slot variables).  Data-parallel:
        batch-norm moving statistics are averaged over the replicas first (per-replica statistics); rank 0
        writes."""
        store = self.sess._ensure_store()
        if average_state:              # (a collective: every rank must call save_weights -- _do_validation averages once itself)
            self._average_replica_state()
        if not self._is_writer():
            return
        blob = dict(store.export())
        for name, per_var in store.export_slots().items():
            for slot, val in per_var.items():
                blob[name + '/' + slot] = val
        step = int(store.step.cpu().numpy()[0])
        if format == 'tf':
            from phiseg_code_amd.tfwrapper import tf_checkpoint
            if path.endswith('.npz'):
                path = path[:-4]
            if store.adam_m is not None:
                # TF 1.x AdamOptimizer's non-slot variables: beta_power = beta^(t + 1) after t updates; minimize() counts global_step
                b1, b2 = optimizers.AdamOptimizer.beta1, optimizers.AdamOptimizer.beta2
                blob['beta1_power'] = np.asarray(b1 ** (step + 1), dtype=np.float32)
                blob['beta2_power'] = np.asarray(b2 ** (step + 1), dtype=np.float32)
            blob['global_step'] = np.asarray(step, dtype=np.int64)
            tf_checkpoint.write(path, blob)
            d = os.path.dirname(os.path.abspath(path))
            if keep_prefix:
                self._note_checkpoint(keep_prefix, path)
            kept = self._prune_checkpoints(d, keep_prefix, max_to_keep) if keep_prefix else None
            tf_checkpoint.update_checkpoint_state(d, os.path.basename(path), all_paths=[os.path.basename(k) for k in kept] if kept else None)
            return
        if format != 'npz':
            raise ValueError("save_weights: format is 'npz' or 'tf'")
        if not path.endswith('.npz'):
            path += '.npz'
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = path + '.tmp.npz'
        np.savez(tmp, __step__=np.asarray([step], dtype=np.int32), **blob)
        os.replace(tmp, path)
        if keep_prefix:
            self._note_checkpoint(keep_prefix, path)
            self._prune_checkpoints(os.path.dirname(os.path.abspath(path)), keep_prefix, max_to_keep)

    def load_weights(self, log_dir=None, type='latest', **kwargs):
        """phiseg_model.py:505-525 (+ 'best_ncc', which the reference writes but cannot load -- SURVEY.md Q9).  `log_dir` may
        also be a checkpoint file / prefix.  Restores variables, the slots of the model's own optimiser ('<var>/Adam' + '<var>/Adam_1'
        or '<var>/Momentum') and the step; a checkpoint without them -- weights only, or written under the other optimiser -- loads
        the variables, resets the optimiser state and the step, and logs one warning.  A prefix with a `.index` file next to it is a TensorFlow
        tensor-bundle checkpoint -- one written by the reference's tf.train.Saver or by save_weights(format='tf') -- and is
        read directly (tfwrapper/tf_checkpoint.py); variables the checkpoint lacks keep their values, as Saver.restore of a
        sub-graph would."""
        from phiseg_code_amd.tfwrapper import utils as tfutils
        if not log_dir:
            log_dir = getattr(self, 'log_dir', None)
        path = log_dir
        if os.path.isdir(log_dir):
            names = {'latest': 'model.ckpt', 'best_dice': 'model_best_dice.ckpt', 'best_loss': 'model_best_loss.ckpt',
                     'best_ged': 'model_best_ged.ckpt', 'best_ncc': 'model_best_ncc.ckpt'}
            if type == 'iter':
                assert 'iteration' in kwargs, "argument 'iteration' must be provided for type='iter'"
                path = os.path.join(log_dir, 'model.ckpt-%d' % kwargs['iteration'])
            elif type in names:
                path = tfutils.get_latest_model_checkpoint_path(log_dir, names[type])
                if path is False:
                    raise FileNotFoundError('no %s checkpoint in %s' % (type, log_dir))
            else:
                raise ValueError('Argument type=%s is unknown. type can be latest/iter.' % type)
        store = self.sess._ensure_store()
        names = set(self.graph.variables)
        if os.path.exists(path + '.index') and not os.path.exists(path + '.npz'):
            from phiseg_code_amd.tfwrapper import tf_checkpoint
            ck = tf_checkpoint.read(path)
            files = list(ck)
            if 'global_step' in ck:
                step = int(ck['global_step'])
            elif 'beta1_power' in ck:            # beta1^(t + 1) after t updates
                step = max(0, int(round(np.log(float(ck['beta1_power'])) / np.log(optimizers.AdamOptimizer.beta1))) - 1)
            else:
                step = 0
        else:
            if not os.path.exists(path) and os.path.exists(path + '.npz'):
                path += '.npz'
            ck = np.load(path)
            files = ck.files
            step = int(ck['__step__'][0]) if '__step__' in files else 0
        store.load({k: ck[k] for k in files if k in names})
        missing = sorted(names - set(files))
        if missing:                      # (a name-mapping error would otherwise pass silently: those variables keep their values)
            logging.warning('load_weights: %d of %d graph variables are not in %s and keep their values (first: %s)',
                            len(missing), len(names), path, ', '.join(missing[:3]))
        self.last_load_missing = missing
        fset = set(files)
        slots = {}
        for name, v in self.graph.variables.items():
            if v.trainable and all(name + '/' + sn in fset for sn in store.slot_names):
                slots[name] = {sn: ck[name + '/' + sn] for sn in store.slot_names}
        if slots:
            store.load_slots(slots)
            store.set_step(step)
        else:
            other = [sn for sn in ('Adam', 'Momentum') if sn not in store.slot_names and any(k.endswith('/' + sn) for k in files)]
            want = ' + '.join("'<var>/%s'" % sn for sn in store.slot_names)
            logging.warning('load_weights: %s holds %s, not the %s slots of this model\'s optimiser: weights only -- the optimiser '
                            'state and the step are reset', path, "'<var>/%s' slots" % other[0] if other else 'no optimiser slots', want)
            store.reset_optimizer()
        self.sess._lr = None
        if self.dist is not None and self.dist.active:
            for t in [store.params, store.state] + store.slot_arenas():
                self.dist.broadcast_(t)
            engine.device_sync()

    def set_weights(self, values):
        self.sess._ensure_store().load(values)

    # ---- inference API (phiseg_model.py:313-375) -------------------------------------------------
    def generate_prior_samples(self, x_in, return_params=False):
        fd = {self.training_pl: False, self.x_inp: x_in}
        if return_params:
            z, mu, sg = self.sess.run([self.prior_z_list_gen, self.prior_mu_list_gen, self.prior_sigma_list_gen], fd)
            return z, mu, sg
        return self.sess.run(self.prior_z_list_gen, fd)

    def sampling_graph(self, num_samples):
        """(s_out_eval, s_out_eval_sm) of a graph instance that draws `num_samples` segmentations PER fed image in one pass:
        the prior's encoder -- a function of x alone -- runs once per image, its features are repeated num_samples times
        (graph.tile_batch) and the latent path + likelihood run at batch B * num_samples.  prob_unet2D: the prior encoder AND the
        likelihood's U-Net run once per image, mu / sigma are repeated and only the recombination layers run per sample.  Same variables (scope reuse) and
        the same Philox stream as s_out_eval_sm; output rows b * num_samples + k = sample k of image b."""
        if num_samples not in self._multi:
            cfg = self.exp_config
            net_kw = dict(n0=cfg.n0, resolution_levels=cfg.resolution_levels, latent_levels=cfg.latent_levels, norm=cfg.layer_norm)
            G.set_default_graph(self.graph)
            z_gen, _, _ = cfg.prior(self.z_list, self.x_inp, zdim_0=cfg.zdim0, n_classes=cfg.nlabels, training=self.training_pl,
                                    generation_mode=True, scope_reuse=True, tile_samples=num_samples, **net_kw)
            s_list = cfg.likelihood(z_gen, self.training_pl, scope_reuse=True, n_classes=cfg.nlabels, image_size=cfg.image_size,
                                    x=self.x_inp, **net_kw)
            self._multi[num_samples] = G.aggregate_logits(s_list)
        return self._multi[num_samples]

    def _one_pass_prior(self):
        """Do predict / the Monte-Carlo map methods draw their samples through sampling_graph?  Always for the phiseg prior; for
        prob_unet2D only with exp_config.one_pass_sampling = True (absent = False: x tiled / looped, as the reference does)."""
        name = getattr(self.exp_config.prior, '__name__', '')
        return name == 'phiseg' or (name == 'prob_unet2D' and bool(getattr(self.exp_config, 'one_pass_sampling', False)))

    def predict(self, x_in, num_samples=50, return_softmax=False):
        """phiseg_model.py:337-354: mean soft-max over num_samples prior samples, arg-max.  One pass per call when the prior
        has an x-only encoder to share (sampling_graph); prob_unet2D keeps the reference's loop unless exp_config.one_pass_sampling
        is set (then its U-Net and prior encoder run once and only the recombination layers run per sample)."""
        fd = {self.training_pl: False, self.x_inp: x_in}
        if num_samples > 1 and self._one_pass_prior():
            _, sm = self.sampling_graph(num_samples)
            sm_all = self.sess.run(sm, feed_dict=fd)                          # [B * n, X, Y, C]
            self._advance_noise()
            cumsum_sm = sm_all.reshape((-1, num_samples) + sm_all.shape[1:]).sum(axis=1)
            if return_softmax:
                return np.argmax(cumsum_sm, axis=-1), cumsum_sm / num_samples
            return np.argmax(cumsum_sm, axis=-1)
        cumsum_sm = self.sess.run(self.s_out_eval_sm, feed_dict=fd)
        for _ in range(num_samples - 1):
            self._advance_noise()
            cumsum_sm = cumsum_sm + self.sess.run(self.s_out_eval_sm, feed_dict=fd)
        self._advance_noise()
        if return_softmax:
            return np.argmax(cumsum_sm, axis=-1), cumsum_sm / num_samples
        return np.argmax(cumsum_sm, axis=-1)

    def predict_segmentation_sample(self, x_in, return_softmax=False):
        fd = {self.training_pl: False, self.x_inp: x_in}
        out = self.sess.run(self.s_out_eval_sm if return_softmax else self.s_out_eval, feed_dict=fd)
        self._advance_noise()
        return out if return_softmax else np.argmax(out, axis=-1)

    def predict_segmentation_sample_levels(self, x_in, return_softmax=False):
        fd = {self.training_pl: False, self.x_inp: x_in}
        lv = self.sess.run(self.s_out_eval_list, feed_dict=fd)
        self._advance_noise()
        if return_softmax:
            e = [np.exp(v - v.max(axis=-1, keepdims=True)) for v in lv]
            return [v / v.sum(axis=-1, keepdims=True) for v in e]
        return lv

    # ---- graph nodes the reference builds in __init__ and this class adds on first use, as sampling_graph does: __init__'s graph,
    # its op order and the plans compiled from it stay exactly as they are for everyone who never asks for these ------------------
    def _lazy_node(self, name, build):
        if name not in self._lazy:
            G.set_default_graph(self.graph)
            self._lazy[name] = build()
        return self._lazy[name]

    @property
    def eval_xent(self):
        """tf.nn.softmax_cross_entropy_with_logits_v2(labels=s_inp_oh, logits=s_out_eval) (phiseg_model.py:111): [B, X, Y]"""
        return self._lazy_node("eval_xent", lambda: G.softmax_xent_map(self.s_out_eval, self.s_inp))

    @property
    def s_out_eval_sm_list(self):
        """softmax of every level of s_out_eval_list (phiseg_model.py:100-102)"""
        return self._lazy_node("s_out_eval_sm_list", lambda: [G.aggregate_logits([t])[1] for t in self.s_out_eval_list])

    def _s_out_sum(self):
        """_aggregate_output_list(s_out_list) without labels: self.s_out is an output of the loss operator and needs s_inp."""
        return self._lazy_node("s_out_sum", lambda: G.aggregate_logits(self.s_out_list)[0])

    # ---- latents in, latents out (phiseg_model.py:313-322, 478-502) ---------------------------------------------------------------
    def generate_samples_from_z(self, z_list, x_in, output_all_levels=False):
        """Decode chosen latents: z_list[l] is fed for level l ([B, h_l, w_l, zdim]); a shorter list (or None entries) leaves the
        remaining levels to the posterior, which then needs s_inp -- use sess.run with a feed_dict for that."""
        fd = {t: d for t, d in zip(self.z_list, z_list) if d is not None}
        fd[self.training_pl] = False
        fd[self.x_inp] = x_in
        if output_all_levels:
            return self.sess.run(self.s_out_list, feed_dict=fd)
        return self.sess.run(self._s_out_sum(), feed_dict=fd)

    def generate_samples_from_prior(self, x_in, output_all_levels=False):
        """(The reference passes output_all_levels in the x_in slot of generate_samples_from_z, SURVEY.md Q8: fixed here.)"""
        z_samples = self.generate_prior_samples(x_in)
        out = self.generate_samples_from_z(z_samples, x_in, output_all_levels)
        self._advance_noise()
        return out

    def generate_posterior_samples(self, x_in, s_in, return_params=False):
        fd = {self.training_pl: False, self.x_inp: x_in, self.s_inp: s_in}
        if return_params:            # one run: mu and sigma are the parameters of the very samples returned
            out = tuple(self.sess.run([self.z_list, self.mu_list, self.sigma_list], feed_dict=fd))
        else:
            out = self.sess.run(self.z_list, feed_dict=fd)
        self._advance_noise()
        return out

    def generate_all_output_levels(self, x_in, s_in=None):
        """s_out_list is the likelihood of POSTERIOR samples: it needs s_inp, which the reference's method forgets to feed."""
        fd = {self.x_inp: x_in, self.training_pl: False}
        if s_in is not None:
            fd[self.s_inp] = s_in
        y_list = self.sess.run(self.s_out_list, feed_dict=fd)
        self._advance_noise()
        return y_list

    # ---- Monte-Carlo uncertainty / error maps (phiseg_model.py:378-475): one sampling pass, maps formed on the device ---------------
    def _mc_maps(self, x_in, num_samples, maps, s_gt=None, amax=False):
        """Draw num_samples segmentations per image in ONE pass (sampling_graph where the prior shares an x-only encoder -- phiseg, and
        prob_unet2D with exp_config.one_pass_sampling --, x tiled to batch B * num_samples on s_out_eval otherwise: inference-mode normalisation makes the rows independent), hand the plan's
        device buffers to phx_mc_stats on the plan's stream and copy back only the maps.  -> (dict name -> [B, X, Y], arg-max of
        the mean soft-max [B, X, Y] or None).  Advances the noise step once."""
        import torch
        from phiseg_code_amd import uncertainty as unc
        n = int(num_samples)
        if n < 2 or n > 1024:
            raise ValueError("num_samples must be 2 .. 1024 (got %d)" % n)
        x = np.asarray(x_in)
        B = x.shape[0]
        if self._one_pass_prior():
            lg_t, sm_t = self.sampling_graph(n)
        else:
            lg_t, sm_t = self.s_out_eval, self.s_out_eval_sm
            x = np.repeat(x, n, axis=0)                                        # rows b * n + k, as sampling_graph lays them out
        need_lg = any(m in ("xent_mean", "cov_trace") for m in maps)
        need_sm = amax or any(m not in ("xent_mean", "cov_trace") for m in maps)
        tensors = ([lg_t] if need_lg else []) + ([sm_t] if need_sm else [])
        plan, bufs = self.sess.run_buffers(tensors, {self.training_pl: False, self.x_inp: x})
        lg = bufs[0] if need_lg else None
        sm = bufs[-1] if need_sm else None
        X, Y, C = (lg or sm).shape[1:]
        sref = None
        if s_gt is not None:
            sref = torch.as_tensor(np.ascontiguousarray(np.asarray(s_gt).reshape((B, X, Y)), dtype=np.uint8)).to((lg or sm).t.device)
            torch.cuda.current_stream().synchronize()                          # uploaded on torch's stream, read on the plan's
        out, _, amax_t = unc.mc_stats_device(lg.ptr if lg else None, sm.ptr if sm else None, None, sref.data_ptr() if sref is not None else None,
                                             B, n, 0, X * Y, C, list(maps), plan.stream, amax=amax)
        plan.sync()
        res = {m: out[:, unc.PLANE[m]].cpu().numpy().reshape((B, X, Y)) for m in maps}
        am = amax_t.cpu().numpy().reshape((B, X, Y)) if amax else None
        self._advance_noise()
        return res, am

    @staticmethod
    def _per_image(a):
        """The reference squeezes the batch axis of a single image: [1, X, Y] -> [X, Y]; B > 1 keeps [B, X, Y] (an extension)."""
        return a[0] if a.shape[0] == 1 else a

    def predict_segmentation_sample_variance_sm_cov(self, x_in, num_samples):
        """phiseg_model.py:378-403: the sum of the eigenvalues (= trace) of the covariance over the samples of the clipped LOGITS of
        all classes but the last."""
        res, _ = self._mc_maps(x_in, num_samples, ("cov_trace",))
        return self._per_image(res["cov_trace"])

    def predict_segmentation_sample_variance_sm_cov_bf(self, x_in, num_samples, drop_last_class=False):
        """phiseg_model.py:406-430: determinant of the unbiased sample covariance of the soft-max.  With every class in it that
        matrix is singular (rows sum to one) and the value is rounding noise, in the reference too; drop_last_class=True is the
        reference's commented-out line 419 and gives the meaningful determinant."""
        name = "cov_det_drop_last" if drop_last_class else "cov_det"
        res, _ = self._mc_maps(x_in, num_samples, (name,))
        return self._per_image(res[name])

    def get_crossentropy_error_map(self, s_gt, x_in, num_samples=100):
        """phiseg_model.py:433-446: mean over the samples of eval_xent -> [B, X, Y] (the reference does not squeeze this one)."""
        res, _ = self._mc_maps(x_in, num_samples, ("xent_mean",), s_gt=s_gt)
        return res["xent_mean"]

    def predict_mean_variance_and_error_maps(self, s_gt, x_in, num_samples):
        """phiseg_model.py:449-475 -> (arg-max of the mean soft-max, mean over classes of the per-pixel std, mean eval_xent)."""
        res, am = self._mc_maps(x_in, num_samples, ("std_mean", "xent_mean"), s_gt=s_gt, amax=True)
        return self._per_image(am.astype(np.int64)), self._per_image(res["std_mean"]), self._per_image(res["xent_mean"])

    def _advance_noise(self):
        """Every sampling call must see fresh noise (TF's stateful RNG): bump the Philox step word."""
        store = self.sess._ensure_store()
        store.noise_step += 1
        engine.device_sync()          # torch's stream -> the plans' own HIP streams
