"""PPO actor update (reference ``sac_eo/algs/model_free/ppo.py``) on the device.

``PPO(actor, update_kwargs)`` takes the reference's ``_setup`` keys (``ppo.py:13-39``) and
``update(rollout_data)`` the reference's 6-tuple ``(s, a, adv, _, _, _)``; it returns the
reference's eight log values.  Every minibatch step (gather, forward, the clipped surrogate
with the entropy term, alpha's step, the global-norm clip, Keras Adam) runs in libsacx
(``sacx_ppo_begin / _steps / _end``); the host draws the minibatch shuffles from the global
NumPy stream, which lives on the device between calls, exactly as ``SACBase._host_rng`` does.

The trainable engine (``EngineConfig(actor_gaussian="train")``) is built on the first
``update`` and the actor bound to it, unless the actor is already bound to one.  Its two
bounds are fixed then: the rollout rows (``buffer_capacity``) and the minibatch rows
(``batch``) -- by default the first update's ``n`` and ``int(n / actor_nminibatch)``; a run
whose rollouts grow passes ``update_kwargs['rollout_capacity']`` (rows).

Readable state: ``.alpha`` (a float, the reference's ``self.alpha.numpy()``), ``.actor_lr``
(the CURRENT rate of the actor's Adam; the reference's
``self.actor_optimizer.learning_rate`` is served as ``.actor_optimizer.learning_rate`` with
a ``.numpy()`` too).  ``expert_reg`` (the reference's unreachable regulariser branch) is not built;
``TRPO`` is ``sac_eo.algs.model_free.trpo.TRPO``.
"""
import contextlib

import numpy as np

from ...engine import Engine, EngineConfig


def _on_device(x):
    """Whether x is a CUDA tensor (rows that are on the device already)."""
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def aggregate_rows(parts):
    """aggregate_data (buffer_utils.py) for rows that may live on the device: torch.cat there."""
    parts = list(parts)
    if parts and _on_device(parts[0]):
        import torch
        return torch.cat(parts, 0)
    return np.concatenate(parts, 0)


def minibatches(n_samples, nminibatch, idx):
    """The split of ``ppo.py:48-62``: ``idx`` (a shuffled arange) cut at multiples of
    ``n_batch = int(n / nminibatch)``, the short last part dropped; -> [parts, n_batch]."""
    n_batch = int(n_samples / nminibatch)
    if n_batch < 1:
        raise ValueError(f"PPO: {n_samples} rollout rows give no minibatch with actor_nminibatch = {nminibatch}")
    parts = n_samples // n_batch
    return np.asarray(idx[:parts * n_batch], np.int32).reshape(parts, n_batch)


class _Rate:
    """``actor_optimizer.learning_rate`` of the reference: ``.numpy()`` and ``.assign``."""

    def __init__(self, owner):
        self._o = owner

    def numpy(self):
        return np.float32(self._o.actor_lr)

    def assign(self, v):
        self._o.actor_lr = float(np.float32(v))


class _Opt:
    def __init__(self, owner):
        self.learning_rate = _Rate(owner)


class PPO:
    """Algorithm class for PPO actor updates (``ppo.py:6-147``, ``:225-239``)."""

    def __init__(self, actor, update_kwargs):
        self.actor = actor
        if getattr(actor, "squash", False):
            raise ValueError("PPO trains the plain GaussianActor (no --actor_squash)")
        self._setup(update_kwargs)
        self.engine = None

    def _setup(self, kw):
        self.actor_lr = float(np.float32(kw['actor_lr']))          # tf.keras Adam keeps it in f32
        self.actor_optimizer = _Opt(self)
        self.actor_update_it = int(kw['actor_update_it'])
        self.actor_nminibatch = int(kw['actor_nminibatch'])
        self.adv_center = bool(kw['adv_center'])
        self.adv_scale = bool(kw['adv_scale'])
        self.eps = kw['eps_ppo']
        self.max_grad_norm = kw['max_grad_norm']
        self.adaptlr = kw['adaptlr']
        self.adapt_factor = kw['adapt_factor']
        self.adapt_minthresh = kw['adapt_minthresh']
        self.adapt_maxthresh = kw['adapt_maxthresh']
        self.ent_reg = bool(kw['ent_reg'])
        self.ent_targ = kw['ent_targ']
        self.alpha_lr = kw['alpha_lr']
        self._rollout_capacity = kw.get('rollout_capacity')
        # VCritics (of the actor's layers) on the engine this class builds (0: none, today's engine), so that
        # VCriticUpdate and TrajectoryBuffer.get_update_info run on the actor's engine
        self._vcritics = int(kw.get('vcritics') or 0)

    @property
    def alpha(self):
        """The entropy weight (starts at 0, ``ppo.py:36``)."""
        return np.float32(self.engine.ppo_alpha()) if self.engine is not None else np.float32(0.0)

    # ------------------------------------------------------------------ engine
    def _ensure_engine(self, n, n_batch):
        a = self.actor
        eng = getattr(a, "_engine", None)
        if eng is not None and getattr(eng.cfg, "trainable_gaussian", False):
            self.engine = eng
        self._softmax = bool(getattr(a, "softmax", False))     # a SoftMaxActor: one action index per row
        if self.engine is None:
            cfg = EngineConfig(
                s_dim=a.s_dim, a_dim=a.a_dim, hidden=tuple(a.layers), activation=a.activation,
                actor_activations=a.activations, batch=int(n_batch),
                buffer_capacity=int(max(n, self._rollout_capacity or 0)), per_state_std=a.per_state_std,
                actor_gaussian="train", actor_std_mult=float(a.std_mult), actor_output_norm=a.output_norm,
                actor_layer_norm=a.layer_norm, graph_steps=1, stats_capacity=4096, vcritics=self._vcritics,
                softmax=self._softmax)
            self.engine = Engine(cfg)
            w = a.get_weights()
            a._bind(self.engine, "actor", with_logstd=False)
            a.set_weights(w)                               # (weights and logstd of a formerly bound actor too)
            self.engine.rng_set_state(np.random.get_state())   # adopt the global stream
        cfg = self.engine.cfg
        if n > cfg.buffer_capacity or n_batch > cfg.batch:
            raise ValueError(f"PPO: rollout of {n} rows / minibatches of {n_batch} exceed the engine's bounds "
                             f"({cfg.buffer_capacity} / {cfg.batch}); pass update_kwargs['rollout_capacity'] or an "
                             "actor bound to a larger trainable engine")
        rms = getattr(a, "s_rms", None)
        if rms is not None:                                # BaseActor._transform_state (base_actor.py:35-39)
            S = cfg.s_dim
            f = lambda x: np.broadcast_to(np.asarray(x, np.float32), (S,)).reshape(1, S).copy()
            import torch
            self.engine.v["norm.s_mean"].copy_(torch.as_tensor(f(rms.mean)))
            self.engine.v["norm.s_den"].copy_(torch.as_tensor(f(rms.den())))

    @contextlib.contextmanager
    def _host_rng(self):
        np.random.set_state(self.engine.rng_get_state())
        try:
            yield
        finally:
            self.engine.rng_set_state(np.random.get_state())

    # ------------------------------------------------------------------ update
    def update(self, rollout_data, expert_reg=None):
        """Updates actor (``ppo.py:41-119``): prepare, the minibatch steps, finish."""
        if expert_reg is not None:
            raise NotImplementedError("PPO.update: the expert_reg branch (ppo.py:148-223) is not built")
        ctx = self.update_prepare(rollout_data)
        self.update_steps(ctx)
        return self.update_finish(ctx)

    def step_params(self):
        """The run-time inputs of the minibatch steps that every learner of a packed call shares."""
        return dict(eps_ppo=self.eps, max_grad_norm=self.max_grad_norm, ent_targ=self.ent_targ, ent_reg=self.ent_reg,
                    alpha_lr=self.alpha_lr, adv_center=self.adv_center, adv_scale=self.adv_scale)

    def update_prepare(self, rollout_data):
        """``ppo.py:43-62``: the rollout becomes the table (``ppo_begin``) and the minibatch shuffles are drawn
        from this learner's stream, in the reference's order.  -> the steps' inputs: ``idx[n_steps, mb]``, ``lr``."""
        s_all, a_all, adv_all, _, _, _ = rollout_data
        # CUDA tensors (Engine.sim_collect / Engine.gae rows) go to ppo_begin as they are: no host copy
        dev = _on_device(s_all)
        if not dev:
            s_all = np.asarray(s_all, np.float32)
        n = int(s_all.shape[0])
        n_batch = int(n / self.actor_nminibatch)
        if n_batch < 1:
            raise ValueError(f"PPO: {n} rollout rows give no minibatch with actor_nminibatch = {self.actor_nminibatch}")
        self._ensure_engine(n, n_batch)
        eng = self.engine
        acols = () if self._softmax else (-1,)            # the action column: [n] indices, or [n, A]
        if dev:
            eng.ppo_begin(s_all.reshape(n, -1), a_all.reshape(n, *acols), adv_all.reshape(n))
        else:
            eng.ppo_begin(s_all.reshape(n, -1), np.asarray(a_all, np.float32).reshape(n, *acols),
                          np.asarray(adv_all, np.float32).reshape(n))
        with self._host_rng():                             # one np.random.shuffle per iteration (:55-62)
            parts = []
            for _ in range(self.actor_update_it):
                idx = np.arange(n)
                np.random.shuffle(idx)
                parts.append(minibatches(n, self.actor_nminibatch, idx))
        return dict(idx=np.concatenate(parts, 0), lr=self.actor_lr)

    def update_steps(self, ctx):
        """``ppo.py:63-83``: every minibatch step of the update, on this learner's engine
        (``sac_eo.algs.model_free.packed.update_packed`` runs K learners' steps in one call instead)."""
        self.engine.ppo_steps(ctx["idx"], actor_lr=ctx["lr"], **self.step_params())

    def update_finish(self, ctx):
        """``ppo.py:86-119``: the whole-rollout passes (``ppo_end``), the log, the adaptlr rule."""
        lr = ctx["lr"]
        out = self.engine.ppo_end(self.eps)
        tv = out['tv']
        log_actor = {
            'ent': out['ent'],
            'tv': tv,
            'kl': out['kl'],
            'alpha': out['alpha'],
            'actor_lr': np.float32(lr),
            'outside_clip': np.float64(out['outside_clip']),
            'actor_grad_norm_pre': out['actor_grad_norm_pre'],
            'actor_grad_norm': out['actor_grad_norm'],
        }
        if self.adaptlr:                                   # ppo.py:109-117 (f64 arithmetic, assigned as f32)
            if tv > (self.adapt_maxthresh * 0.5 * self.eps):
                self.actor_optimizer.learning_rate.assign(float(lr) / (1 + self.adapt_factor))
            elif tv < (self.adapt_minthresh * 0.5 * self.eps):
                self.actor_optimizer.learning_rate.assign(float(lr) * (1 + self.adapt_factor))
        return log_actor
