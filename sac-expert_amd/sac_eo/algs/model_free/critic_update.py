"""The critic update of the on-policy loop (reference ``BaseOnPolicyAlg._update_critics`` /
``_apply_critic_grads``, ``base_onpolicy_alg.py:219-283``) on the device.

``VCriticUpdate(critics, update_kwargs, actor=None)`` takes the reference's keys ``critic_lr``,
``critic_update_it``, ``critic_nminibatch``; ``update(rollout_data_all, B)`` takes the reference's
tuple of per-batch lists ``(s_all_list, _, _, rtg_all_list, _, _)`` and the batch count ``B`` of
the loop, and returns ``[{'critic_loss': ...}, ...]``, one dict per critic.  Every minibatch step
(gather, every critic's forward, the summed loss, backward, ONE Keras Adam over all critics'
variables) runs in libsacx (``sacx_vcritic_begin / _steps / _end``); the host draws one
``np.random.shuffle`` per iteration from the global NumPy stream, which lives on the device
between calls, exactly as ``PPO._host_rng`` does.

The engine: the critics' own if they are bound; else the actor's, if it is bound to a trainable
engine with enough critics of the critics' layers and activations; else one is built on the first
``update`` (bounds as ``PPO``'s: ``update_kwargs['rollout_capacity']`` rows, else the first update's).  ``s_rms`` and ``ret_rms`` of
the critics (``set_rms``) are pushed into ``norm.s_*`` / ``norm.ret_den`` at every update."""
import contextlib

import numpy as np

from ...common.buffer_utils import aggregate_data
from ...engine import Engine, EngineConfig
from .ppo import _on_device, aggregate_rows, minibatches


class VCriticUpdate:
    def __init__(self, critics, update_kwargs, actor=None):
        self.critics = list(critics)
        if not self.critics:
            raise ValueError("VCriticUpdate needs at least one critic")
        self.actor = actor
        self.critic_lr = float(np.float32(update_kwargs['critic_lr']))     # tf.keras Adam keeps it in f32
        self.critic_update_it = int(update_kwargs['critic_update_it'])
        self.critic_nminibatch = int(update_kwargs['critic_nminibatch'])
        self._rollout_capacity = update_kwargs.get('rollout_capacity')
        self.engine = None

    # ------------------------------------------------------------------ engine
    def _ensure_engine(self, n_max, n_batch):
        nc = len(self.critics)
        if self.engine is None:
            bound = [getattr(c, "_engine", None) for c in self.critics]
            if all(e is not None for e in bound):
                if any(e is not bound[0] for e in bound) or [c._net for c in self.critics] != [f"v{k}" for k in range(nc)]:
                    raise ValueError("VCriticUpdate: the critics must be bound to one engine as v0 .. v<n-1>")
                self.engine = bound[0]
            else:
                eng = getattr(self.actor, "_engine", None)
                if (eng is not None and getattr(eng.cfg, "trainable_gaussian", False) and int(eng.cfg.vcritics) >= nc
                        and all(self._fits(eng, k, c) for k, c in enumerate(self.critics))):
                    self.engine = eng
                else:
                    c0 = self.critics[0]
                    s_dim = int(np.asarray(c0.get_weights()[0]).shape[0])
                    a_dim = int(getattr(self.actor, "a_dim", 1))
                    self.engine = Engine(EngineConfig(
                        s_dim=s_dim, a_dim=a_dim, hidden=tuple(c0.layers), activation=c0.activation,
                        critic_hidden=tuple(c0.layers), critic_activations=c0.activations, batch=int(n_batch),
                        buffer_capacity=int(max(n_max, self._rollout_capacity or 0)), actor_gaussian="train",
                        graph_steps=1, stats_capacity=4096, vcritics=nc))
                    self.engine.rng_set_state(np.random.get_state())   # adopt the global stream
                for k, c in enumerate(self.critics):
                    w = c.get_weights()
                    c._bind(self.engine, f"v{k}")
                    c.set_weights(w)
        cfg = self.engine.cfg
        if n_max > cfg.buffer_capacity or n_batch > cfg.batch:
            raise ValueError(f"VCriticUpdate: tables of {n_max} rows / minibatches of {n_batch} exceed the engine's bounds "
                             f"({cfg.buffer_capacity} / {cfg.batch}); pass update_kwargs['rollout_capacity'] or critics "
                             "bound to a larger trainable engine")
        c0 = self.critics[0]
        import torch
        if getattr(c0, "s_rms", None) is not None:         # VCritic._forward's s_rms.normalize (critics.py:32)
            S = cfg.s_dim
            f = lambda x: np.broadcast_to(np.asarray(x, np.float32), (S,)).reshape(1, S).copy()
            self.engine.v["norm.s_mean"].copy_(torch.as_tensor(f(c0.s_rms.mean)))
            self.engine.v["norm.s_den"].copy_(torch.as_tensor(f(c0.s_rms.den())))
        if getattr(c0, "ret_rms", None) is not None:       # ret_rms.normalize(., center=False) (:39, :46-47)
            self.engine.v["norm.ret_den"].fill_(float(np.float32(np.asarray(c0.ret_rms.den()).reshape(-1)[0])))

    @staticmethod
    def _fits(eng, k, critic):
        """Whether the engine's net v<k> has the critic's layers and activations (PPO's ``vcritics`` option
        builds critics of the actor's description: critics of another get an engine of their own)."""
        have = [tuple(t.shape) for t in eng._layers(f"v{k}")]
        want = [(np.shape(w)[0] + 1, np.shape(w)[1]) for w in critic.get_weights()[0::2]]
        acts = EngineConfig._acts(critic.activations, critic.activation, len(critic.layers), "critic")
        return have == want and list(eng.cfg.nets()[1][1]) == acts

    @contextlib.contextmanager
    def _host_rng(self):
        np.random.set_state(self.engine.rng_get_state())
        try:
            yield
        finally:
            self.engine.rng_set_state(np.random.get_state())

    # ------------------------------------------------------------------ update
    def update(self, rollout_data_all, B):
        """Updates critics (``base_onpolicy_alg.py:219-266``): prepare, the minibatch steps, finish."""
        ctx = self.update_prepare(rollout_data_all, B)
        self.update_steps(ctx)
        return self.update_finish(ctx)

    def update_prepare(self, rollout_data_all, B):
        """``base_onpolicy_alg.py:219-242``: every critic's table (``vcritic_begin``) and the minibatch shuffles
        drawn from this learner's stream, in the reference's order.  -> the steps' inputs: ``idx[n_steps, mb]``
        (None without steps), ``lr``."""
        s_all_list, _, _, rtg_all_list, _, _ = rollout_data_all
        if len(self.critics) != B:
            s_all_list = [aggregate_rows(s_all_list)]           # (torch.cat for rows on the device)
            rtg_all_list = [aggregate_rows(rtg_all_list)]
        if len(s_all_list) != len(self.critics):
            raise ValueError(f"VCriticUpdate: {len(s_all_list)} tables for {len(self.critics)} critics")
        n_samples = int(np.min([len(rtg_all) for rtg_all in rtg_all_list]))
        n_batch = int(n_samples / self.critic_nminibatch)
        if n_batch < 1:
            raise ValueError(f"VCriticUpdate: {n_samples} rows give no minibatch with critic_nminibatch = "
                             f"{self.critic_nminibatch}")
        self._ensure_engine(int(np.max([len(rtg_all) for rtg_all in rtg_all_list])), n_batch)
        eng = self.engine
        for k, (s_all, rtg_all) in enumerate(zip(s_all_list, rtg_all_list)):
            n = len(rtg_all)
            if _on_device(s_all):                          # CUDA rows: handed over without a host copy
                eng.vcritic_begin(k, s_all.reshape(n, -1), rtg_all.reshape(n))
            else:
                eng.vcritic_begin(k, np.asarray(s_all, np.float32).reshape(n, -1), np.asarray(rtg_all, np.float32).reshape(n))
        with self._host_rng():                             # one np.random.shuffle per iteration (:235-242)
            parts = []
            for _ in range(self.critic_update_it):
                idx = np.arange(n_samples)
                np.random.shuffle(idx)
                parts.append(minibatches(n_samples, self.critic_nminibatch, idx))
        return dict(idx=np.concatenate(parts, 0) if parts else None, lr=self.critic_lr)

    def update_steps(self, ctx):
        """``base_onpolicy_alg.py:244-251``: every minibatch step of the update, on this learner's engine
        (``sac_eo.algs.model_free.packed.update_packed`` runs K learners' steps in one call instead)."""
        if ctx["idx"] is not None:
            self.engine.vcritic_steps(ctx["idx"], critic_lr=ctx["lr"])

    def update_finish(self, ctx):
        """``base_onpolicy_alg.py:253-264``: every critic's loss over its whole table."""
        out = self.engine.vcritic_end()
        return [{'critic_loss': out['critic_loss'][k]} for k in range(len(self.critics))]
