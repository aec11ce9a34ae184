"""TRPO actor update (reference ``sac_eo/algs/model_free/trpo.py``) on the device.

``TRPO(actor, update_kwargs)`` takes the reference's ``_setup`` keys (``trpo.py:15-32``: ``adv_center``,
``adv_scale``, ``delta_trpo``, ``cg_it``, ``trust_sub``, ``trust_damp``, ``kl_maxfactor``, ``ent_reg``,
``ent_targ``, ``alpha_lr``) and ``update(rollout_data)`` the reference's 6-tuple ``(s, a, adv, _, _, _)``
as NumPy rows or CUDA tensors.  It returns ``_backtrack``'s seven log values (``ent tv_pre kl_pre tv kl
adj improve``) plus ``alpha``.

The semantics are the ``expert_reg is None`` branch with the one reading that makes the reference run:
``grad_final := neg_pg`` (the reference reads ``grad_final``, ``epsilon``, ``norm_pg`` and ``norm_MSE``,
which exist only with ``expert_reg``; those three keys are not logged).  The surrogate gradient, every
Fisher-vector product, conjugate gradient and the line search run in libsacx (``sacx_trpo_begin /
_step``); TRPO draws nothing from the NumPy stream.  A degenerate solve (``vFv <= 0``, where the
reference carries NaNs into the weights) raises and leaves the weights untouched.

The trainable engine (``EngineConfig(actor_gaussian="train", trpo=True)``) is built on the first
``update`` and the actor bound to it, unless the actor is already bound to one that has the TRPO
segments.  ``update_kwargs['rollout_capacity']`` (rows) and ``update_kwargs['vcritics']`` are the extras
``PPO`` has.  The class is importable by its module path only: ``sac_eo.algs.model_free`` does not
re-export it and ``init_alg`` still refuses ``mf_algo='trpo'`` (two pinned tests hold those doors).
"""
import numpy as np

from ...engine import Engine, EngineConfig
from .ppo import _on_device


class TRPO:
    """Algorithm class for TRPO actor updates (``trpo.py:8-317``)."""

    KEYS = ("ent", "tv_pre", "kl_pre", "tv", "kl", "adj", "improve", "alpha")

    def __init__(self, actor, update_kwargs):
        self.actor = actor
        if getattr(actor, "squash", False):
            raise ValueError("TRPO trains the plain GaussianActor (no --actor_squash)")
        self._setup(update_kwargs)
        self.engine = None

    def _setup(self, kw):
        self.adv_center = bool(kw['adv_center'])
        self.adv_scale = bool(kw['adv_scale'])
        self.delta = float(kw['delta_trpo'])
        self.cg_it = int(kw['cg_it'])
        self.trust_sub = int(kw['trust_sub'])
        self.trust_damp = float(kw['trust_damp'])
        self.kl_maxfactor = float(kw['kl_maxfactor'])
        self.ent_reg = bool(kw['ent_reg'])
        self.ent_targ = kw['ent_targ']
        self.alpha_lr = kw['alpha_lr']
        self._rollout_capacity = kw.get('rollout_capacity')
        self._vcritics = int(kw.get('vcritics') or 0)

    @property
    def alpha(self):
        """The entropy weight (starts at 0, ``trpo.py:29``)."""
        return np.float32(self.engine.ppo_alpha()) if self.engine is not None else np.float32(0.0)

    def _params(self):
        return dict(delta=self.delta, cg_it=self.cg_it, trust_sub=self.trust_sub, trust_damp=self.trust_damp,
                    kl_maxfactor=self.kl_maxfactor, ent_reg=self.ent_reg, ent_targ=float(self.ent_targ),
                    alpha_lr=float(self.alpha_lr), adv_center=self.adv_center, adv_scale=self.adv_scale)

    # ------------------------------------------------------------------ engine
    def _ensure_engine(self, n):
        a = self.actor
        eng = getattr(a, "_engine", None)
        if eng is not None and getattr(eng.cfg, "trainable_gaussian", False):
            if not getattr(eng.cfg, "trpo", False):
                raise RuntimeError("TRPO: the actor is bound to a trainable engine without the TRPO segments "
                                   "(EngineConfig(trpo=True))")
            self.engine = eng
        self._softmax = bool(getattr(a, "softmax", False))     # a SoftMaxActor: one action index per row
        if self.engine is None:
            cfg = EngineConfig(
                s_dim=a.s_dim, a_dim=a.a_dim, hidden=tuple(a.layers), activation=a.activation,
                actor_activations=a.activations, batch=int(min(n, 1024)),
                buffer_capacity=int(max(n, self._rollout_capacity or 0)), per_state_std=a.per_state_std,
                actor_gaussian="train", actor_std_mult=float(a.std_mult), actor_output_norm=a.output_norm,
                actor_layer_norm=a.layer_norm, graph_steps=1, stats_capacity=4096, vcritics=self._vcritics, trpo=True,
                softmax=self._softmax)
            self.engine = Engine(cfg)
            w = a.get_weights()
            a._bind(self.engine, "actor", with_logstd=False)
            a.set_weights(w)
            self.engine.rng_set_state(np.random.get_state())   # the engine's stream follows the global one
        cfg = self.engine.cfg
        if n > cfg.buffer_capacity:
            raise ValueError(f"TRPO: rollout of {n} rows exceeds the engine's bound ({cfg.buffer_capacity}); pass "
                             "update_kwargs['rollout_capacity'] or an actor bound to a larger trainable engine")
        rms = getattr(a, "s_rms", None)
        if rms is not None:                                # BaseActor._transform_state (base_actor.py:35-39)
            S = cfg.s_dim
            f = lambda x: np.broadcast_to(np.asarray(x, np.float32), (S,)).reshape(1, S).copy()
            import torch
            self.engine.v["norm.s_mean"].copy_(torch.as_tensor(f(rms.mean)))
            self.engine.v["norm.s_den"].copy_(torch.as_tensor(f(rms.den())))

    # ------------------------------------------------------------------ update
    def update(self, rollout_data, expert_reg=None):
        """Updates actor (``trpo.py:34-198``)."""
        if expert_reg is not None:
            raise NotImplementedError("TRPO.update: the expert_reg branch (trpo.py:65-167) is not built")
        s_all, a_all, adv_all, _, _, _ = rollout_data
        dev = _on_device(s_all)
        if not dev:
            s_all = np.asarray(s_all, np.float32)
        n = int(s_all.shape[0])
        self._ensure_engine(n)
        eng = self.engine
        par = self._params()
        acols = () if self._softmax else (-1,)            # the action column: [n] indices, or [n, A]
        if dev:
            eng.trpo_begin(s_all.reshape(n, -1), a_all.reshape(n, *acols), adv_all.reshape(n), **par)
        else:
            eng.trpo_begin(s_all.reshape(n, -1), np.asarray(a_all, np.float32).reshape(n, *acols),
                           np.asarray(adv_all, np.float32).reshape(n), **par)
        out = eng.trpo_step(**par)
        return {k: out[k] for k in self.KEYS}
