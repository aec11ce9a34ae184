"""MFRLOnPolicyAlg -- the model-free on-policy loop (reference ``sac_eo/algs/base_onpolicy_alg.py:17-374``
with the ``_update`` it leaves abstract) on ONE device engine:
``EngineConfig(actor_gaussian="train", vcritics=1, trpo=(mf_algo == "trpo"), softmax=<SoftMaxActor>)``.
No world models and no device ring: the env batch lives in the host ``TrajectoryBuffer`` and every update
trains on the batch just collected.

``_update`` (the order of ``mbrl_onpolicy_alg.py:124-174``): ``env_data.get_update_info(critics[0])`` (one
``Engine.gae`` call), the critic update on ``([s], None, None, [rtg], None, None)`` with ``B = 1``, the
actor update (``PPO`` or ``TRPO``) on the same rows, the log, ``env_data.reset()``.

This is how an expert is trained here: a GaussianActor run's log holds ``actor_weights``, ``critic_weights``
and ``rms_stats`` (``base_onpolicy_alg.py:351-364``) and is a valid ``--expert_file`` of ``sac_imit`` / ``bc``.
A Discrete action space gives the SoftMaxActor: the host store keeps the action index as one f32 column,
``PPO`` / ``TRPO`` get ``[n]`` indices, and acting runs on the device (``actor.device_sample``).
"""
import time

import numpy as np

from ..common.buffers import TrajectoryBuffer
from ..common.corruptor import TrajectoryCorruptor
from ..common.logger import Logger
from ..common.normalizer import RunningNormalizers
from ..engine import Engine, EngineConfig
from .model_free import PPO, VCriticUpdate
from .onpolicy_base import OnPolicyLoop

MAX_ROWS = 1 << 24          # the trainable handle's bound on buffer_capacity


class MFRLOnPolicyAlg(OnPolicyLoop):
    """Model-free RL with on-policy updates (``base_onpolicy_alg.py:17-64``)."""

    def __init__(self, idx, env, env_eval, actor, critics, alg_kwargs, mf_update_kwargs):
        self._setup_base(alg_kwargs)
        if self.mf_algo_name not in ("ppo", "trpo"):
            raise ValueError(f"alg_type mfrl: invalid mf_algo {self.mf_algo_name!r} (ppo or trpo)")
        self.env, self.env_eval = env, env_eval
        self.actor, self.critics = actor, list(critics)
        self.discrete = bool(getattr(actor, "softmax", False))
        if getattr(actor, "squash", False):
            raise ValueError("alg_type mfrl trains the plain GaussianActor: --actor_squash is not supported")
        if getattr(actor, "output_norm", False):
            raise ValueError("alg_type mfrl: --actor_output_norm has no backward on the device")
        if len(self.critics) != 1:
            # the reference's _update_critics indexes one table per critic out of a one-table list
            raise ValueError(f"alg_type mfrl trains exactly one VCritic (got {len(self.critics)}): "
                             "--critic_ensemble does not apply")
        self.s_dim = int(np.prod(env.observation_space.shape))
        self.a_dim = int(actor.a_dim) if self.discrete else int(np.prod(env.action_space.shape))   # flatdim
        self.a_cols = 1 if self.discrete else self.a_dim         # a Discrete action: the index, one f32 column
        self.normalizer = RunningNormalizers(self.s_dim, self.a_cols, self.gamma, self.init_rms_stats)
        self.B = 1
        self.num_critics = len(self.critics)
        self.env_data = TrajectoryBuffer(self.s_dim, self.a_cols, self.gamma, self.lam, self.env_buffer_size)
        self.corruptor = TrajectoryCorruptor(self.s_noise_std, self.s_noise_type)
        mf_update_kwargs = dict(mf_update_kwargs)
        mf_update_kwargs["ent_targ"] = self.a_dim * -1                       # base_onpolicy_alg.py:54
        self.logger = Logger()
        self.checkpoint_name = f"{self.checkpoint_file}_{idx}"
        self.current_reward = 0
        self.engine = self._build_engine(mf_update_kwargs)
        if self.mf_algo_name == "trpo":
            from .model_free.trpo import TRPO
            self.mf_algo = TRPO(self.actor, mf_update_kwargs)
        else:
            self.mf_algo = PPO(self.actor, mf_update_kwargs)
        self.critic_update = VCriticUpdate(self.critics, dict(critic_lr=self.critic_lr,
                                                              critic_update_it=self.critic_update_it,
                                                              critic_nminibatch=self.critic_nminibatch), self.actor)
        if self.discrete:
            self.actor.device_sample = True

    # ------------------------------------------------------------------ engine
    def _capacity(self):
        """The most rows one env batch can hold (base_onpolicy_alg.py:115-151): the batch size in steps, or with
        --env_batch_type traj in trajectories of up to env_horizon steps each.  (An env_buffer_size below that
        only makes the host store drop rows: the tables never hold more than the store.)"""
        per = int(self.env_horizon) if self.env_batch_type != "steps" else 1
        cap = max(int(self.env_batch_size_init), int(self.env_batch_size)) * per
        if cap > MAX_ROWS:
            raise NotImplementedError(f"alg_type mfrl: {cap} rows exceed the device bound of 2^24")
        return max(1, int(cap))

    def _batch(self, mf):
        """Rows of the largest minibatch: the critic's split alone under TRPO (no actor minibatches)."""
        trpo = self.mf_algo_name == "trpo"
        nmb = int(self.critic_nminibatch) if trpo else min(int(mf["actor_nminibatch"]), int(self.critic_nminibatch))
        return max(1, self._capacity() // max(1, nmb))

    def _build_engine(self, mf):
        a, c0 = self.actor, self.critics[0]
        cfg = EngineConfig(
            s_dim=self.s_dim, a_dim=self.a_dim, hidden=tuple(a.layers), activation=a.activation,
            actor_activations=a.activations, critic_hidden=tuple(c0.layers), critic_activations=c0.activations,
            batch=self._batch(mf), buffer_capacity=self._capacity(), per_state_std=a.per_state_std,
            actor_gaussian="train", actor_std_mult=float(a.std_mult), actor_layer_norm=a.layer_norm, graph_steps=1,
            stats_capacity=4096, vcritics=1, trpo=self.mf_algo_name == "trpo", softmax=self.discrete,
            act_limit=1.0 if self.discrete else float(np.max(a.act_limit)), gamma=self.gamma)
        eng = Engine(cfg)
        a._bind(eng, "actor")
        c0._bind(eng, "v0")
        self.normalizer.push_to(eng)
        eng.rng_set_state(np.random.get_state())       # adopt the global stream
        return eng

    def _action_rows(self, a):
        return np.asarray(a, np.float32).reshape(-1, self.a_cols)

    # ------------------------------------------------------------------ update
    def _update(self):
        return self._drive(self._update_gen())

    def _update_gen(self):
        """The update base_onpolicy_alg.py:206-208 leaves abstract, on the batch just collected: critic first,
        actor second (mbrl_onpolicy_alg.py:124-174)."""
        s, a, adv, rtg, sp, rtg_sp = self.env_data.get_update_info(self.critics[0])
        if self.discrete:
            a = a.reshape(-1)
        t1 = time.time()
        log_critics = yield ("critic_update", ([s], None, None, [rtg], None, None), 1)
        t2 = time.time()
        log_actor = yield ("actor_update", (s, a, adv, rtg, sp, rtg_sp))
        t3 = time.time()
        self.logger.log_train({"steps_update": int(np.shape(s)[0]), "time_critic": t2 - t1, "time_actor": t3 - t2})
        self.logger.log_train(log_actor)
        self.logger.log_train_ensemble(log_critics)
        self.env_data.reset()
