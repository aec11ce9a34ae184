"""MBRLOnPolicyAlg -- the model-based on-policy loop (reference ``sac_eo/algs/mbrl_onpolicy_alg.py``
over ``sac_eo/algs/base_onpolicy_alg.py``) on ONE device engine.

The engine (``EngineConfig(actor_gaussian="train", world_models=True, vcritics=len(critics))``) carries
the PPO-trained GaussianActor, the VCritics and the world models; the replay ring is the env data.

* ``_collect_env_data`` (``base_onpolicy_alg.py:115-172``): ``trajectory_sampler`` with the corruptor;
  every trajectory updates the normalisers (pushed to the engine), goes into the host
  ``TrajectoryBuffer`` and is appended to the device ring.
* ``_update_models`` (``mbrl_onpolicy_alg.py:176-298``): the reference's holdout split and epoch shuffles
  from the global stream (the draws ``SAC_exp._update_models`` makes: ``base.epoch_minibatches``), the
  steps on the device (``sacx_model_fit``), the holdout early stop, the five per-model losses.
* ``_update_actor_critic`` (``:124-174``): per policy update, one ``Engine.sim_collect`` per pass and
  model (index draw, ring rows, rollout: one device call), ``Engine.gae`` per model, the critic update
  and the PPO update on ``torch.cat`` of the parts.  The rollout rows never leave the device.

Packed runs (``--pack_runs``): ``alg_kwargs['_pack'] = (shared engine or None, learner, K)`` makes the learner
one of K on one ``EngineConfig(learners=K)`` engine (through its ``SeedView``), and ``_train_loop`` -- the loop
as a generator, as ``SACBase._train_loop`` -- hands the critic update and the actor update of
``_update_actor_critic`` to the lock-step driver (``sac_eo.algs.lockstep.run_lockstep_onpolicy``), which
answers a round of K requests with one packed steps call.  ``train`` answers them itself, one learner.

TRPO (``alg_kwargs['mf_algo'] == 'trpo'``) runs when the class is constructed directly: it builds
``sac_eo.algs.model_free.trpo.TRPO`` and an engine with ``trpo=True``, and the loop logs whatever keys
``update`` returns.  ``init_alg`` (the front door of ``python -m sac_eo.train``) still refuses it.
"""
import dataclasses
import time

import numpy as np

from ..common.buffers import TrajectoryBuffer
from ..common.corruptor import TrajectoryCorruptor
from ..common.logger import Logger
from ..common.normalizer import RunningNormalizers
from ..engine import Engine, EngineConfig
from .base import epoch_minibatches
from .onpolicy_base import OnPolicyLoop
from .model_free import PPO, VCriticUpdate
from .model_free.ppo import aggregate_rows

MAX_ROWS = 1 << 24          # the trainable handle's bound on buffer_capacity


class MBRLOnPolicyAlg(OnPolicyLoop):
    """Base class for MBRL algorithms with on-policy updates (``mbrl_onpolicy_alg.py:11-33``)."""

    def __init__(self, idx, env, env_eval, actor, critics, models, alg_kwargs, mf_update_kwargs):
        if getattr(actor, "softmax", False):
            raise ValueError("alg_type mbrl does not run a SoftMaxActor: the world models take continuous actions, and "
                             "the reference defines no encoding of a discrete one")
        self._pack = alg_kwargs.pop("_pack", None)
        self._setup(alg_kwargs)
        self.env, self.env_eval = env, env_eval
        self.actor, self.critics, self.models = actor, list(critics), list(models)
        if getattr(actor, "squash", False):
            raise ValueError("alg_type mbrl trains the plain GaussianActor: --actor_squash is not supported")
        if getattr(actor, "output_norm", False):
            raise ValueError("alg_type mbrl: --actor_output_norm has no backward on the device")
        if not 1 <= len(self.models) <= 8:
            raise ValueError("alg_type mbrl runs 1 to 8 world models on the device")
        self.s_dim = int(np.prod(env.observation_space.shape))
        self.a_dim = int(np.prod(env.action_space.shape))
        self.normalizer = RunningNormalizers(self.s_dim, self.a_dim, self.gamma, self.init_rms_stats)
        self.B = len(self.models)
        self.num_critics = len(self.critics)
        self.sim_batch_size_per_model = int(self.sim_batch_size / self.B)
        self.env_data = TrajectoryBuffer(self.s_dim, self.a_dim, self.gamma, self.lam, self.env_buffer_size)
        self.corruptor = TrajectoryCorruptor(self.s_noise_std, self.s_noise_type)
        mf_update_kwargs = dict(mf_update_kwargs)
        mf_update_kwargs["ent_targ"] = self.a_dim * -1                       # base_onpolicy_alg.py:54
        self.logger = Logger()
        self.checkpoint_name = f"{self.checkpoint_file}_{idx}"
        self.current_reward = 0
        self.engine = self._build_engine(alg_kwargs, mf_update_kwargs)
        if self.mf_algo_name == "trpo":                 # (reached by direct construction only: init_alg refuses it)
            from .model_free.trpo import TRPO
            self.mf_algo = TRPO(self.actor, mf_update_kwargs)
        else:
            self.mf_algo = PPO(self.actor, mf_update_kwargs)
        self.critic_update = VCriticUpdate(self.critics, dict(critic_lr=self.critic_lr,
                                                              critic_update_it=self.critic_update_it,
                                                              critic_nminibatch=self.critic_nminibatch), self.actor)

    # ------------------------------------------------------------------ setup
    def _setup(self, k):
        """base_onpolicy_alg.py:66-109 (OnPolicyLoop._setup_base) and mbrl_onpolicy_alg.py:35-59."""
        self._setup_base(k)
        self.sim_buffer_size = int(k["sim_buffer_size"]) if k.get("sim_buffer_size") else None
        self.sim_horizon, self.sim_batch_type, self.sim_batch_size = k["sim_horizon"], k["sim_batch_type"], k["sim_batch_size"]
        self.model_lr = k["model_lr"]
        self.reset_model_optimizer = k["reset_model_optimizer"]
        self.model_num_epochs, self.model_batch_size = k["model_num_epochs"], k["model_batch_size"]
        self.model_batch_shuffle = k["model_batch_shuffle"]
        self.model_max_updates, self.model_max_grad_norm = k["model_max_updates"], k["model_max_grad_norm"]
        self.model_holdout_ratio = float(k.get("model_holdout_ratio") or 0.0)
        self.model_holdout_epochs = k.get("model_holdout_epochs", 5)

    def _sim_rows(self):
        """Rows one policy update's rollouts hold at most (all models)."""
        per = self.sim_batch_size_per_model * (1 if self.sim_batch_type == "steps" else self.sim_horizon)
        return self.B * max(1, per)

    def _env_rows_bound(self):
        """The most env rows a run can collect (base_onpolicy_alg.py:324-327, :115-151): the last batch starts
        while fewer than total_timesteps rows are held, and a batch adds at most its size in steps -- or, with
        --env_batch_type traj, its size in trajectories of up to env_horizon steps each."""
        per = int(self.env_horizon) if self.env_batch_type != "steps" else 1
        largest = max(int(self.env_batch_size_init), int(self.env_batch_size)) * per
        return max(0, self.total_timesteps - 1) + largest

    def _capacity(self):
        """max(env-buffer bound, per-update sim rows): the ring holds the env data, the PPO / critic tables
        one update's rollout rows.  env_buffer_size=None: the most env rows the run can collect
        (_env_rows_bound), so the ring never drops a row the host buffer keeps.  An env_buffer_size BELOW one
        update's simulated rows is refused rather than given a larger ring: the device draws start states from,
        and fits the models on, every row the ring holds, and a larger ring would hold rows the reference's
        FIFO has dropped."""
        sim = self._sim_rows()
        if self.env_buffer_size:
            if self.env_buffer_size < sim:
                # a larger ring would keep env rows the reference's FIFO has already dropped
                raise NotImplementedError(f"alg_type mbrl: --env_buffer_size {self.env_buffer_size} below the "
                                          f"{sim} simulated rows of a policy update")
            cap = self.env_buffer_size
        else:
            cap = max(sim, self._env_rows_bound())
        if cap > MAX_ROWS:
            raise NotImplementedError(f"alg_type mbrl: {cap} rows exceed the device bound of 2^24")
        return int(cap)

    def _build_engine(self, k, mf):
        a, c0, m0 = self.actor, self.critics[0], self.models[0]
        sim = self._sim_rows()
        trpo = self.mf_algo_name == "trpo"              # no actor minibatches: the critics' alone size the batch
        nmb = int(self.critic_nminibatch) if trpo else min(int(mf["actor_nminibatch"]), int(self.critic_nminibatch))
        batch = max(1, int(sim / max(1, nmb)))
        gm = bool(getattr(m0, "gaussian", False))
        cfg = EngineConfig(
            s_dim=self.s_dim, a_dim=self.a_dim, hidden=tuple(a.layers), activation=a.activation,
            actor_activations=a.activations, critic_hidden=tuple(c0.layers), critic_activations=c0.activations,
            batch=batch, buffer_capacity=self._capacity(), per_state_std=a.per_state_std, actor_gaussian="train",
            actor_std_mult=float(a.std_mult), actor_layer_norm=a.layer_norm, graph_steps=1, stats_capacity=4096,
            vcritics=self.num_critics, world_models=True, trpo=trpo, act_limit=float(np.max(a.act_limit)), gamma=self.gamma,
            model_hidden=tuple(m0.layers), model_activation=m0.activation, model_activations=m0.activations,
            model_batch=int(self.model_batch_size), lr_model=self.model_lr, reward_loss_coef=m0.reward_loss_coef,
            num_models=self.B, model_max_grad_norm=float(self.model_max_grad_norm or 0.0),
            delta_clip_loss=float(m0.delta_clip_loss or 0.0), reward_clip_loss=float(m0.reward_clip_loss or 0.0),
            delta_clip_pred=float(m0.delta_clip_pred or 0.0), gaussian_model=gm,
            scale_model_loss=bool(m0.scale_model_loss) and gm, separate_reward_nn=bool(m0.separate_reward_nn))
        if cfg.separate_reward_nn:
            cfg.reward_hidden = tuple(m0.reward_layers)
            cfg.reward_activations = tuple(m0.reward_activations)
        if self._pack is None:
            eng = Engine(cfg)
        else:                                          # one learner of a packed engine (sac_eo.algs.lockstep)
            shared, learner, n = self._pack
            pcfg = dataclasses.replace(cfg, learners=int(n))
            if shared is None:
                shared = Engine(pcfg)
            elif shared.cfg != pcfg:
                raise ValueError("packed runs need one configuration (shapes and hyper-parameters)")
            eng = shared.seed_view(learner)
        a._bind(eng, "actor")
        for i, c in enumerate(self.critics):
            c._bind(eng, f"v{i}")
        for i, m in enumerate(self.models):
            m._bind(eng, f"m{i}")
        self.normalizer.push_to(eng)
        eng.rng_set_state(np.random.get_state())       # adopt the global stream
        return eng

    def _rms_users(self):
        """The world models share the normalizers too (mbrl :61-65)."""
        return self.models

    # ------------------------------------------------------------------ env data
    def _store_trajectory(self, s, a, r, sp, d):
        """The host TrajectoryBuffer, and the device ring the world models and the rollouts read."""
        self.env_data.add(s, a, r, sp, d)
        self.engine.append(s, a, r, sp, np.asarray(d, np.float32))

    # ------------------------------------------------------------------ update
    def _update(self):
        self._update_models()
        self._update_actor_critic()

    def _update_gen(self):
        self._update_models()
        yield from self._update_actor_critic_gen()

    def _fit(self, batches, rows, base):
        """The device steps of a list of [B, model_batch] index arrays into the training rows."""
        if batches:
            idx = np.stack([b if rows is None else rows[b] for b in batches]) + base
            self.engine.model_fit(idx.astype(np.int32))

    def _update_models(self):
        """mbrl_onpolicy_alg.py:176-298."""
        t0 = time.time()
        s_all, a_all, sp_all, r_all = self.env_data.get_model_info()
        n_all = len(r_all)
        # the host buffer's rows are the ring's, oldest first
        base = int(self.engine.ctl()["cur_size"]) - n_all
        if base != 0:
            raise RuntimeError("the device ring and the host env buffer hold different rows")
        ent_all = np.array([np.mean(m.entropy(s_all, a_all)) for m in self.models])
        holdout = self.model_holdout_ratio > 0.0
        rows, n_train = None, n_all
        ep, num_updates, stop = -1, 0, False
        holdout_best, since_best = np.inf, 0
        pending = []
        hold = None
        with self._host_rng():
            if holdout:
                n_train = int(n_all * (1 - self.model_holdout_ratio))
                idx = np.arange(n_all)
                np.random.shuffle(idx)
                rows, hidx = idx[:n_train], idx[n_train:]
                hold = (s_all[hidx], sp_all[hidx], a_all[hidx], r_all[hidx])
        for ep in range(self.model_num_epochs):
            with self._host_rng():
                parts = epoch_minibatches(n_train, self.B, self.model_batch_size, self.model_batch_shuffle)
            for p in parts:
                pending.append(p)
                num_updates += 1
                if num_updates >= self.model_max_updates:
                    stop = True
                    break
            if holdout or stop:
                self._fit(pending, rows, base)             # one epoch per model_fit call
                pending = []
            if stop:
                break
            if holdout:
                loss = 0.0
                for m in self.models:
                    loss += float(m.get_loss(*hold))
                if loss < holdout_best:
                    holdout_best, since_best = loss, 0
                else:
                    since_best += 1
                if since_best >= self.model_holdout_epochs:
                    break
        self._fit(pending, rows, base)                     # without holdout: one call for all epochs
        if self.reset_model_optimizer:
            self.engine.reset_model_optimizer()
        train = (s_all, sp_all, a_all, r_all) if rows is None else (s_all[rows], sp_all[rows], a_all[rows], r_all[rows])
        logs = []
        for m in self.models:
            loss_train = m.get_loss(*train)
            loss_holdout = m.get_loss(*hold) if holdout else np.inf
            loss_all = m.get_loss(s_all, sp_all, a_all, r_all)
            mse, rl = m.get_losses_eval(s_all, sp_all, a_all, r_all)
            logs.append({"model_loss": np.float32(loss_all), "model_loss_train": np.float32(loss_train),
                         "model_loss_holdout": np.float32(loss_holdout), "model_loss_mse": np.float32(mse),
                         "model_loss_reward": np.float32(rl)})
        self.logger.log_train({"time_model_fit": time.time() - t0, "model_ent": ent_all, "model_loss_epochs": ep + 1})
        self.logger.log_train_ensemble(logs)

    def _collect_sim_data(self, idx):
        """mbrl_onpolicy_alg.py:72-100 for model idx, on the device: -> (s, a, r, sp, d, traj) CUDA rows."""
        m = self.models[idx]
        parts, cur, traj0 = [], 0, 0
        while cur < self.sim_batch_size_per_model:
            remaining = self.sim_batch_size_per_model - cur
            if self.sim_batch_type == "steps":
                num_traj, horizon = int(remaining / self.sim_horizon), self.sim_horizon
                if num_traj == 0:
                    num_traj, horizon = 1, remaining
            else:
                num_traj, horizon = remaining, self.sim_horizon
            out = self.engine.sim_collect(idx, num_traj, horizon, deterministic=False,
                                          delta_clip=m.delta_clip_pred or 0.0, reward_clip=m.reward_clip_pred or 0.0)
            parts.append(out[:5] + (out[5] + traj0,))
            traj0 += num_traj
            cur += num_traj * horizon if self.sim_batch_type == "steps" else num_traj
        rows = tuple(aggregate_rows(x) for x in zip(*parts)) if len(parts) > 1 else parts[0]
        if self.sim_buffer_size and int(rows[2].shape[0]) > self.sim_buffer_size:
            rows = tuple(x[-self.sim_buffer_size:] for x in rows)     # TrajectoryBuffer's FIFO truncation
        return rows

    def _update_actor_critic(self):
        """mbrl_onpolicy_alg.py:124-174."""
        return self._drive(self._update_actor_critic_gen())

    def _update_actor_critic_gen(self):
        """mbrl_onpolicy_alg.py:124-174 as a generator: yields ("critic_update", rollout_data_all, B) and
        ("actor_update", rollout_data_agg) and takes the update's log back; everything else runs here."""
        t_ac = time.time()
        env_states = self.env_data.get_states()
        ent = np.mean(self.actor.entropy(env_states))
        kl_info = self.actor.get_kl_info(env_states)
        for _ in range(self.num_mf_updates):
            t0 = time.time()
            per_model = []
            for idx in range(self.B):
                s, a, r, sp, d, traj = self._collect_sim_data(idx)
                critic = idx if self.num_critics == self.B else 0
                adv, rtg, rtg_sp = self.engine.gae(critic, s, r, sp, d, traj, self.gamma, self.lam)
                per_model.append((s, a, adv, rtg, sp, rtg_sp))
            rollout_data_all = tuple(zip(*per_model))
            rollout_data_agg = tuple(aggregate_rows(x) for x in rollout_data_all)
            steps_update = int(rollout_data_agg[0].shape[0])
            t1 = time.time()
            log_critics = yield ("critic_update", rollout_data_all, self.B)
            t2 = time.time()
            log_actor = yield ("actor_update", rollout_data_agg)
            t3 = time.time()
            self.logger.log_train({"steps_update": steps_update, "time_actor": t3 - t2, "time_critic": t2 - t1,
                                   "time_sim_data": t1 - t0})
            self.logger.log_train(log_actor)
            self.logger.log_train_ensemble(log_critics)
        kl = np.mean(self.actor.kl(env_states, kl_info))
        self.logger.log_train({"ent_agg": np.float32(ent), "kl_agg": np.float32(kl), "alpha_agg": self.mf_algo.alpha,
                               "time_ac_agg": time.time() - t_ac})

    # ------------------------------------------------------------------ log
    def _dump_stats(self):
        """base_onpolicy_alg.py:351-364 + mbrl_onpolicy_alg.py:321-329."""
        return {**super()._dump_stats(),
                "model_weights": [m.get_weights() for m in self.models],
                "reward_weights": [m.get_reward_weights() for m in self.models]}
