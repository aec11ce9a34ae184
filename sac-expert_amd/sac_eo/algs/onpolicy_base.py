"""OnPolicyLoop -- what the on-policy algorithms share (reference ``sac_eo/algs/base_onpolicy_alg.py``):
the ``_setup`` keys, ``_collect_env_data``, ``_evaluate``, ``_set_rms``, the ``train`` loop and
``_dump_and_save``.  ``MBRLOnPolicyAlg`` (world models, a device ring) and ``MFRLOnPolicyAlg`` (the
true environment only) supply the engine, ``_update_gen`` and ``_dump_stats``.

The loop is a generator (``_train_loop``): an update hands its critic and actor steps out as requests
(``("critic_update", rollout_data_all, B)``, ``("actor_update", rollout_data)``) and takes the update's
log back, so a lock-step driver can answer K learners' requests with one packed call; ``train``
answers them on this learner's own engine (``_answer``).
"""
import contextlib
import time

import numpy as np

from ..common.samplers import trajectory_sampler


class OnPolicyLoop:
    """base_onpolicy_alg.py:17-374 without the update itself."""

    # ------------------------------------------------------------------ setup
    def _setup_base(self, k):
        """base_onpolicy_alg.py:66-109."""
        self.gamma, self.lam = k["gamma"], k["lam"]
        self.env_buffer_size = int(k["env_buffer_size"]) if k.get("env_buffer_size") else None
        self.init_rms_stats = k.get("init_rms_stats")
        self.save_path, self.checkpoint_file = k.get("save_path", "./logs"), k.get("checkpoint_file", "TEMPLOG")
        self.save_freq, self.eval_freq = k.get("save_freq"), k.get("eval_freq")
        self.last_eval = 0
        self.eval_num_traj = k.get("eval_num_traj", 5)
        self.mf_algo_name = k["mf_algo"]
        self.total_timesteps = int(k.get("total_timesteps", 0) or 0)
        self.env_horizon = k["env_horizon"]
        self.env_batch_type = k["env_batch_type"]
        self.env_batch_size_init, self.env_batch_size = k["env_batch_size_init"], k["env_batch_size"]
        self.s_noise_std, self.s_noise_type = float(k.get("s_noise_std") or 0.0), k.get("s_noise_type", "all")
        self.critic_lr = k["critic_lr"]
        self.critic_update_it, self.critic_nminibatch = k["critic_update_it"], k["critic_nminibatch"]
        self.num_mf_updates = k["num_mf_updates"]
        self.alg_seed = k.get("alg_seed")
        self.rng = np.random.default_rng(self.alg_seed)

    @contextlib.contextmanager
    def _host_rng(self):
        np.random.set_state(self.engine.rng_get_state())
        try:
            yield
        finally:
            self.engine.rng_set_state(np.random.get_state())

    def _rms_users(self):
        """Further objects that share the normalizers, after the actor, the critics and the corruptor."""
        return ()

    def _set_rms(self):
        """Shares normalizers with all relevant classes (base :199-204, mbrl :61-65)."""
        self.actor.set_rms(self.normalizer)
        for critic in self.critics:
            critic.set_rms(self.normalizer)
        self.corruptor.set_rms(self.normalizer)
        for user in self._rms_users():
            user.set_rms(self.normalizer)
        self.normalizer.push_to(self.engine)

    # ------------------------------------------------------------------ env data
    def _collect_expert_data(self):
        return None

    def _store_trajectory(self, s, a, r, sp, d):
        """One env trajectory into the algorithm's stores (the host TrajectoryBuffer; a device ring too)."""
        self.env_data.add(s, a, r, sp, d)

    def _collect_env_data(self, num_timesteps, update_normalizers=True):
        """base_onpolicy_alg.py:115-172."""
        t0 = time.time()
        batch_size = self.env_batch_size_init if num_timesteps == 0 else self.env_batch_size
        steps_start, traj_start = self.env_data.steps_total, self.env_data.traj_total
        cur, J_all = 0, []
        while cur < batch_size:
            horizon = int(np.minimum(batch_size - cur, self.env_horizon)) if self.env_batch_type == "steps" \
                else self.env_horizon
            s, a, r, sp, d, J = trajectory_sampler(self.env, self.actor, horizon, eval=True, corruptor=self.corruptor)
            a = self._action_rows(a)
            if update_normalizers:
                self.normalizer.update_rms(s, a, r, sp)
                self.normalizer.push_to(self.engine)
            self._store_trajectory(s, a, r, sp, d)
            if horizon == self.env_horizon:
                J_all.append(J)
            cur = self.env_data.steps_total - steps_start if self.env_batch_type == "steps" \
                else self.env_data.traj_total - traj_start
        steps_new = self.env_data.steps_total - steps_start
        J_ave = float(np.mean(J_all)) if J_all else float("nan")
        self.current_reward = J_ave
        self.logger.log_train({"J_tot": J_ave, "steps": steps_new, "traj": self.env_data.traj_total - traj_start,
                               "time_env_data": time.time() - t0})
        return steps_new

    def _action_rows(self, a):
        """The sampled actions as the stores keep them ([T, A] as sampled)."""
        return a

    def _evaluate(self, num_timesteps):
        """base_onpolicy_alg.py:174-197."""
        t0 = time.time()
        J = [trajectory_sampler(self.env_eval, self.actor, self.env_horizon, eval=True, deterministic=True)[-1]
             for _ in range(self.eval_num_traj)]
        self.logger.log_train({"J_tot_eval": float(np.mean(J)), "steps_eval": num_timesteps - self.last_eval,
                               "time_eval": time.time() - t0})
        self.last_eval = num_timesteps

    # ------------------------------------------------------------------ requests
    def _answer(self, req):
        """One learner's own answer to a request of the loop: the update on its engine."""
        if req[0] == "critic_update":
            return self.critic_update.update(req[1], req[2])
        if req[0] == "actor_update":
            return self.mf_algo.update(req[1])
        raise ValueError(req[0])

    def _drive(self, gen):
        """Runs a generator of the loop to its end, answering every request on this learner."""
        try:
            req = next(gen)
            while True:
                req = gen.send(self._answer(req))
        except StopIteration as stop:
            return stop.value

    # ------------------------------------------------------------------ loop
    def _update_gen(self):
        """The update after an env batch (base :206-208, abstract there), as a generator of requests."""
        raise NotImplementedError

    def train(self, total_timesteps, params):
        """base_onpolicy_alg.py:285-349."""
        return self._drive(self._train_loop(total_timesteps, params))

    def _train_loop(self, total_timesteps, params):
        """base_onpolicy_alg.py:285-349 as a generator (the requests of _update_gen)."""
        self._set_rms()
        self._collect_expert_data()
        pts = lambda freq: np.concatenate((np.arange(0, total_timesteps, freq)[1:], [total_timesteps]))
        checkpoints = np.array([total_timesteps]) if self.save_freq is None else pts(self.save_freq)
        evaluate = self.eval_freq is not None
        eval_points = pts(self.eval_freq) if evaluate else None
        ck = ev = 0
        num_timesteps = 0
        if evaluate:
            self._evaluate(num_timesteps)
        while num_timesteps < total_timesteps:
            num_timesteps += self._collect_env_data(num_timesteps)
            yield from self._update_gen()
            if evaluate and num_timesteps >= eval_points[ev]:
                self._evaluate(num_timesteps)
                ev = min(ev + 1, len(eval_points) - 1)
            if num_timesteps >= checkpoints[ck]:
                self._dump_and_save(params)
                ck = min(ck + 1, len(checkpoints) - 1)
        self._dump_and_save(params)
        return self.checkpoint_name

    def _dump_stats(self):
        """base_onpolicy_alg.py:351-364."""
        return {"actor_weights": self.actor.get_weights(),
                "critic_weights": [c.get_weights() for c in self.critics],
                "rms_stats": self.normalizer.get_rms_stats()}

    def _dump_and_save(self, params):
        self.logger.log_params(params)
        self.logger.log_final(self._dump_stats())
        self.logger.dump_and_save(self.save_path, self.checkpoint_name)
        self.logger.reset()
