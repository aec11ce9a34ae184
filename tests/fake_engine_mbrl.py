"""The CPU stand-in engine (tests/fake_engine.py) for ``alg_type mbrl``: the calls MBRLOnPolicyAlg, PPO and
VCriticUpdate make on a world-models engine.  It consumes the global stream as the device does --
``sim_collect``: randint(rows held, size=n), then per step normal(size=(n, A)) (and normal(size=(n, S)) with
GaussianModels); stochastic actions -- and returns finite stand-in numbers of the right shapes (CPU
tensors, so the host classes take their NumPy path).  It computes no arithmetic (tests/test_gpu_mbrl.py
does, against tests/mbrl_ref.py)."""
import numpy as np
import torch

from fake_engine import FakeEngine


class FakeEngineMBRL(FakeEngine):
    def _new_seed(self):
        st = super()._new_seed()
        S = self.cfg.s_dim
        st["v"].update({"norm.s_mean": torch.zeros(1, S), "norm.s_den": torch.ones(1, S),
                        "norm.ret_den": torch.ones(1, 1), "ppo.alpha": torch.zeros(1, 3)})
        st.update(ppo_n=0, ppo_steps=0, vc_steps=0, mlog={})
        return st

    def set_model_logstd(self, k, l):
        self.S["mlog"][int(k)] = np.asarray(l, np.float32).reshape(1, -1).copy()

    def get_model_logstd(self, k):
        return self.S["mlog"][int(k)].copy()

    # ------------------------------------------------------------------ the actor's distribution calls
    def dist(self, s):
        n, A = np.asarray(s).reshape(-1, self.cfg.s_dim).shape[0], self.cfg.a_dim
        return torch.zeros(n, A), torch.zeros(n, A), torch.full((n,), 1.5)

    def kl(self, s, mean_ref, logstd_ref):
        return torch.full((np.asarray(s).reshape(-1, self.cfg.s_dim).shape[0],), 0.01)

    # ------------------------------------------------------------------ sim data
    def sim_collect(self, model, n_traj, horizon, deterministic=False, delta_clip=0.0, reward_clip=0.0):
        cfg, rs = self.cfg, self.S["rs"]
        n, H, S, A = int(n_traj), int(horizon), cfg.s_dim, cfg.a_dim
        assert self.S["rows"] > 0 and 0 <= int(model) < int(cfg.num_models)
        self.calls.append(("sim_collect", int(model), n, H))
        rs.randint(self.S["rows"], size=n)
        for _ in range(H):
            if not deterministic:
                rs.normal(size=(n, A))
            if cfg.gaussian_model:
                rs.normal(size=(n, S))
        return (torch.zeros(n * H, S), torch.zeros(n * H, A), torch.ones(n * H), torch.zeros(n * H, S),
                torch.zeros(n * H, dtype=torch.bool), torch.arange(n, dtype=torch.int32).repeat_interleave(H))

    def gae(self, critic, s, r, sp, d, traj, gamma, lam):
        n = int(np.shape(r)[0])
        assert 0 <= int(critic) < int(self.cfg.vcritics) and int(np.shape(traj)[0]) == n
        return torch.ones(n), torch.ones(n), torch.ones(n)

    # ------------------------------------------------------------------ the updates
    def ppo_begin(self, s, a, adv):
        self.S["ppo_n"], self.S["ppo_steps"] = int(np.shape(adv)[0]), 0
        assert self.S["ppo_n"] <= int(self.cfg.buffer_capacity)
        return self.S["ppo_n"]

    def ppo_steps(self, idx, **kw):
        idx = np.asarray(idx)
        assert idx.shape[1] <= int(self.cfg.batch) and idx.max() < self.S["ppo_n"]
        self.S["ppo_steps"] += idx.shape[0]

    def ppo_end(self, eps):
        f = np.float32
        return dict(ent=f(1.5), tv=f(0.01), kl=f(0.001), outside_clip=np.float64(0.0), actor_grad_norm_pre=f(1.0),
                    actor_grad_norm=f(0.5), alpha=f(0.0), n_steps=self.S["ppo_steps"])

    def ppo_alpha(self):
        return 0.0

    def vcritic_begin(self, critic, s, rtg):
        assert int(np.shape(rtg)[0]) <= int(self.cfg.buffer_capacity)
        return int(np.shape(rtg)[0])

    def vcritic_steps(self, idx, critic_lr, **kw):
        assert np.asarray(idx).shape[1] <= int(self.cfg.batch)
        self.S["vc_steps"] += np.asarray(idx).shape[0]

    def vcritic_end(self):
        return dict(critic_loss=[np.float32(0.25)] * int(self.cfg.vcritics), n_steps=self.S["vc_steps"])

    def vcritic_value(self, critic, s, value=True):
        return torch.zeros(np.asarray(s).reshape(-1, self.cfg.s_dim).shape[0])

    # ------------------------------------------------------------------ the models
    def model_fit(self, idx, eager=False):
        idx = np.asarray(idx)
        assert idx.ndim == 3 and idx.shape[1:] == (int(self.cfg.num_models), int(self.cfg.model_batch))
        assert idx.min() >= 0 and idx.max() < self.S["rows"]
        self.calls.append(("model_fit", idx.shape[0]))
        super().model_fit(idx, eager)

    def model_loss(self, model, s, sp, a, r, delta_clip_loss=0.0, reward_clip_loss=0.0):
        return 0.5

    def model_losses_eval(self, model, s, sp, a, r):
        return 0.4, 0.1


def install(monkeypatch):
    """Routes the engine MBRLOnPolicyAlg builds to FakeEngineMBRL."""
    import sac_eo.algs.mbrl_onpolicy_alg as m
    monkeypatch.setattr(m, "Engine", FakeEngineMBRL)
