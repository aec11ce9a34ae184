"""The CPU stand-in engine for packed on-policy learners (``EngineConfig(learners=K)``): K independent
stand-in engines (tests/fake_engine_mbrl.py, one state each) behind the packed interface --
``select_seed`` / ``seed_view`` address one learner, ``ppo_steps_packed`` / ``vcritic_steps_packed`` advance
every learner, and the one-learner steps raise on a packed engine as the library's do.

So that two runs' logs differ and the adaptlr rule moves each learner's rate its own way, ``ppo_end``'s ``tv``
and ``vcritic_end``'s losses are read off the learner's own stream position (no arithmetic: tests/
test_gpu_packed_onpolicy.py holds that to the one-learner path).  Every steps call is recorded per learner
(``S["steps_log"]``: kind, index shape, an index checksum, the rate) and per engine (``calls``)."""
import numpy as np

from fake_engine_mbrl import FakeEngineMBRL

ENGINES = []            # every engine built since the last install(), in order


class FakeEnginePacked(FakeEngineMBRL):
    def __init__(self, cfg, *a, **k):
        super().__init__(cfg, *a, **k)
        K = int(getattr(cfg, "learners", 0) or 0)
        if K:
            self.seeds = K
            self._st = [self._new_seed() for _ in range(K)]
        ENGINES.append(self)

    def _new_seed(self):
        st = super()._new_seed()
        st["steps_log"] = []
        return st

    def _word(self):
        """A number in [0, 1) off the learner's stream as it stands (no draw)."""
        state = self.S["rs"].get_state()
        return float(state[1][state[2] % 624] % 1000) / 1000.0

    def _log(self, kind, idx, lr):
        idx = np.asarray(idx)
        self.S["steps_log"].append((kind, idx.shape, int(idx.astype(np.int64).sum()), float(np.float32(lr))))

    # ------------------------------------------------------------------ one learner
    def ppo_steps(self, idx, **kw):
        if self.seeds > 1:
            raise RuntimeError("the engine holds several learners: use ppo_steps_packed")
        super().ppo_steps(idx, **kw)
        self._log("ppo", idx, kw["actor_lr"])

    def vcritic_steps(self, idx, critic_lr, **kw):
        if self.seeds > 1:
            raise RuntimeError("the engine holds several learners: use vcritic_steps_packed")
        super().vcritic_steps(idx, critic_lr, **kw)
        self._log("vc", idx, critic_lr)

    def ppo_end(self, eps):
        out = super().ppo_end(eps)
        out["tv"] = np.float32(0.02 + 0.13 * self._word())       # both sides of the adaptlr thresholds
        return out

    def vcritic_end(self):
        out = super().vcritic_end()
        out["critic_loss"] = [np.float32(0.25 + self._word() + k) for k in range(int(self.cfg.vcritics))]
        return out

    # ------------------------------------------------------------------ every learner
    def ppo_steps_packed(self, idx, *, actor_lr, **kw):
        idx = np.asarray(idx)
        assert idx.ndim == 3 and idx.shape[0] == self.seeds
        self.calls.append(("ppo_steps_packed",) + idx.shape)
        lrs = np.broadcast_to(np.asarray(actor_lr, np.float64), (self.seeds,))
        for k in range(self.seeds):
            self._k = k
            FakeEngineMBRL.ppo_steps(self, idx[k], actor_lr=lrs[k], **kw)
            self._log("ppo", idx[k], lrs[k])

    def vcritic_steps_packed(self, idx, *, critic_lr, **kw):
        idx = np.asarray(idx)
        assert idx.ndim == 3 and idx.shape[0] == self.seeds
        self.calls.append(("vcritic_steps_packed",) + idx.shape)
        lrs = np.broadcast_to(np.asarray(critic_lr, np.float64), (self.seeds,))
        for k in range(self.seeds):
            self._k = k
            FakeEngineMBRL.vcritic_steps(self, idx[k], lrs[k], **kw)
            self._log("vc", idx[k], lrs[k])


def install(monkeypatch):
    """Routes the engine MBRLOnPolicyAlg builds to FakeEnginePacked and forgets the engines built before."""
    import sac_eo.algs.mbrl_onpolicy_alg as m
    del ENGINES[:]
    monkeypatch.setattr(m, "Engine", FakeEnginePacked)
