"""The CPU stand-in engine (tests/fake_engine.py) for ``alg_type bc``: its ``step`` consumes what the
device BC update draws from the global stream -- the expert normals of the one or two sections
(``len(sec0) * A`` then ``len(sec1) * A``; every expert row with one model) and nothing else: no
randint, no target / policy / alpha noise."""
import numpy as np

from fake_engine import FakeEngine


def bc_rows(expert_batch: int, num_models: int) -> int:
    """Expert rows an update uses: all with one model, else the first two array_split sections."""
    if num_models <= 1:
        return int(expert_batch)
    return sum(len(s) for s in np.array_split(np.arange(expert_batch), num_models)[:2])


class FakeEngineBC(FakeEngine):
    def step(self, n=1, num_timesteps=0, ts_increment=1, **k):
        cfg = self.cfg
        if not getattr(cfg, "bc", False):
            return super().step(n, num_timesteps, ts_increment, **k)
        self.calls.append(("step", n, num_timesteps, ts_increment))
        nm = int(cfg.num_models or 2)
        for st in self._st:
            for _ in range(n):
                if nm <= 1:
                    st["rs"].normal(size=(cfg.expert_batch, cfg.a_dim))
                else:
                    for sec in np.array_split(np.arange(cfg.expert_batch), nm)[:2]:
                        st["rs"].normal(size=(len(sec), cfg.a_dim))
                st["seq"] += 1
            st["nts"] = num_timesteps + n * ts_increment

    def stats(self, n):
        if not getattr(self.cfg, "bc", False):
            return super().stats(n)
        s = self.S["seq"]
        return np.array([[0.0, 0.0, 2.0, 0.0, 0.1, 2.0, 0.0, float(i)] for i in range(s - n, s)], np.float32)


def install(monkeypatch):
    """Routes every Engine the algorithms build (sac_eo.algs.*, BC's included, and the expert engine)
    to FakeEngineBC."""
    import sac_eo.algs.base as base
    import sac_eo.algs.SAC_expert as sx
    import sac_eo.algs.BC as bc
    monkeypatch.setattr(base, "Engine", FakeEngineBC)
    monkeypatch.setattr(sx, "Engine", FakeEngineBC)
    monkeypatch.setattr(bc, "Engine", FakeEngineBC, raising=False)
