"""Generates tests/golden/mbrl_ref.npz: what the REFERENCE's own ``TrajectoryBuffer.get_states(batch_size)``,
``batch_simtrajectory_sampler``, ``add_batch`` and ``get_update_info`` (``sac_eo/common/buffers.py``,
``samplers.py``, ``buffer_utils.py``; NumPy and scipy only) return along the passes of
``MBRLOnPolicyAlg._collect_sim_data`` (``mbrl_onpolicy_alg.py:76-100``), with a duck Gaussian actor
(``oracle/sac_oracle.py`` forward + the global stream), ``ref_ducks.OracleModelEnv`` and a duck critic,
under a seeded global stream.  A generator only: data out, no reference source text stored; no test runs it.

Run:  python tests/golden/make_mbrl_fixtures.py <path of a checkout of the reference>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import sac_oracle as O                      # noqa: E402
from helpers import nontrivial_normalizers  # noqa: E402
from ref_ducks import OracleModelEnv        # noqa: E402

S, A, GAMMA, LAM = 3, 2, 0.99, 0.95
CAP, APPENDED, PER_MODEL, HORIZON, MODEL, SEED = 40, 50, 23, 5, 1, 4242


class _T(np.ndarray):
    def numpy(self):
        return np.asarray(self)


def case():
    """The seeded state both the generator and tests/test_mbrl_ref.py build."""
    cfg = O.Config(S=S, A=A, hidden=(16, 16), act="tanh", model_hidden=(16, 16), num_models=2, act_limit=1.0)
    st = O.init_state(cfg, seed=7, with_models=True, bias_scale=0.05, actor_gain=0.5, model_gain=0.3).astype(np.float64)
    st.logstd = np.full((1, A), 0.3)
    rs = np.random.RandomState(99)
    nrm = nontrivial_normalizers(rs, S, A)
    rows = (rs.normal(size=(APPENDED, S)) * 1.5).astype(np.float32)
    return cfg, st, nrm, rows


class DuckActor:
    """GaussianActor.sample / clip on oracle weights, the noise from the GLOBAL stream; one state row too."""

    def __init__(self, st, cfg, nrm):
        self.st, self.cfg, self.nrm = st, cfg, nrm

    def sample(self, s, deterministic=False):
        s2 = np.asarray(s, np.float64).reshape(-1, S)
        u = np.zeros((s2.shape[0], A)) if deterministic else O.f32_noise(np.random.normal(size=(s2.shape[0], A)))
        a = O.gaussian_actor_sample(self.st.actor, self.st.logstd, self.cfg, self.nrm, s2, u)
        return (a[0] if np.ndim(s) == 1 else a).view(_T)

    def clip(self, a):
        return np.clip(a, -self.cfg.act_limit, self.cfg.act_limit)


class RowEnv(OracleModelEnv):
    """OracleModelEnv for one state row as well (the short last pass: np.squeeze gives s_init of shape [S])."""

    def reset(self, s_init):
        self.one = np.ndim(s_init) == 1
        super().reset(np.asarray(s_init).reshape(-1, S))
        return self.s[0] if self.one else self.s

    def step(self, a):
        sp, r, d, info = super().step(np.asarray(a).reshape(-1, A))
        return (sp[0], r[0], bool(d[0]), info) if self.one else (sp, r, d, info)


class DuckCritic:
    def value(self, s):
        s = np.asarray(s, np.float64)
        return (2.0 * np.tanh(s @ np.array([0.7, -1.3, 0.4])) + 0.3 * np.sin(3.0 * s[:, 0])).astype(np.float32).view(_T)


def main(ref_root):
    sys.path.insert(0, ref_root)
    from sac_eo.common.buffers import TrajectoryBuffer                  # noqa: E402
    from sac_eo.common.samplers import batch_simtrajectory_sampler      # noqa: E402
    import sac_eo
    assert os.path.abspath(sac_eo.__file__).startswith(os.path.abspath(ref_root)), sac_eo.__file__
    sys.path.pop(0)
    cfg, st, nrm, rows = case()
    env_data = TrajectoryBuffer(S, A, GAMMA, LAM, CAP)
    z = lambda n, *sh: np.zeros((n,) + sh, np.float32)
    for lo, hi in ((0, 30), (30, APPENDED)):                             # the second add truncates to CAP rows
        env_data.add(rows[lo:hi], z(hi - lo, A), z(hi - lo), rows[lo:hi], np.zeros(hi - lo))
    actor, model, critic = DuckActor(st, cfg, nrm), RowEnv(O, st, cfg, nrm, MODEL), DuckCritic()
    buf = TrajectoryBuffer(S, A, GAMMA, LAM, None)
    np.random.seed(SEED)
    out, p, cur = {}, 0, 0
    while cur < PER_MODEL:                                               # mbrl_onpolicy_alg.py:76-100, 'steps'
        remaining = PER_MODEL - cur
        num_traj, horizon = int(remaining / HORIZON), HORIZON
        if num_traj == 0:
            num_traj, horizon = 1, remaining
        s_init = np.squeeze(env_data.get_states(batch_size=num_traj))
        held = env_data.get_states()
        out[f"idx{p}"] = np.array([int(np.flatnonzero((held == row).all(1))[0]) for row in s_init.reshape(-1, S)])
        out[f"shape{p}"] = np.array([num_traj, horizon])
        buf.add_batch(*batch_simtrajectory_sampler(model, actor, horizon, s_init))
        cur = buf.steps_total
        p += 1
    out["passes"] = np.array(p)
    for name in ("s_all", "a_all", "r_all", "sp_all", "d_all", "idx_all"):
        out[name] = np.asarray(getattr(buf, name))
    for name, x in zip(("s", "a", "adv", "rtg", "sp", "rtg_sp"), buf.get_update_info(critic)):
        out["upd_" + name] = np.asarray(x)
    out["next_draws"] = np.random.randint(1 << 30, size=4)               # the global stream afterwards
    out["held"] = env_data.get_states()
    np.savez_compressed(os.path.join(HERE, "mbrl_ref.npz"), **out)
    print({k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
