"""Generates tests/golden/gae_ref.npz: what the REFERENCE's own ``TrajectoryBuffer`` and ``gae_batch``
(``sac_eo/common/buffers.py:5-186``, ``buffer_utils.py:8-83``; NumPy and scipy only) return on seeded
inputs, with a duck critic whose values are recorded arrays.  A generator only: data out, no reference
source text stored; no test runs it.

Run:  python tests/golden/make_gae_fixtures.py <path of a checkout of the reference>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
S, A, GAMMA, LAM = 3, 2, 0.99, 0.95


class DuckCritic:
    """value(s).numpy() of a fixed smooth function of the state rows (float32, as a TF critic returns)."""

    class _Out(np.ndarray):
        def numpy(self):
            return np.asarray(self)

    def value(self, s):
        s = np.asarray(s, np.float64)
        w = np.array([0.7, -1.3, 0.4])
        return (2.0 * np.tanh(s @ w) + 0.3 * np.sin(3.0 * s[:, 0])).astype(np.float32).view(self._Out)


def trajectory(rng, n, done_last):
    s = rng.normal(size=(n, S)).astype(np.float32)
    sp = np.concatenate([s[1:], rng.normal(size=(1, S)).astype(np.float32)], 0)
    a = rng.normal(size=(n, A)).astype(np.float32)
    r = (rng.normal(size=n) + 0.5).astype(np.float32)
    d = np.zeros(n)
    d[-1] = float(done_last)
    return s, a, r, sp, d


def main(ref_root):
    sys.path.insert(0, ref_root)
    from sac_eo.common.buffers import TrajectoryBuffer          # noqa: E402
    from sac_eo.common.buffer_utils import gae_batch            # noqa: E402
    import sac_eo
    assert os.path.abspath(sac_eo.__file__).startswith(os.path.abspath(ref_root)), sac_eo.__file__
    sys.path.pop(0)

    rng = np.random.RandomState(20260)
    critic = DuckCritic()
    out = {}
    # gae_batch on one batch of trajectories (lengths 1 .. 70, dones at some ends)
    lens = [1, 1, 5, 63, 64, 65, 2, 70, 1]
    trajs = [trajectory(rng, n, i % 2 == 0) for i, n in enumerate(lens)]
    s, a, r, sp, d = [np.concatenate([t[k] for t in trajs], 0) for k in range(5)]
    idx_all = np.concatenate([np.full(n, i, np.float64) for i, n in enumerate(lens)])
    adv, rtg, rtg_sp = gae_batch(critic, GAMMA, LAM, s, r, sp, d, idx_all)
    out.update(s=s, r=r, sp=sp, d=d, idx_all=idx_all, v_s=critic.value(s).numpy(), v_sp=critic.value(sp).numpy(),
               adv=adv, rtg=rtg, rtg_sp=rtg_sp, gamma=GAMMA, lam=LAM)
    # a TrajectoryBuffer trace: add x 4 into a buffer of 100 rows (the third add truncates), the counters
    # after every add, get_update_info whole and with a batch_size draw from a seeded global stream
    buf = TrajectoryBuffer(S, A, GAMMA, LAM, buffer_size=100)
    tlens = [40, 37, 45, 9]
    ttraj = [trajectory(rng, n, i == 1) for i, n in enumerate(tlens)]
    counters = []
    for i, t in enumerate(ttraj):
        buf.add(*t)
        counters.append([buf.traj_total, buf.steps_total, buf.current_size])
        for k, name in enumerate(("s", "a", "r", "sp", "d")):
            out[f"t_in{i}_{name}"] = t[k]
    out["t_counters"] = np.asarray(counters, np.int64)
    for name in ("s_all", "a_all", "r_all", "sp_all", "d_all", "idx_all"):
        out["t_" + name] = getattr(buf, name)
    whole = buf.get_update_info(critic)
    for name, x in zip(("s", "a", "adv", "rtg", "sp", "rtg_sp"), whole):
        out["t_whole_" + name] = x
    np.random.seed(77)
    sub = buf.get_update_info(critic, batch_size=16)
    for name, x in zip(("s", "a", "adv", "rtg", "sp", "rtg_sp"), sub):
        out["t_sub_" + name] = x
    out["t_sub_next_draw"] = np.random.randint(1 << 30, size=2)     # the global stream after the draw
    out["t_v_s"] = critic.value(buf.s_all).numpy()
    out["t_v_sp"] = critic.value(buf.sp_all).numpy()
    path = os.path.join(HERE, "gae_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
