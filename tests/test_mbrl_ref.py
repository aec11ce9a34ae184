"""tests/mbrl_ref.py against tests/golden/mbrl_ref.npz: what the reference's own TrajectoryBuffer.get_states,
batch_simtrajectory_sampler, add_batch and get_update_info produced along the passes of
_collect_sim_data (tests/golden/make_mbrl_fixtures.py).  Indices and the stream afterwards are exact;
rows match to f32 rounding."""
import os
import sys

import numpy as np

import mbrl_ref as M
import vcritic_ref as V

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_mbrl_fixtures as G      # noqa: E402  (the seeded case and the duck critic; its main() is not run)

FIX = np.load(os.path.join(HERE, "golden", "mbrl_ref.npz"))


def _close(a, b, tol=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b)))


def test_ring_rows_and_pass_arithmetic():
    cfg, st, nrm, rows = G.case()
    assert np.array_equal(M.ring_rows(rows, G.CAP), FIX["held"]) and FIX["held"].shape[0] == G.CAP
    passes = M.sim_passes(G.PER_MODEL, G.HORIZON)
    assert len(passes) == int(FIX["passes"]) == 2
    assert [tuple(FIX[f"shape{p}"]) for p in range(len(passes))] == passes == [(4, 5), (1, 3)]


def test_sim_collect_reproduces_the_reference_rows():
    cfg, st, nrm, rows = G.case()
    held = M.ring_rows(rows, G.CAP)
    rs = np.random.RandomState(G.SEED)
    parts, t0 = [], 0
    for p, (n, h) in enumerate(M.sim_passes(G.PER_MODEL, G.HORIZON)):
        idx, out = M.sim_collect(st, cfg, nrm, held, n, h, G.MODEL, rs)
        assert np.array_equal(idx, FIX[f"idx{p}"]), p                   # the index draw, exactly
        parts.append(out[:5] + (out[5] + t0,))
        t0 += n
    s, a, r, sp, d, traj = [np.concatenate(x, 0) for x in zip(*parts)]
    for name, got in (("s_all", s), ("a_all", a), ("r_all", r), ("sp_all", sp)):
        assert _close(got, FIX[name]), name
    assert not FIX["d_all"].any() and not d.any()
    assert np.array_equal(traj, FIX["idx_all"].astype(np.int32))        # add_batch's running trajectory index
    assert np.array_equal(rs.randint(1 << 30, size=4), FIX["next_draws"])   # the stream afterwards, exactly
    # the raw action is stored: some exceed act_limit, which the model never saw
    assert np.any(np.abs(FIX["a_all"]) > cfg.act_limit)
    # get_update_info (gae_batch per trajectory) on those rows
    c = G.DuckCritic()
    adv, rtg, rtg_sp, _ = V.gae_batch_loop(c.value(FIX["s_all"]).numpy(), c.value(FIX["sp_all"]).numpy(),
                                           FIX["r_all"], FIX["d_all"], FIX["idx_all"], G.GAMMA, G.LAM)
    assert _close(adv, FIX["upd_adv"]) and _close(rtg, FIX["upd_rtg"]) and _close(rtg_sp, FIX["upd_rtg_sp"])
    assert np.array_equal(FIX["upd_s"], FIX["s_all"]) and np.array_equal(FIX["upd_a"], FIX["a_all"])
