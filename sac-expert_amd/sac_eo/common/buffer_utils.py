"""Helper functions used by buffers (reference ``sac_eo/common/buffer_utils.py``).

``gae`` is the reference's arithmetic in NumPy (f64 wherever the reference is: the done flags and
``gamma`` are f64 there).  ``gae_batch`` with a critic that is bound to a device engine is ONE
``Engine.gae`` call over the whole batch -- both value passes and the segmented f64 scan on the GPU,
restarted at every change of the trajectory index -- instead of the reference's loop over the
trajectories; any other critic object (``.value(s).numpy()``) takes that loop on the host."""
import numpy as np

from .normalizer import discounted_sum     # y_t = x_t + rate * y_{t+1} in f64: lfilter's recurrence (:8-9)


def aggregate_data(data):
    return np.concatenate(data, 0)


def _values(critic, s):
    v = critic.value(s)
    return np.asarray(v.numpy() if hasattr(v, "numpy") else v)


def gae(critic, gamma, lam, s_traj, r_traj, sp_traj, d_traj):
    """Generalized Advantage Estimation over one trajectory (buffer_utils.py:11-42) -> float32 arrays
    (adv, rtg, rtg_sp).  NumPy's promotion makes every intermediate f64: gamma and the done flags are."""
    v_now, v_next = _values(critic, s_traj), _values(critic, sp_traj)
    td_error = r_traj + gamma * (1 - d_traj) * v_next - v_now
    advantage = discounted_sum(td_error, gamma * lam)
    reward_to_go = advantage + v_now
    next_reward_to_go = (reward_to_go - r_traj) / gamma
    return tuple(x.astype(np.float32) for x in (advantage, reward_to_go, next_reward_to_go))


def _bound_engine(critic):
    eng = getattr(critic, "_engine", None)
    return eng if eng is not None and int(getattr(eng.cfg, "vcritics", 0)) > 0 else None


def gae_batch(critic, gamma, lam, s_batch, r_batch, sp_batch, d_batch, idx_batch):
    """Advantage estimates for a batch of trajectories (buffer_utils.py:44-83); ``idx_batch`` holds
    the trajectory index of every row, and a new trajectory starts wherever it changes."""
    eng = _bound_engine(critic)
    if eng is not None and len(idx_batch) > 0:
        adv, rtg, rtg_sp = eng.gae(critic._index, s_batch, r_batch, sp_batch, d_batch, idx_batch, gamma, lam)
        return adv.cpu().numpy(), rtg.cpu().numpy(), rtg_sp.cpu().numpy()

    # the host path: one gae() per trajectory, the float32 pieces joined in order
    starts = np.flatnonzero(idx_batch[1:] - idx_batch[:-1]) + 1
    pieces = [[np.empty((0,), np.float32)] for _ in range(3)]
    for rows in np.array_split(np.arange(len(idx_batch)), starts):
        one = gae(critic, gamma, lam, s_batch[rows], r_batch[rows], sp_batch[rows], d_batch[rows])
        for acc, x in zip(pieces, one):
            acc.append(x)
    return tuple(aggregate_data(acc) for acc in pieces)
