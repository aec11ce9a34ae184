"""TrajectoryBuffer (reference ``sac_eo/common/buffers.py:5-186``): the host store of on-policy
trajectories.  A NumPy restatement that keeps the reference's behaviour as written -- the FIFO
truncation to ``buffer_size`` rows, the three counters, ``add_batch``'s ``[term_idx]`` indexing
(one row, not a slice), and one ``np.random.randint`` draw per ``batch_size`` call from the
global stream.  ``get_update_info(critic)`` goes through ``gae_batch``: with a critic bound to
a device engine that is one ``Engine.gae`` call."""
import numpy as np

from .buffer_utils import aggregate_data, gae_batch


class TrajectoryBuffer:
    """Class for storing and processing trajectory data."""

    def __init__(self, s_dim, a_dim, gamma, lam, buffer_size=None):
        self.s_dim = s_dim
        self.a_dim = a_dim
        self.gamma = gamma
        self.lam = lam
        self.buffer_size = buffer_size      # max number of steps to store, if not None
        self.reset()

    # the stored arrays, empty: rewards, states and actions are float32, the
    # done flags and the trajectory indices NumPy's default f64, as the reference keeps them
    def _empty(self):
        return dict(s_all=np.empty((0, self.s_dim), np.float32), a_all=np.empty((0, self.a_dim), np.float32),
                    r_all=np.empty((0,), np.float32), sp_all=np.empty((0, self.s_dim), np.float32),
                    d_all=np.empty((0,)), idx_all=np.empty((0,)))

    def reset(self):
        """Empties the store and the three counters (buffers.py:28-39): trajectories and steps ever added,
        steps held now."""
        for name, arr in self._empty().items():
            setattr(self, name, arr)
        self.traj_total = self.steps_total = self.current_size = 0

    _FIELDS = ("s_all", "a_all", "r_all", "sp_all", "d_all", "idx_all")

    def add(self, s_traj, a_traj, r_traj, sp_traj, d_traj):
        """Stores one trajectory (buffers.py:41-71)."""
        idx_traj = np.ones_like(r_traj) * self.traj_total
        for name, new in zip(self._FIELDS, (s_traj, a_traj, r_traj, sp_traj, d_traj, idx_traj)):
            setattr(self, name, aggregate_data((getattr(self, name), new)))

        if self.buffer_size and (len(self.r_all) > self.buffer_size):
            for name in self._FIELDS:
                setattr(self, name, getattr(self, name)[-self.buffer_size:])

        self.current_size = len(self.r_all)
        self.traj_total += 1
        self.steps_total += len(r_traj)

    def add_batch(self, s_batch, a_batch, r_batch, sp_batch, d_batch):
        """Stores a batch of trajectories (buffers.py:73-105)."""
        if len(r_batch.shape) == 1:
            self.add(s_batch, a_batch, r_batch, sp_batch, d_batch)
            return
        for idx in range(len(r_batch)):
            traj = [x[idx] for x in (s_batch, a_batch, r_batch, sp_batch, d_batch)]
            if np.any(traj[4]):
                term_idx = np.argmax(traj[4]) + 1
                traj = [x[term_idx] for x in traj]      # (as written: the row at term_idx)
            self.add(*traj)

    def _draw(self, batch_size):
        return np.random.randint(self.current_size, size=batch_size)

    def get_model_info(self, batch_size=None):
        """States, actions, next states, rewards (buffers.py:107-124)."""
        if batch_size:
            idx = self._draw(batch_size)
            return self.s_all[idx], self.a_all[idx], self.sp_all[idx], self.r_all[idx]
        return self.s_all, self.a_all, self.sp_all, self.r_all

    def get_offmodel_info(self, batch_size=None):
        """States, actions, next states, rewards, done flags (buffers.py:126-144)."""
        if batch_size:
            idx = self._draw(batch_size)
            return self.s_all[idx], self.a_all[idx], self.sp_all[idx], self.r_all[idx], self.d_all[idx]
        return self.s_all, self.a_all, self.sp_all, self.r_all, self.d_all

    def get_states(self, batch_size=None):
        if batch_size:
            return self.s_all[self._draw(batch_size)]
        return self.s_all

    def get_update_info(self, critic, batch_size=None):
        """States, actions, advantages, rewards to go, next states, next-state rewards to go
        (buffers.py:161-186); the GAE of the whole store first, then the draw."""
        adv_batch, rtg_batch, rtg_sp_batch = gae_batch(critic, self.gamma, self.lam, self.s_all, self.r_all,
                                                       self.sp_all, self.d_all, self.idx_all)
        if batch_size:
            idx = self._draw(batch_size)
            return (self.s_all[idx], self.a_all[idx], adv_batch[idx], rtg_batch[idx], self.sp_all[idx],
                    rtg_sp_batch[idx])
        return self.s_all, self.a_all, adv_batch, rtg_batch, self.sp_all, rtg_sp_batch
