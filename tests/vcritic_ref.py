"""The critic side of the on-policy loop restated in NumPy on the oracle's primitives: ``VCritic``
(reference ``sac_eo/critics/critics.py:30-49``), ``gae`` as a plain loop (``buffer_utils.py:11-42``) and
``_update_critics`` / ``_apply_critic_grads`` (``base_onpolicy_alg.py:219-283``: the summed loss, one Keras
Adam over every critic's variables).  Test infrastructure only.

The compute dtype is the state's: fp64 for the parity bars, fp32 for the drift envelope.
"""
import dataclasses
from typing import List

import numpy as np

import sac_oracle as O


@dataclasses.dataclass
class VState:
    critics: List[List[np.ndarray]]      # per critic, Keras get_weights() order
    opt: O.AdamState                     # ONE optimiser over all critics' variables, in critic order

    @property
    def dt(self):
        return self.critics[0][0].dtype.type

    def trainables(self):
        return [w for c in self.critics for w in c]

    def copy(self):
        return self.astype(self.dt)

    def astype(self, dt):
        c = lambda xs: [np.asarray(x, dt).copy() for x in xs]
        return VState([c(w) for w in self.critics], O.AdamState(self.opt.t, c(self.opt.m), c(self.opt.v)))


def init_state(S, hidden, n_critics, seed=1, gain=1.0, bias_scale=0.1, dt=np.float64):
    """n_critics VCritics [S] -> hidden -> 1; weights are f32 values (what the device holds) cast to dt."""
    rng = np.random.RandomState(seed)
    critics = [O.init_mlp(rng, S, 1, hidden, gain, bias_scale) for _ in range(n_critics)]
    st = VState(critics, None)
    st.opt = O.AdamState.zeros_like(st.trainables())
    return st.astype(dt)


def forward(w, acts, nrm, s, dt):
    """VCritic._forward (:30-34): the net on the normalised state -> ([n] outputs, xn, hs)."""
    nrm = nrm.cast(dt)
    xn = O._norm(np.asarray(s, dt), nrm.s_mean, nrm.s_den)
    out, hs = O.mlp_forward(w, xn, list(acts))
    return out[:, 0], xn, hs


def value(w, acts, nrm, s, dt=np.float64):
    """VCritic.value (:36-40): the output times max(ret_rms.std, 1e-8)."""
    return forward(w, acts, nrm, s, dt)[0] * O._F(dt, nrm.ret_den)


def loss_and_grads(w, acts, nrm, s, rtg, dt=np.float64):
    """VCritic.get_loss (:42-49) and its gradient: 0.5 mean((rtg / ret_den - value / ret_den)^2)."""
    F = lambda x: O._F(dt, x)
    v, xn, hs = forward(w, acts, nrm, s, dt)
    rden = F(nrm.ret_den)
    v_norm = (v * rden) / rden
    diff = np.asarray(rtg, dt) / rden - v_norm
    n = diff.shape[0]
    loss = F(0.5) * np.mean(diff * diff)
    dout = (-diff * F(1.0 / n))[:, None]                     # (value * ret_den / ret_den: the identity)
    grads, _ = O.mlp_backward(w, xn, hs, dout, list(acts))
    return loss, grads


def critic_step(st, acts, nrm, s_list, rtg_list, lr, keep=None):
    """One ``_apply_critic_grads`` (:269-283) in place on ``st``: the loss is the sum over the critics
    (critic k on s_list[k], rtg_list[k]), one Adam step over all variables.  Returns the summed loss and
    each critic's."""
    dt = st.dt
    losses, grads = [], []
    total = O._F(dt, 0.0)
    for w, s, rtg in zip(st.critics, s_list, rtg_list):
        l, g = loss_and_grads(w, acts, nrm, s, rtg, dt)
        losses.append(float(l))
        grads += g
        total = total + l
    if keep is not None:
        keep.update(grads=grads)
    O.adam_step(st.trainables(), grads, st.opt, lr, dt)
    return dict(loss=float(total), losses=losses)


def gae_loop(v_s, v_sp, r, d, gamma, lam, f64=False):
    """gae (buffer_utils.py:11-42) on given values of ONE trajectory, as a plain f64 loop:
    -> (adv, rtg, rtg_sp) float32 (f64: before that rounding), and delta (f64)."""
    v_s, v_sp, r = np.asarray(v_s), np.asarray(v_sp), np.asarray(r)
    d = np.asarray(d, np.float64)
    gamma = float(gamma)
    delta = r + gamma * (1 - d) * v_sp - v_s
    rate = gamma * float(lam)
    adv = np.empty(len(delta), np.float64)
    acc = 0.0
    for t in range(len(delta) - 1, -1, -1):
        acc = delta[t] + rate * acc
        adv[t] = acc
    rtg = adv + v_s
    rtg_sp = (rtg - r) / gamma
    if f64:
        return adv, rtg, rtg_sp, delta
    return adv.astype(np.float32), rtg.astype(np.float32), rtg_sp.astype(np.float32), delta


def gae_batch_loop(v_s, v_sp, r, d, traj, gamma, lam, f64=False):
    """gae_batch (:44-83) on given values: the loop restarted wherever the trajectory index changes."""
    traj = np.asarray(traj)
    cuts = list(np.flatnonzero(traj[1:] != traj[:-1]) + 1)
    outs = [[], [], [], []]
    for a, b in zip([0] + cuts, cuts + [len(traj)]):
        for o, x in zip(outs, gae_loop(v_s[a:b], v_sp[a:b], r[a:b], d[a:b], gamma, lam, f64)):
            o.append(x)
    return tuple(np.concatenate(o) for o in outs)


class VCriticUpdateRef:
    """``_update_critics`` (:219-266) over the restatement; the shuffles come from ``rs``."""

    def __init__(self, st, acts, nrm, kw, rs):
        self.st, self.acts, self.nrm, self.kw, self.rs = st, acts, nrm, dict(kw), rs

    def update(self, s_all_list, rtg_all_list, B):
        st, kw = self.st, self.kw
        if len(st.critics) != B:
            s_all_list = [np.concatenate(s_all_list, 0)]
            rtg_all_list = [np.concatenate(rtg_all_list, 0)]
        n_samples = np.min([len(x) for x in rtg_all_list])
        n_batch = int(n_samples / kw["critic_nminibatch"])
        steps = []
        for _ in range(kw["critic_update_it"]):
            idx = np.arange(n_samples)
            self.rs.shuffle(idx)
            sections = np.arange(0, n_samples, n_batch)[1:]
            batches = np.array_split(idx, sections)
            if n_samples % n_batch != 0:
                batches = batches[:-1]
            for b in batches:
                steps.append(critic_step(st, self.acts, self.nrm, [s[b] for s in s_all_list],
                                         [x[b] for x in rtg_all_list], kw["critic_lr"]))
        log = [dict(critic_loss=float(loss_and_grads(w, self.acts, self.nrm, s, x, st.dt)[0]))
               for w, s, x in zip(st.critics, s_all_list, rtg_all_list)]
        return log, steps
