"""The BC update (reference ``sac_eo/algs/BC.py:309-363``) composed from the oracle's primitives,
and the BC training loop on top of the loop oracle.  Test infrastructure only.

``bc_update`` restates ``BC._update_actor``: ``actor.sample(s_e)`` per section, the section's world
model (``MSEModel.sample(deterministic=True)``: the model's own normaliser, ``--delta_clip_pred``),
``MSE_loss = mean(0.5 sum (sp_e - sp_pred)^2)`` (two sections: their squared errors added row by row
before the 0.5 and the mean, :350-355), its gradient to the actor and one Keras Adam step on the actor
variables (Dense layers, layer-norm gamma / beta, logstd).  Nothing else of the state moves.
``oracle/sac_oracle.py::sac_update`` with ``Expert.epsilon = 1.0`` computes the same actor step (its
policy rows carry weight ``1 - epsilon = 0``); tests/test_bc_oracle.py pins the two against each other
and ``bc_update`` against torch autograd.
"""
import numpy as np

import sac_oracle as O
from sac_loop import LoopOracle


def bc_sections(perm, num_models):
    """The expert rows of the update: every row in order with one model (BC.py:318-327), else the first
    two sections of ``np.array_split(perm, num_models)`` (:331-339)."""
    if num_models == 1:
        return [np.asarray(perm)]
    return [np.asarray(s) for s in np.array_split(perm, num_models)[:2]]


def bc_update(st, cfg, nrm, halves, mnrm=None, keep=None):
    """One ``BC._update_actor`` in place on ``st``.  ``halves``: [(s_e, sp_e, noise)] of the one or two
    sections (model k takes halves[k]); ``mnrm``: the world models' normaliser (None: ``nrm``).
    Returns {"mse_loss"}; ``keep`` receives actor_grads / g_logstd / heads (the sections' head caches)."""
    dt = st.alpha.dtype.type
    F = lambda x: O._F(dt, x)
    nrm = nrm.cast(dt)
    mnrm = nrm if mnrm is None else mnrm.cast(dt)
    S, lim = cfg.S, cfg.act_limit
    caches, diffs = [], []
    for k, (se, spe, u) in enumerate(halves):
        se, spe, u = np.asarray(se, dt), np.asarray(spe, dt), np.asarray(u, dt)
        se_n = O._norm(se, nrm.s_mean, nrm.s_den)
        out, hs = O.actor_forward(st.actor, se_n, cfg)
        mu, ls = O.split_head(out, st.logstd, cfg)
        ca, cache = O.head_sample(mu, ls, u, lim, dt)
        xm = np.concatenate([O._norm(se, mnrm.s_mean, mnrm.s_den), O._norm(ca, mnrm.a_mean, mnrm.a_den)], axis=1)
        om, hsm = O.mlp_forward(st.models[k], xm, cfg.model_act)
        dn = om[:, :S]
        dpass = np.ones_like(dn)
        if cfg.delta_clip_pred:            # tf.clip_by_value: zero gradient outside, passes at the bounds
            c = F(cfg.delta_clip_pred)
            dpass = ((dn >= -c) & (dn <= c)).astype(dt)
            dn = np.minimum(np.maximum(dn, -c), c)
        sp_hat = se + (dn * mnrm.d_den + mnrm.d_mean)
        diffs.append(spe - sp_hat)
        caches.append((se_n, hs, cache, xm, hsm, om.shape[1], dpass))
    sq = (diffs[0] ** 2).sum(-1)
    if len(diffs) == 2:
        sq = sq + (diffs[1] ** 2).sum(-1)
    mse = np.mean(F(0.5) * sq)
    n = diffs[0].shape[0]
    X, H, DMU, DL = [], [], [], []
    for k, (se_n, hs, cache, xm, hsm, width, dpass) in enumerate(caches):
        dout = np.zeros((n, width), dt)
        dout[:, :S] = -F(1.0 / n) * diffs[k] * mnrm.d_den * dpass
        _, dxm = O.mlp_backward(st.models[k], xm, hsm, dout, cfg.model_act, need_dx=True, need_dw=False)
        dmu, dl = O.head_backward(dxm[:, S:] / mnrm.a_den, None, cache, lim, dt)
        X.append(se_n); H.append(hs); DMU.append(dmu); DL.append(dl)
    X = np.concatenate(X, 0)
    Hs = [np.concatenate([h[l] for h in H], 0) for l in range(len(H[0]))]
    DMU, DL = np.concatenate(DMU, 0), np.concatenate(DL, 0)
    if cfg.per_state_std:
        dout_a, g_logstd = np.concatenate([DMU, DL], axis=1), np.zeros_like(st.logstd)
    else:
        dout_a, g_logstd = DMU, DL.sum(axis=0, keepdims=True)
    grads = O.actor_backward(st.actor, X, Hs, dout_a, cfg)
    if keep is not None:
        keep.update(actor_grads=grads, g_logstd=g_logstd, heads=[c[2] for c in caches])
    O.adam_step(st.actor + [st.logstd], grads + [g_logstd], st.opt_actor, cfg.lr_pi, dt)
    return {"mse_loss": float(mse)}


class BCLoopOracle(LoopOracle):
    """``BC.train``: SAC_exp's loop with ``BC._update`` (BC.py:303-363) -- the permutation from the
    algorithm's Generator, the one or two noise draws from the global stream, nothing else."""

    def __init__(self, cfg, st, env, env_expert, expert, k, rs_state, alg_seed, **kw):
        super().__init__("sac_imit", cfg, st, env, env_expert, expert, k, rs_state, alg_seed, **kw)

    def _update(self, num_timesteps):
        A, rs = self.cfg.A, self.rs
        s_e, sp_e = self.s_e_cur, self.sp_e_cur
        nm = int(self.k.get("num_models", 2))
        perm = np.arange(len(s_e))
        if nm > 1:
            self.gen.shuffle(perm)                                           # BC.py:331-333
        halves = []
        for sec in bc_sections(perm, nm):
            halves.append((s_e[sec], sp_e[sec], O.f32_noise(rs.normal(size=(len(sec), A)))))
        self.update_stats.append(bc_update(self.st, self.cfg, self._nrm(), halves, self._mnrm()))
