"""The PPO actor update of a plain GaussianActor (reference ``sac_eo/algs/model_free/ppo.py:41-147``,
``:225-239`` over ``sac_eo/actors/continuous_actors.py:74-192``) restated in NumPy on the oracle's
primitives (MLP forward / backward, layer norm, the normaliser, Keras Adam).  Test infrastructure only.

The compute dtype is the state's (``PPOState.astype``): fp64 for the parity bars, fp32 for the drift
envelope.  TF's gradient rules are written out: ``maximum`` sends the gradient to its first argument on
ties (the surrogate branch for every row inside the clip range; the unfloored logstd at the floor),
``clip_by_value`` passes on the closed interval, ``clip_by_global_norm`` scales by
``clip * min(1 / norm, 1 / clip)`` (``oracle/sac_oracle.py:model_fit_step``).
"""
import dataclasses
from typing import List

import numpy as np

import sac_oracle as O


@dataclasses.dataclass
class PPOState:
    actor: List[np.ndarray]          # Keras get_weights() order (layer norm: gamma, beta behind b0)
    logstd: np.ndarray               # (1, A); a trainable only without per_state_std
    opt_actor: O.AdamState
    alpha: np.ndarray                # 0-d, starts at 0 (ppo.py:36)
    opt_alpha: O.AdamState
    std_mult: float = 1.0

    def trainables(self, cfg):
        return self.actor + ([] if cfg.per_state_std else [self.logstd])

    def copy(self):
        c = lambda xs: [np.array(x) for x in xs]
        return PPOState(c(self.actor), np.array(self.logstd),
                        O.AdamState(self.opt_actor.t, c(self.opt_actor.m), c(self.opt_actor.v)), np.array(self.alpha),
                        O.AdamState(self.opt_alpha.t, c(self.opt_alpha.m), c(self.opt_alpha.v)), self.std_mult)

    def astype(self, dt):
        c = lambda xs: [np.asarray(x, dt).copy() for x in xs]
        return PPOState(c(self.actor), np.asarray(self.logstd, dt).copy(),
                        O.AdamState(self.opt_actor.t, c(self.opt_actor.m), c(self.opt_actor.v)),
                        np.asarray(self.alpha, dt).copy(),
                        O.AdamState(self.opt_alpha.t, c(self.opt_alpha.m), c(self.opt_alpha.v)), self.std_mult)


def init_state(cfg, seed=1, std_mult=1.0, bias_scale=0.1, gain=0.5, logstd=None, dt=np.float64):
    """A GaussianActor: ``cfg`` is the oracle's Config (S, A, hidden, actor_acts, per_state_std,
    layer_norm).  Weights are f32 values (what the device holds) cast to ``dt``."""
    rng = np.random.RandomState(seed)
    out_a = 2 * cfg.A if cfg.per_state_std else cfg.A
    actor = O.init_mlp(rng, cfg.S, out_a, cfg.hidden, gain, bias_scale)
    if cfg.layer_norm:
        H0 = cfg.hidden[0]
        actor = actor[:2] + [(1.0 + 0.1 * rng.normal(size=H0)).astype(np.float32),
                             (0.1 * rng.normal(size=H0)).astype(np.float32)] + actor[2:]
    ls = np.zeros((1, cfg.A), np.float32) if logstd is None else np.asarray(logstd, np.float32).reshape(1, cfg.A)
    alpha = np.zeros((), np.float32)
    st = PPOState(actor, ls, None, alpha, O.AdamState.zeros_like([alpha]), std_mult)
    st.opt_actor = O.AdamState.zeros_like(st.trainables(cfg))
    return st.astype(dt)


def logstd_init(cfg, std_mult):
    """continuous_actors.py:39-44: a float32 array."""
    return np.float32(np.log(std_mult) - (np.log(np.log(2)) if cfg.per_state_std else 0.0))


@dataclasses.dataclass
class Dist:
    mean: np.ndarray
    ls: np.ndarray
    xn: np.ndarray
    hs: list
    raw: np.ndarray        # per_state_std: the net's second half (None otherwise)
    ls_un: np.ndarray      # the unfloored logstd
    floor: float


def forward(st, cfg, nrm, s):
    """GaussianActor._forward (:74-100): (mean, logstd) with what the backward needs."""
    dt = st.alpha.dtype.type
    F = lambda x: O._F(dt, x)
    nrm = nrm.cast(dt)
    xn = O._norm(np.asarray(s, dt), nrm.s_mean, nrm.s_den)
    out, hs = O.actor_forward(st.actor, xn, cfg)
    lsi = F(logstd_init(cfg, st.std_mult))
    raw = None
    if cfg.per_state_std:
        mean, raw = out[:, :cfg.A], out[:, cfg.A:]
        ls_un = np.log(O.softplus(raw)) + lsi
    else:
        mean = out
        ls_un = np.broadcast_to(st.logstd, out.shape) + lsi
    floor = F(np.log(F(1e-3)))
    return Dist(mean, np.maximum(ls_un, floor), xn, hs, raw, ls_un, floor)


def _log2pi(dt):
    return O._F(dt, np.log(O._F(dt, 2 * np.pi)))


def neglogp_of(d, a):
    dt = d.mean.dtype.type
    z = (np.asarray(a, dt) - d.mean) / np.exp(d.ls)
    return O._F(dt, 0.5) * (z * z + O._F(dt, 2) * d.ls + _log2pi(dt)).sum(-1)


def entropy_of(d):
    dt = d.mean.dtype.type
    return O._F(dt, 0.5) * (O._F(dt, 2) * d.ls + _log2pi(dt) + O._F(dt, 1)).sum(-1)


def kl_of(d, mean_ref, ls_ref):
    dt = d.mean.dtype.type
    two = O._F(dt, 2)
    mean_ref, ls_ref = np.asarray(mean_ref, dt), np.asarray(ls_ref, dt)
    num = (d.mean - mean_ref) ** 2 + np.exp(two * ls_ref)
    return O._F(dt, 0.5) * (num / np.exp(two * d.ls) + two * d.ls - two * ls_ref - O._F(dt, 1)).sum(-1)


def neglogp(st, cfg, nrm, s, a):
    return neglogp_of(forward(st, cfg, nrm, s), a)


def entropy(st, cfg, nrm, s):
    return entropy_of(forward(st, cfg, nrm, s))


def kl(st, cfg, nrm, s, mean_ref, ls_ref):
    return kl_of(forward(st, cfg, nrm, s), mean_ref, ls_ref)


DEFAULTS = dict(eps_ppo=0.2, max_grad_norm=None, ent_targ=0.0, ent_reg=False, alpha_lr=0.0, adv_center=True,
                adv_scale=True, actor_lr=3e-4)


def normalise_adv(adv, par, dt):
    """ppo.py:71-77: mean and population std of the uncentred minibatch first."""
    adv = np.asarray(adv, dt)
    m, sd = np.mean(adv), np.std(adv) + O._F(dt, 1e-8)
    if par["adv_center"]:
        adv = adv - m
    if par["adv_scale"]:
        adv = adv / sd
    return adv


def ppo_step(st, cfg, nrm, s, a, adv, nlp_old, par, keep=None):
    """One ``_apply_actor_grad`` (ppo.py:122-147, :225-239, expert_reg None) in place on ``st``; ``adv``
    is the raw minibatch (normalised here).  Returns loss, ent, the two norms, alpha (after its step);
    ``keep`` receives grads (before the clip), clipped, alpha_grad, r, take (the surrogate branch)."""
    par = {**DEFAULTS, **par}
    dt = st.alpha.dtype.type
    F = lambda x: O._F(dt, x)
    adv = normalise_adv(adv, par, dt)
    nlp_old = np.asarray(nlp_old, dt)
    a = np.asarray(a, dt)
    n = a.shape[0]
    d = forward(st, cfg, nrm, s)
    sd = np.exp(d.ls)
    z = (a - d.mean) / sd
    nlp = F(0.5) * (z * z + F(2) * d.ls + _log2pi(dt)).sum(-1)
    ent = entropy_of(d)
    lo, hi = F(np.float32(1.0 - par["eps_ppo"])), F(np.float32(1.0 + par["eps_ppo"]))
    r = np.exp(nlp_old - nlp)
    rc = np.minimum(np.maximum(r, lo), hi)
    surr, clp = -(r * adv), -(rc * adv)
    take = surr >= clp                             # TF maximum: ties to the first argument
    pg = np.mean(np.maximum(surr, clp))
    em = np.mean(ent)
    alpha = st.alpha.copy()
    loss = pg - alpha * (em - F(par["ent_targ"]))
    # backward
    gn = np.where(take, adv * r, F(0)) * F(1.0 / n)            # d loss / d nlp_cur
    dmean = gn[:, None] * (-(z / sd))
    dls = gn[:, None] * (F(1) - z * z) - alpha * F(1.0 / n)
    dls = dls * (d.ls_un >= d.floor)
    if cfg.per_state_std:
        draw = (dls * (F(1) / O.softplus(d.raw))) / (np.exp(-d.raw) + F(1))   # LogGrad, SoftplusGrad
        grads = O.actor_backward(st.actor, d.xn, d.hs, np.concatenate([dmean, draw], 1), cfg)
    else:
        grads = O.actor_backward(st.actor, d.xn, d.hs, dmean, cfg) + [dls.sum(0, keepdims=True)]
    alpha_grad = em - F(par["ent_targ"])           # alpha_grad * -1 (ppo.py:225-227)
    if par["ent_reg"]:
        av = [np.array(st.alpha, dt)]              # (a 0-d array: adam_step updates in place)
        O.adam_step(av, [np.asarray(alpha_grad)], st.opt_alpha, par["alpha_lr"], dt)
        st.alpha = np.array(np.maximum(av[0], F(0)), dt)
    norm = np.sqrt(sum(np.sum(g * g) for g in grads)).astype(dt)
    clipped = grads
    if par["max_grad_norm"]:
        clip = F(par["max_grad_norm"])
        scale = clip * np.minimum(F(1) / norm, F(1) / clip)
        clipped = [g * scale for g in grads]
    post = np.sqrt(sum(np.sum(g * g) for g in clipped)).astype(dt)
    if keep is not None:
        keep.update(grads=grads, clipped=clipped, alpha_grad=alpha_grad, r=r, take=take, ls_un=d.ls_un, adv=adv,
                    floor=d.floor)
    O.adam_step(st.trainables(cfg), clipped, st.opt_actor, par["actor_lr"], dt)
    return dict(loss=float(loss), ent=float(em), grad_norm_pre=float(norm), grad_norm_post=float(post),
                alpha=float(st.alpha), pg_loss=float(pg))


def split_minibatches(n_samples, nminibatch, idx):
    """The arithmetic the device path uses: [parts, n_batch] of a shuffled index."""
    n_batch = int(n_samples / nminibatch)
    if n_batch < 1:
        raise ValueError("no minibatch")
    parts = n_samples // n_batch
    return np.asarray(idx[:parts * n_batch]).reshape(parts, n_batch)


def split_reference(n_samples, nminibatch, idx):
    """A literal transcription of ppo.py:55-62 (np.array_split at multiples of n_batch, the short
    last part dropped)."""
    n_batch = int(n_samples / nminibatch)
    sections = np.arange(0, n_samples, n_batch)[1:]
    batches = np.array_split(idx, sections)
    if (n_samples % n_batch != 0):
        batches = batches[:-1]
    return batches


class PPORef:
    """``PPO`` (ppo.py:6-119) over the restatement: ``update`` draws its shuffles from ``rs`` (the global
    stream) and returns the reference's eight log values."""

    def __init__(self, st, cfg, nrm, kw, rs):
        self.st, self.cfg, self.nrm, self.kw, self.rs = st, cfg, nrm, dict(kw), rs
        self.actor_lr = np.float32(kw["actor_lr"])

    def update(self, s_all, a_all, adv_all, keep=None):
        st, cfg, nrm, kw = self.st, self.cfg, self.nrm, self.kw
        dt = st.alpha.dtype.type
        d0 = forward(st, cfg, nrm, s_all)
        nlp_old = neglogp_of(d0, a_all)
        mean_ref, ls_ref = d0.mean.copy(), d0.ls.copy()
        ent = np.mean(entropy_of(d0))
        n = s_all.shape[0]
        n_batch = int(n / kw["actor_nminibatch"])
        if n_batch < 1:
            raise ValueError("no minibatch")
        pre = post = dt(0)
        steps = 0
        par = dict(eps_ppo=kw["eps_ppo"], max_grad_norm=kw["max_grad_norm"], ent_targ=kw["ent_targ"],
                   ent_reg=kw["ent_reg"], alpha_lr=kw["alpha_lr"], adv_center=kw["adv_center"],
                   adv_scale=kw["adv_scale"], actor_lr=float(self.actor_lr))
        for _ in range(kw["actor_update_it"]):
            idx = np.arange(n)
            self.rs.shuffle(idx)
            for b in split_reference(n, kw["actor_nminibatch"], idx):
                o = ppo_step(st, cfg, nrm, s_all[b], a_all[b], adv_all[b], nlp_old[b], par)
                pre, post = pre + dt(o["grad_norm_pre"]), post + dt(o["grad_norm_post"])
                steps += 1
        d1 = forward(st, cfg, nrm, s_all)
        rdiff = np.abs(np.exp(nlp_old - neglogp_of(d1, a_all)) - dt(1))
        tv = dt(0.5) * np.mean(rdiff)
        log = dict(ent=float(ent), tv=float(tv), kl=float(np.mean(kl_of(d1, mean_ref, ls_ref))), alpha=float(st.alpha),
                   actor_lr=float(self.actor_lr), outside_clip=float(np.mean(rdiff > np.float32(kw["eps_ppo"]))),
                   actor_grad_norm_pre=float(pre / steps), actor_grad_norm=float(post / steps))
        if keep is not None:
            keep.update(rdiff=rdiff, steps=steps)
        if kw["adaptlr"]:
            if tv > (kw["adapt_maxthresh"] * 0.5 * kw["eps_ppo"]):
                self.actor_lr = np.float32(float(self.actor_lr) / (1 + kw["adapt_factor"]))
            elif tv < (kw["adapt_minthresh"] * 0.5 * kw["eps_ppo"]):
                self.actor_lr = np.float32(float(self.actor_lr) * (1 + kw["adapt_factor"]))
        return log
