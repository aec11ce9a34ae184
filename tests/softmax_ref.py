"""SoftMaxActor (reference ``sac_eo/actors/discrete_actors.py:8-117``, read as
``_nn = create_nn(s_dim, a_dim, ...)`` with the net's variables the only trainables) under the PPO and
TRPO actor updates (``ppo.py:41-147``, ``:225-239``; ``trpo.py:34-317`` with ``grad_final := neg_pg``),
restated in NumPy on the primitives of ``ppo_ref`` / ``trpo_ref`` / ``sac_oracle``.  Test infrastructure
only.

The compute dtype is the state's (fp64 for the parity bars, fp32 for the drift envelope).  Every row
function works on the max-shifted logits, as the reference does.  The gradients are written out:
``d neglogp / d l_j = p_j - onehot_j`` on a labelled row and 0 on a row whose index is outside ``[0, A)``
(``tf.one_hot``'s all-zero row: neglogp is the constant 0 there), ``d ent / d l_j = -p_j (log p_j + ent)``.
The Fisher product is the Gauss-Newton form with ``M_i = diag(p_i) - p_i p_i^T``, which is the Hessian of
the mean kl at cur = ref (``test_softmax_ref.py`` pins it to torch's double backward).
"""
import dataclasses
import types
from typing import List

import numpy as np

import ppo_ref as R
import sac_oracle as O
import trpo_ref as T


@dataclasses.dataclass
class SMState:
    actor: List[np.ndarray]          # Keras get_weights() order (layer norm: gamma, beta behind b0)
    opt_actor: O.AdamState
    alpha: np.ndarray                # 0-d, starts at 0
    opt_alpha: O.AdamState

    def trainables(self, cfg=None):
        return self.actor

    def astype(self, dt):
        c = lambda xs: [np.asarray(x, dt).copy() for x in xs]
        return SMState(c(self.actor), O.AdamState(self.opt_actor.t, c(self.opt_actor.m), c(self.opt_actor.v)),
                       np.asarray(self.alpha, dt).copy(),
                       O.AdamState(self.opt_alpha.t, c(self.opt_alpha.m), c(self.opt_alpha.v)))

    def copy(self):
        return self.astype(self.alpha.dtype.type)


def state_of(actor_weights, dt=np.float64):
    alpha = np.zeros((), np.float32)
    w = [np.asarray(x, np.float32) for x in actor_weights]
    return SMState(w, O.AdamState.zeros_like(w), alpha, O.AdamState.zeros_like([alpha])).astype(dt)


def init_state(cfg, seed=1, bias_scale=0.1, gain=0.5, dt=np.float64):
    """A SoftMaxActor of ``cfg`` (the oracle's Config: S, A = the action count, hidden, actor_acts,
    layer_norm): f32 values cast to ``dt``."""
    rng = np.random.RandomState(seed)
    actor = O.init_mlp(rng, cfg.S, cfg.A, cfg.hidden, gain, bias_scale)
    if cfg.layer_norm:
        H0 = cfg.hidden[0]
        actor = actor[:2] + [(1.0 + 0.1 * rng.normal(size=H0)).astype(np.float32),
                             (0.1 * rng.normal(size=H0)).astype(np.float32)] + actor[2:]
    return state_of(actor, dt)


def forward(st, cfg, nrm, s):
    """The raw logits [n, A] with what the backward needs (xn, hs)."""
    dt = st.alpha.dtype.type
    nrm = nrm.cast(dt)
    xn = O._norm(np.asarray(s, dt), nrm.s_mean, nrm.s_den)
    out, hs = O.actor_forward(st.actor, xn, cfg)
    return out, xn, hs


# ------------------------------------------------------------------ the class's row functions on logits
def logp_of(logits):
    """(log p, p) on the max-shifted logits (:33, :49, :58-64)."""
    x = logits - logits.max(-1, keepdims=True)
    e = np.exp(x)
    z = e.sum(-1, keepdims=True)
    return x - np.log(z), e / z


def onehot(a, A, dt):
    """tf.one_hot: an index outside [0, A) is an all-zero row."""
    a = np.asarray(a).reshape(-1)
    ai = a.astype(np.int64)
    ok = (a >= 0) & (a < A)
    out = np.zeros((a.shape[0], A), dt)
    out[np.nonzero(ok)[0], ai[ok]] = 1
    return out


def neglogp_of(logits, a):
    """softmax_cross_entropy_with_logits(one_hot(a), logits) (:47-54)."""
    lp, _ = logp_of(logits)
    return -(onehot(a, logits.shape[-1], logits.dtype.type) * lp).sum(-1)


def entropy_of(logits):
    lp, p = logp_of(logits)
    return -(p * lp).sum(-1)


def kl_of(logits, logits_ref):
    """sum_j p_cur ((l_cur - lse_cur) - (l_ref - lse_ref)) (:68-96)."""
    lp, p = logp_of(logits)
    lpr, _ = logp_of(np.asarray(logits_ref, logits.dtype))
    return (p * (lp - lpr)).sum(-1)


def gumbel_argmax(logits32, u):
    """sample (:22-42) as the host class computes it: the Gumbel noise g = float32(-log(-log u)) formed in
    f64, the first-index argmax of the f32 (logits - max) + g, which is the reference's
    argmax(a_logits - np.log(-np.log(u))); u None: the deterministic form."""
    x = np.asarray(logits32, np.float32)
    x = x - x.max(-1, keepdims=True)
    if u is not None:
        x = x + (-np.log(-np.log(np.asarray(u, np.float64)))).astype(np.float32)
    return np.argmax(x, -1)


def neglogp(st, cfg, nrm, s, a):
    return neglogp_of(forward(st, cfg, nrm, s)[0], a)


def entropy(st, cfg, nrm, s):
    return entropy_of(forward(st, cfg, nrm, s)[0])


def kl(st, cfg, nrm, s, logits_ref):
    return kl_of(forward(st, cfg, nrm, s)[0], logits_ref)


# ------------------------------------------------------------------ gradients at the logits
def dnlp_dlogits(logits, a):
    lp, p = logp_of(logits)
    oh = onehot(a, logits.shape[-1], logits.dtype.type)
    return (p - oh) * oh.sum(-1, keepdims=True)            # an unlabelled row: neglogp is the constant 0


def dent_dlogits(logits):
    lp, p = logp_of(logits)
    ent = -(p * lp).sum(-1, keepdims=True)
    return -(p * (lp + ent))


def dkl_dlogits(logits, logits_ref):
    """d kl / d l_j = p_j ((log p_j - log p_ref_j) - kl)."""
    lp, p = logp_of(logits)
    lpr, _ = logp_of(np.asarray(logits_ref, logits.dtype))
    k = (p * (lp - lpr)).sum(-1, keepdims=True)
    return p * ((lp - lpr) - k)


# ------------------------------------------------------------------ PPO
def ppo_step(st, cfg, nrm, s, a, adv, nlp_old, par, keep=None):
    """One ``_apply_actor_grad`` (ppo.py:122-147, :225-239) with the categorical neglogp and entropy, in
    place on ``st``; the same returns and ``keep`` entries as ``ppo_ref.ppo_step``."""
    par = {**R.DEFAULTS, **par}
    dt = st.alpha.dtype.type
    F = lambda x: O._F(dt, x)
    adv = R.normalise_adv(adv, par, dt)
    nlp_old = np.asarray(nlp_old, dt)
    n = adv.shape[0]
    logits, xn, hs = forward(st, cfg, nrm, s)
    nlp = neglogp_of(logits, a)
    ent = entropy_of(logits)
    lo, hi = F(np.float32(1.0 - par["eps_ppo"])), F(np.float32(1.0 + par["eps_ppo"]))
    r = np.exp(nlp_old - nlp)
    rc = np.minimum(np.maximum(r, lo), hi)
    surr, clp = -(r * adv), -(rc * adv)
    take = surr >= clp
    pg = np.mean(np.maximum(surr, clp))
    em = np.mean(ent)
    alpha = st.alpha.copy()
    loss = pg - alpha * (em - F(par["ent_targ"]))
    gn = np.where(take, adv * r, F(0)) * F(1.0 / n)
    dl = gn[:, None] * dnlp_dlogits(logits, a) - (alpha * F(1.0 / n)) * dent_dlogits(logits)
    grads = O.actor_backward(st.actor, xn, hs, dl, cfg)
    alpha_grad = em - F(par["ent_targ"])
    if par["ent_reg"]:
        av = [np.array(st.alpha, dt)]
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
        keep.update(grads=grads, clipped=clipped, alpha_grad=alpha_grad, r=r, take=take, adv=adv, dl=dl)
    O.adam_step(st.actor, clipped, st.opt_actor, par["actor_lr"], dt)
    return dict(loss=float(loss), ent=float(em), grad_norm_pre=float(norm), grad_norm_post=float(post),
                alpha=float(st.alpha), pg_loss=float(pg))


class PPORef:
    """``PPO`` (ppo.py:6-119) over the restatement, as ``ppo_ref.PPORef``."""

    def __init__(self, st, cfg, nrm, kw, rs):
        self.st, self.cfg, self.nrm, self.kw, self.rs = st, cfg, nrm, dict(kw), rs
        self.actor_lr = np.float32(kw["actor_lr"])

    def update(self, s_all, a_all, adv_all, keep=None):
        st, cfg, nrm, kw = self.st, self.cfg, self.nrm, self.kw
        dt = st.alpha.dtype.type
        l0 = forward(st, cfg, nrm, s_all)[0]
        nlp_old = neglogp_of(l0, a_all)
        ref = l0.copy()
        ent = np.mean(entropy_of(l0))
        n = s_all.shape[0]
        pre = post = dt(0)
        steps = 0
        par = dict(eps_ppo=kw["eps_ppo"], max_grad_norm=kw["max_grad_norm"], ent_targ=kw["ent_targ"],
                   ent_reg=kw["ent_reg"], alpha_lr=kw["alpha_lr"], adv_center=kw["adv_center"],
                   adv_scale=kw["adv_scale"], actor_lr=float(self.actor_lr))
        for _ in range(kw["actor_update_it"]):
            idx = np.arange(n)
            self.rs.shuffle(idx)
            for b in R.split_reference(n, kw["actor_nminibatch"], idx):
                o = ppo_step(st, cfg, nrm, s_all[b], a_all[b], adv_all[b], nlp_old[b], par)
                pre, post = pre + dt(o["grad_norm_pre"]), post + dt(o["grad_norm_post"])
                steps += 1
        l1 = forward(st, cfg, nrm, s_all)[0]
        rdiff = np.abs(np.exp(nlp_old - neglogp_of(l1, a_all)) - dt(1))
        tv = dt(0.5) * np.mean(rdiff)
        log = dict(ent=float(ent), tv=float(tv), kl=float(np.mean(kl_of(l1, ref))), alpha=float(st.alpha),
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


# ------------------------------------------------------------------ TRPO
def surrogate_grad(st, cfg, nrm, s, a, adv_n, nlp_old, ent_targ):
    """trpo.py:52-63: (neg_pg as the trainables' list, mean entropy, the loss)."""
    dt = st.alpha.dtype.type
    F = lambda x: O._F(dt, x)
    adv_n, nlp_old = np.asarray(adv_n, dt), np.asarray(nlp_old, dt)
    n = adv_n.shape[0]
    logits, xn, hs = forward(st, cfg, nrm, s)
    r = np.exp(nlp_old - neglogp_of(logits, a))
    em = np.mean(entropy_of(logits))
    loss = np.mean(-(r * adv_n)) - st.alpha * (em - F(ent_targ))
    gn = (adv_n * r) * F(1.0 / n)
    dl = gn[:, None] * dnlp_dlogits(logits, a) - (st.alpha * F(1.0 / n)) * dent_dlogits(logits)
    return O.actor_backward(st.actor, xn, hs, dl, cfg), em, loss


def tangent(st, cfg, xn, hs, V):
    """J x at the forward pass: the logits' tangent for the direction V (the trainables' list), by
    ``trpo_ref.tangent`` on a distribution without a logstd."""
    dt = st.alpha.dtype.type
    d = types.SimpleNamespace(xn=xn, hs=hs, raw=None, ls_un=np.zeros((), dt), floor=dt(-1))
    c = dataclasses.replace(cfg, per_state_std=False)
    return T.tangent(st, c, d, list(V) + [np.zeros((1, cfg.A), dt)])[0]


def fvp(st, cfg, nrm, s_sub, x, damp):
    """_make_F's F(x) (trpo.py:200-227): (1 / n) sum_i J_i^T (diag(p_i) - p_i p_i^T) J_i x + damp x."""
    dt = st.alpha.dtype.type
    F = lambda v: O._F(dt, v)
    logits, xn, hs = forward(st, cfg, nrm, s_sub)
    n = logits.shape[0]
    t = tangent(st, cfg, xn, hs, x)
    _, p = logp_of(logits)
    u = (p * (t - (p * t).sum(-1, keepdims=True))) * F(1.0 / n)
    g = O.actor_backward(st.actor, xn, hs, u, cfg)
    return [gi + F(damp) * np.asarray(xi, dt).reshape(gi.shape) for gi, xi in zip(g, x)]


def set_weights(st, weights):
    """discrete_actors.py:109-117: nothing is floored."""
    dt = st.alpha.dtype.type
    st.actor = [np.asarray(w, dt).reshape(o.shape).copy() for w, o in zip(weights, st.actor)]


def _figures(st, cfg, nrm, s, a, adv2, nlp_old, ref):
    dt = st.alpha.dtype.type
    logits = forward(st, cfg, nrm, s)[0]
    ratio = np.exp(nlp_old - neglogp_of(logits, a))
    return (np.mean(ratio * adv2), dt(0.5) * np.mean(np.abs(ratio - dt(1))), np.mean(kl_of(logits, ref)))


def backtrack(st, cfg, nrm, step, s, a, adv_n, nlp_old, par, keep=None):
    """_backtrack (trpo.py:229-317) in place on ``st``, as ``trpo_ref.backtrack``."""
    dt = st.alpha.dtype.type
    l0 = forward(st, cfg, nrm, s)[0]
    ent = np.mean(entropy_of(l0))
    ref = l0.copy()
    saved = [np.array(w) for w in st.actor]
    adv2 = R.normalise_adv(adv_n, par, dt)
    nlp_old = np.asarray(nlp_old, dt)
    fig = lambda: _figures(st, cfg, nrm, s, a, adv2, nlp_old, ref)
    surr_before = fig()[0]
    step = np.asarray(step, dt).copy()
    kl_max = dt(np.float32(par["kl_maxfactor"] * par["delta_trpo"]))

    def apply(stp):
        set_weights(st, [w + i for w, i in zip(saved, T.from_flat(saved, stp))])

    apply(step)
    surr, tv, klv = fig()
    improve = surr - surr_before
    tv_pre, kl_pre = tv, klv
    adj, trials, ok = 1.0, [(float(klv), float(improve))], False
    for _ in range(10):
        if not (klv > kl_max) and not (improve < 0):
            ok = True
            break
        adj = adj / np.sqrt(2)
        step = step / dt(np.float32(np.sqrt(2)))
        apply(step)
        surr, tv, klv = fig()
        improve = surr - surr_before
        trials.append((float(klv), float(improve)))
    if not ok:
        adj = 0
        set_weights(st, saved)
        surr, tv, klv = fig()
        improve = surr - surr_before
    if keep is not None:
        keep.update(trials=trials[:10] if not ok else trials, kl_max=float(kl_max), saved=saved)
    return dict(ent=float(ent), tv_pre=float(tv_pre), kl_pre=float(kl_pre), tv=float(tv), kl=float(klv), adj=float(adj),
                improve=float(improve))


class TRPORef:
    """``TRPO`` (trpo.py:8-317) over the restatement, as ``trpo_ref.TRPORef``."""

    def __init__(self, st, cfg, nrm, kw, dots64=False):
        self.st, self.cfg, self.nrm, self.kw, self.dots64 = st, cfg, nrm, {**T.DEFAULTS, **kw}, dots64

    def update(self, s_all, a_all, adv_all, keep=None):
        st, cfg, nrm, kw = self.st, self.cfg, self.nrm, self.kw
        dt = st.alpha.dtype.type
        F = lambda x: O._F(dt, x)
        nlp_old = neglogp(st, cfg, nrm, s_all, a_all)
        adv_n = R.normalise_adv(adv_all, kw, dt)
        neg_pg, em, _ = surrogate_grad(st, cfg, nrm, s_all, a_all, adv_n, nlp_old, kw["ent_targ"])
        if kw["ent_reg"]:
            av = [np.array(st.alpha, dt)]
            O.adam_step(av, [np.asarray(em - F(kw["ent_targ"]))], st.opt_alpha, kw["alpha_lr"], dt)
            st.alpha = np.array(np.maximum(av[0], F(0)), dt)
        pg_vec = T.to_flat(neg_pg) * -1
        like = st.actor
        info = dict(pg_vec=pg_vec)
        if np.allclose(pg_vec, 0) or kw["delta_trpo"] == 0.0:
            step = np.zeros_like(pg_vec)
            info.update(zero=True)
        else:
            s_sub = s_all[::kw["trust_sub"]]
            Fx = lambda x: T.to_flat(fvp(st, cfg, nrm, s_sub, T.from_flat(like, x), kw["trust_damp"]))
            v = T.cg(Fx, pg_vec, cg_iters=kw["cg_it"], keep=info, dots64=self.dots64)
            vFv = T.dot64(v, Fx(v)) if self.dots64 else np.dot(v, Fx(v))
            eta = np.sqrt(2 * np.float64(np.float32(kw["delta_trpo"])) / vFv) if self.dots64 else \
                np.sqrt(F(2) * F(kw["delta_trpo"]) / vFv)
            step = dt(eta) * v
            info.update(zero=False, vFv=float(vFv), eta=float(eta))
        log = backtrack(st, cfg, nrm, step, s_all, a_all, adv_n, nlp_old, kw, info)
        log["alpha"] = float(st.alpha)
        if keep is not None:
            keep.update(info)
        return log
