"""The TRPO actor update of a plain GaussianActor (reference ``sac_eo/algs/model_free/trpo.py:34-317``, the
``expert_reg is None`` branch with the one reading that makes it run, ``grad_final := neg_pg``;
``update_utils.py:4-24``; ``continuous_actors.py:201-234``) restated in NumPy on the primitives of
``ppo_ref`` / ``sac_oracle``.  Test infrastructure only.

The compute dtype is the state's (fp64 for the parity bars, fp32 for the drift envelope).  The Fisher
product is in the Gauss-Newton form ``(1 / n_sub) sum_i J_i^T M_i J_i x + damp x``, which equals the
Hessian of the mean KL at the reference point exactly (``test_trpo_ref.py`` pins it to torch's double
backward): a tangent forward, the scale by ``M / n_sub``, the backward ``ppo_ref`` uses.  Flat vectors are
the trainables in the Keras order raveled and joined (``list_to_flat``).
"""
import numpy as np

import ppo_ref as R
import sac_oracle as O

DEFAULTS = dict(delta_trpo=0.02, cg_it=20, trust_sub=1, trust_damp=0.01, kl_maxfactor=1.5, ent_reg=False, ent_targ=0.0,
                alpha_lr=0.0, adv_center=True, adv_scale=True)
LOG_KEYS = ("ent", "tv_pre", "kl_pre", "tv", "kl", "adj", "improve", "alpha")


def to_flat(arrays):
    return np.concatenate([np.asarray(x).reshape(-1) for x in arrays], -1)


def from_flat(like, flat):
    out, o = [], 0
    for x in like:
        out.append(np.asarray(flat[o:o + x.size]).reshape(x.shape))
        o += x.size
    assert o == flat.size
    return out


def _act(acts, l):
    return acts[l] if isinstance(acts, (list, tuple)) else acts


def surrogate_grad(st, cfg, nrm, s, a, adv_n, nlp_old, ent_targ):
    """trpo.py:52-63: (neg_pg as the trainables' list, mean entropy, the loss) of
    loss = mean(-r adv) - alpha (mean(ent) - ent_targ); adv_n is already normalised."""
    dt = st.alpha.dtype.type
    F = lambda x: O._F(dt, x)
    a, adv_n, nlp_old = np.asarray(a, dt), np.asarray(adv_n, dt), np.asarray(nlp_old, dt)
    n = a.shape[0]
    d = R.forward(st, cfg, nrm, s)
    sd = np.exp(d.ls)
    z = (a - d.mean) / sd
    nlp = F(0.5) * (z * z + F(2) * d.ls + R._log2pi(dt)).sum(-1)
    r = np.exp(nlp_old - nlp)
    em = np.mean(R.entropy_of(d))
    loss = np.mean(-(r * adv_n)) - st.alpha * (em - F(ent_targ))
    gn = (adv_n * r) * F(1.0 / n)                              # d loss / d nlp_cur
    dmean = gn[:, None] * (-(z / sd))
    dls = gn[:, None] * (F(1) - z * z) - st.alpha * F(1.0 / n)
    dls = dls * (d.ls_un >= d.floor)
    if cfg.per_state_std:
        draw = (dls * (F(1) / O.softplus(d.raw))) / (np.exp(-d.raw) + F(1))
        grads = O.actor_backward(st.actor, d.xn, d.hs, np.concatenate([dmean, draw], 1), cfg)
    else:
        grads = O.actor_backward(st.actor, d.xn, d.hs, dmean, cfg) + [dls.sum(0, keepdims=True)]
    return grads, em, loss


def tangent(st, cfg, d, V):
    """J x at the forward pass ``d``: (t_mean, t_ls) for the direction V (the trainables' list)."""
    dt = st.alpha.dtype.type
    F = lambda x: O._F(dt, x)
    P, acts = st.actor, cfg.aacts
    Va = [np.asarray(v, dt) for v in V[:len(P)]]
    if cfg.layer_norm:
        h1, rest, xh, rstd = d.hs[0], d.hs[1:-2], d.hs[-2], d.hs[-1]
        tz = d.xn @ Va[0] + Va[1]
        txh = rstd * ((tz - tz.mean(-1, keepdims=True)) - xh * (tz * xh).mean(-1, keepdims=True))
        ty = P[2] * txh + Va[2] * xh + Va[3]
        t = (F(1) - h1 * h1) * ty
        Pm, Vm, hs, am, h_in = P[4:], Va[4:], rest, acts[1:] if isinstance(acts, (list, tuple)) else acts, h1
    else:
        t, Pm, Vm, hs, am, h_in = None, P, Va, d.hs, acts, d.xn
    nl = len(Pm) // 2
    tout = None
    for l in range(nl):
        pre = h_in @ Vm[2 * l] + Vm[2 * l + 1]
        if t is not None:
            pre = pre + t @ Pm[2 * l]
        if l < nl - 1:
            t = O.act_grad(hs[l], _act(am, l)) * pre
            h_in = hs[l]
        else:
            tout = pre
    if cfg.per_state_std:
        tm, traw = tout[:, :cfg.A], tout[:, cfg.A:]
        tl = (traw * (F(1) / O.softplus(d.raw))) / (np.exp(-d.raw) + F(1))
    else:
        tm = tout
        tl = np.broadcast_to(np.asarray(V[-1], dt).reshape(1, cfg.A), tout.shape)
    return tm, tl * (d.ls_un >= d.floor)


def fvp(st, cfg, nrm, s_sub, x, damp):
    """_make_F's F(x) (trpo.py:200-227) in the Gauss-Newton form; x and the result are trainables' lists."""
    dt = st.alpha.dtype.type
    F = lambda v: O._F(dt, v)
    d = R.forward(st, cfg, nrm, s_sub)
    n = d.mean.shape[0]
    tm, tl = tangent(st, cfg, d, x)
    um = (tm / np.exp(F(2) * d.ls)) * F(1.0 / n)
    ul = (F(2) * tl) * F(1.0 / n) * (d.ls_un >= d.floor)
    if cfg.per_state_std:
        draw = (ul * (F(1) / O.softplus(d.raw))) / (np.exp(-d.raw) + F(1))
        g = O.actor_backward(st.actor, d.xn, d.hs, np.concatenate([um, draw], 1), cfg)
    else:
        g = O.actor_backward(st.actor, d.xn, d.hs, um, cfg) + [ul.sum(0, keepdims=True)]
    return [gi + F(damp) * np.asarray(xi, dt).reshape(gi.shape) for gi, xi in zip(g, x)]


def dot64(x, y):
    """A dot product accumulated in f64 whatever the vectors' dtype (what the device does)."""
    return np.dot(np.asarray(x, np.float64), np.asarray(y, np.float64))


def cg(f_Ax, b, cg_iters=20, residual_tol=1e-10, keep=None, dots64=False):
    """update_utils.cg (:4-24) on flat vectors in b's dtype.  ``dots64``: the dot products accumulated in
    f64 and the two scalars of an iteration rounded to the vectors' dtype -- the arithmetic the device is
    specified to use, another faithful execution in that dtype."""
    dt = b.dtype.type
    dot = dot64 if dots64 else (lambda x, y: x.dot(y))
    p, r, x = b.copy(), b.copy(), np.zeros_like(b)
    rdotr = dot(r, r)
    its, hist = 0, [float(rdotr)]
    for _ in range(cg_iters):
        z = f_Ax(p)
        v = dt(rdotr / dot(p, z))
        x += v * p
        r -= v * z
        newrdotr = dot(r, r)
        mu = dt(newrdotr / rdotr)
        p = r + mu * p
        rdotr = newrdotr
        its += 1
        hist.append(float(rdotr))
        if rdotr < residual_tol:
            break
    if keep is not None:
        keep.update(cg_iters=its, rdotr=float(rdotr), rr_hist=hist)
    return x


def set_weights(st, cfg, weights):
    """GaussianActor.set_weights (continuous_actors.py:211-234): the raw state-independent logstd is
    floored at log 1e-3 whenever it is set."""
    dt = st.alpha.dtype.type
    na = len(st.actor)
    st.actor = [np.asarray(w, dt).reshape(o.shape).copy() for w, o in zip(weights[:na], st.actor)]
    if not cfg.per_state_std:
        st.logstd = np.maximum(np.asarray(weights[na], dt).reshape(st.logstd.shape), O._F(dt, np.float32(np.log(1e-3))))


def _figures(st, cfg, nrm, s, a, adv2, nlp_old, mean_ref, ls_ref):
    dt = st.alpha.dtype.type
    d = R.forward(st, cfg, nrm, s)
    ratio = np.exp(nlp_old - R.neglogp_of(d, a))
    return (np.mean(ratio * adv2), dt(0.5) * np.mean(np.abs(ratio - dt(1))), np.mean(R.kl_of(d, mean_ref, ls_ref)))


def backtrack(st, cfg, nrm, step, s, a, adv_n, nlp_old, par, keep=None):
    """_backtrack (trpo.py:229-317) in place on ``st``; ``step`` is the flat eta_v; ``adv_n`` the advantages
    update() normalised, normalised here a second time as the reference does."""
    dt = st.alpha.dtype.type
    d0 = R.forward(st, cfg, nrm, s)
    ent = np.mean(R.entropy_of(d0))
    mean_ref, ls_ref = d0.mean.copy(), d0.ls.copy()
    saved = [np.array(w) for w in st.trainables(cfg)]
    adv2 = R.normalise_adv(adv_n, par, dt)
    nlp_old, a = np.asarray(nlp_old, dt), np.asarray(a, dt)
    surr_before = _figures(st, cfg, nrm, s, a, adv2, nlp_old, mean_ref, ls_ref)[0]
    step = np.asarray(step, dt).copy()
    kl_max = dt(np.float32(par["kl_maxfactor"] * par["delta_trpo"]))

    def apply(stp):
        set_weights(st, cfg, saved)
        inc = from_flat(saved, stp)
        set_weights(st, cfg, [w + i for w, i in zip(st.trainables(cfg), inc)])

    apply(step)
    surr, tv, kl = _figures(st, cfg, nrm, s, a, adv2, nlp_old, mean_ref, ls_ref)
    improve = surr - surr_before
    tv_pre, kl_pre = tv, kl
    adj, trials, ok = 1.0, [(float(kl), float(improve))], False
    for _ in range(10):
        if not (kl > kl_max) and not (improve < 0):
            ok = True
            break
        adj = adj / np.sqrt(2)
        step = step / dt(np.float32(np.sqrt(2)))
        apply(step)
        surr, tv, kl = _figures(st, cfg, nrm, s, a, adv2, nlp_old, mean_ref, ls_ref)
        improve = surr - surr_before
        trials.append((float(kl), float(improve)))
    if not ok:
        adj = 0
        set_weights(st, cfg, saved)
        surr, tv, kl = _figures(st, cfg, nrm, s, a, adv2, nlp_old, mean_ref, ls_ref)
        improve = surr - surr_before
    if keep is not None:
        # every line-search decision: (kl - kl_max, improve) of each trial that was tested
        keep.update(trials=trials[:10] if not ok else trials, kl_max=float(kl_max), saved=saved)
    return dict(ent=float(ent), tv_pre=float(tv_pre), kl_pre=float(kl_pre), tv=float(tv), kl=float(kl), adj=float(adj),
                improve=float(improve))


class TRPORef:
    """``TRPO`` (trpo.py:8-317) over the restatement; ``update`` returns the eight log values."""

    def __init__(self, st, cfg, nrm, kw, dots64=False):
        self.st, self.cfg, self.nrm, self.kw, self.dots64 = st, cfg, nrm, {**DEFAULTS, **kw}, dots64

    def update(self, s_all, a_all, adv_all, keep=None):
        st, cfg, nrm, kw = self.st, self.cfg, self.nrm, self.kw
        dt = st.alpha.dtype.type
        F = lambda x: O._F(dt, x)
        nlp_old = R.neglogp(st, cfg, nrm, s_all, a_all)
        adv_n = R.normalise_adv(adv_all, kw, dt)
        neg_pg, em, _ = surrogate_grad(st, cfg, nrm, s_all, a_all, adv_n, nlp_old, kw["ent_targ"])
        if kw["ent_reg"]:                                  # Keras Adam on alpha with gradient mean(ent) - ent_targ
            av = [np.array(st.alpha, dt)]
            O.adam_step(av, [np.asarray(em - F(kw["ent_targ"]))], st.opt_alpha, kw["alpha_lr"], dt)
            st.alpha = np.array(np.maximum(av[0], F(0)), dt)
        pg_vec = to_flat(neg_pg) * -1
        like = st.trainables(cfg)
        info = dict(pg_vec=pg_vec)
        if np.allclose(pg_vec, 0) or kw["delta_trpo"] == 0.0:
            step = np.zeros_like(pg_vec)
            info.update(zero=True)
        else:
            s_sub = s_all[::kw["trust_sub"]]
            Fx = lambda x: to_flat(fvp(st, cfg, nrm, s_sub, from_flat(like, x), kw["trust_damp"]))
            v = cg(Fx, pg_vec, cg_iters=kw["cg_it"], keep=info, dots64=self.dots64)
            vFv = dot64(v, Fx(v)) if self.dots64 else np.dot(v, Fx(v))
            eta = np.sqrt(2 * np.float64(np.float32(kw["delta_trpo"])) / vFv) if self.dots64 else \
                np.sqrt(F(2) * F(kw["delta_trpo"]) / vFv)
            step = dt(eta) * v
            info.update(zero=False, vFv=float(vFv), eta=float(eta))
        log = backtrack(st, cfg, nrm, step, s_all, a_all, adv_n, nlp_old, kw, info)
        log["alpha"] = float(st.alpha)
        if keep is not None:
            keep.update(info)
        return log
