"""tests/softmax_ref.py against torch autograd in f64 on the CPU: the gradients of neglogp, entropy, kl and
the PPO loss, and the Fisher product against the autograd Hessian of the mean kl at the reference point.
Random inputs from well-conditioned logits to logits of +-80; agreement to 1e-10 of each tensor's largest
entry.  This tests the restatement, not the device."""
import numpy as np
import pytest
import torch

import ppo_ref as R
import sac_oracle as O
import softmax_ref as SM
import trpo_ref as T
from helpers import nontrivial_normalizers, relerr

TOL = 1e-10
SPANS = [1.0, 10.0, 80.0]           # the logits' half-range


def _logits(span, n=37, A=5, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.normal(size=(n, A))
    x = x / np.abs(x).max() * span
    ref = x + 0.3 * rng.normal(size=(n, A))
    a = rng.randint(0, A, size=n).astype(np.float64)
    a[3] = -1.0                      # tf.one_hot's all-zero rows
    a[7] = A
    return x, ref, a


def _t_logp(l):
    x = l - l.max(-1, keepdim=True).values.detach()
    return x - torch.log(torch.exp(x).sum(-1, keepdim=True))


def _t_nlp(l, a):
    A = l.shape[-1]
    ai = torch.as_tensor(np.asarray(a, np.int64))
    ok = (ai >= 0) & (ai < A)
    oh = torch.zeros(l.shape, dtype=l.dtype)
    oh[ok, ai[ok]] = 1
    return -(oh * _t_logp(l)).sum(-1)


def _t_ent(l):
    lp = _t_logp(l)
    return -(torch.exp(lp) * lp).sum(-1)


def _t_kl(l, ref):
    lp, lpr = _t_logp(l), _t_logp(ref)
    return (torch.exp(lp) * (lp - lpr)).sum(-1)


@pytest.mark.parametrize("span", SPANS)
def test_row_values_and_gradients_at_the_logits(span):
    x, ref, a = _logits(span)
    l = torch.tensor(x, requires_grad=True)
    w = torch.tensor(np.random.RandomState(1).normal(size=x.shape[0]))      # a weight per row
    cases = [("neglogp", _t_nlp(l, a), SM.neglogp_of(x, a), SM.dnlp_dlogits(x, a)),
             ("entropy", _t_ent(l), SM.entropy_of(x), SM.dent_dlogits(x)),
             ("kl", _t_kl(l, torch.tensor(ref)), SM.kl_of(x, ref), SM.dkl_dlogits(x, ref))]
    for name, tv, val, grad in cases:
        g, = torch.autograd.grad((tv * w).sum(), l, retain_graph=True)
        assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad)), name
        assert relerr(val, tv.detach().numpy()) < TOL, (name, span)
        assert relerr(grad * w.numpy()[:, None], g.numpy()) < TOL, (name, span)
    assert SM.neglogp_of(x, a)[3] == 0 and SM.neglogp_of(x, a)[7] == 0
    assert not SM.dnlp_dlogits(x, a)[[3, 7]].any()
    one = np.full((4, 1), 3.7)       # one action: everything is exactly 0
    assert not SM.neglogp_of(one, np.zeros(4)).any() and not SM.entropy_of(one).any() and not SM.kl_of(one, one - 2).any()


def _case(span, seed=3, n=41, S=5, A=4, hidden=(16, 12)):
    cfg = O.Config(S=S, A=A, hidden=hidden, actor_acts=("tanh", "tanh"))
    st = SM.init_state(cfg, seed=seed)
    rng = np.random.RandomState(seed + 7)
    nrm = nontrivial_normalizers(rng, S, A)
    s = rng.normal(size=(n, S))
    lg = SM.forward(st, cfg, nrm, s)[0]
    k = span / np.abs(lg - lg.mean(-1, keepdims=True)).max()       # scale the last layer: logits of about +-span
    st.actor[-2] *= k
    st.actor[-1] *= k
    a = rng.randint(0, A, size=n).astype(np.float64)
    a[5] = A + 2
    adv = rng.normal(size=n) * 1.5 + 0.4
    return cfg, st, nrm, s, a, adv


def _t_forward(ws, nrm, s):
    h = (torch.tensor(s) - torch.tensor(np.asarray(nrm.s_mean, np.float64))) / torch.tensor(np.asarray(nrm.s_den, np.float64))
    for i in range(0, len(ws) - 2, 2):
        h = torch.tanh(h @ ws[i] + ws[i + 1])
    return h @ ws[-2] + ws[-1]


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("opts", [dict(max_grad_norm=None), dict(max_grad_norm=0.5, adv_center=False, adv_scale=False)])
def test_ppo_loss_gradient(span, opts):
    cfg, st, nrm, s, a, adv = _case(span)
    st.alpha = np.array(0.3)
    st0 = st.copy()
    rng = np.random.RandomState(4)
    for w in st0.actor:              # the rollout's policy: off the current one
        w *= 1.0 + 0.3 * rng.normal(size=w.shape)
    nlp_old = SM.neglogp(st0, cfg, nrm, s, a)
    par = {**R.DEFAULTS, "ent_targ": 0.7, **opts}
    keep = {}
    out = SM.ppo_step(st.copy(), cfg, nrm, s, a, adv, nlp_old, par, keep)
    ws = [torch.tensor(w, requires_grad=True) for w in st.actor]
    l = _t_forward(ws, nrm, s)
    advn = torch.tensor(R.normalise_adv(adv, par, np.float64))
    r = torch.exp(torch.tensor(nlp_old) - _t_nlp(l, a))
    lo, hi = float(np.float32(1 - par["eps_ppo"])), float(np.float32(1 + par["eps_ppo"]))
    loss = torch.maximum(-(r * advn), -(torch.clamp(r, lo, hi) * advn)).mean() - 0.3 * (_t_ent(l).mean() - 0.7)
    gs = torch.autograd.grad(loss, ws)
    assert abs(out["loss"] - loss.item()) <= TOL * max(1.0, abs(loss.item()))
    assert 3 <= keep["take"].sum() <= len(a) - 3                    # both branches of the clip occur
    for g, gt in zip(keep["grads"], gs):
        assert relerr(g, gt.numpy()) < TOL, span


@pytest.mark.parametrize("span", SPANS)
def test_fisher_product_is_the_hessian_of_the_mean_kl_at_the_reference_point(span):
    cfg, st, nrm, s, a, adv = _case(span, seed=5)
    rng = np.random.RandomState(9)
    x = [rng.normal(size=w.shape) for w in st.actor]
    got = SM.fvp(st, cfg, nrm, s, x, damp=0.0)
    ws = [torch.tensor(w, requires_grad=True) for w in st.actor]
    l = _t_forward(ws, nrm, s)
    klm = _t_kl(l, l.detach()).mean()
    g1 = torch.autograd.grad(klm, ws, create_graph=True)
    hv = torch.autograd.grad(sum((g * torch.tensor(v)).sum() for g, v in zip(g1, x)), ws)
    scale = max(float(h.abs().max()) for h in hv)
    for g, h in zip(got, hv):
        assert float(np.max(np.abs(g - h.numpy()))) < TOL * scale, span
    # damping, and the flat helpers round-trip
    gd = SM.fvp(st, cfg, nrm, s, x, damp=0.25)
    assert relerr(T.to_flat(gd), T.to_flat(got) + 0.25 * T.to_flat(x)) < 1e-14


def test_trpo_surrogate_gradient_and_update_run():
    cfg, st, nrm, s, a, adv = _case(10.0, seed=2)
    st.alpha = np.array(0.2)
    nlp_old = SM.neglogp(st, cfg, nrm, s, a)
    advn = R.normalise_adv(adv, T.DEFAULTS, np.float64)
    grads, em, loss = SM.surrogate_grad(st, cfg, nrm, s, a, advn, nlp_old, 0.5)
    ws = [torch.tensor(w, requires_grad=True) for w in st.actor]
    l = _t_forward(ws, nrm, s)
    tl = (-(torch.exp(torch.tensor(nlp_old) - _t_nlp(l, a)) * torch.tensor(advn))).mean() - 0.2 * (_t_ent(l).mean() - 0.5)
    for g, gt in zip(grads, torch.autograd.grad(tl, ws)):
        assert relerr(g, gt.numpy()) < TOL
    st.alpha = np.array(0.0)
    before = [w.copy() for w in st.actor]
    keep = {}
    log = SM.TRPORef(st, cfg, nrm, dict(delta_trpo=0.02, cg_it=10)).update(s, a, adv, keep)
    assert sorted(log) == sorted(T.LOG_KEYS) and keep["vFv"] > 0 and log["adj"] > 0
    assert log["kl"] <= 1.5 * 0.02 and log["improve"] >= 0 and any((w != b).any() for w, b in zip(st.actor, before))
    assert SM.gumbel_argmax(np.array([[0.0, 5.0, 5.0]], np.float32), None)[0] == 1      # the first index on a tie
