"""The PPO restatement (tests/ppo_ref.py) on the CPU.

* ``ppo_ref.ppo_step`` in fp64 against torch autograd (float64) of the loss of ``ppo.py:132-143`` written
  out directly: the loss, every parameter gradient, alpha's gradient, the clipped gradients, both norms
  and the weights after Keras Adam agree to <= 1e-10 relative.  Cases: state-independent std and
  ``per_state_std``, layer norm, 1 / 2 / 3 layers, ``max_grad_norm`` None / clipping / not clipping,
  ``adv_center`` / ``adv_scale`` off, ``ent_reg`` over 3 consecutive steps (alpha leaves 0), one logstd
  dimension below the floor and one above, every minibatch with rows in all three clip regimes.
* the minibatch split against a literal transcription of ``ppo.py:55-62``.
"""
import numpy as np
import pytest
import torch

import ppo_ref as R
import sac_oracle as O

CASES = {
    "ind_2": dict(hidden=(16, 12), acts=("tanh", "tanh"), par=dict(max_grad_norm=None)),
    "pss_1": dict(hidden=(20,), acts=("elu",), per_state_std=True, par=dict(max_grad_norm=0.05)),
    "ln_3": dict(hidden=(16, 12, 10), acts=("tanh", "relu", "elu"), layer_norm=True,
                 par=dict(max_grad_norm=1e4, adv_center=False)),
    "ind_raw_adv": dict(hidden=(12, 12), acts=("relu", "tanh"), par=dict(adv_center=False, adv_scale=False,
                                                                         max_grad_norm=0.5)),
    "pss_ln_2": dict(hidden=(12, 8), acts=("tanh", "elu"), per_state_std=True, layer_norm=True, std_mult=0.7,
                     par=dict(max_grad_norm=None, adv_scale=False)),
    "ent_reg": dict(hidden=(12, 12), acts=("tanh", "tanh"), par=dict(ent_reg=True, alpha_lr=0.02, ent_targ=9.0,
                                                                     max_grad_norm=0.5, actor_lr=1e-4), steps=3),
}
S, A, N = 5, 3, 40


def make_case(name, seed=3, dt=np.float64):
    c = dict(CASES[name])
    cfg = O.Config(S=S, A=A, hidden=c["hidden"], actor_acts=c["acts"], per_state_std=c.get("per_state_std", False),
                   layer_norm=c.get("layer_norm", False))
    rng = np.random.RandomState(seed)
    # one logstd dimension below the floor log(1e-3) = -6.9, the others above
    st_old = R.init_state(cfg, seed=seed, std_mult=c.get("std_mult", 1.0), logstd=[-8.0, 0.1, -0.3], dt=dt)
    if cfg.per_state_std:
        st_old.actor[-1][A] = -8.0                      # raw of dimension 0: log(softplus(-8)) + init < floor
    # dimension 0 has std 1e-3 (the floor): its mean is its bias alone, so that the ratio stays finite
    st_old.actor[-2][:, 0] = 0.0
    nrm = O.Normalizers.identity(S, A)
    nrm.s_mean = rng.normal(size=S).astype(np.float32) * 0.2
    nrm.s_den = (0.5 + rng.uniform(size=S)).astype(np.float32)
    s = rng.normal(size=(N, S)).astype(np.float32)
    d0 = R.forward(st_old, cfg, nrm, s)
    a = (d0.mean + np.exp(d0.ls) * rng.normal(size=(N, A))).astype(np.float32)
    adv = rng.normal(size=N).astype(np.float32) * 2.0 + 0.5
    nlp_old = R.neglogp_of(d0, a)
    st = st_old.copy()                                  # the current policy: moved away from the old one
    w0, b0 = st.actor[-2][:, 0].copy(), st.actor[-1][0]
    for w in st.actor:
        w += 0.08 * rng.normal(size=w.shape)
    st.actor[-2][:, 0] = w0
    st.actor[-1][0] = b0 + 3e-4 * rng.normal()
    st.logstd += 0.05 * rng.normal(size=st.logstd.shape)
    par = {**R.DEFAULTS, "actor_lr": 3e-3, **c["par"]}
    return cfg, st, nrm, s, a, adv, nlp_old, par, c.get("steps", 1)


def torch_step(st, cfg, nrm, s, a, adv, nlp_old, par):
    """Loss and gradients by autograd; returns loss, grads (trainables order), alpha_grad."""
    T = lambda x: torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)
    ws = [T(w).requires_grad_(True) for w in st.actor]
    logstd = T(st.logstd).requires_grad_(True)
    alpha = T(st.alpha).requires_grad_(True)
    acts = {"relu": torch.relu, "tanh": torch.tanh, "elu": torch.nn.functional.elu}
    h = (T(s) - T(nrm.s_mean)) / T(nrm.s_den)
    rest, names = ws, list(cfg.aacts)
    if cfg.layer_norm:
        z = h @ ws[0] + ws[1]
        d = z - z.mean(-1, keepdim=True)
        xh = d / torch.sqrt((d * d).mean(-1, keepdim=True) + O.LN_EPS)
        h = torch.tanh(ws[2] * xh + ws[3])
        rest, names = ws[4:], names[1:]
    nl = len(rest) // 2
    for l in range(nl):
        h = h @ rest[2 * l] + rest[2 * l + 1]
        if l < nl - 1:
            h = acts[names[l]](h)
    lsi = float(R.logstd_init(cfg, st.std_mult))
    if cfg.per_state_std:
        mean, raw = h[:, :A], h[:, A:]
        ls_un = torch.log(torch.log1p(torch.exp(raw))) + lsi
    else:
        mean, ls_un = h, logstd * torch.ones_like(h) + lsi
    ls = torch.maximum(ls_un, T(np.log(np.float64(1e-3))))
    adv_n = T(R.normalise_adv(adv, par, np.float64))
    z = (T(a) - mean) / torch.exp(ls)
    log2pi = float(np.log(2 * np.pi))
    nlp = 0.5 * (z * z + 2 * ls + log2pi).sum(-1)
    ent = 0.5 * (2 * ls + log2pi + 1).sum(-1)
    r = torch.exp(T(nlp_old) - nlp)
    rc = torch.clamp(r, float(np.float32(1 - par["eps_ppo"])), float(np.float32(1 + par["eps_ppo"])))
    loss = torch.maximum(r * adv_n * -1, rc * adv_n * -1).mean() - alpha * (ent.mean() - par["ent_targ"])
    loss.backward()
    tr = ws + ([] if cfg.per_state_std else [logstd])
    return float(loss.detach()), [w.grad.numpy() for w in tr], -float(alpha.grad)


def rel(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.max(np.abs(x - y)) / max(1e-300, np.max(np.abs(y))))


@pytest.mark.parametrize("case", list(CASES))
def test_ppo_step_matches_autograd(case):
    cfg, st, nrm, s, a, adv, nlp_old, par, steps = make_case(case)
    alphas = []
    for step in range(steps):
        ref_st = st.copy()
        loss_t, grads_t, ag_t = torch_step(st, cfg, nrm, s, a, adv, nlp_old, par)
        keep = {}
        out = R.ppo_step(st, cfg, nrm, s, a, adv, nlp_old, par, keep)
        # the minibatch exercises every branch: inside the range, zero gradient above and below it
        lo, hi = np.float32(1 - par["eps_ppo"]), np.float32(1 + par["eps_ppo"])
        r, take = keep["r"], keep["take"]
        assert np.sum(take & (r >= lo) & (r <= hi)) >= 3 and np.sum(~take & (r > hi)) >= 1 and np.sum(~take & (r < lo)) >= 1
        assert np.any(keep["ls_un"] < keep["floor"]) and np.any(keep["ls_un"] > keep["floor"])
        assert abs(out["loss"] - loss_t) <= 1e-10 * abs(loss_t)
        assert len(keep["grads"]) == len(grads_t)
        for g, gt in zip(keep["grads"], grads_t):
            assert rel(np.asarray(g).reshape(gt.shape), gt) <= 1e-10
        assert abs(float(keep["alpha_grad"]) - ag_t) <= 1e-10 * abs(ag_t)
        # the clip, both norms and Keras Adam from the autograd gradients
        norm = np.sqrt(sum(np.sum(g * g) for g in grads_t))
        clipped = grads_t
        if par["max_grad_norm"]:
            c = par["max_grad_norm"]
            clipped = [g * (c * min(1 / norm, 1 / c)) for g in grads_t]
            if case in ("pss_1", "ind_raw_adv", "ent_reg"):
                assert norm > c                          # clipping
            else:
                assert norm < c                          # not clipping
        post = np.sqrt(sum(np.sum(g * g) for g in clipped))
        assert abs(out["grad_norm_pre"] - norm) <= 1e-10 * norm and abs(out["grad_norm_post"] - post) <= 1e-10 * post
        if par["max_grad_norm"] is None:
            assert out["grad_norm_pre"] == out["grad_norm_post"]
        for g, gt in zip(keep["clipped"], clipped):
            assert rel(np.asarray(g).reshape(gt.shape), gt) <= 1e-10
        tr = ref_st.trainables(cfg)
        O.adam_step(tr, [np.asarray(g).reshape(w.shape) for g, w in zip(clipped, tr)], ref_st.opt_actor,
                    par["actor_lr"], np.float64)
        for w, wr in zip(st.trainables(cfg), tr):
            assert rel(w, wr) <= 1e-10
        if cfg.per_state_std:
            assert np.array_equal(st.logstd, ref_st.logstd)      # no trainable
        alphas.append(out["alpha"])
    if par["ent_reg"]:
        assert alphas[0] > 0 and alphas[2] > alphas[1] > alphas[0]     # alpha leaves 0 (entropy below its target)
        assert abs(alphas[0] - par["alpha_lr"]) <= 1e-6                # Adam's first step is lr * sign(g)
    else:
        assert alphas == [0.0] * steps


def test_alpha_is_clamped_at_zero():
    cfg, st, nrm, s, a, adv, nlp_old, par, _ = make_case("ent_reg")
    par = {**par, "ent_targ": -50.0}                 # entropy above its target: alpha would go negative
    out = R.ppo_step(st, cfg, nrm, s, a, adv, nlp_old, par)
    assert out["alpha"] == 0.0 and st.opt_alpha.t == 1


def test_fp32_restatement_tracks_fp64():
    cfg, st, nrm, s, a, adv, nlp_old, par, _ = make_case("ind_2")
    st32 = st.astype(np.float32)
    o64 = R.ppo_step(st, cfg, nrm, s, a, adv, nlp_old, par)
    o32 = R.ppo_step(st32, cfg, nrm, s, a, adv, nlp_old.astype(np.float32), par)
    assert st32.actor[0].dtype == np.float32
    assert abs(o32["loss"] - o64["loss"]) <= 1e-4 * abs(o64["loss"])


@pytest.mark.parametrize("n,nmb", [(1000, 32), (64, 32), (10000, 32), (33, 32)])
def test_minibatch_split_matches_reference(n, nmb):
    from sac_eo.algs.model_free import minibatches
    idx = np.arange(n)
    np.random.RandomState(n).shuffle(idx)
    ref = R.split_reference(n, nmb, idx)
    n_batch = int(n / nmb)
    assert all(len(b) == n_batch for b in ref)
    for got in (R.split_minibatches(n, nmb, idx), minibatches(n, nmb, idx)):
        assert got.shape == (len(ref), n_batch)
        assert np.array_equal(got, np.stack(ref))
    if (n, nmb) == (10000, 32):
        assert got.shape == (32, 312)                # the 16-row remainder is dropped


def test_too_few_rows_raise():
    from sac_eo.algs.model_free import minibatches
    with pytest.raises(ValueError):
        R.split_minibatches(5, 32, np.arange(5))
    with pytest.raises(ValueError):
        minibatches(5, 32, np.arange(5))


def test_update_log_and_adaptlr():
    cfg, st, nrm, s, a, adv, _, _, _ = make_case("ind_2")
    kw = dict(actor_lr=3e-3, actor_update_it=2, actor_nminibatch=4, adv_center=True, adv_scale=True, eps_ppo=0.2,
              max_grad_norm=0.5, adaptlr=True, adapt_factor=0.03, adapt_minthresh=0.0, adapt_maxthresh=1.0,
              ent_reg=False, ent_targ=0.0, alpha_lr=0.0)
    rs = np.random.RandomState(1)
    ref = R.PPORef(st, cfg, nrm, kw, rs)
    keep = {}
    log = ref.update(s, a, adv, keep)
    assert sorted(log) == sorted(["ent", "tv", "kl", "alpha", "actor_lr", "outside_clip", "actor_grad_norm_pre",
                                  "actor_grad_norm"])
    assert keep["steps"] == 8 and st.opt_actor.t == 8
    assert log["actor_lr"] == float(np.float32(3e-3))            # the value before adaptation
    want = float(np.float32(float(np.float32(3e-3)) / 1.03)) if log["tv"] > 0.1 else float(np.float32(3e-3))
    assert float(ref.actor_lr) == want
    # the stream advanced by exactly two shuffles of arange(N)
    rs2 = np.random.RandomState(1)
    for _ in range(2):
        rs2.shuffle(np.arange(N))
    assert rs.get_state()[2] == rs2.get_state()[2] and np.array_equal(rs.get_state()[1], rs2.get_state()[1])
