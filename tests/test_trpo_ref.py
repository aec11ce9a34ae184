"""tests/trpo_ref.py pinned on the CPU: its Fisher product (the Gauss-Newton form) against torch's double
backward of the mean KL in fp64 (<= 1e-10 of the tensor's max), ``cg`` against a dense solve, the three
outcomes of the line search by construction, and the flat get / set round trip of ``GaussianActor``
including the logstd floor."""
import numpy as np
import pytest

import ppo_ref as R
import sac_oracle as O
import trpo_ref as T
from helpers import nontrivial_normalizers

torch = pytest.importorskip("torch")


def make(acts=("tanh", "tanh"), hidden=(24, 40), S=3, A=2, per_state_std=False, layer_norm=False, floor=False, seed=3,
         std_mult=1.0, n=37):
    cfg = O.Config(S=S, A=A, hidden=hidden, actor_acts=acts, per_state_std=per_state_std, layer_norm=layer_norm)
    rng = np.random.RandomState(seed + 50)
    logstd = (0.2 * rng.normal(size=A) - 0.3).astype(np.float32)
    if floor:
        logstd[0] = -8.0
    st = R.init_state(cfg, seed=seed, std_mult=std_mult, logstd=logstd, bias_scale=0.1, gain=0.5)
    if floor and per_state_std:
        st.actor[-2][:, A] = 0.0
        st.actor[-1][A] = -8.0
    nrm = nontrivial_normalizers(rng, S, A)
    s = (rng.normal(size=(n, S)) * rng.uniform(0.3, 2.0, S)).astype(np.float32)
    d = R.forward(st, cfg, nrm, s)
    a = (d.mean + np.exp(d.ls) * rng.normal(size=(n, A))).astype(np.float32)
    adv = (rng.normal(size=n) * 1.5 + 0.4).astype(np.float32)
    return cfg, st, nrm, s, a, adv


def torch_forward(P, cfg, nrm, s, std_mult):
    """GaussianActor._forward in torch fp64 on the trainables' list P."""
    dt = torch.float64
    f = {"relu": torch.relu, "tanh": torch.tanh, "elu": torch.nn.functional.elu}
    x = (torch.as_tensor(s, dtype=dt) - torch.as_tensor(nrm.s_mean, dtype=dt)) / torch.as_tensor(nrm.s_den, dtype=dt)
    W = list(P if cfg.per_state_std else P[:-1])
    acts = list(cfg.aacts)
    h = x @ W[0] + W[1]
    if cfg.layer_norm:
        h = (h - h.mean(-1, keepdim=True)) / torch.sqrt(h.var(-1, unbiased=False, keepdim=True) + O.LN_EPS) * W[2] + W[3]
        h = torch.tanh(h)
        W = W[4:]
    else:
        h = f[acts[0]](h)
        W = W[2:]
    for l in range(len(W) // 2):
        h = h @ W[2 * l] + W[2 * l + 1]
        if l < len(W) // 2 - 1:
            h = f[acts[l + 1]](h)
    lsi = float(R.logstd_init(cfg, std_mult))
    if cfg.per_state_std:
        mean, raw = h[:, :cfg.A], h[:, cfg.A:]
        ls = torch.log(torch.nn.functional.softplus(raw)) + lsi
    else:
        mean, ls = h, P[-1].expand(h.shape[0], cfg.A) + lsi
    return mean, torch.maximum(ls, torch.tensor(float(np.log(1e-3)), dtype=dt))


CASES = {
    "relu": dict(acts=("relu", "relu")),
    "tanh": dict(acts=("tanh", "tanh")),
    "elu": dict(acts=("elu", "elu")),
    "mixed3": dict(acts=("relu", "tanh", "elu"), hidden=(24, 40, 20)),
    "layer_norm": dict(acts=("tanh", "relu"), layer_norm=True),
    "per_state_std": dict(acts=("tanh", "elu"), per_state_std=True, std_mult=0.8),
    "floor": dict(acts=("tanh", "tanh"), floor=True),
    "pss_floor": dict(acts=("tanh", "tanh"), per_state_std=True, floor=True),
}


@pytest.mark.parametrize("trust_sub", [1, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fisher_product_is_the_hessian_of_the_mean_kl(case, trust_sub):
    kw = CASES[case]
    cfg, st, nrm, s, _, _ = make(**kw)
    s_sub = s[::trust_sub]
    rng = np.random.RandomState(9)
    like = st.trainables(cfg)
    x = [rng.normal(size=w.shape) for w in like]            # (a non-zero logstd entry among them)
    damp = 0.05
    got = T.fvp(st, cfg, nrm, s_sub, x, damp)
    P = [torch.tensor(np.asarray(w, np.float64), requires_grad=True) for w in like]
    sm = kw.get("std_mult", 1.0)
    m0, l0 = [t.detach() for t in torch_forward(P, cfg, nrm, s_sub, sm)]
    m, l = torch_forward(P, cfg, nrm, s_sub, sm)
    kl = (0.5 * (((m - m0) ** 2 + torch.exp(2 * l0)) / torch.exp(2 * l) + 2 * l - 2 * l0 - 1).sum(-1)).mean()
    gr = torch.autograd.grad(kl, P, create_graph=True)
    assert max(float(g.detach().abs().max()) for g in gr) <= 1e-15     # the first-order factor vanishes at the reference point
    xt = [torch.tensor(v) for v in x]
    hv = torch.autograd.grad(sum((g * v).sum() for g, v in zip(gr, xt)), P, allow_unused=True)
    for i, (g, h, v) in enumerate(zip(got, hv, x)):
        want = (np.zeros_like(v) if h is None else h.numpy()) + damp * v
        err = float(np.max(np.abs(g.reshape(want.shape) - want))) / max(float(np.max(np.abs(want))), 1e-30)
        assert err <= 1e-10, (case, i, err)
    if kw.get("floor") and not cfg.per_state_std:               # a floored column: only the damping is left
        assert abs(got[-1][0, 0] - damp * x[-1][0, 0]) <= 1e-15


def test_surrogate_gradient_against_autograd():
    for case in ("tanh", "layer_norm", "per_state_std", "floor"):
        kw = CASES[case]
        cfg, st, nrm, s, a, adv = make(**kw)
        st.alpha = np.array(0.3)
        nlp_old = R.neglogp(st, cfg, nrm, s, a) + 0.05 * np.random.RandomState(2).normal(size=len(s))
        adv_n = R.normalise_adv(adv, T.DEFAULTS, np.float64)
        g, em, loss = T.surrogate_grad(st, cfg, nrm, s, a, adv_n, nlp_old, ent_targ=-2.0)
        P = [torch.tensor(np.asarray(w, np.float64), requires_grad=True) for w in st.trainables(cfg)]
        m, l = torch_forward(P, cfg, nrm, s, kw.get("std_mult", 1.0))
        at = torch.as_tensor(a, dtype=torch.float64)
        nlp = 0.5 * ((((at - m) / torch.exp(l)) ** 2) + 2 * l + np.log(2 * np.pi)).sum(-1)
        ent = (0.5 * (2 * l + np.log(2 * np.pi) + 1).sum(-1)).mean()
        lt = (torch.exp(torch.as_tensor(nlp_old) - nlp) * torch.as_tensor(adv_n) * -1).mean() - 0.3 * (ent - (-2.0))
        assert abs(float(lt.detach()) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
        for gi, ti in zip(g, torch.autograd.grad(lt, P, allow_unused=True)):
            want = np.zeros_like(gi) if ti is None else ti.numpy().reshape(gi.shape)
            assert np.max(np.abs(gi - want)) <= 1e-10 * max(np.max(np.abs(want)), 1e-30), case


def test_cg_against_a_dense_solve():
    cfg, st, nrm, s, _, _ = make(hidden=(5, 4), A=1, n=64)
    like = st.trainables(cfg)
    nv = sum(w.size for w in like)
    Fx = lambda x: T.to_flat(T.fvp(st, cfg, nrm, s, T.from_flat(like, x), 0.1))
    M = np.stack([Fx(e) for e in np.eye(nv)], 1)
    assert np.max(np.abs(M - M.T)) <= 1e-12 * np.max(np.abs(M)) and np.all(np.linalg.eigvalsh(M) > 0)
    b = np.random.RandomState(1).normal(size=nv)
    keep = {}
    x = T.cg(Fx, b, cg_iters=4 * nv, residual_tol=1e-26, keep=keep)
    want = np.linalg.solve(M, b)
    assert np.max(np.abs(x - want)) <= 1e-8 * np.max(np.abs(want)), keep
    keep = {}
    T.cg(Fx, b, cg_iters=4 * nv, keep=keep)                  # the default break: r.r < 1e-10 ends it early
    assert keep["cg_iters"] < 4 * nv and keep["rdotr"] < 1e-10


def _update(kw, n=60, seed=3, **mk):
    cfg, st, nrm, s, a, adv = make(n=n, seed=seed, **mk)
    ref = T.TRPORef(st.copy(), cfg, nrm, kw)
    keep = {}
    log = ref.update(s, a, adv, keep)
    return ref, log, keep, st


def test_backtrack_accepts_the_full_step():
    ref, log, keep, st0 = _update(dict(delta_trpo=0.01, kl_maxfactor=1.5, trust_damp=0.1, cg_it=10))
    assert log["adj"] == 1.0 and len(keep["trials"]) == 1
    assert 0 < log["kl"] <= keep["kl_max"] and log["improve"] >= 0 and log["kl"] == log["kl_pre"] and log["tv"] == log["tv_pre"]
    assert sorted(log) == sorted(T.LOG_KEYS)
    assert any(np.max(np.abs(x - y)) > 0 for x, y in zip(ref.st.trainables(ref.cfg), st0.trainables(ref.cfg)))


def test_backtrack_shrinks_k_times():
    # kl scales with the square of the step: kl_maxfactor = 0.3 needs the step halved once (two shrinks)
    ref, log, keep, _ = _update(dict(delta_trpo=0.01, kl_maxfactor=0.3, trust_damp=0.1, cg_it=10))
    k = len(keep["trials"]) - 1
    assert k >= 1 and log["adj"] == pytest.approx(2.0 ** (-k / 2), rel=1e-12)
    for kl, imp in keep["trials"][:-1]:
        assert kl > keep["kl_max"] or imp < 0
    assert log["kl"] <= keep["kl_max"] and log["improve"] >= 0 and log["kl"] < log["kl_pre"]


def test_backtrack_gives_up_and_restores():
    # kl only halves per shrink: 2^-10 of kl_pre stays above 1e-6 * delta, so all ten trials fail
    ref, log, keep, st0 = _update(dict(delta_trpo=0.01, kl_maxfactor=1e-6, trust_damp=0.1, cg_it=10))
    assert log["adj"] == 0.0 and len(keep["trials"]) == 10
    assert log["kl"] == 0.0 and log["improve"] == 0.0 and log["tv"] == 0.0 and log["kl_pre"] > 0
    for x, y in zip(ref.st.trainables(ref.cfg), st0.trainables(ref.cfg)):
        assert np.array_equal(x, y)


def test_zero_steps():
    for kw, mk in ((dict(delta_trpo=0.0), {}), (dict(delta_trpo=0.01, adv_center=False), dict())):
        cfg, st, nrm, s, a, adv = make(n=40)
        if kw["delta_trpo"]:
            adv = np.zeros_like(adv)
        ref = T.TRPORef(st.copy(), cfg, nrm, kw)
        keep = {}
        log = ref.update(s, a, adv, keep)
        assert keep["zero"] and log["adj"] == 1.0 and log["kl"] == 0.0 and log["improve"] == 0.0
        for x, y in zip(ref.st.trainables(cfg), st.trainables(cfg)):
            assert np.array_equal(x, y)


class _Box:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, np.float32), np.ones(n, np.float32)


class _Env:
    observation_space, action_space = _Box(3), _Box(2)


def test_flat_get_set_round_trip_and_the_logstd_floor():
    from sac_eo.actors.continuous_actors import GaussianActor
    for ln in (False, True):
        actor = GaussianActor(_Env(), [24, 40], ["tanh"], 0.01, "orthogonal", ln, rng=np.random.default_rng(0))
        w = actor.get_weights()
        flat = actor.get_weights(flat=True)
        assert flat.ndim == 1 and flat.size == sum(x.size for x in w)
        assert np.array_equal(flat, np.concatenate([x.reshape(-1) for x in w]))
        rng = np.random.RandomState(0)
        new = rng.normal(size=flat.size).astype(np.float32)
        new[-2:] = (-0.5, -9.0)                              # logstd: one entry below log 1e-3
        actor.set_weights(new, from_flat=True)
        got = actor.get_weights(flat=True)
        assert np.array_equal(got[:-1], new[:-1]) and got[-1] == np.float32(np.log(1e-3))
        inc = rng.normal(size=flat.size).astype(np.float32) * 0.1
        inc[-1] = -1.0                                       # stays at the floor
        actor.set_weights(inc, from_flat=True, increment=True)
        got2 = actor.get_weights(flat=True)
        assert np.array_equal(got2[:-1], (got[:-1] + inc[:-1]).astype(np.float32)) and got2[-1] == np.float32(np.log(1e-3))
        # the plain call keeps what it is given (today's behaviour), shapes as the list's
        lst = actor.get_weights()
        lst[-1] = np.full((1, 2), -9.0, np.float32)
        actor.set_weights(lst)
        assert np.array_equal(actor.get_weights()[-1], lst[-1])
        assert [x.shape for x in actor.get_weights()] == [x.shape for x in w]
    pss = GaussianActor(_Env(), [24, 40], ["tanh"], 0.01, "orthogonal", False, per_state_std=True,
                        rng=np.random.default_rng(0))
    f = pss.get_weights(flat=True)
    assert f.size == sum(x.size for x in pss.get_weights()) == 3 * 24 + 24 + 24 * 40 + 40 + 40 * 4 + 4
    pss.set_weights(f * 2, from_flat=True)
    assert np.array_equal(pss.get_weights(flat=True), f * 2)
    with pytest.raises(ValueError):
        pss.set_weights(f[:-1], from_flat=True)
