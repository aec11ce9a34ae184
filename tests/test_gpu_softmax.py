"""SoftMaxActor on the trainable handle (``EngineConfig(softmax=True)``, ``sacx_softmax_init``) on the device
against tests/softmax_ref.py.

* the row functions (neglogp, the raw logits, entropy, kl) at 2e-5 -- absolute for tensors up to 1 in
  magnitude, of the tensor's largest entry above: n in {1, 5, 313} x A in {1, 2, 3, 17, 32} (A = 1 gives exact
  zeros), S 3 and 17, a layer-norm, a three-layer and a 520-wide net, logits of about +-80 (no inf / NaN), an
  action index outside [0, A) (neglogp 0);
* one PPO minibatch step (mb 16 / 17 / 33, A 2 / 3 / 17, every option on and off) at the bars DESIGN 6.10
  records for the Gaussian step: loss, both norms and alpha 2e-5, gradients (through Adam's first moment) 2e-4,
  weights after Adam 1e-6; ``actor.logstd`` and its moments stay untouched;
* ``PPO.update`` end to end (n = 200, 4 minibatches, 3 iterations, two updates): the host stream bit for bit,
  ``outside_clip`` exact, the other figures by the rule of tests/test_gpu_ppo.py's end-to-end test (the larger
  of the single-step bar and the restatement's fp32 envelope under ``sac_oracle.MATMUL_ORDERS``);
* TRPO: gradient and Fisher product (n 33 and 4,097, A 3) at 2e-4, the whole step by tests/test_gpu_trpo.py's
  rule, a degenerate solve (vFv not positive) refused with the weights untouched;
* graph replay == eager bit for bit, launch counts against a Gaussian handle, ``sample`` and the stream.
"""
import numpy as np
import pytest

import ppo_ref as R
import sac_oracle as O
import softmax_ref as SM
import trpo_ref as T
from helpers import nontrivial_normalizers, relerr
from test_gpu_ppo import _layer_grads, _moment, _pargs, _state_bytes
from test_gpu_trpo import par_of

pytestmark = pytest.mark.gpu

NETS = {
    "h64": dict(hidden=(64, 64), acts=("tanh", "tanh")),
    "ln": dict(hidden=(64, 48), acts=("tanh", "relu"), layer_norm=True),
    "three": dict(hidden=(32, 48, 40), acts=("relu", "tanh", "elu")),
    "wide1": dict(hidden=(520,), acts=("tanh",)),
    "odd": dict(hidden=(23, 41), acts=("tanh", "elu")),      # widths off the 4-grid
}


def make_state(net, S, A, seed, span=None):
    """(oracle cfg, fp64 state holding f32 values, normaliser); span: the last layer scaled so that the
    logits of `probe` rows span about +-span."""
    c = NETS[net]
    cfg = O.Config(S=S, A=A, hidden=c["hidden"], actor_acts=c["acts"], layer_norm=c.get("layer_norm", False))
    st = SM.init_state(cfg, seed=seed, bias_scale=0.1, gain=0.5)
    nrm = nontrivial_normalizers(np.random.RandomState(seed + 50), S, A)
    if span is not None:
        s = states(S, 64, seed)
        lg = SM.forward(st, cfg, nrm, s)[0]
        k = np.float32(span / np.abs(lg - lg.mean(-1, keepdims=True)).max())
        st.actor[-2] = np.asarray(np.asarray(st.actor[-2] * k, np.float32), np.float64)
        st.actor[-1] = np.asarray(np.asarray(st.actor[-1] * k, np.float32), np.float64)
    return cfg, st, nrm


def states(S, n, seed):
    rng = np.random.RandomState(seed + 900)
    return (rng.normal(size=(n, S)) * rng.uniform(0.3, 2.0, S)).astype(np.float32)


def rollout(cfg, st, nrm, n, seed):
    """On-policy rows: s, a ~ pi(s) (the Gumbel argmax on the state's logits), adv."""
    s = states(cfg.S, n, seed)
    rng = np.random.RandomState(seed + 901)
    lg = SM.forward(st, cfg, nrm, s)[0]
    a = np.argmax(lg - np.log(-np.log(rng.random_sample(size=lg.shape))), -1).astype(np.float32)
    adv = (rng.normal(size=n) * 1.5 + 0.4).astype(np.float32)
    return s, a, adv


def moved(st, seed, scale):
    rng = np.random.RandomState(seed + 1700)
    new = st.copy()
    for w in new.actor:
        w += (scale * rng.normal(size=w.shape)).astype(np.float32)
    new.actor = [np.asarray(np.asarray(w, np.float32), np.float64) for w in new.actor]
    return new


def make_engine(net, S, A, batch, capacity, **kw):
    from sac_eo.engine import Engine, EngineConfig
    c = NETS[net]
    return Engine(EngineConfig(s_dim=S, a_dim=A, hidden=c["hidden"], actor_activations=c["acts"], batch=batch,
                               buffer_capacity=capacity, actor_gaussian="train", actor_layer_norm=c.get("layer_norm", False),
                               graph_steps=1, softmax=kw.pop("softmax", True), **kw))


def load(eng, st, nrm):
    eng.set_net("actor", [np.asarray(w, np.float32) for w in st.actor])
    eng.set_normalizers(nrm.s_mean, nrm.s_den, nrm.a_mean, nrm.a_den)


def bar_err(got, want):
    """The row-function bar's error: absolute for a tensor up to 1 in magnitude, relative to its max above."""
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / max(1.0, float(np.max(np.abs(want)))))


# ---------------------------------------------------------------------------------------------- rows
ROWS = [("h64", (3, 17)[(i + j) % 2], A, n, None) for i, n in enumerate((1, 5, 313)) for j, A in enumerate((1, 2, 3, 17, 32))]
ROWS += [("ln", 7, 3, 33, None), ("three", 7, 3, 33, None), ("wide1", 7, 3, 33, None), ("h64", 17, 17, 33, 80.0),
         ("odd", 7, 3, 33, None)]


@pytest.mark.parametrize("net,S,A,n,span", ROWS)
def test_row_functions(gpu_available, net, S, A, n, span):
    import torch
    cfg, st, nrm = make_state(net, S, A, seed=2, span=span)
    eng = make_engine(net, S, A, batch=16, capacity=max(n, 16))
    load(eng, st, nrm)
    s, a, _ = rollout(cfg, st, nrm, n, seed=4)
    lg = SM.forward(st, cfg, nrm, s)[0]
    if span is not None:
        a = (np.arange(n) % A).astype(np.float32)           # labels off the arg max too: neglogp up to the span
        assert np.ptp(lg, -1).max() > 1.5 * span and SM.neglogp_of(lg, a).max() > span      # the premise
    logits, none, ent = eng.dist(s)
    assert none is None and logits.shape == (n, A)
    logits, ent = logits.cpu().numpy(), ent.cpu().numpy()
    nlp = eng.neglogp(s, a).cpu().numpy()
    errs = dict(logits=bar_err(logits, lg), ent=bar_err(ent, SM.entropy_of(lg)), nlp=bar_err(nlp, SM.neglogp_of(lg, a)))
    # an index outside [0, A): CUDA rows go through as they are; NumPy rows are range-checked on the host
    bad = a.copy()
    bad[0], bad[-1] = A, -1.0
    with pytest.raises(ValueError, match="action indices"):
        eng.neglogp(s, bad)
    nlp_bad = eng.neglogp(s, torch.as_tensor(bad).cuda()).cpu().numpy()
    assert nlp_bad[0] == 0 and nlp_bad[-1] == 0 and np.array_equal(nlp_bad[1:-1], nlp[1:-1])
    # kl of the moved policy against this one's logits
    st2 = moved(st, 5, 0.02 if span is None else 0.002)
    load(eng, st2, nrm)
    kl = eng.kl(s, lg.astype(np.float32), None).cpu().numpy()
    klr = SM.kl_of(SM.forward(st2, cfg, nrm, s)[0], lg.astype(np.float32))
    errs["kl"] = bar_err(kl, klr)
    print(f"{net} S={S} A={A} n={n} span={span}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for x in (logits, ent, nlp, kl):
        assert np.all(np.isfinite(x))
    if A == 1:
        assert not nlp.any() and not ent.any() and not kl.any()
    else:
        assert np.all(klr > 0) if span is None else (klr.max() > 1e-2 and klr.min() > -1e-12)
    assert max(errs.values()) < 2e-5, errs
    eng.close()


# ---------------------------------------------------------------------------------------------- one step
STEP_CASES = {
    # name: S, A, minibatch rows, table rows, parameters, weight move
    "a2_16": dict(S=3, A=2, mb=16, n=16, par=dict(max_grad_norm=0.5), move=0.2, seed=3),
    "a3_17_bad_index": dict(S=17, A=3, mb=17, n=40, par=dict(max_grad_norm=None, adv_center=False), move=0.1, seed=1, bad=True),
    "a17_33": dict(S=17, A=17, mb=33, n=50, par=dict(max_grad_norm=0.05, adv_scale=False), move=0.1, seed=1),
    "a3_33_plain": dict(S=3, A=3, mb=33, n=50, par=dict(max_grad_norm=None, adv_center=False, adv_scale=False), move=0.1, seed=1),
    "ent_reg": dict(S=17, A=3, mb=33, n=64, par=dict(max_grad_norm=0.5, ent_reg=True, alpha_lr=0.02, ent_targ=2.0), move=0.1,
                    seed=1, steps=3),
    "odd_17": dict(S=17, A=3, mb=17, n=40, net="odd", par=dict(max_grad_norm=None), move=0.2, seed=1),
}
_STEP_CACHE = {}


def step_case(name):
    """Everything of a step case the CPU decides, once: states, rows, indices, the restatement's results and
    the premise (asserted here, from the fp64 restatement)."""
    if name in _STEP_CACHE:
        return _STEP_CACHE[name]
    c = STEP_CASES[name]
    cfg, st0, nrm = make_state(c.get("net", "h64"), c["S"], c["A"], c["seed"])
    s, a, adv = rollout(cfg, st0, nrm, c["n"], c["seed"])
    st = moved(st0, c["seed"], c["move"])
    rng = np.random.RandomState(c["seed"] + 31)
    steps = c.get("steps", 1)
    idx = np.stack([rng.permutation(c["n"])[:c["mb"]] for _ in range(steps)]).astype(np.int32)
    if c.get("bad"):
        a[idx[0][0]] = c["A"] + 4                         # tf.one_hot's all-zero row inside the minibatch
    par = {**R.DEFAULTS, "actor_lr": 1e-4, **c["par"]}
    nlp_old = SM.neglogp(st0, cfg, nrm, s, a)
    ref, keeps, outs = st.copy(), [], []
    lo, hi = np.float32(1 - par["eps_ppo"]), np.float32(1 + par["eps_ppo"])
    for k in range(steps):
        keep = {}
        b = idx[k]
        outs.append(SM.ppo_step(ref, cfg, nrm, s[b], a[b], adv[b], nlp_old[b], par, keep))
        r, take = keep["r"], keep["take"]
        inside, above, below = take & (r >= lo) & (r <= hi), ~take & (r > hi), ~take & (r < lo)
        assert inside.sum() >= 2 and above.sum() >= 2 and below.sum() >= 2, (name, inside.sum(), above.sum(), below.sum())
        assert np.min(np.abs(r - lo)) >= 1e-4 and np.min(np.abs(r - hi)) >= 1e-4, name
        assert abs(outs[-1]["loss"]) >= 0.05, (name, outs[-1]["loss"])      # (a relative bar on a mean of signed terms)
        if par["max_grad_norm"]:
            assert outs[-1]["grad_norm_pre"] > par["max_grad_norm"], (name, outs[-1])      # the clip acts
        keeps.append(keep)
    _STEP_CACHE[name] = dict(c=c, cfg=cfg, st0=st0, st=st, nrm=nrm, s=s, a=a, adv=adv, idx=idx, par=par, ref=ref, outs=outs,
                             keeps=keeps, steps=steps)
    return _STEP_CACHE[name]


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_premise_of_the_step_cases_on_the_cpu(case):
    step_case(case)


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_one_minibatch_step(gpu_available, case):
    import torch
    k = step_case(case)
    c, cfg, par = k["c"], k["cfg"], k["par"]
    eng = make_engine(c.get("net", "h64"), c["S"], c["A"], batch=c["mb"], capacity=c["n"])
    load(eng, k["st0"], k["nrm"])
    eng.set_logstd(np.full((1, c["A"]), 0.25, np.float32))      # no trainable here: it must come back as it is
    eng.v["grad"].fill_(3.0)                        # a reused arena: ppo_begin clears the gradient words it reads
    rows = (k["s"], k["a"], k["adv"])
    if c.get("bad"):
        rows = tuple(torch.as_tensor(x).cuda() for x in rows)
    eng.ppo_begin(*rows)
    load(eng, k["st"], k["nrm"])                    # the policy moved since the rollout
    for j in range(k["steps"]):
        eng.ppo_steps(k["idx"][j:j + 1], **_pargs(par))
        eng.sync()
        row, o = eng.ppo_stats(1)[0], k["outs"][j]
        print(f"{case} step {j}: loss {row[0]:.6g} vs {o['loss']:.6g}, ent {row[1]:.6g} vs {o['ent']:.6g}, norms {row[2]:.6g} / "
              f"{row[3]:.6g} vs {o['grad_norm_pre']:.6g} / {o['grad_norm_post']:.6g}, alpha {row[4]:.6g} vs {o['alpha']:.6g}")
        assert abs(row[0] - o["loss"]) <= 2e-5 * abs(o["loss"]), (row[0], o["loss"])
        assert abs(row[1] - o["ent"]) <= 2e-5 * abs(o["ent"])
        assert abs(row[2] - o["grad_norm_pre"]) <= 2e-5 * o["grad_norm_pre"]
        assert abs(row[3] - o["grad_norm_post"]) <= 2e-5 * o["grad_norm_post"]
        assert abs(row[4] - o["alpha"]) <= 2e-5 * abs(o["alpha"]) and row[7] == j + 1
        if par["max_grad_norm"] is None:
            assert row[2] == row[3]
        if j == 0:                                  # gradients (clipped), through Adam's first moment
            ga, go = _layer_grads(eng), list(k["keeps"][0]["clipped"])
            assert len(ga) == len(go)
            for i, (gd, gr) in enumerate(zip(ga, go)):
                print(f"{case}: gradient {i} {gr.shape} error {relerr(gd, gr):.2e}")
                assert relerr(gd, gr) < 2e-4, ("actor", i, relerr(gd, gr))
    werr = max(float(np.max(np.abs(x - y))) for x, y in zip(eng.get_net("actor"), k["ref"].actor))
    print(f"{case}: weights after Adam max abs error {werr:.2e}")
    assert werr < 1e-6
    assert np.all(eng.v["actor.logstd"].cpu().numpy() == np.float32(0.25)) and not _moment(eng, "actor.logstd").any()
    if par["ent_reg"]:
        assert k["outs"][-1]["alpha"] > k["outs"][0]["alpha"] > 0       # alpha left 0
    ctl = eng.v["ppo.ctl"][0].cpu().numpy()
    assert ctl[0] == ctl[1] == ctl[3] == k["steps"] and ctl[2] == (k["steps"] if par["ent_reg"] else 0)
    eng.close()


# ---------------------------------------------------------------------------------------------- PPO.update
class _Obs:
    def __init__(self, n):
        self.shape = (n,)


class _Discrete:
    def __init__(self, n):
        self.n, self.shape = n, ()


class _Env:
    def __init__(self, S, A):
        self.observation_space, self.action_space = _Obs(S), _Discrete(A)


UPD_KW = dict(actor_lr=3e-4, actor_update_it=3, actor_nminibatch=4, adv_center=True, adv_scale=True, eps_ppo=0.2,
              max_grad_norm=0.5, adaptlr=True, adapt_factor=0.03, adapt_minthresh=0.7, adapt_maxthresh=1.0, ent_reg=True,
              ent_targ=3.0, alpha_lr=1e-3)         # (the entropy of 6 actions is below 3: alpha grows from 0)
LOG_KEYS = ("ent", "tv", "kl", "alpha", "actor_lr", "outside_clip", "actor_grad_norm_pre", "actor_grad_norm")
_UPD_CACHE = {}


class _Rms:
    def __init__(self, mean, den):
        self.mean, self._den = mean, den

    def den(self):
        return self._den


def update_case(seed=3, n=200):
    """The actor, the rollouts and the restatement's runs (fp64, and fp32 under every summation order), once."""
    if "case" in _UPD_CACHE:
        return _UPD_CACHE["case"]
    from sac_eo.actors.discrete_actors import SoftMaxActor
    S, A = 17, 6
    actor = SoftMaxActor(_Env(S, A), [64, 64], ["tanh"], 0.5, rng=np.random.default_rng(seed))
    cfg = O.Config(S=S, A=A, hidden=(64, 64), actor_acts=("tanh", "tanh"))
    w0 = actor.get_weights()
    st = SM.state_of(w0, np.float32)
    nrm = nontrivial_normalizers(np.random.RandomState(seed), S, A)
    data = [rollout(cfg, st.astype(np.float64), nrm, n, seed + 10 * u) for u in range(2)]
    refs = {}
    for key in ("f64",) + tuple(O.MATMUL_ORDERS):
        rs = np.random.RandomState(11)
        ref = SM.PPORef(st.astype(np.float64 if key == "f64" else np.float32), cfg, nrm, UPD_KW, rs)
        logs, keeps = [], []
        O.MATMUL_ORDER = "default" if key == "f64" else key
        try:
            for (s, a, adv) in data:
                keep = {}
                logs.append(ref.update(s, a, adv, keep))
                keeps.append((keep, rs.get_state()))
        finally:
            O.MATMUL_ORDER = "default"
        refs[key] = (ref, logs, keeps)
    ref, logs, keeps = refs["f64"]
    assert float(ref.actor_lr) != float(np.float32(UPD_KW["actor_lr"]))     # the rate adapts
    for keep, _ in keeps:                                # no row near the boundary of outside_clip
        assert np.min(np.abs(keep["rdiff"] - np.float32(UPD_KW["eps_ppo"]))) >= 1e-4
        assert keep["steps"] == 12
    _UPD_CACHE["case"] = (actor, w0, cfg, nrm, data, refs)
    return _UPD_CACHE["case"]


def test_premise_of_the_end_to_end_update_on_the_cpu():
    actor, w0, cfg, nrm, data, refs = update_case()
    for u in range(2):
        for key in LOG_KEYS:
            l64 = refs["f64"][1][u]
            env = max(abs(refs[o][1][u][key] - l64[key]) for o in O.MATMUL_ORDERS) / max(abs(l64[key]), 1e-30)
            assert env < 1e-2, (u, key, env)


def test_ppo_update_end_to_end(gpu_available):
    from sac_eo.algs.model_free import PPO
    actor, w0, cfg, nrm, data, refs = update_case()
    actor.set_weights(w0)
    ref, logs, keeps = refs["f64"]
    actor.s_rms = _Rms(nrm.s_mean, nrm.s_den)
    np.random.seed(0)
    np.random.set_state(np.random.RandomState(11).get_state())
    ppo = PPO(actor, UPD_KW)
    figures = []                                         # (what, device error, fp32 envelope, single-step bar)
    for u, (s, a, adv) in enumerate(data):
        log = ppo.update((s, a, adv, None, None, None))
        assert sorted(log) == sorted(LOG_KEYS) and ppo.engine.cfg.softmax
        dev, want = ppo.engine.rng_get_state(), keeps[u][1]
        assert np.array_equal(dev[1], want[1]) and dev[2] == want[2]         # the host stream, bit for bit
        l64 = logs[u]
        assert log["outside_clip"] == l64["outside_clip"]
        assert float(log["actor_lr"]) == l64["actor_lr"]
        for key in LOG_KEYS:
            env = max(abs(refs[o][1][u][key] - l64[key]) for o in O.MATMUL_ORDERS) / max(abs(l64[key]), 1e-30)
            err = abs(float(log[key]) - l64[key]) / max(abs(l64[key]), 1e-30)
            print(f"update {u} {key}: device {float(log[key]):.7g} ref {l64[key]:.7g} error {err:.2e} fp32 envelope {env:.2e}")
            figures.append((f"update {u} {key}", err, env, 2e-5))
        assert np.array_equal(ppo.engine.ppo_stats(12)[:, 7], 12 * u + np.arange(1, 13, dtype=np.float32))
    assert float(ppo.actor_lr) == float(ref.actor_lr) and ppo.engine.v["ppo.ctl"][0, 1].item() == 24
    assert float(ppo.alpha) > 0
    for i, (x, y) in enumerate(zip(actor.get_weights(), ref.st.actor)):
        env = max(float(np.max(np.abs(np.asarray(refs[o][0].st.actor[i], np.float64) - y))) for o in O.MATMUL_ORDERS)
        err = float(np.max(np.abs(np.asarray(x, np.float64).reshape(y.shape) - y)))
        print(f"final weights {y.shape}: device error {err:.2e} fp32 envelope {env:.2e}")
        figures.append((f"final weights {i}", err, env, 1e-6))
    for what, err, env, bar in figures:                  # every figure is printed before the first assertion
        assert env < 1e-2, (what, env)
        assert err <= max(bar, env), (what, err, env)
    ppo.engine.close()


# ---------------------------------------------------------------------------------------------- TRPO
TS, TA, THID = 3, 3, "tr"
NETS[THID] = dict(hidden=(24, 40), acts=("tanh", "tanh"))
CHUNK = 4096


@pytest.mark.parametrize("n,net,sub", [pytest.param(33, THID, 1, id="33"), pytest.param(CHUNK + 1, THID, 1, id=str(CHUNK + 1)),
                                       pytest.param(100, "odd", 3, id="odd-100-3")])
def test_trpo_gradient_and_fisher_product(gpu_available, n, net, sub):
    import torch
    cfg, st, nrm = make_state(net, TS, TA, seed=2)
    s, a, adv = rollout(cfg, st, nrm, n, seed=4)
    kw = dict(trust_sub=sub, trust_damp=0.05, ent_targ=0.5)
    eng = make_engine(net, TS, TA, batch=16, capacity=n, trpo=True)
    load(eng, st, nrm)
    eng.v["ppo.alpha"][0, 0] = 0.3                       # the entropy term takes part
    st.alpha = np.array(np.float64(np.float32(0.3)))
    assert eng.trpo_begin(s, a, adv, **par_of(kw)) == n
    got_g = eng.trpo_grad()
    assert eng.trpo_flat_len() == (eng.segments["actor.logstd"]["offset"] - eng.segments["actor.l0"]["offset"]) // 4
    nlp_old = SM.neglogp(st, cfg, nrm, s, a)
    adv_n = R.normalise_adv(adv, {**T.DEFAULTS, **kw}, np.float64)
    neg_pg, _, _ = SM.surrogate_grad(st, cfg, nrm, s, a, adv_n, nlp_old, kw["ent_targ"])
    rng = np.random.RandomState(7)
    x = [rng.normal(size=w.shape).astype(np.float32) for w in st.actor]
    got_f = eng.trpo_fvp(x)
    want_f = SM.fvp(st, cfg, nrm, s[::sub], [np.asarray(v, np.float64) for v in x], kw["trust_damp"])
    assert len(got_g) == len(got_f) == len(neg_pg) == 6
    errs = []
    for i, (g, f, ng, wf) in enumerate(zip(got_g, got_f, neg_pg, want_f)):
        eg = float(np.max(np.abs(g.reshape(ng.shape) + ng))) / max(float(np.max(np.abs(ng))), 1e-30)
        ef = float(np.max(np.abs(f.reshape(wf.shape) - wf))) / max(float(np.max(np.abs(wf))), 1e-30)
        print(f"n={n} tensor {i} {ng.shape}: gradient {eg:.2e} (max {np.max(np.abs(ng)):.3g}) "
              f"fisher product {ef:.2e} (max {np.max(np.abs(wf)):.3g})")
        errs.append((eg, ef))
    xf = eng.trpo_pack(x)
    f0, f1 = eng.trpo_fvp(xf), eng.trpo_fvp(xf, eager=True)
    plan = eng.trpo_plan_info((n + sub - 1) // sub)
    chunks = ((n + sub - 1) // sub + CHUNK - 1) // CHUNK
    assert max(e[0] for e in errs) < 2e-4 and max(e[1] for e in errs) < 2e-4, errs
    assert torch.equal(f0, f1)
    assert [p["name"] for p in plan].count("trpo.acc") == chunks
    eng.close()


TRPO_UPDATES = {
    "n33": dict(n=33, kw=dict(delta_trpo=0.01, kl_maxfactor=1.5, trust_damp=0.5, cg_it=20)),
    "chunk_plus_one": dict(n=CHUNK + 1, kw=dict(delta_trpo=0.01, kl_maxfactor=1.5, trust_damp=0.5, cg_it=20, ent_reg=True,
                                                 alpha_lr=0.02, ent_targ=2.0), alpha0=0.2),
}
FP32_RUNS = tuple(O.MATMUL_ORDERS) + tuple(o + "+dots64" for o in O.MATMUL_ORDERS)
_TR_CACHE = {}


def trpo_case(name):
    """As tests/test_gpu_trpo.py's update_case: the fp64 restatement, its fp32 runs, and the premise (every
    line-search decision and the CG break have margin; CG has converged)."""
    if name in _TR_CACHE:
        return _TR_CACHE[name]
    c = TRPO_UPDATES[name]
    cfg, st, nrm = make_state(THID, TS, TA, seed=3)
    st.alpha = np.array(np.float64(np.float32(c.get("alpha0", 0.0))))
    s, a, adv = rollout(cfg, st, nrm, c["n"], seed=5)
    runs = {}
    for key in ("f64",) + FP32_RUNS:
        ref = SM.TRPORef(st.astype(np.float64 if key == "f64" else np.float32), cfg, nrm, c["kw"], dots64=key.endswith("+dots64"))
        O.MATMUL_ORDER = "default" if key == "f64" else key.split("+")[0]
        try:
            keep = {}
            log = ref.update(s, a, adv, keep)
        finally:
            O.MATMUL_ORDER = "default"
        runs[key] = (ref, log, keep)
    ref, log, keep = runs["f64"]
    kw = {**T.DEFAULTS, **c["kw"]}
    adv2 = R.normalise_adv(R.normalise_adv(adv, kw, np.float64), kw, np.float64)
    scale = float(np.mean(np.abs(adv2)))
    kl_max = keep["kl_max"]
    for t, (kl, imp) in enumerate(keep["trials"]):
        if kl > kl_max:
            assert kl - kl_max >= 100 * 2e-5 * kl, (name, t, kl, kl_max)
        else:
            assert kl_max - kl >= 100 * 2e-5 * kl_max and abs(imp) >= 100 * 2e-5 * scale, (name, t, kl, imp)
    hist = keep["rr_hist"]
    assert keep["rdotr"] <= 1e-6 * hist[0], (name, keep["rdotr"], hist[0])
    assert all(rr >= 1e-9 or rr <= 1e-11 for rr in hist[1:]), (name, hist)
    for key in FP32_RUNS:
        assert runs[key][1]["adj"] == log["adj"], (name, key)
    assert log["adj"] > 0 and not keep["zero"], (name, log)
    _TR_CACHE[name] = (cfg, st, nrm, s, a, adv, runs, scale)
    return _TR_CACHE[name]


def _rel(key, val, l64, scale):
    floor = dict(tv=abs(l64["tv_pre"]), kl=abs(l64["kl_pre"]), improve=scale).get(key, 0.0)
    return abs(val - l64[key]) / max(abs(l64[key]), floor, 1e-30)


def trpo_envelope(name):
    cfg, st, nrm, s, a, adv, runs, scale = trpo_case(name)
    r64, l64, _ = runs["f64"]
    out = [(key, max(_rel(key, runs[o][1][key], l64, scale) for o in FP32_RUNS), 2e-5) for key in T.LOG_KEYS]
    for i, y in enumerate(r64.st.actor):
        env = max(float(np.max(np.abs(np.asarray(runs[o][0].st.actor[i], np.float64) - y))) for o in FP32_RUNS)
        out.append((f"final weights {i}", env, 1e-6))
    return out


@pytest.mark.parametrize("name", sorted(TRPO_UPDATES))
def test_premise_of_the_trpo_updates_on_the_cpu(name):
    for fig, env, _ in trpo_envelope(name):
        assert env < 1e-2, (name, fig, env)


@pytest.mark.parametrize("name", sorted(TRPO_UPDATES))
def test_trpo_step(gpu_available, name):
    c = TRPO_UPDATES[name]
    cfg, st, nrm, s, a, adv, runs, scale = trpo_case(name)
    r64, l64, k64 = runs["f64"]
    envs = trpo_envelope(name)
    eng = make_engine(THID, TS, TA, batch=16, capacity=c["n"], trpo=True)
    load(eng, st, nrm)
    eng.v["ppo.alpha"][0, 0] = float(np.float32(c.get("alpha0", 0.0)))
    par = par_of(c["kw"])
    eng.trpo_begin(s, a, adv, **par)
    log = eng.trpo_step(**par)
    info = eng.trpo_solve_info()
    print(f"{name}: device vFv {info['vFv']:.6g} eta {info['eta']:.6g} cg iterations {info['cg_iters']} | "
          f"restatement vFv {k64['vFv']:.6g} eta {k64['eta']:.6g} cg iterations {k64['cg_iters']}")
    assert sorted(log) == sorted(T.LOG_KEYS)
    after = eng.get_net("actor")
    figures = []
    for (key, env, bar) in envs[:len(T.LOG_KEYS)]:
        err = _rel(key, float(log[key]), l64, scale)
        print(f"{name} {key}: device {float(log[key]):.7g} ref {l64[key]:.7g} error {err:.2e} fp32 envelope {env:.2e}")
        figures.append((key, err, env, bar))
    for (what, env, bar), x, y in zip(envs[len(T.LOG_KEYS):], after, r64.st.actor):
        err = float(np.max(np.abs(np.asarray(x, np.float64).reshape(y.shape) - y)))
        print(f"{name} {what} {y.shape}: device error {err:.2e} fp32 envelope {env:.2e}")
        figures.append((what, err, env, bar))
    assert float(log["adj"]) == pytest.approx(l64["adj"], rel=1e-12, abs=0)
    for what, err, env, bar in figures:                    # (every figure is printed before the first assertion)
        assert env < 1e-2, (what, env)
        assert err <= max(bar, env), (what, err, env)
    assert any(not np.array_equal(x, np.asarray(y, np.float32).reshape(x.shape)) for x, y in zip(after, st.actor))
    if c["kw"].get("ent_reg"):
        assert float(log["alpha"]) != float(np.float32(c["alpha0"])) and int(eng.v["ppo.ctl"][0, 2].item()) == 1
    eng.close()


def test_trpo_degenerate_solve_is_refused_and_the_weights_stay(gpu_available):
    """Logit 0 a thousand above the others: every p is exactly one-hot in fp32, M = diag(p) - p p^T is 0 on
    every row, and without damping the Fisher product is 0: vFv is not positive."""
    from sac_eo import _native as N
    cfg, st, nrm = make_state(THID, TS, TA, seed=2)
    st.actor[-1][0] += 1000.0
    s, _, adv = rollout(cfg, st, nrm, 33, seed=4)
    a = (np.arange(33) % TA).astype(np.float32)           # labels off the arg max too: a gradient that is not 0
    eng = make_engine(THID, TS, TA, batch=16, capacity=33, trpo=True)
    load(eng, st, nrm)
    par = par_of(dict(delta_trpo=0.01, trust_damp=0.0, cg_it=3))
    eng.trpo_begin(s, a, adv, **par)
    eng.sync()
    before = [w.copy() for w in eng.get_net("actor")]
    assert not any(np.any(f) for f in eng.trpo_fvp([np.ones_like(w) for w in before]))
    with pytest.raises(N.SacxError, match="degenerate"):
        eng.trpo_step(**par)
    assert all(np.array_equal(x, y) for x, y in zip(eng.get_net("actor"), before))
    eng.close()


# ---------------------------------------------------------------------------------------------- forms
def test_graph_replay_equals_eager_bit_for_bit(gpu_available):
    S, A, mb, steps, n = 17, 3, 17, 5, 40
    cfg, st0, nrm = make_state("h64", S, A, 1)
    s, a, adv = rollout(cfg, st0, nrm, n, 1)
    st = moved(st0, 1, 0.1)
    idx = np.stack([np.random.RandomState(5 + j).permutation(n)[:mb] for j in range(steps)]).astype(np.int32)
    par = {**R.DEFAULTS, "actor_lr": 3e-4, "max_grad_norm": 0.5, "ent_reg": True, "alpha_lr": 1e-3, "ent_targ": 2.0}
    got = []
    for eager in (False, True):
        eng = make_engine("h64", S, A, batch=mb, capacity=n)
        load(eng, st0, nrm)
        eng.ppo_begin(s, a, adv)
        load(eng, st, nrm)
        eng.ppo_steps(idx, eager=eager, **_pargs(par))
        eng.sync()
        got.append(_state_bytes(eng, steps))
        assert eng.ppo_end(par["eps_ppo"])["n_steps"] == steps
        eng.close()
    for key in got[0]:
        assert np.array_equal(got[0][key], got[1][key]), key
    assert got[0]["params:actor.l0"].any() and got[0]["adam_m:actor.l2"].any()


def test_launch_counts_do_not_exceed_the_gaussian_handles(gpu_available):
    S, A, mb, rows = 17, 6, 312, 4097
    counts = {}
    for softmax in (False, True):
        eng = make_engine("h64", S, A, batch=mb, capacity=rows, trpo=True, softmax=softmax)
        counts[softmax] = (len(eng.ppo_plan_info(mb)), len(eng.trpo_plan_info(rows)), len(eng.trpo_plan_info(33)))
        if softmax:
            kernels = [p["kernel"] for p in eng.ppo_plan_info(mb)]
            assert "k_ppo_head" in kernels and "k_ppo_gather" in kernels
        eng.close()
    print(f"launches (PPO step, Fisher product over {rows} rows, over 33): gaussian {counts[False]} softmax {counts[True]}")
    assert all(x <= y for x, y in zip(counts[True], counts[False])), counts


def test_sample_draws_from_the_engines_stream(gpu_available):
    from sac_eo._native import SacxError
    from sac_eo.actors.discrete_actors import SoftMaxActor
    S, A, n, seed = 17, 5, 7, 12
    cfg, st, nrm = make_state("h64", S, A, seed=3)
    s = states(S, n, 8)
    lg = SM.forward(st, cfg, nrm, s)[0]
    rs = np.random.RandomState(seed)
    u = rs.random_sample(size=(n, A))
    pert = (lg - lg.max(-1, keepdims=True)) - np.log(-np.log(u))    # the reference's a_logits - np.log(-np.log(u))
    top = np.sort(pert, -1)
    assert np.all(top[:, -1] - top[:, -2] > 1e-4)          # the premise, in fp64: no row's arg max is a near tie
    want = np.argmax(pert, -1)
    actor = SoftMaxActor(_Env(S, A), [64, 64], ["tanh"], 0.5, rng=np.random.default_rng(0))
    actor.set_weights([np.asarray(w, np.float32) for w in st.actor])
    eng = make_engine("h64", S, A, batch=16, capacity=16)
    actor._bind(eng)
    eng.set_normalizers(nrm.s_mean, nrm.s_den, nrm.a_mean, nrm.a_den)
    eng.rng_set_state(np.random.RandomState(seed).get_state())
    got = actor.sample(s)
    dev, ref = eng.rng_get_state(), rs.get_state()
    assert np.array_equal(dev[1], ref[1]) and dev[2] == ref[2]
    assert got.shape == (n,) and np.array_equal(np.asarray(got), want)
    assert np.array_equal(np.asarray(got), SM.gumbel_argmax(lg.astype(np.float32), u))
    det = actor.sample(s, deterministic=True)              # draws nothing
    dev2 = eng.rng_get_state()
    assert np.array_equal(dev2[1], ref[1]) and dev2[2] == ref[2] and np.array_equal(np.asarray(det), np.argmax(lg, -1))
    assert actor.sample(s[0]).shape == ()                  # tf.squeeze
    # the class's row functions through the engine, with the reference's shapes
    a = np.asarray(det)
    assert bar_err(actor.neglogp(s, a), SM.neglogp_of(lg, a)) < 2e-5 and np.asarray(actor.neglogp(s[0], a[0])).shape == ()
    assert bar_err(actor.entropy(s), SM.entropy_of(lg)) < 2e-5 and bar_err(actor.get_kl_info(s), lg) < 2e-5
    assert np.max(np.abs(np.asarray(actor.kl(s, actor.get_kl_info(s))))) < 1e-6
    # the device samplers refuse a softmax handle; the init call refuses a bound one
    for call in (lambda: eng.act(s), lambda: eng.act_host(s[:1])):
        with pytest.raises(SacxError, match="samples on the host"):
            call()
    assert eng.lib.sacx_softmax_init(eng.h) != 0 and b"must precede sacx_bind" in eng.lib.sacx_last_error(eng.h)
    eng.close()
