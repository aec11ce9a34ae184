"""The TRPO actor update of a trainable GaussianActor handle on the device against tests/trpo_ref.py.

* the surrogate gradient (``trpo_begin`` / ``trpo_grad``) and the Fisher-vector product (``trpo_fvp``) against
  the fp64 restatement at ``test_gpu_ppo.py``'s gradient bar, 2e-4 of each parameter tensor's max; S = 3,
  A = 1 and 2, hidden widths (24, 40) -- no multiple of 16 --, one 3-layer, one layer-norm, one
  ``per_state_std`` and one floored-column case; 1 row, one chunk + 1 (4,097 rows) and 100 rows with
  ``trust_sub = 3`` (34 rows of the Fisher product); every direction has non-zero ``logstd`` entries;
* eager == graph and run == run, bit for bit;
* whole updates over the three outcomes of the line search (adj = 1, adj = 2^-k/2, adj = 0), with alpha's step
  under ``ent_reg``: the restatement first asserts that every line-search decision has margin -- a trial that
  is rejected for its kl has ``kl - kl_max >= 100 x 2e-5 x kl``, an accepted one ``kl_max - kl >= 100 x 2e-5
  x kl_max`` and ``|improve| >= 100 x 2e-5 x mean|adv|`` (the scale of the terms whose means ``improve``
  subtracts) -- so that fp32 cannot flip a branch; then the eight figures and the final weights within the
  larger of the single-step bars (2e-5 figures, 1e-6 weights) and the restatement's own fp32-against-fp64
  envelope, itself < 1e-2.  ``trust_damp`` (0.5; 1.5 for the 4,097-row case) and ``cg_it`` are chosen so that conjugate gradient converges
  (r.r <= 1e-6 b.b in fp64) and its break, a branch too, has a factor 10 of margin: either it comes with that
  margin and leaves iterations the device must skip through its flag, or ``cg_it`` ends the loop before any
  arithmetic could break.  A figure is measured relative to its fp64 value; ``tv`` / ``kl`` / ``improve``,
  which vanish by construction when the step is rejected, relative to the larger of that and ``tv_pre`` /
  ``kl_pre`` / ``mean|adv|``.  For adj = 0 the weights equal the saved ones bit for bit;
* zero steps (``delta_trpo = 0``; all-zero advantages), CUDA rows == NumPy rows bit for bit, and one
  ``MBRLOnPolicyAlg._update()`` with ``mf_algo='trpo'`` (constructed directly).
"""
import numpy as np
import pytest

import ppo_ref as R
import sac_oracle as O
import trpo_ref as T
from helpers import nontrivial_normalizers

pytestmark = pytest.mark.gpu

CHUNK = 4096
SHAPES = {
    "a1": dict(A=1, hidden=(24, 40), acts=("tanh", "tanh")),
    "a2_floor": dict(A=2, hidden=(24, 40), acts=("relu", "elu"), floor=True),
    "three": dict(A=2, hidden=(24, 40, 20), acts=("relu", "tanh", "elu")),
    "ln": dict(A=2, hidden=(24, 40), acts=("tanh", "relu"), layer_norm=True),
    "pss": dict(A=2, hidden=(24, 40), acts=("tanh", "elu"), per_state_std=True, std_mult=0.8),
    # widths off the 4-grid; the flat range is 1,282 floats, so the vectors' last float4 is half padding
    # (tests/test_trpo_config.py holds that on the CPU)
    "odd": dict(A=2, hidden=(23, 41), acts=("tanh", "elu")),
}
S = 3


def make_state(shape, seed):
    c = SHAPES[shape]
    cfg = O.Config(S=S, A=c["A"], hidden=c["hidden"], actor_acts=c["acts"], per_state_std=c.get("per_state_std", False),
                   layer_norm=c.get("layer_norm", False))
    rng = np.random.RandomState(seed + 50)
    logstd = (0.2 * rng.normal(size=cfg.A) - 0.3).astype(np.float32)
    if c.get("floor"):
        logstd[0] = -8.0
    st = R.init_state(cfg, seed=seed, std_mult=c.get("std_mult", 1.0), logstd=logstd, bias_scale=0.1, gain=0.5)
    if c.get("floor"):
        st.actor[-2][:, 0] = 0.0                 # (the mean of a std-1e-3 dimension is its bias alone: finite ratios)
    nrm = nontrivial_normalizers(rng, cfg.S, cfg.A)
    return cfg, st, nrm


def rollout(cfg, st, nrm, n, seed):
    rng = np.random.RandomState(seed + 900)
    s = (rng.normal(size=(n, cfg.S)) * rng.uniform(0.3, 2.0, cfg.S)).astype(np.float32)
    d = R.forward(st, cfg, nrm, s)
    a = (d.mean + np.exp(d.ls) * rng.normal(size=(n, cfg.A))).astype(np.float32)
    adv = (rng.normal(size=n) * 1.5 + 0.4).astype(np.float32)
    return s, a, adv


def make_engine(shape, capacity, **kw):
    from sac_eo.engine import Engine, EngineConfig
    c = SHAPES[shape]
    return Engine(EngineConfig(s_dim=S, a_dim=c["A"], hidden=c["hidden"], actor_activations=c["acts"], batch=16,
                               buffer_capacity=capacity, per_state_std=c.get("per_state_std", False),
                               actor_gaussian="train", actor_std_mult=c.get("std_mult", 1.0),
                               actor_layer_norm=c.get("layer_norm", False), graph_steps=1, trpo=True, **kw))


def load(eng, st, nrm):
    eng.set_net("actor", [np.asarray(w, np.float32) for w in st.actor])
    eng.set_logstd(np.asarray(st.logstd, np.float32))
    eng.set_normalizers(nrm.s_mean, nrm.s_den, nrm.a_mean, nrm.a_den)


def par_of(kw):
    kw = {**T.DEFAULTS, **kw}
    return dict(delta=kw["delta_trpo"], cg_it=kw["cg_it"], trust_sub=kw["trust_sub"], trust_damp=kw["trust_damp"],
                kl_maxfactor=kw["kl_maxfactor"], ent_reg=kw["ent_reg"], ent_targ=kw["ent_targ"], alpha_lr=kw["alpha_lr"],
                adv_center=kw["adv_center"], adv_scale=kw["adv_scale"])


# ------------------------------------------------------------------------------------- gradient, Fisher product
GF = [("a1", 1, 1), ("a1", CHUNK + 1, 1), ("a2_floor", 100, 3), ("three", 100, 3), ("ln", CHUNK + 1, 3), ("pss", 100, 3),
      ("odd", 100, 3)]


@pytest.mark.parametrize("shape,n,sub", GF)
def test_gradient_and_fisher_product(gpu_available, shape, n, sub):
    import torch
    cfg, st, nrm = make_state(shape, seed=2)
    s, a, adv = rollout(cfg, st, nrm, n, seed=4)
    kw = dict(trust_sub=sub, trust_damp=0.05, ent_targ=-1.5, adv_center=n > 1, adv_scale=n > 1)
    eng = make_engine(shape, capacity=max(n, 16))
    load(eng, st, nrm)
    eng.v["ppo.alpha"][0, 0] = 0.3                       # the entropy term takes part
    st.alpha = np.array(np.float64(np.float32(0.3)))
    assert eng.trpo_begin(s, a, adv, **par_of(kw)) == n
    got_g = eng.trpo_grad()
    nlp_old = R.neglogp(st, cfg, nrm, s, a)
    adv_n = R.normalise_adv(adv, {**T.DEFAULTS, **kw}, np.float64)
    neg_pg, _, _ = T.surrogate_grad(st, cfg, nrm, s, a, adv_n, nlp_old, kw["ent_targ"])
    like = st.trainables(cfg)
    rng = np.random.RandomState(7)
    x = [rng.normal(size=w.shape).astype(np.float32) for w in like]
    got_f = eng.trpo_fvp(x)
    want_f = T.fvp(st, cfg, nrm, s[::sub], [np.asarray(v, np.float64) for v in x], kw["trust_damp"])
    errs = []
    for i, (g, f, ng, wf) in enumerate(zip(got_g, got_f, neg_pg, want_f)):
        eg = float(np.max(np.abs(g.reshape(ng.shape) + ng))) / max(float(np.max(np.abs(ng))), 1e-30)
        ef = float(np.max(np.abs(f.reshape(wf.shape) - wf))) / max(float(np.max(np.abs(wf))), 1e-30)
        print(f"{shape} n={n} sub={sub} tensor {i} {ng.shape}: gradient {eg:.2e} (max {np.max(np.abs(ng)):.3g}) "
              f"fisher product {ef:.2e} (max {np.max(np.abs(wf)):.3g})")
        errs.append((eg, ef))
    # eager == graph, run == run, bit for bit (flat vectors, the padding included)
    xf = eng.trpo_pack(x)
    f0 = eng.trpo_fvp(xf)
    f1 = eng.trpo_fvp(xf, eager=True)
    f2 = eng.trpo_fvp(xf)
    g0 = eng.trpo_grad(flat=True)
    eng.trpo_begin(s, a, adv, **par_of(kw))
    g1 = eng.trpo_grad(flat=True)
    plan = eng.trpo_plan_info((n + sub - 1) // sub)
    chunks = ((n + sub - 1) // sub + CHUNK - 1) // CHUNK
    print(f"launches of one Fisher product over {(n + sub - 1) // sub} rows: {len(plan)} ({chunks} chunk(s))")
    assert max(e[0] for e in errs) < 2e-4 and max(e[1] for e in errs) < 2e-4, errs
    assert torch.equal(f0, f1) and torch.equal(f0, f2) and torch.equal(g0, g1)
    assert np.array_equal(eng.trpo_unpack(f0)[-1], got_f[-1])
    assert len(plan) % chunks == 0 and [p["name"] for p in plan].count("trpo.acc") == chunks
    if SHAPES[shape].get("floor"):                       # the floored column: no gradient, only the damping
        assert got_g[-1][0, 0] == 0.0 and got_f[-1][0, 0] == np.float32(np.float32(0.05) * x[-1][0, 0])
    eng.close()


# ------------------------------------------------------------------------------------- whole updates
UPDATES = {
    # name: shape, rows, the update's keys, the outcome.  cg_it: 20 where the break (r.r < 1e-10) comes with a
    # factor 10 of margin on both sides in fp64 (it then leaves iterations the device must skip), else the last
    # iteration count at which r.r is still >= 1e-9, so that no arithmetic breaks (update_case asserts both)
    "accept": dict(shape="a1", n=150, kw=dict(delta_trpo=0.01, kl_maxfactor=1.5, trust_damp=0.5, cg_it=20), adj="one"),
    "accept_chunks": dict(shape="ln", n=CHUNK + 1, kw=dict(delta_trpo=0.01, kl_maxfactor=1.5, trust_damp=1.5, cg_it=8,
                                                            trust_sub=3), adj="one"),
    "shrink": dict(shape="three", n=150, kw=dict(delta_trpo=0.01, kl_maxfactor=0.3, trust_damp=0.5, cg_it=8, trust_sub=3),
                   adj="k"),
    "reject": dict(shape="pss", n=150, kw=dict(delta_trpo=0.01, kl_maxfactor=1e-6, trust_damp=0.5, cg_it=10), adj="zero"),
    "ent_reg": dict(shape="a1", n=150, kw=dict(delta_trpo=0.01, kl_maxfactor=1.5, trust_damp=0.5, cg_it=20, ent_reg=True,
                                                alpha_lr=0.02, ent_targ=-3.0), adj="one", alpha0=0.2),
}
# the faithful fp32 executions that set the envelope: every summation order of the forward products
# (sac_oracle.MATMUL_ORDERS), each with NumPy's f32 dot products in conjugate gradient and with the dot products
# accumulated in f64 (what the device is specified to do)
FP32_RUNS = tuple(O.MATMUL_ORDERS) + tuple(o + "+dots64" for o in O.MATMUL_ORDERS)
_CACHE = {}


def update_case(name):
    """Everything the CPU decides, computed once: the fp64 restatement, its fp32 runs under every summation
    order, the premise (every line-search decision has margin)."""
    if name in _CACHE:
        return _CACHE[name]
    c = UPDATES[name]
    cfg, st, nrm = make_state(c["shape"], seed=c.get("seed", 3))
    st.alpha = np.array(np.float64(np.float32(c.get("alpha0", 0.0))))
    s, a, adv = rollout(cfg, st, nrm, c["n"], seed=c.get("seed", 3) + 2)
    runs = {}
    for key in ("f64",) + FP32_RUNS:
        ref = T.TRPORef(st.astype(np.float64 if key == "f64" else np.float32), cfg, nrm, c["kw"], dots64=key.endswith("+dots64"))
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
    for t, (kl, imp) in enumerate(keep["trials"]):         # the premise: fp32 cannot flip a branch
        if kl > kl_max:
            assert kl - kl_max >= 100 * 2e-5 * kl, (name, t, kl, kl_max)
        else:
            assert kl_max - kl >= 100 * 2e-5 * kl_max and abs(imp) >= 100 * 2e-5 * scale, (name, t, kl, imp)
    # ... conjugate gradient has converged in fp64 (r.r <= 1e-6 b.b when it stops): an iterate of a CG cut
    # short is no stable function of rounding, only the converged solve F^-1 b is (its fp32 error is cond(F) eps)
    # ... and its break is a branch like the line search's: every r.r it tested lies a factor 10 from 1e-10
    hist = keep["rr_hist"]
    assert keep["rdotr"] <= 1e-6 * hist[0], (name, keep["rdotr"], hist[0])
    assert all(rr >= 1e-9 or rr <= 1e-11 for rr in hist[1:]), (name, hist)
    for key in FP32_RUNS:                                  # ... and no branch flipped in the fp32 restatement
        assert runs[key][1]["adj"] == log["adj"], (name, key)
    want = dict(one=lambda x: x == 1.0, k=lambda x: 0 < x < 1, zero=lambda x: x == 0.0)[c["adj"]]
    assert want(log["adj"]) and not keep["zero"], (name, log)
    _CACHE[name] = (cfg, st, nrm, s, a, adv, runs, scale)
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(UPDATES))
def test_premise_of_the_whole_updates_on_the_cpu(name):
    """The margins and the restatement's own envelope (no device call: CPU arithmetic only)."""
    cfg, st, nrm, s, a, adv, runs, scale = update_case(name)
    _, l64, k64 = runs["f64"]
    for fig, env, _ in envelope_of(name):
        assert env < 1e-2, (name, fig, env)


def _rel(name, key, val, l64, scale):
    floor = dict(tv=abs(l64["tv_pre"]), kl=abs(l64["kl_pre"]), improve=scale).get(key, 0.0)
    return abs(val - l64[key]) / max(abs(l64[key]), floor, 1e-30)


def envelope_of(name):
    """[(figure, fp32 envelope, bar)] of the restatement: the eight figures, then the final weight tensors."""
    cfg, st, nrm, s, a, adv, runs, scale = update_case(name)
    r64, l64, _ = runs["f64"]
    out = []
    for key in T.LOG_KEYS:
        out.append((key, max(_rel(name, key, runs[o][1][key], l64, scale) for o in FP32_RUNS), 2e-5))
    for i, y in enumerate(r64.st.trainables(cfg)):
        env = max(float(np.max(np.abs(np.asarray(runs[o][0].st.trainables(cfg)[i], np.float64) - y))) for o in FP32_RUNS)
        out.append((f"final weights {i}", env, 1e-6))
    return out


@pytest.mark.parametrize("name", sorted(UPDATES))
def test_whole_update(gpu_available, name):
    c = UPDATES[name]
    cfg, st, nrm, s, a, adv, runs, scale = update_case(name)
    r64, l64, k64 = runs["f64"]
    envs = envelope_of(name)
    eng = make_engine(c["shape"], capacity=max(c["n"], 16))
    load(eng, st, nrm)
    eng.v["ppo.alpha"][0, 0] = float(np.float32(c.get("alpha0", 0.0)))
    before = [np.asarray(w, np.float32) for w in st.trainables(cfg)]
    par = par_of(c["kw"])
    eng.trpo_begin(s, a, adv, **par)
    log = eng.trpo_step(**par)
    info = eng.trpo_solve_info()
    print(f"{name}: device vFv {info['vFv']:.6g} eta {info['eta']:.6g} cg iterations {info['cg_iters']} | "
          f"restatement vFv {k64['vFv']:.6g} eta {k64['eta']:.6g} cg iterations {k64['cg_iters']}")
    assert sorted(log) == sorted(T.LOG_KEYS)
    after = eng.get_net("actor") + ([] if cfg.per_state_std else [eng.v["actor.logstd"].cpu().numpy().copy()])
    figures = []
    for (key, env, bar) in envs[:len(T.LOG_KEYS)]:
        err = _rel(name, key, float(log[key]), l64, scale)
        print(f"{name} {key}: device {float(log[key]):.7g} ref {l64[key]:.7g} error {err:.2e} fp32 envelope {env:.2e}")
        figures.append((key, err, env, bar))
    for i, ((what, env, bar), x, y) in enumerate(zip(envs[len(T.LOG_KEYS):], after, r64.st.trainables(cfg))):
        err = float(np.max(np.abs(np.asarray(x, np.float64).reshape(y.shape) - y)))
        print(f"{name} {what} {y.shape}: device error {err:.2e} fp32 envelope {env:.2e}")
        figures.append((what, err, env, bar))
    assert float(log["adj"]) == pytest.approx(l64["adj"], rel=1e-12, abs=0)
    for what, err, env, bar in figures:                    # (every figure is printed before the first assertion)
        assert env < 1e-2, (what, env)
        assert err <= max(bar, env), (what, err, env)
    if c["adj"] == "zero":                                 # no policy update: the saved weights, bit for bit
        for x, y in zip(after, before):
            assert np.array_equal(x.reshape(y.shape), y)
    else:
        assert any(not np.array_equal(x.reshape(y.shape), y) for x, y in zip(after, before))
    if c["kw"].get("ent_reg"):
        assert float(log["alpha"]) != float(np.float32(c["alpha0"])) and int(eng.v["ppo.ctl"][0, 2].item()) == 1
    eng.close()


def test_eager_update_equals_the_graph_and_repeats(gpu_available):
    import torch
    c = UPDATES["shrink"]
    cfg, st, nrm, s, a, adv, runs, scale = update_case("shrink")
    par = par_of(c["kw"])
    outs = []
    for eager in (False, True, False):
        eng = make_engine(c["shape"], capacity=c["n"])
        load(eng, st, nrm)
        eng.trpo_begin(s, a, adv, **par)
        log = eng.trpo_step(eager=eager, **par)
        outs.append((log, eng.v["trpo.vec"].clone().cpu(), [torch.as_tensor(w) for w in eng.get_net("actor")]))
        eng.close()
    for log, vec, w in outs[1:]:
        assert all(np.float32(log[k]) == np.float32(outs[0][0][k]) for k in T.LOG_KEYS)
        assert torch.equal(vec, outs[0][1]) and all(torch.equal(x, y) for x, y in zip(w, outs[0][2]))


@pytest.mark.parametrize("how", ["delta_zero", "zero_advantages"])
def test_zero_steps(gpu_available, how):
    cfg, st, nrm = make_state("a2_floor" if how == "delta_zero" else "a1", seed=2)
    shape = "a2_floor" if how == "delta_zero" else "a1"
    s, a, adv = rollout(cfg, st, nrm, 50, seed=4)
    kw = dict(delta_trpo=0.0) if how == "delta_zero" else dict(delta_trpo=0.01, adv_center=False)
    if how == "zero_advantages":
        adv = np.zeros_like(adv)
    eng = make_engine(shape, capacity=64)
    load(eng, st, nrm)
    par = par_of(kw)
    eng.trpo_begin(s, a, adv, **par)
    if how == "zero_advantages":
        assert all(np.all(g == 0) for g in eng.trpo_grad())
    log = eng.trpo_step(**par)
    want = T.TRPORef(st.copy(), cfg, nrm, kw).update(s, a, adv)
    assert log["adj"] == 1.0 == want["adj"] and float(log["improve"]) == 0.0
    assert abs(float(log["kl"])) <= 1e-9 and abs(float(log["tv"])) <= 1e-6 and abs(float(log["ent"]) - want["ent"]) <= 2e-5 * abs(want["ent"])
    assert not eng.v["trpo.vec"][6].any()                  # the step
    after = eng.get_net("actor") + [eng.v["actor.logstd"].cpu().numpy().copy()]
    floor = np.float32(np.log(1e-3))
    for i, (x, y) in enumerate(zip(after, st.trainables(cfg))):
        y = np.asarray(y, np.float32)
        if i == len(after) - 1:                            # set_weights floors the raw logstd (a function-preserving change)
            y = np.maximum(y, floor)
        assert np.array_equal(x.reshape(y.shape), y), i
    eng.close()


def test_degenerate_and_misuse_are_refused(gpu_available):
    from sac_eo import _native as N
    from sac_eo.engine import Engine, EngineConfig
    cfg, st, nrm = make_state("a1", seed=2)
    s, a, adv = rollout(cfg, st, nrm, 20, seed=4)
    eng = make_engine("a1", capacity=32)
    load(eng, st, nrm)
    with pytest.raises(N.SacxError, match="sacx_trpo_begin first"):
        eng.trpo_step(**par_of({}))
    with pytest.raises(N.SacxError, match="cg_it"):
        eng.trpo_begin(s, a, adv, **par_of(dict(cg_it=0)))
    assert eng.lib.sacx_trpo_init(eng.h) != 0 and b"must precede sacx_bind" in eng.lib.sacx_last_error(eng.h)
    eng.close()
    plain = Engine(EngineConfig(s_dim=S, a_dim=1, hidden=(24, 40), batch=16, buffer_capacity=32, actor_gaussian="train",
                                graph_steps=1))
    with pytest.raises(RuntimeError, match="trpo=True"):
        plain.trpo_begin(s, a, adv, **par_of({}))
    out = (__import__("ctypes").c_double * 8)()
    par = N.TrpoParams(delta=0.01, trust_damp=0.1, kl_maxfactor=1.5, cg_it=5, trust_sub=1)
    assert plain.lib.sacx_trpo_step(plain.h, par, 0, out) != 0 and b"sacx_trpo_init was not called" in plain.lib.sacx_last_error(plain.h)
    plain.close()


# ------------------------------------------------------------------------------------- the host class
KW = dict(adv_center=True, adv_scale=True, delta_trpo=0.01, cg_it=10, trust_sub=3, trust_damp=0.1, kl_maxfactor=0.3,
          ent_reg=True, ent_targ=5.0, alpha_lr=0.01)        # (the entropy is below its target: alpha grows from 0)


class _Box:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, np.float32), np.ones(n, np.float32)


class _Env:
    observation_space, action_space = _Box(S), _Box(2)


def test_update_takes_device_rows_as_numpy_rows(gpu_available):
    import torch
    from sac_eo.actors.continuous_actors import GaussianActor
    from sac_eo.algs.model_free.trpo import TRPO
    cfg, st, nrm = make_state("three", seed=3)
    s, a, adv = rollout(cfg, st, nrm, 150, seed=5)
    outs = []
    for dev in (False, True):
        actor = GaussianActor(_Env(), [24, 40, 20], ["relu", "tanh", "elu"], 0.5, "orthogonal", False, rng=np.random.default_rng(0))
        actor.set_weights([np.asarray(w, np.float32) for w in st.trainables(cfg)])
        t = TRPO(actor, dict(KW, vcritics=1))
        stream = np.random.get_state()
        rows = tuple(torch.as_tensor(x).cuda() for x in (s, a, adv)) if dev else (s, a, adv)
        log = t.update(rows + (None, None, None))
        now = np.random.get_state()
        assert np.array_equal(now[1], stream[1]) and now[2] == stream[2]       # TRPO draws nothing
        assert sorted(log) == sorted(T.LOG_KEYS) and float(log["alpha"]) == float(t.alpha) > 0
        assert "v0.l0" in t.engine.segments and t.engine.cfg.trpo
        flat = actor.get_weights(flat=True)
        assert flat.size == sum(np.asarray(w).size for w in st.trainables(cfg))
        outs.append((log, flat))
        t.engine.close()
    assert all(np.float32(outs[0][0][k]) == np.float32(outs[1][0][k]) for k in T.LOG_KEYS)
    assert np.array_equal(outs[0][1], outs[1][1]) and 0 < outs[0][0]["adj"]


def test_one_mbrl_update_with_trpo(gpu_available):
    """MBRLOnPolicyAlg constructed directly with mf_algo='trpo' at the shapes of test_gpu_mbrl's whole update:
    the eight keys, finite values, and the global stream where the restatement of the loop leaves it with
    the PPO update taken out (TRPO draws nothing)."""
    import mbrl_ref as M
    import test_gpu_mbrl as G
    from sac_eo.algs.mbrl_onpolicy_alg import MBRLOnPolicyAlg
    nc, holdout = 2, 0.0
    case = G.update_case(nc, holdout, 1)
    akw = dict(G.alg_kwargs(nc, holdout), mf_algo="trpo")
    tkw = dict(adv_center=True, adv_scale=True, delta_trpo=0.01, cg_it=10, trust_sub=1, trust_damp=0.1, kl_maxfactor=1.5,
               ent_reg=False, ent_targ=-float(G.UPD["A"]), alpha_lr=3e-4)
    rows = case["rows"]
    ref = M.UpdateRef(case["sac"].astype(np.float64), case["ppo"].astype(np.float64), case["vst"].astype(np.float64),
                      case["cfg"], ("tanh", "tanh"), case["nrm"], (rows["s"], rows["a"], rows["sp"], rows["r"]),
                      G.alg_kwargs(nc, holdout), G.PPO_KW, np.random.RandomState(31))
    ref.ppo_ref = T.TRPORef(ref.ppo, case["cfg"], case["nrm"], tkw)       # no draw from the stream
    l64 = ref.update()
    stream = ref.rs.get_state()
    alg = MBRLOnPolicyAlg(0, G._UEnv(), G._UEnv(), case["actor"], case["critics"], case["models"], akw, dict(tkw))
    assert type(alg.mf_algo).__name__ == "TRPO" and alg.engine.cfg.trpo
    alg.normalizer = case["norm"]
    alg._set_rms()
    n = G.UPD["rows"]
    for lo in (0, n // 2):
        part = [rows[k][lo:lo + n // 2] for k in ("s", "a", "r", "sp", "d")]
        alg.env_data.add(*part)
        alg.engine.append(*part[:4], part[4].astype(np.float32))
    alg.engine.rng_set_state(np.random.RandomState(31).get_state())
    alg._update()
    tr = alg.logger.train_dict
    for key in T.LOG_KEYS:
        vals = [float(x) for x in tr[key]]
        print(f"{key}: device {vals} restatement {[u[key] for u in l64['updates']]}")
        assert len(vals) == G.UPD["mf"] and np.all(np.isfinite(vals)), key
    for key in ("actor_lr", "outside_clip", "actor_grad_norm", "epsilon", "norm_pg", "norm_MSE"):
        assert key not in tr
    got = alg.engine.rng_get_state()
    assert np.array_equal(got[1], stream[1]) and got[2:5] == stream[2:5]
    assert all(float(x) > 0 for x in tr["adj"])
    alg.engine.close()
