"""The PPO actor update of a trainable GaussianActor handle on the device against tests/ppo_ref.py.

* the row functions (neglogp, (mean, logstd), entropy, forward kl) at 2e-5 of the tensor's max (the bar
  tests/test_gpu_engine.py uses for the actor's nlp);
* one minibatch step (fp32 device, fp64 restatement) at the bars of tests/test_gpu_bc.py: loss 2e-5,
  gradients (through Adam's first moment after step 1) 2e-4, weights 1e-6; alpha and both norms 2e-5.
  The weights move between ``ppo_begin`` and the step (the public ``set_net`` / ``set_logstd``) so that the
  minibatch leaves r = 1; the restatement asserts the premise: >= 3 rows inside the clip range, >= 3 with
  zero gradient above 1 + eps, >= 3 below 1 - eps, no row within 1e-4 of a clip bound, no logstd within
  1e-4 of the floor;
* ``PPO.update`` end to end (n = 200, 4 minibatches, 3 iterations: 12 steps, then a second update at the
  adapted rate): the host stream bit-equal to the restatement's after each call, ``outside_clip`` exactly
  equal, the other log values and the final weights within the larger of the single-step bars and the
  fp32 drift envelope (the restatement in fp32 against its fp64 run; itself < 1e-2);
* graph replay == eager == one step per call, bit for bit (12 steps: graphs of 8 and 1; 72 steps: one
  of 64 and one of 8); an inference-only GaussianActor handle acts as before; the SAC step on the trainable handle and the PPO step on a SAC handle fail and touch nothing.
"""
import numpy as np
import pytest

import ppo_ref as R
import sac_oracle as O
from helpers import B1, nontrivial_normalizers, relerr

pytestmark = pytest.mark.gpu

SHAPES = {
    "pendulum": dict(S=3, A=1, hidden=(64, 64), acts=("tanh", "tanh")),
    "halfcheetah": dict(S=17, A=6, hidden=(64, 64), acts=("tanh", "tanh")),
    "pss17": dict(S=17, A=17, hidden=(64, 64), acts=("tanh", "elu"), per_state_std=True, std_mult=0.8),
    "layer_norm": dict(S=7, A=3, hidden=(64, 48), acts=("tanh", "relu"), layer_norm=True),
    "three": dict(S=7, A=3, hidden=(32, 48, 40), acts=("relu", "tanh", "elu")),
    "wide1": dict(S=7, A=3, hidden=(520,), acts=("tanh",)),
    # widths off the 4-grid: every activation / delta row and W_ext row at an odd stride
    "odd": dict(S=7, A=3, hidden=(23, 41), acts=("tanh", "elu")),
}


def ocfg_of(shape):
    c = SHAPES[shape]
    return O.Config(S=c["S"], A=c["A"], hidden=c["hidden"], actor_acts=c["acts"],
                    per_state_std=c.get("per_state_std", False), layer_norm=c.get("layer_norm", False))


def make_state(shape, seed, floor_dim=False):
    """(oracle cfg, fp64 state holding f32 values, normaliser, std_mult).  floor_dim: logstd dimension 0
    below the floor (its mean is then its bias alone, so the ratio stays finite at std 1e-3)."""
    c = SHAPES[shape]
    cfg = ocfg_of(shape)
    rng = np.random.RandomState(seed + 50)
    logstd = (0.2 * rng.normal(size=cfg.A) - 0.3).astype(np.float32)
    if floor_dim:
        logstd[0] = -8.0
    st = R.init_state(cfg, seed=seed, std_mult=c.get("std_mult", 1.0), logstd=logstd, bias_scale=0.1, gain=0.5)
    if floor_dim:
        st.actor[-2][:, 0] = 0.0
        if cfg.per_state_std:
            st.actor[-2][:, cfg.A] = 0.0
            st.actor[-1][cfg.A] = -8.0
    nrm = nontrivial_normalizers(rng, cfg.S, cfg.A)
    return cfg, st, nrm


def make_engine(shape, batch, capacity, **kw):
    from sac_eo.engine import Engine, EngineConfig
    c = SHAPES[shape]
    return Engine(EngineConfig(s_dim=c["S"], a_dim=c["A"], hidden=c["hidden"], actor_activations=c["acts"],
                               batch=batch, buffer_capacity=capacity, per_state_std=c.get("per_state_std", False),
                               actor_gaussian=kw.pop("actor_gaussian", "train"), actor_std_mult=c.get("std_mult", 1.0),
                               actor_layer_norm=c.get("layer_norm", False), graph_steps=1, **kw))


def load(eng, st, nrm):
    eng.set_net("actor", [np.asarray(w, np.float32) for w in st.actor])
    eng.set_logstd(np.asarray(st.logstd, np.float32))
    eng.set_normalizers(nrm.s_mean, nrm.s_den, nrm.a_mean, nrm.a_den)


def rollout(cfg, st, nrm, n, seed):
    """On-policy rows of the state: s, a ~ pi(s), adv."""
    rng = np.random.RandomState(seed + 900)
    s = (rng.normal(size=(n, cfg.S)) * rng.uniform(0.3, 2.0, cfg.S)).astype(np.float32)
    d = R.forward(st, cfg, nrm, s)
    a = (d.mean + np.exp(d.ls) * rng.normal(size=(n, cfg.A))).astype(np.float32)
    adv = (rng.normal(size=n) * 1.5 + 0.4).astype(np.float32)
    return s, a, adv


def moved(st, cfg, seed, scale, floor_dim=False):
    """The state a few updates later: every weight perturbed (f32 values)."""
    rng = np.random.RandomState(seed + 1700)
    new = st.copy()
    keep = (new.actor[-2][:, 0].copy(), float(new.actor[-1][0]))
    for w in new.actor:
        w += (scale * rng.normal(size=w.shape)).astype(np.float32)
    new.logstd += (0.03 * rng.normal(size=new.logstd.shape)).astype(np.float32)
    if floor_dim:
        new.actor[-2][:, 0] = keep[0]
        new.actor[-1][0] = keep[1] + 2e-4 * rng.normal()
        if cfg.per_state_std:
            new.actor[-2][:, cfg.A] = 0.0
            new.actor[-1][cfg.A] = -8.0
    new.actor = [np.asarray(np.asarray(w, np.float32), np.float64) for w in new.actor]
    new.logstd = np.asarray(np.asarray(new.logstd, np.float32), np.float64)
    return new


# ---------------------------------------------------------------------------------------------- rows
ROWS = [("pendulum", 1), ("pendulum", 17), ("pendulum", 300), ("halfcheetah", 313), ("pss17", 33), ("layer_norm", 33),
        ("three", 33), ("wide1", 33), ("odd", 33)]


@pytest.mark.parametrize("shape,n", ROWS)
def test_row_functions(gpu_available, shape, n):
    cfg, st, nrm = make_state(shape, seed=2, floor_dim=cfg_has_floor(shape))
    eng = make_engine(shape, batch=16, capacity=max(n, 16))
    load(eng, st, nrm)
    s, a, _ = rollout(cfg, st, nrm, n, seed=4)
    ref0 = R.forward(st, cfg, nrm, s)
    st2 = moved(st, cfg, 5, 0.02, cfg_has_floor(shape))
    d = R.forward(st, cfg, nrm, s)
    mean, ls, ent = [x.cpu().numpy() for x in eng.dist(s)]
    nlp = eng.neglogp(s, a).cpu().numpy()
    assert mean.shape == (n, cfg.A) and nlp.shape == (n,)
    errs = dict(mean=relerr(mean, d.mean), ls=relerr(ls, d.ls), ent=relerr(ent, R.entropy_of(d)),
                nlp=relerr(nlp, R.neglogp_of(d, a)))
    # kl of the moved policy against this one's distribution
    load(eng, st2, nrm)
    kl = eng.kl(s, ref0.mean.astype(np.float32), ref0.ls.astype(np.float32)).cpu().numpy()
    klr = R.kl_of(R.forward(st2, cfg, nrm, s), ref0.mean.astype(np.float32), ref0.ls.astype(np.float32))
    errs["kl"] = relerr(kl, klr)
    print(f"{shape} n={n}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert np.all(klr > 0) and max(errs.values()) < 2e-5, errs
    eng.close()


def cfg_has_floor(shape):
    return SHAPES[shape]["A"] >= 3


# ---------------------------------------------------------------------------------------------- one step
STEP_CASES = {
    # name: shape, minibatch rows, table rows, parameters, weight move
    "pendulum_312": dict(shape="pendulum", mb=312, n=400, par=dict(max_grad_norm=0.5), move=0.03, seed=5),
    "hc_33_floor": dict(shape="halfcheetah", mb=33, n=64, par=dict(max_grad_norm=None), move=0.012, seed=5, floor=True),
    "pss_17": dict(shape="pss17", mb=17, n=40, par=dict(max_grad_norm=50.0, adv_center=False), move=0.006, seed=1),
    "ln_16": dict(shape="layer_norm", mb=16, n=16, par=dict(max_grad_norm=0.05, adv_scale=False), move=0.04, seed=6),
    "three_33": dict(shape="three", mb=33, n=50, par=dict(max_grad_norm=None, adv_center=False, adv_scale=False),
                     move=0.02, seed=2),
    "wide_33": dict(shape="wide1", mb=33, n=50, par=dict(max_grad_norm=0.2), move=0.03, seed=7),
    "ent_reg": dict(shape="halfcheetah", mb=33, n=64, par=dict(max_grad_norm=0.5, ent_reg=True, alpha_lr=0.02,
                                                                 ent_targ=12.0), move=0.018, seed=22, steps=3),
    "odd_17": dict(shape="odd", mb=17, n=40, par=dict(max_grad_norm=None), move=0.04, seed=11),
}


def step_case(name):
    """Everything of a step case the CPU decides: states, rows, indices, the restatement's results and
    the premise (asserted here, from the fp64 restatement)."""
    c = STEP_CASES[name]
    floor = c.get("floor", False)
    cfg, st0, nrm = make_state(c["shape"], c["seed"], floor)
    s, a, adv = rollout(cfg, st0, nrm, c["n"], c["seed"])
    st = moved(st0, cfg, c["seed"], c["move"], floor)
    rng = np.random.RandomState(c["seed"] + 31)
    steps = c.get("steps", 1)
    idx = np.stack([rng.permutation(c["n"])[:c["mb"]] for _ in range(steps)]).astype(np.int32)
    par = {**R.DEFAULTS, "actor_lr": 1e-4, **c["par"]}
    nlp_old = R.neglogp(st0, cfg, nrm, s, a)
    ref, keeps = st.copy(), []
    outs = []
    lo, hi = np.float32(1 - par["eps_ppo"]), np.float32(1 + par["eps_ppo"])
    for k in range(steps):
        keep = {}
        b = idx[k]
        outs.append(R.ppo_step(ref, cfg, nrm, s[b], a[b], adv[b], nlp_old[b], par, keep))
        r, take = keep["r"], keep["take"]
        inside, above, below = take & (r >= lo) & (r <= hi), ~take & (r > hi), ~take & (r < lo)
        assert inside.sum() >= 3 and above.sum() >= 3 and below.sum() >= 3, (name, inside.sum(), above.sum(), below.sum())
        assert np.min(np.abs(r - lo)) >= 1e-4 and np.min(np.abs(r - hi)) >= 1e-4, name
        assert np.min(np.abs(keep["ls_un"] - keep["floor"])) >= 1e-4, name
        if floor:
            assert np.any(keep["ls_un"] < keep["floor"]) and np.any(keep["ls_un"] > keep["floor"])
        # the loss is a mean of signed terms of magnitude ~ |adv|: a RELATIVE bar on it needs a loss that is
        # not a near-cancellation of them
        assert abs(outs[-1]["loss"]) >= 0.05, (name, outs[-1]["loss"])
        if par["max_grad_norm"]:
            clipping = outs[-1]["grad_norm_pre"] > par["max_grad_norm"]
            assert clipping == (name in ("pendulum_312", "ln_16", "wide_33", "ent_reg")), (name, outs[-1])
        keeps.append(keep)
    return dict(c=c, cfg=cfg, st0=st0, st=st, nrm=nrm, s=s, a=a, adv=adv, idx=idx, par=par, ref=ref, outs=outs,
                keeps=keeps, steps=steps)


def _moment(eng, name):
    seg = eng.segments[name]
    off, n = seg["offset"] // 4, seg["rows"] * seg["cols"]
    return eng.v["adam_m"][0][off: off + n].cpu().numpy().reshape(seg["rows"], seg["cols"]) / B1


def _layer_grads(eng):
    out, i = [], 0
    while f"actor.l{i}" in eng.segments:
        w = _moment(eng, f"actor.l{i}")
        out += [w[:-1], w[-1]]
        i += 1
    return out


def _pargs(par):
    return dict(eps_ppo=par["eps_ppo"], actor_lr=par["actor_lr"], max_grad_norm=par["max_grad_norm"],
                ent_targ=par["ent_targ"], ent_reg=par["ent_reg"], alpha_lr=par["alpha_lr"],
                adv_center=par["adv_center"], adv_scale=par["adv_scale"])


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_one_minibatch_step(gpu_available, case):
    k = step_case(case)
    c, cfg, par = k["c"], k["cfg"], k["par"]
    eng = make_engine(c["shape"], batch=c["mb"], capacity=c["n"])
    load(eng, k["st0"], k["nrm"])
    eng.v["grad"].fill_(3.0)                        # a reused arena: ppo_begin clears the gradient words it reads
    eng.ppo_begin(k["s"], k["a"], k["adv"])
    load(eng, k["st"], k["nrm"])                    # the policy moved since the rollout
    for j in range(k["steps"]):
        eng.ppo_steps(k["idx"][j:j + 1], **_pargs(par))
        eng.sync()
        row, o = eng.ppo_stats(1)[0], k["outs"][j]
        print(f"{case} step {j}: {[l['name'] for l in eng.ppo_plan_info(c['mb'])] if j == 0 else ''} loss {row[0]:.6g} "
              f"vs {o['loss']:.6g}, norms {row[2]:.6g} / {row[3]:.6g} vs {o['grad_norm_pre']:.6g} / "
              f"{o['grad_norm_post']:.6g}, alpha {row[4]:.6g} vs {o['alpha']:.6g}")
        assert abs(row[0] - o["loss"]) <= 2e-5 * abs(o["loss"]), (row[0], o["loss"])
        assert abs(row[1] - o["ent"]) <= 2e-5 * abs(o["ent"])
        assert abs(row[2] - o["grad_norm_pre"]) <= 2e-5 * o["grad_norm_pre"]
        assert abs(row[3] - o["grad_norm_post"]) <= 2e-5 * o["grad_norm_post"]
        assert abs(row[4] - o["alpha"]) <= 2e-5 * abs(o["alpha"]) and row[7] == j + 1
        if par["max_grad_norm"] is None:
            assert row[2] == row[3]
        if j == 0:                                  # gradients (clipped), through Adam's first moment
            go = list(k["keeps"][0]["clipped"])
            if not cfg.per_state_std:
                assert relerr(_moment(eng, "actor.logstd"), go[-1]) < 2e-4
                go = go[:-1]
            if cfg.layer_norm:
                gb = _moment(eng, "actor.ln")
                for i in range(2):
                    assert relerr(gb[i], go[2 + i]) < 2e-4, ("actor.ln", i)
                go = go[:2] + go[4:]
            ga = _layer_grads(eng)
            assert len(ga) == len(go)
            for i, (gd, gr) in enumerate(zip(ga, go)):
                assert relerr(gd, gr) < 2e-4, ("actor", i, relerr(gd, gr))
    ref = k["ref"]
    werr = max(float(np.max(np.abs(x - y))) for x, y in zip(eng.get_net("actor"), ref.actor))
    werr = max(werr, float(np.max(np.abs(eng.v["actor.logstd"].cpu().numpy() - ref.logstd))))
    print(f"{case}: weights after Adam max abs error {werr:.2e}")
    assert werr < 1e-6
    if par["ent_reg"]:
        assert k["outs"][-1]["alpha"] > k["outs"][0]["alpha"] > 0       # alpha left 0
    ctl = eng.v["ppo.ctl"][0].cpu().numpy()
    assert ctl[0] == ctl[1] == ctl[3] == k["steps"] and ctl[2] == (k["steps"] if par["ent_reg"] else 0)
    eng.close()


# ---------------------------------------------------------------------------------------------- PPO.update
class _Box:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, np.float32), np.ones(n, np.float32)


class _Env:
    def __init__(self, S, A):
        self.observation_space, self.action_space = _Box(S), _Box(A)


UPD_KW = dict(actor_lr=3e-4, actor_update_it=3, actor_nminibatch=4, adv_center=True, adv_scale=True, eps_ppo=0.2,
              max_grad_norm=0.5, adaptlr=True, adapt_factor=0.03, adapt_minthresh=0.7, adapt_maxthresh=1.0, ent_reg=True,
              ent_targ=8.0, alpha_lr=1e-3)
LOG_KEYS = ("ent", "tv", "kl", "alpha", "actor_lr", "outside_clip", "actor_grad_norm_pre", "actor_grad_norm")


def update_case(seed=3, n=200):
    from sac_eo.actors.continuous_actors import GaussianActor
    S, A = 17, 6
    actor = GaussianActor(_Env(S, A), [64, 64], ["tanh"], 0.5, "orthogonal", False, rng=np.random.default_rng(seed))
    cfg = O.Config(S=S, A=A, hidden=(64, 64), actor_acts=("tanh", "tanh"))
    w = actor.get_weights()
    rng = np.random.RandomState(seed)
    w[-1] = (0.2 * rng.normal(size=(1, A)) - 0.3).astype(np.float32)
    actor.set_weights(w)
    alpha = np.zeros((), np.float32)
    st = R.PPOState([x.copy() for x in w[:-1]], w[-1].copy(), None, alpha, O.AdamState.zeros_like([alpha]), 1.0)
    st.opt_actor = O.AdamState.zeros_like(st.trainables(cfg))
    nrm = nontrivial_normalizers(rng, S, A)
    data = []
    for u in range(2):                                   # two rollouts (the second is not on-policy: fine)
        data.append(rollout(cfg, st.astype(np.float64), nrm, n, seed + 10 * u))
    return actor, cfg, st, nrm, data


class _Rms:
    def __init__(self, mean, den):
        self.mean, self._den = mean, den

    def den(self):
        return self._den


def test_ppo_update_end_to_end(gpu_available):
    from sac_eo.algs.model_free import PPO
    actor, cfg, st, nrm, data = update_case()
    # the fp64 restatement, and the fp32 executions setting the envelope: the same restatement in fp32
    # under each summation order of the forward products (sac_oracle.MATMUL_ORDERS, every one a faithful
    # fp32 execution; tests/test_gpu_schedule.py)
    refs = {}
    for key in ("f64",) + tuple(O.MATMUL_ORDERS):
        rs = np.random.RandomState(11)
        ref = R.PPORef(st.astype(np.float64 if key == "f64" else np.float32), cfg, nrm, UPD_KW, rs)
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
    assert logs[0]["tv"] < UPD_KW["adapt_minthresh"] * 0.5 * UPD_KW["eps_ppo"]      # the rate adapts after update 0
    for keep, _ in keeps:                                # no row near the boundary of outside_clip
        assert np.min(np.abs(keep["rdiff"] - np.float32(UPD_KW["eps_ppo"]))) >= 1e-4
        assert keep["steps"] == 12
    actor.s_rms = _Rms(nrm.s_mean, nrm.s_den)
    np.random.seed(0)
    np.random.set_state(np.random.RandomState(11).get_state())
    ppo = PPO(actor, UPD_KW)
    figures = []                                         # (what, device error, fp32 envelope, single-step bar)
    for u, (s, a, adv) in enumerate(data):
        log = ppo.update((s, a, adv, None, None, None))
        assert sorted(log) == sorted(LOG_KEYS)
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
        st_ppo = ppo.engine.ppo_stats(12)
        assert np.array_equal(st_ppo[:, 7], 12 * u + np.arange(1, 13, dtype=np.float32))
    assert float(ppo.actor_lr) == float(ref.actor_lr) and ppo.engine.v["ppo.ctl"][0, 1].item() == 24
    assert float(ppo.alpha) > 0
    r64 = ref.st
    for i, (x, y) in enumerate(zip(actor.get_weights(), r64.trainables(cfg))):
        env = max(float(np.max(np.abs(np.asarray(refs[o][0].st.trainables(cfg)[i], np.float64) - y)))
                  for o in O.MATMUL_ORDERS)
        err = float(np.max(np.abs(np.asarray(x, np.float64).reshape(y.shape) - y)))
        print(f"final weights {y.shape}: device error {err:.2e} fp32 envelope {env:.2e}")
        figures.append((f"final weights {i}", err, env, 1e-6))
    for what, err, env, bar in figures:                  # every figure is printed before the first assertion
        assert env < 1e-2, (what, env)
        assert err <= max(bar, env), (what, err, env)
    ppo.engine.close()


# ---------------------------------------------------------------------------------------------- forms
def _state_bytes(eng, steps=12):
    out = {}
    for name, seg in eng.segments.items():
        if name.startswith("actor"):
            off, n = seg["offset"] // 4, seg["rows"] * seg["cols"]
            for blk in ("params", "adam_m", "adam_v"):
                out[f"{blk}:{name}"] = eng.v[blk][0][off: off + n].cpu().numpy().copy()
    for name in ("ppo.alpha", "ppo.ctl", "ppo.acc"):
        out[name] = eng.v[name].cpu().numpy().copy()
    out["stats"] = eng.ppo_stats(steps)
    return out


@pytest.mark.parametrize("steps,mb", [(12, 33), (72, 16)])
def test_graph_eager_and_single_steps_bit_identical(gpu_available, steps, mb):
    """12 steps replay as graphs of 8, 1, 1, 1, 1; 72 steps as one graph of 64 and one of 8."""
    cfg, st0, nrm = make_state("halfcheetah", 1)
    s, a, adv = rollout(cfg, st0, nrm, 80, 1)
    st = moved(st0, cfg, 1, 0.012)
    idx = np.stack([np.random.RandomState(5 + j).permutation(80)[:mb] for j in range(steps)]).astype(np.int32)
    par = {**R.DEFAULTS, "actor_lr": 3e-4, "max_grad_norm": 0.5, "ent_reg": True, "alpha_lr": 1e-3, "ent_targ": 9.0}
    got = []
    for mode in ("graph", "eager", "single"):
        eng = make_engine("halfcheetah", batch=40, capacity=80)
        load(eng, st0, nrm)
        eng.ppo_begin(s, a, adv)
        load(eng, st, nrm)
        if mode == "single":
            for j in range(steps):
                eng.ppo_steps(idx[j:j + 1], **_pargs(par))
        else:
            eng.ppo_steps(idx, eager=mode == "eager", **_pargs(par))
        eng.sync()
        got.append(_state_bytes(eng, steps))
        out = eng.ppo_end(par["eps_ppo"])
        got[-1]["end"] = np.array([float(out[k]) for k in ("ent", "tv", "kl", "outside_clip", "actor_grad_norm_pre",
                                                           "actor_grad_norm", "alpha")])
        assert out["n_steps"] == steps
        eng.close()
    for other in got[1:]:
        for key in got[0]:
            assert np.array_equal(got[0][key], other[key]), key


def test_inference_only_handle_acts_as_before(gpu_available):
    """An actor_gaussian = 1 handle and the trainable one hold the same actor: the same actions, bit for
    bit, deterministic and sampled (the same stream), and the inference-only layout has no ppo.* segment."""
    cfg, st, nrm = make_state("halfcheetah", 2)
    obs = rollout(cfg, st, nrm, 40, 3)[0]
    outs = []
    for ag in (True, "train"):
        eng = make_engine("halfcheetah", batch=16, capacity=64, actor_gaussian=ag)
        load(eng, st, nrm)
        assert any(n.startswith("ppo.") for n in eng.segments) == (ag == "train")
        eng.rng_set_state(np.random.RandomState(9).get_state())
        outs.append((eng.act(obs, deterministic=True).cpu().numpy(), eng.act(obs, deterministic=False).cpu().numpy(),
                     eng.act(obs[0], deterministic=False).cpu().numpy()))
        eng.close()
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    d = R.forward(st, cfg, nrm, obs)
    assert relerr(outs[0][0], d.mean) < 2e-5


def test_wrong_handle_kinds_fail_and_touch_nothing(gpu_available):
    from sac_eo._native import SacxError
    from sac_eo.engine import Engine, EngineConfig
    cfg, st, nrm = make_state("pendulum", 1)
    s, a, adv = rollout(cfg, st, nrm, 32, 1)
    idx = np.arange(16, dtype=np.int32)[None]
    eng = make_engine("pendulum", batch=16, capacity=32)
    load(eng, st, nrm)
    with pytest.raises(SacxError, match="sacx_ppo_begin first"):
        eng.ppo_steps(idx, eps_ppo=0.2, actor_lr=1e-3)
    eng.ppo_begin(s, a, adv)
    eng.sync()
    before = eng.arena_all.clone()
    with pytest.raises(SacxError, match="trainable GaussianActor handle"):
        eng.step(1)
    with pytest.raises(SacxError, match="outside"):
        eng.ppo_steps(np.arange(17, dtype=np.int32)[None], eps_ppo=0.2, actor_lr=1e-3)      # mb > batch
    with pytest.raises(SacxError, match="index outside"):
        eng.ppo_steps(idx + 17, eps_ppo=0.2, actor_lr=1e-3)
    with pytest.raises(SacxError, match="buffer_capacity"):
        eng.ppo_begin(np.zeros((33, 3), np.float32), np.zeros((33, 1), np.float32), np.zeros(33, np.float32))
    eng.sync()
    assert bool((eng.arena_all == before).all())
    eng.close()
    sac = Engine(EngineConfig(s_dim=3, a_dim=1, hidden=(64, 64), batch=16, buffer_capacity=64, graph_steps=1))
    sac.sync()
    before = sac.arena_all.clone()
    for call in (lambda: sac.ppo_steps(idx, eps_ppo=0.2, actor_lr=1e-3), lambda: sac.ppo_begin(s, a, adv),
                 lambda: sac.neglogp(s, a), lambda: sac.dist(s), lambda: sac.ppo_end(0.2)):
        with pytest.raises(SacxError, match="not a trainable GaussianActor handle"):
            call()
    sac.sync()
    assert bool((sac.arena_all == before).all())
    sac.close()
