"""Nets of any depth and more than two world models on the device, against the oracle (round 6).

The reference builds every net with ``create_nn`` over a ``layers`` list of any length
(sac_eo/common/nn_utils.py:100-138; ``--actor_layers`` / ``--critic_layers`` / ``--model_layers`` /
``--reward_layers`` are ``nargs='+'``, train_parser.py:56-57, :107-108) and fits ``--num_models``
world models in one Adam step (mbrl_onpolicy_alg.py:301-319), the SAC-EO expert term using the
first two of ``np.array_split(perm, num_models)`` (SAC_expert.py:297-336).  Nets of other than two
hidden layers run libsacx's generic plans (every Dense layer a problem of its level's forward /
dX / dW launch, the heads on the row kernels); ``SACX_GENERIC=1`` runs those plans at two layers,
which checks them against the same oracle the fused plans meet.

Compared (fp32 device vs fp64 oracle, the bars of test_gpu_engine.py): one update's four losses
(2e-5 relative) and every gradient through Adam's first moment (2e-4 relative to the tensor's max);
a 60-update graph-replayed trajectory (Q losses 1e-4, alpha loss 1e-3) with the device stream
bit-exact; graph == eager bit for bit; model-fit steps (losses 1e-4, weights 5e-5); the object
calls, the rollout and the diagnostics (2e-5 / 1e-4).

The model count runs to its advertised end, 8, through every entry point, with and without the separate
reward nets (whose layers double the problems of every fit level: from 5 models on each level is two
launches, layer 0 included), at the same bars; the diagnostics at the ends of their row range."""
import numpy as np
import pytest

import sac_oracle as O
from helpers import B1, make_pair, oracle_step, relerr

pytestmark = pytest.mark.gpu


def _same_stream(eng, rs):
    dev, ref = eng.rng_get_state(), rs.get_state()
    return np.array_equal(dev[1], ref[1]) and dev[2] == ref[2] and dev[3] == ref[3] and dev[4] == ref[4]


def _adam_grads(eng, net, B):
    """The gradient of every Dense layer of `net` from Adam's first moment (m_1 = g (1 - beta_1))."""
    m = eng.v["adam_m"][0]
    out = []
    i = 0
    while f"{net}.l{i}" in eng.segments:
        seg = eng.segments[f"{net}.l{i}"]
        off = seg["offset"] // 4
        w = m[off: off + seg["rows"] * seg["cols"]].cpu().numpy().reshape(seg["rows"], seg["cols"]) / B1
        out += [w[:-1], w[-1]]
        i += 1
    return out


CASES = {
    # name: make_pair keyword arguments
    "actor3": dict(hidden=(96, 64, 80)),
    "actor1": dict(hidden=(112,)),
    "critic3": dict(hidden=(64, 64), wm=dict(critic_hidden=(80, 48, 32))),
    "critic1": dict(hidden=(64, 64), wm=dict(critic_hidden=(96,))),
    "all4": dict(hidden=(64, 48, 48, 32), wm=dict(critic_hidden=(64, 64, 32, 48)), act="tanh"),
    "ln3": dict(hidden=(64, 80, 48), layer_norm=True),
    "ln1": dict(hidden=(64,), layer_norm=True),
    "pss3": dict(hidden=(64, 64, 64), per_state_std=True, act="elu"),
    "generic2": dict(hidden=(96, 64), generic=True),
    "eo_models3": dict(hidden=(64, 64), use_expert=True, model_hidden=(96, 64, 80)),
    "eo_models1": dict(hidden=(64, 64, 64), use_expert=True, model_hidden=(128,)),
    "eo_nm3": dict(hidden=(64, 64), use_expert=True, model_hidden=(96, 96), num_models=3, ne=20),
    "eo_nm4_deep": dict(hidden=(48, 64, 48), use_expert=True, model_hidden=(64, 96, 64), num_models=4, ne=16,
                        wm=dict(critic_hidden=(64, 32, 64))),
    "eo_generic2": dict(hidden=(64, 64), use_expert=True, model_hidden=(96, 128), generic=True),
    # the advertised maximum: 8 world models, expert sections of 2 rows each (16 % 8 != 1)
    "eo_nm8": dict(hidden=(64, 64), use_expert=True, model_hidden=(64, 64), num_models=8, ne=16),
}


def _pair(monkeypatch, case, B=64, seed=0, **over):
    kw = dict(CASES[case])
    kw.update(over)
    if kw.pop("generic", False):
        monkeypatch.setenv("SACX_GENERIC", "1")
    kw.setdefault("ne", 12)
    kw.setdefault("act", "relu")
    out = make_pair(B=B, seed=seed, normalizers="random", **kw)
    monkeypatch.delenv("SACX_GENERIC", raising=False)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_one_update_any_depth(gpu_available, monkeypatch, case, B=64):
    eng, ocfg, st, buf, nrm, expert = _pair(monkeypatch, case, B=B, seed=3)
    eo = expert is not None
    nm = eng.cfg.num_models
    N = buf["r"].shape[0]
    rs = np.random.RandomState(17)
    gen = np.random.default_rng(4)
    eng.rng_set_state(rs.get_state())
    R = O.draw_step_randoms(rs, N, B, ocfg.A, n_expert=eng.cfg.expert_batch if eo else 0, gen=gen, n_models=nm)
    if eo and nm > 1:
        eng.push_perms(R["perm"][None])
    keep = {}
    ref = oracle_step(st, ocfg, nrm, buf, R, expert, keep)
    eng.step(1, eager=True)
    eng.sync()
    row = eng.stats(1)[0]
    print(f"update {case} B={B}: launches " + " ".join(p["name"] for p in eng.plan_info()))
    print(f"update {case}: loss errors " + " ".join(f"{abs(row[i] - ref[k]) / abs(ref[k]):.2e}" for i, k in enumerate(
        ("q1_loss", "q2_loss", "p_loss", "alpha_loss"))) + (f" mse {abs(row[5] - ref['mse_loss']) / abs(ref['mse_loss']):.2e}"
                                                           if eo else "") + " (bar 2e-5)")
    for i, k in enumerate(("q1_loss", "q2_loss", "p_loss", "alpha_loss")):
        assert abs(row[i] - ref[k]) <= 2e-5 * abs(ref[k]) + 1e-7, (k, row[i], ref[k])
    if eo:
        assert abs(row[5] - ref["mse_loss"]) <= 2e-5 * abs(ref["mse_loss"]), (row[5], ref["mse_loss"])
    assert np.array_equal(eng.v["slot0.idx"][0].cpu().numpy(), R["idx"])
    assert _same_stream(eng, rs)
    for k in range(2):
        for gd, go in zip(_adam_grads(eng, f"q{k}", B), keep[f"q{k}_grads"]):
            assert relerr(gd, go) < 2e-4, (f"q{k}", relerr(gd, go))
        for a_, b_ in zip(eng.get_net(f"t{k}"), st.q_targ[k]):        # Polyak
            assert np.max(np.abs(a_ - b_)) < 1e-5
    ga = _adam_grads(eng, "actor", B)
    go = list(keep["actor_grads"])
    if ocfg.layer_norm:               # the oracle's list carries gamma / beta after b0; compare the Dense layers
        go = go[:2] + go[4:]
    assert len(ga) == len(go)
    print(f"update {case}: actor gradient error {max(relerr(gd, gr) for gd, gr in zip(ga, go)):.2e} (bar 2e-4)")
    for i, (gd, gr) in enumerate(zip(ga, go)):
        assert relerr(gd, gr) < 2e-4, ("actor", i, relerr(gd, gr))
    eng.close()


@pytest.mark.parametrize("case", ["all4", "eo_nm4_deep", "ln1", "generic2"])
def test_trajectory_any_depth(gpu_available, monkeypatch, case):
    """60 graph-replayed updates (graphs of 8 with the sampler forked ahead, alpha branches folded
    into the next update) against 60 oracle updates; the device stream bit-exact at the end."""
    B = 128
    eng, ocfg, st, buf, nrm, expert = _pair(monkeypatch, case, B=B, seed=11)
    eo = expert is not None
    nm = eng.cfg.num_models
    N = buf["r"].shape[0]
    rs = np.random.RandomState(123)
    gen = np.random.default_rng(77)
    eng.rng_set_state(rs.get_state())
    steps = 60
    Rs = [O.draw_step_randoms(rs, N, B, ocfg.A, n_expert=eng.cfg.expert_batch if eo else 0, gen=gen, n_models=nm)
          for _ in range(steps)]
    if eo:
        eng.push_perms(np.stack([R["perm"] for R in Rs]))
    eng.step(steps)
    eng.sync()
    dev = eng.stats(steps)
    ref = np.array([[o["q1_loss"], o["q2_loss"], o["alpha_loss"]]
                    for o in (oracle_step(st, ocfg, nrm, buf, R, expert) for R in Rs)])
    rel = np.abs(dev[:, :2] - ref[:, :2]) / np.abs(ref[:, :2])
    assert rel.max() < 1e-4, rel.max()
    rel_a = np.abs(dev[:, 3] - ref[:, 2]) / np.abs(ref[:, 2])
    assert rel_a.max() < 1e-3, rel_a.max()
    assert _same_stream(eng, rs)
    eng.close()


@pytest.mark.parametrize("case", ["actor3", "eo_nm3", "critic1"])
def test_graph_equals_eager_any_depth(gpu_available, monkeypatch, case):
    """The generic plan replayed from graphs == the same launches eager, bit for bit (19 updates)."""
    outs = []
    n = 19
    for eager in (True, False):
        eng, ocfg, st, buf, nrm, _ = _pair(monkeypatch, case, B=64, seed=21)
        eng.rng_set_state(np.random.RandomState(5).get_state())
        if eng.cfg.use_expert:
            rs = np.random.RandomState(8)
            eng.push_perms(np.stack([rs.permutation(eng.cfg.expert_batch) for _ in range(n)]))
        eng.step(n, eager=eager)
        eng.sync()
        outs.append((eng.stats(n).copy(), eng.v["params"].cpu().numpy().copy()))
        eng.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])


FIT = {
    "deep3": dict(model_hidden=(96, 64, 80)),
    "one": dict(model_hidden=(128,)),
    "nm3": dict(model_hidden=(96, 96), num_models=3),
    "nm5_clip": dict(model_hidden=(64, 96), num_models=5, model_max_grad_norm=0.05),
    "gauss_reward_deep": dict(model_hidden=(64, 48, 64), num_models=3,
                              wm=dict(gaussian_model=True, scale_model_loss=True, separate_reward_nn=True,
                                      reward_hidden=(48, 32, 40), reward_act="tanh")),
    "reward_mixed_depth": dict(model_hidden=(64,), wm=dict(separate_reward_nn=True, reward_hidden=(32, 48, 40),
                                                           reward_act="elu")),
    # 6 .. 8 models (the advertised range ends at 8).  A launch holds 8 problems: 8 models of 2 / 3 hidden
    # layers are 24 / 32 dW problems (3 / 4 model.adam launches); with reward nets every level holds 2 nm
    # problems, so from 5 models on each forward / backward level is two launches, layer 0 included
    "nm6": dict(model_hidden=(64, 96), num_models=6),
    "nm8": dict(model_hidden=(64, 96), num_models=8),
    "nm8_deep_clip": dict(model_hidden=(64, 48, 64), num_models=8, model_max_grad_norm=0.05),
    "nm5_reward": dict(model_hidden=(64, 96), num_models=5,
                       wm=dict(separate_reward_nn=True, reward_hidden=(32, 48), reward_act="elu")),
    "nm8_gauss_reward_clip": dict(model_hidden=(64,), num_models=8, model_max_grad_norm=0.05,
                                  wm=dict(gaussian_model=True, scale_model_loss=True, separate_reward_nn=True,
                                          reward_hidden=(48, 32, 40), reward_act="tanh")),
}
MAXP = 8      # GEMM problems of one launch (GEMM_MAXP)


def _launches(plan, base):
    """The launches add_gemm_split names `base`, `base`.1, `base`.2, ... in a plan, in order."""
    return [p for p in plan if p["name"] == base or (p["name"].startswith(base + ".") and p["name"][len(base) + 1:].isdigit())]


def _check_fit_plan(eng, ocfg, nm, clip):
    """What the fit plan exposes of its split levels (names and grids; the problems themselves are not
    exposed): one dW launch per 8 of the nm (D + 1) layers of the model nets and of the reward nets;
    with reward nets layer 0 as ceil(2 nm / 8) launches whose grids are the 16x16 tiles of exactly the
    nm model and nm reward layer-0 problems, 8 to a launch in that order."""
    plan = eng.model_plan_info()
    names = [p["name"] for p in plan]
    mb = eng.cfg.model_batch
    dw = "grad" if clip else "adam"
    assert len(_launches(plan, f"model.{dw}")) == -(-nm * (len(ocfg.model_hidden) + 1) // MAXP), names
    if clip:      # the stored gradients' global norm, then ONE Adam over the models' whole range
        assert names.count("model.gnorm") == 1 and names.count("model.adam") == 1, names
    if not ocfg.separate_reward_nn:
        assert not any(n.startswith("reward.") for n in names), names
        return
    assert len(_launches(plan, f"reward.{dw}")) == -(-nm * (len(ocfg.reward_hidden) + 1) // MAXP), names
    tiles = [-(-mb // 16) * -(-h // 16) for h in [ocfg.model_hidden[0]] * nm + [ocfg.reward_hidden[0]] * nm]
    want = [sum(tiles[i: i + MAXP]) for i in range(0, 2 * nm, MAXP)]
    lv0 = _launches(plan, "model.fwd0")
    assert [p["name"] for p in lv0] == ["model.fwd0"] + [f"model.fwd0.{j}" for j in range(1, len(want))], names
    assert [p["grid"] for p in lv0] == want, ([p["grid"] for p in lv0], want)
    assert "model.fwd01" not in names and "model.gather+fwd01" not in names, names
    if 2 * nm > MAXP:      # the heads' dX: the finalisation rides on the first of the two launches
        top = max(len(ocfg.model_hidden), len(ocfg.reward_hidden))
        assert f"model.bwd{top}+final" in names and f"model.bwd{top}.1" in names, names
        assert sum("+final" in n for n in names) == 1, names


@pytest.mark.parametrize("case", list(FIT))
def test_model_fit_any_depth(gpu_available, case):
    """sacx_model_fit of nm models of any depth (and reward nets of another depth): 2 eager steps, 3
    graph-replayed ones, the summed loss of each step and every model variable against the oracle."""
    kw = dict(FIT[case])
    nm = kw.get("num_models", 2)
    max_norm = kw.get("model_max_grad_norm", 0.0)
    eng, ocfg, st, buf, nrm, _ = make_pair(act="relu", hidden=(64, 64), B=64, seed=33, use_expert=True,
                                           normalizers="random", ne=12, **kw)
    N = buf["r"].shape[0]
    mb = eng.cfg.model_batch
    idx = np.random.RandomState(13).randint(N, size=(5, nm, mb))
    eng.model_fit(idx[:2], eager=True)
    eng.model_fit(idx[2:], eager=False)
    eng.sync()
    dev = eng.model_stats(5)
    ref = []
    for j in range(5):
        batches = [(buf["s"][idx[j, k]], buf["a"][idx[j, k]], buf["sp"][idx[j, k]], buf["r"][idx[j, k]])
                   for k in range(nm)]
        ref.append(O.model_fit_step(st, ocfg, nrm, batches, max_grad_norm=max_norm or None))
    ref = np.array(ref)
    werr = max(float(np.max(np.abs(a_ - b_))) for k in range(nm) for a_, b_ in zip(eng.get_net(f"m{k}"), st.models[k]))
    print(f"fit {case}: loss error {np.max(np.abs(dev - ref) / np.abs(ref)):.2e} (bar 1e-4), model weights {werr:.2e} (bar 5e-5)")
    assert np.max(np.abs(dev - ref) / np.abs(ref)) < 1e-4, (dev, ref)
    for k in range(nm):
        for a_, b_ in zip(eng.get_net(f"m{k}"), st.models[k]):
            assert np.max(np.abs(a_ - b_)) < 5e-5
        if ocfg.gaussian_model:
            assert np.max(np.abs(eng.get_model_logstd(k) - st.model_logstd[k])) < 5e-5
        if ocfg.separate_reward_nn:
            for a_, b_ in zip(eng.get_net(f"r{k}"), st.reward_nets[k]):
                assert np.max(np.abs(a_ - b_)) < 5e-5
    assert eng.ctl()["t_model"] == 5
    _check_fit_plan(eng, ocfg, nm, max_norm > 0)
    eng.close()


def _model_bytes(eng, ocfg, nm):
    out = []
    for k in range(nm):
        out += list(eng.get_net(f"m{k}"))
        if ocfg.gaussian_model:
            out.append(eng.get_model_logstd(k))
        if ocfg.separate_reward_nn:
            out += list(eng.get_net(f"r{k}"))
    return [np.array(x, copy=True) for x in out]


@pytest.mark.parametrize("case", ["nm5_reward", "nm8_gauss_reward_clip"])
def test_model_fit_eager_graph_pregather_identical(gpu_available, monkeypatch, case):
    """The same 5 fit steps of 5 / 8 models with reward nets (every level two launches) run eagerly, as
    graph replays, and with the rows gathered per step (SACX_MPRE=0: a gather launch, the layer-0
    launches reading its rows) instead of pre-gathered for the block: the loss of every step and every
    model, logstd and reward-net variable bit for bit."""
    kw = dict(FIT[case])
    nm = kw["num_models"]
    outs = []
    for pre, eager in ((None, True), (None, False), ("0", False)):
        if pre is not None:
            monkeypatch.setenv("SACX_MPRE", pre)
        eng, ocfg, st, buf, nrm, _ = make_pair(act="relu", hidden=(64, 64), B=64, seed=33, use_expert=True,
                                               normalizers="random", ne=12, **kw)
        monkeypatch.delenv("SACX_MPRE", raising=False)
        idx = np.random.RandomState(13).randint(buf["r"].shape[0], size=(5, nm, eng.cfg.model_batch))
        eng.model_fit(idx, eager=eager)
        eng.sync()
        names = [p["name"] for p in eng.model_plan_info()]
        assert ("model.gather" in names) == (pre == "0") and ("model.fwd0.1" in names), names
        _check_fit_plan(eng, ocfg, nm, kw.get("model_max_grad_norm", 0.0) > 0)
        outs.append((eng.model_stats(5).copy(), _model_bytes(eng, ocfg, nm), eng.ctl()["t_model"]))
        eng.close()
    assert np.all(np.isfinite(outs[0][0])) and outs[0][2] == 5
    for other in outs[1:]:
        assert np.array_equal(outs[0][0], other[0]), (outs[0][0], other[0])
        assert len(outs[0][1]) == len(other[1]) and other[2] == 5
        for a_, b_ in zip(outs[0][1], other[1]):
            assert np.array_equal(a_, b_)


def _rows(n, S, A, seed=0):
    r = np.random.RandomState(seed)
    s = (r.normal(size=(n, S)) * 1.5).astype(np.float32)
    a = r.uniform(-1, 1, (n, A)).astype(np.float32)
    sp = (s + r.normal(size=(n, S)) * 0.2).astype(np.float32)
    return s, a, sp


def test_objects_any_depth(gpu_available):
    """actor.evaluate / sample, QCritic._forward / value and MSEModel.sample of nets with 3 / 1 / 4
    hidden layers: within 2e-5 of the oracle, the device stream bit-exact."""
    eng, ocfg, st, buf, nrm, _ = make_pair(act="tanh", hidden=(64, 96, 48), B=64, seed=41, normalizers="random",
                                           use_expert=True, model_hidden=(80, 64, 96, 48), ne=12,
                                           wm=dict(critic_hidden=(72,)))
    S, A = ocfg.S, ocfg.A
    s, a, _ = _rows(1500, S, A, 1)
    rs = np.random.RandomState(19)
    eng.rng_set_state(rs.get_state())
    pi, nlp = [t.cpu().numpy() for t in eng.evaluate(s)]
    rpi, rnlp = O.actor_evaluate(st, ocfg, nrm, s, rs)
    assert relerr(pi, rpi) < 2e-5 and relerr(nlp, rnlp) < 2e-5
    got = np.asarray(eng.act_host(s[:3], False)).reshape(3, A)      # the GEMM path (not the 2-layer rows kernel)
    o, _ = O.actor_forward(st.actor, O._norm(s[:3].astype(np.float64), nrm.s_mean, nrm.s_den), ocfg)
    mu, lraw = O.split_head(o, st.logstd, ocfg)
    ref_a = O.head_sample(mu, lraw, O.f32_noise(rs.normal(size=mu.shape)), ocfg.act_limit, np.float64)[0]
    assert relerr(got, ref_a) < 2e-5
    assert _same_stream(eng, rs)
    for net, params in (("q0", st.q[0]), ("t1", st.q_targ[1])):
        f = eng.critic_forward(net, s, a).cpu().numpy()
        v = eng.critic_forward(net, s, a, value=True).cpu().numpy()
        assert relerr(f, O.critic_forward(params, ocfg, nrm, s, a)) < 2e-5
        assert relerr(v, O.critic_forward(params, ocfg, nrm, s, a, value=True)) < 2e-5
    for k in range(2):
        pred, sp, r = [t.cpu().numpy() for t in eng.model_forward(k, s, a)]
        rp, rsp, rr = O.model_forward(st, ocfg, nrm, k, s, a)
        assert relerr(pred, rp) < 2e-5 and relerr(sp, rsp) < 2e-5 and relerr(r, rr) < 2e-5
    eng.close()


@pytest.mark.parametrize("deterministic", [False, True])
def test_rollout_any_depth(gpu_available, deterministic):
    eng, ocfg, st, buf, nrm, _ = make_pair(act="relu", hidden=(64, 48, 64), B=64, seed=51, use_expert=True,
                                           normalizers="random", model_hidden=(96,), ne=12, num_models=3)
    s0 = (np.random.RandomState(5).normal(size=(300, ocfg.S)) * 1.5).astype(np.float32)
    eng.rng_set_state(np.random.RandomState(23).get_state())
    ref_rs = np.random.RandomState(23)
    got = [t.cpu().numpy() for t in eng.rollout(2, s0, 4, deterministic)]
    ref = O.rollout(st, ocfg, nrm, s0, 4, 2, ref_rs, deterministic)
    for g, r, name in zip(got[:4], ref[:4], ("s", "a", "r", "sp")):
        assert relerr(g, r) < 1e-4, (name, relerr(g, r))
    assert _same_stream(eng, ref_rs)
    eng.close()


@pytest.mark.parametrize("nm,gauss,use_expert_actions", [(3, False, False), (4, True, False), (5, False, True),
                                                         (8, False, False), (8, True, True), (6, False, False)])
def test_expert_diag_many_models(gpu_available, nm, gauss, use_expert_actions):
    """model_MSE_on_expert_data / _counterfactual_action averaged over every model (SAC_expert.py:
    579-608) and _calc_disc (:427-460: every model samples -- GaussianModels draw -- and models 0 / 1
    are compared), with nm world models of 3 hidden layers.  The mean over the models is np.mean of
    the per-model float32 values bit for bit (sequential below 8 values, NumPy's 8-way pairwise block at
    8, one division): a summation order the 1e-4 comparison with the fp64 oracle could not tell apart."""
    eng, ocfg, st, buf, nrm, _ = make_pair(act="relu", hidden=(64, 64), B=64, seed=71, use_expert=True,
                                           normalizers="random", model_hidden=(64, 80, 48), ne=12, num_models=nm,
                                           wm=dict(gaussian_model=gauss) if gauss else None)
    S, A, n = ocfg.S, ocfg.A, 300
    r = np.random.RandomState(9)
    s_e = (r.normal(size=(n, S)) * 2).astype(np.float32)
    a_e = r.uniform(-1, 1, (n, A)).astype(np.float32)
    sp_e = (s_e + r.normal(size=(n, S)) * 0.1).astype(np.float32)
    eng.rng_set_state(np.random.RandomState(29).get_state())
    rs = np.random.RandomState(29)
    got = eng.expert_diag(s_e, a_e, sp_e, use_expert_actions=use_expert_actions)
    m_data, m_cf, per_data, per_cf = O.expert_mse_diag(st, ocfg, nrm, s_e, a_e, sp_e, rs, use_expert_actions)
    assert len(got["mse_expert_data_per_model"]) == nm
    print(f"diag nm={nm} gauss={gauss}: mse {abs(got['mse_expert_data'] - m_data) / abs(m_data):.2e} counterfactual "
          f"{abs(got['mse_counterfactual'] - m_cf) / abs(m_cf):.2e} per model "
          f"{np.max(np.abs(got['mse_expert_data_per_model'] - per_data) / np.abs(per_data)):.2e} / "
          f"{np.max(np.abs(got['mse_counterfactual_per_model'] - per_cf) / np.abs(per_cf)):.2e} (bar 1e-4)")
    assert abs(got["mse_expert_data"] - m_data) <= 1e-4 * abs(m_data)
    assert abs(got["mse_counterfactual"] - m_cf) <= 1e-4 * abs(m_cf)
    assert np.max(np.abs(got["mse_expert_data_per_model"] - per_data) / np.abs(per_data)) < 1e-4
    assert len(got["mse_counterfactual_per_model"]) == nm
    assert np.max(np.abs(got["mse_counterfactual_per_model"] - per_cf) / np.abs(per_cf)) < 1e-4
    for mean, per in (("mse_expert_data", "mse_expert_data_per_model"),
                      ("mse_counterfactual", "mse_counterfactual_per_model")):
        assert got[per].dtype == np.float32
        assert np.float32(got[mean]) == np.mean(got[per]), (mean, got[mean], got[per])
    got_d = eng.expert_diag(s_e, a_e, sp_e, disc=True, use_expert_actions=use_expert_actions)
    ratio, mx, med, tot = O.calc_disc(st, ocfg, nrm, s_e, a_e, rs, use_expert_actions)
    assert abs(got_d["s_disc_total"] - tot) <= 1e-4 * tot
    assert abs(got_d["max_disc"] - mx) <= 1e-4 * mx
    assert relerr(got_d["disc_ratio"], ratio) < 1e-4
    assert _same_stream(eng, rs)
    eng.close()


@pytest.mark.parametrize("nm,gauss", [(8, False), (2, True)])
def test_expert_diag_row_count_edges(gpu_available, nm, gauss):
    """The diagnostics at the ends of their row range [1, 2048]: _calc_disc's bitonic sort around 1024
    and 2048 rows (one thread holds two positions from 1025 rows on; the median of an odd / even count),
    a GaussianModel's noise rows at n = 2048, and the model MSE of 8 models at n = 2048, where model 7's
    rows are the last of the models' output buffer.  2049 rows are refused before anything is drawn."""
    from sac_eo._native import SacxError
    eng, ocfg, st, buf, nrm, _ = make_pair(act="relu", hidden=(64, 64), B=64, seed=73, use_expert=True,
                                           normalizers="random", model_hidden=(64, 48), ne=16, num_models=nm,
                                           wm=dict(gaussian_model=gauss) if gauss else None)
    S, A = ocfg.S, ocfg.A
    r = np.random.RandomState(10)
    s_all = (r.normal(size=(2049, S)) * 2).astype(np.float32)
    a_all = r.uniform(-1, 1, (2049, A)).astype(np.float32)
    sp_all = (s_all + r.normal(size=(2049, S)) * 0.1).astype(np.float32)
    eng.rng_set_state(np.random.RandomState(31).get_state())
    rs = np.random.RandomState(31)
    for n in (1, 2, 1023, 1024, 1025, 2047, 2048):
        s_e, a_e = s_all[:n], a_all[:n]
        got = eng.expert_diag(s_e, a_e, sp_all[:n], disc=True)
        ratio, mx, med, tot = O.calc_disc(st, ocfg, nrm, s_e, a_e, rs)
        errs = (abs(got["s_disc_total"] - tot) / tot, abs(got["max_disc"] - mx) / mx,
                abs(got["median_disc"] - med) / med, relerr(got["disc_ratio"], ratio))
        print(f"nm={nm} gauss={gauss} disc n={n}: total {errs[0]:.2e} max {errs[1]:.2e} median {errs[2]:.2e} "
              f"ratio {errs[3]:.2e}")
        assert got["disc_ratio"].shape == (n,)
        assert max(errs) < 1e-4, (n, errs)
        assert _same_stream(eng, rs), n
    for n in (1, 2048) if nm == 8 else ():
        s_e, a_e, sp_e = s_all[:n], a_all[:n], sp_all[:n]
        got = eng.expert_diag(s_e, a_e, sp_e)
        m_data, m_cf, per_data, per_cf = O.expert_mse_diag(st, ocfg, nrm, s_e, a_e, sp_e, rs)
        assert abs(got["mse_expert_data"] - m_data) <= 1e-4 * abs(m_data)
        assert abs(got["mse_counterfactual"] - m_cf) <= 1e-4 * abs(m_cf)
        assert np.max(np.abs(got["mse_expert_data_per_model"] - per_data) / np.abs(per_data)) < 1e-4
        assert np.max(np.abs(got["mse_counterfactual_per_model"] - per_cf) / np.abs(per_cf)) < 1e-4
        assert np.float32(got["mse_expert_data"]) == np.mean(got["mse_expert_data_per_model"])
        assert np.float32(got["mse_counterfactual"]) == np.mean(got["mse_counterfactual_per_model"])
        assert _same_stream(eng, rs), n
    for disc in (True, False):
        with pytest.raises(SacxError, match=r"\[1, 2048\]"):
            eng.expert_diag(s_all, a_all, sp_all, disc=disc)
        assert _same_stream(eng, rs)
    eng.close()


@pytest.mark.parametrize("nm,k,reward", [(8, 7, False), (5, 4, True)])
@pytest.mark.parametrize("deterministic", [False, True])
def test_rollout_through_the_last_model(gpu_available, deterministic, nm, k, reward):
    """sacx_rollout with the LAST world model as the environment: model 7 of 8, and model 4 of 5 with
    its separate reward net in the same launches."""
    eng, ocfg, st, buf, nrm, _ = make_pair(act="relu", hidden=(64, 48, 64), B=64, seed=53, use_expert=True,
                                           normalizers="random", model_hidden=(96,), ne=2 * nm, num_models=nm,
                                           wm=dict(separate_reward_nn=True, reward_hidden=(32, 48), reward_act="elu")
                                           if reward else None)
    s0 = (np.random.RandomState(5).normal(size=(300, ocfg.S)) * 1.5).astype(np.float32)
    eng.rng_set_state(np.random.RandomState(23).get_state())
    ref_rs = np.random.RandomState(23)
    got = [t.cpu().numpy() for t in eng.rollout(k, s0, 4, deterministic)]
    ref = O.rollout(st, ocfg, nrm, s0, 4, k, ref_rs, deterministic)
    print(f"rollout model {k} of {nm} reward={reward} det={deterministic}: " +
          " ".join(f"{name} {relerr(g, r):.2e}" for g, r, name in zip(got[:4], ref[:4], ("s", "a", "r", "sp"))) + " (bar 1e-4)")
    for g, r, name in zip(got[:4], ref[:4], ("s", "a", "r", "sp")):
        assert relerr(g, r) < 1e-4, (name, relerr(g, r))
    assert _same_stream(eng, ref_rs)
    # the same rows through another model differ by far more than the bar: the index reached the launches
    other = O.rollout(st, ocfg, nrm, s0, 4, 0, np.random.RandomState(23), deterministic)
    assert relerr(got[3], other[3]) > 1e-2
    eng.close()


def test_model_forward_of_eight_models(gpu_available):
    """MSEModel.sample of models 0, 5 and 7 of an 8-model engine: each reads its own weights."""
    eng, ocfg, st, buf, nrm, _ = make_pair(act="relu", hidden=(64, 64), B=64, seed=43, use_expert=True,
                                           normalizers="random", model_hidden=(64, 96), ne=16, num_models=8)
    s, a, _ = _rows(700, ocfg.S, ocfg.A, 2)
    refs = {}
    for k in (0, 5, 7):
        pred, sp, r = [t.cpu().numpy() for t in eng.model_forward(k, s, a)]
        rp, rsp, rr = refs[k] = O.model_forward(st, ocfg, nrm, k, s, a)
        print(f"model_forward {k} of 8: pred {relerr(pred, rp):.2e} sp {relerr(sp, rsp):.2e} r {relerr(r, rr):.2e} (bar 2e-5)")
        assert relerr(pred, rp) < 2e-5 and relerr(sp, rsp) < 2e-5 and relerr(r, rr) < 2e-5, k
    assert relerr(refs[5][0], refs[7][0]) > 1e-2 and relerr(refs[0][0], refs[7][0]) > 1e-2
    eng.close()


def test_generic_plan_is_taken(gpu_available, monkeypatch):
    """The plan a deep handle runs: every hidden layer its own forward problem, the row-kernel heads
    (k_actor_head / k_qhead / k_actor_bwd), no fused launch names; the default depth keeps the fused
    plan (8 launches per update for plain SAC)."""
    eng, *_ = _pair(monkeypatch, "actor3")
    names = [p["name"] for p in eng.plan_info()]
    for n in ("actor.fwd0", "actor.fwd1", "actor.fwd2", "actor.head", "q.head", "pi.q.head", "actor.head.bwd",
              "actor.bwd2", "actor.bwd1", "actor.adam", "critic.adam", "alpha.final"):
        assert n in names, (n, names)
    assert not any("+" in n for n in names), names
    eng.close()
    eng, *_ = make_pair(hidden=(64, 64), B=64, seed=1)
    names = [p["name"] for p in eng.plan_info()]
    assert "q.fwd01+actor.head" in names and "actor.head" not in names, names
    eng.close()
