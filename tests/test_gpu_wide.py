"""Hidden layers 513 .. 1,024 wide on the device, against the oracle.

A handle with a layer above 512 in a used net runs the generic plans (test_gpu_depth.py): every Dense
layer a GEMM problem, the heads on the row kernels' wide variants, which walk a row in two slabs of
512 columns (k_actor_head<16>, k_qhead_wide, k_actor_bwd_wide, k_ln_wide).  The bodies and the bars are
those of test_gpu_depth.py / test_gpu_bc.py / test_gpu_loop.py (called as they are, with the wide
cases entered into their tables), at the smallest shapes that reach each slab boundary: B = 64,
S = 17, A = 6; widths 520 (a 9th, partly filled register), 600 / 776 / 1,000 (ragged middles) and
1,024 (two full slabs).  The fp32 oracle against itself in fp64 at these shapes differs by 1e-8 ..
3e-7 on the losses and 3e-7 .. 6e-7 on the gradients, as at 512 x 2: the bars are not widened."""
import ctypes

import numpy as np
import pytest

import sac_oracle as O
import test_gpu_bc as BC
import test_gpu_depth as D
import test_gpu_loop as L
from bc_oracle import bc_update
from helpers import load_learner, make_learner, make_pair, oracle_step, relerr

pytestmark = pytest.mark.gpu

WIDE = {
    "actor_wide": dict(hidden=(520, 1024)),
    "critic_wide": dict(hidden=(64, 64), wm=dict(critic_hidden=(1024, 520))),
    "ln_wide": dict(hidden=(776, 64), layer_norm=True),
    "pss_wide": dict(S=40, A=17, hidden=(64, 1000), per_state_std=True, act="elu"),
    "eo_wide": dict(hidden=(64, 64), use_expert=True, model_hidden=(1024, 600), ne=12),
    "all1024": dict(hidden=(1024, 1024), wm=dict(critic_hidden=(1024, 1024)), use_expert=True,
                    model_hidden=(1024, 1024), ne=12),
    "one_wide_layer": dict(hidden=(1024,)),
}


def _enter(monkeypatch, case):
    monkeypatch.setitem(D.CASES, case, WIDE[case])


@pytest.mark.parametrize("case", list(WIDE))
def test_one_update_wide(gpu_available, monkeypatch, case):
    """One update vs the fp64 oracle: the four losses, the MSE term, the sampler's indices, the stream,
    every gradient through Adam's first moment, Polyak (the body of test_one_update_any_depth)."""
    _enter(monkeypatch, case)
    D.test_one_update_any_depth(gpu_available, monkeypatch, case)


@pytest.mark.parametrize("case", ["all1024", "ln_wide"])
def test_trajectory_wide(gpu_available, monkeypatch, case):
    """60 graph-replayed updates at B = 128 (the body of test_trajectory_any_depth)."""
    _enter(monkeypatch, case)
    D.test_trajectory_any_depth(gpu_available, monkeypatch, case)


@pytest.mark.parametrize("case", ["critic_wide", "eo_wide"])
def test_graph_equals_eager_wide(gpu_available, monkeypatch, case):
    _enter(monkeypatch, case)
    D.test_graph_equals_eager_any_depth(gpu_available, monkeypatch, case)


def test_wide_handle_takes_the_generic_plan(gpu_available):
    """Every net two layers deep and one of them wide: the generic launch names and no fused one; the
    same handle with 512-wide models keeps the fused plan."""
    eng, *_ = make_pair(B=64, seed=1, normalizers="random", **WIDE["eo_wide"])
    info = eng.plan_info()
    names = [p["name"] for p in info]
    for n in ("actor.fwd0", "actor.fwd1", "actor.head", "q.fwd0", "q.fwd1", "model.head", "q.head", "pi.q.head",
              "model.bwd2", "model.bwd1", "actor.head.bwd", "actor.bwd1", "actor.adam", "critic.adam", "alpha.final"):
        assert n in names, (n, names)
    assert not any("+" in n for n in names), names
    kern = [p["kernel"] for p in info]
    assert "k_fwd2" not in kern, kern
    eng.close()
    kw = dict(WIDE["eo_wide"], model_hidden=(512, 512))
    eng, *_ = make_pair(B=64, seed=1, normalizers="random", **kw)
    names = [p["name"] for p in eng.plan_info()]
    assert any("+" in n for n in names) and "actor.head.bwd" not in names, names
    eng.close()


FIT = {
    "wide2": dict(model_hidden=(1024, 1024)),
    "nm3_clip": dict(model_hidden=(520, 1024), num_models=3, model_max_grad_norm=0.05),
    "gauss_reward": dict(model_hidden=(600,), wm=dict(gaussian_model=True, scale_model_loss=True,
                                                      separate_reward_nn=True, reward_hidden=(1024, 40),
                                                      reward_act="tanh")),
}


@pytest.mark.parametrize("case", list(FIT))
def test_model_fit_wide(gpu_available, monkeypatch, case):
    """2 eager + 3 replayed fit steps, losses 1e-4, weights 5e-5 (the body of test_model_fit_any_depth)."""
    monkeypatch.setitem(D.FIT, case, FIT[case])
    D.test_model_fit_any_depth(gpu_available, case)
    # the fit plan of a wide handle: no k_fwd2 pair, no gather fold
    eng, *_ = make_pair(act="relu", hidden=(64, 64), B=64, seed=33, use_expert=True, normalizers="random", ne=12,
                        **FIT[case])
    plan = eng.model_plan_info()
    eng.close()
    assert plan and not any(p["kernel"] == "k_fwd2" or "fwd01" in p["name"] or "gather+" in p["name"] for p in plan), plan


OBJ = dict(hidden=(1024, 520), wm=dict(critic_hidden=(776,)), model_hidden=(1024, 1024))


def test_objects_wide(gpu_available):
    """evaluate, act (the GEMM path: first layer 1,024 of a 2-layer actor goes to k_act_rows, so 4 rows
    of a 1,500-row call and a batched call are both made), critic_forward / value, model_forward:
    2e-5, the stream bit-exact (the body of test_objects_any_depth)."""
    eng, ocfg, st, buf, nrm, _ = make_pair(act="tanh", B=64, seed=41, normalizers="random", use_expert=True, ne=12,
                                           **OBJ)
    S, A = ocfg.S, ocfg.A
    s, a, _ = D._rows(1500, S, A, 1)
    rs = np.random.RandomState(19)
    eng.rng_set_state(rs.get_state())
    pi, nlp = [t.cpu().numpy() for t in eng.evaluate(s)]
    rpi, rnlp = O.actor_evaluate(st, ocfg, nrm, s, rs)
    assert relerr(pi, rpi) < 2e-5 and relerr(nlp, rnlp) < 2e-5
    for rows in (3, 40):            # k_act_rows (<= 16 rows), then the per-layer GEMMs + k_actor_head
        got = np.asarray(eng.act_host(s[:rows], False)).reshape(rows, A)
        o, _ = O.actor_forward(st.actor, O._norm(s[:rows].astype(np.float64), nrm.s_mean, nrm.s_den), ocfg)
        mu, lraw = O.split_head(o, st.logstd, ocfg)
        ref_a = O.head_sample(mu, lraw, O.f32_noise(rs.normal(size=mu.shape)), ocfg.act_limit, np.float64)[0]
        assert relerr(got, ref_a) < 2e-5, rows
    assert D._same_stream(eng, rs)
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
def test_rollout_wide(gpu_available, deterministic):
    eng, ocfg, st, buf, nrm, _ = make_pair(act="relu", B=64, seed=51, use_expert=True, normalizers="random", ne=12,
                                           **OBJ)
    s0 = (np.random.RandomState(5).normal(size=(300, ocfg.S)) * 1.5).astype(np.float32)
    eng.rng_set_state(np.random.RandomState(23).get_state())
    ref_rs = np.random.RandomState(23)
    got = [t.cpu().numpy() for t in eng.rollout(1, s0, 4, deterministic)]
    ref = O.rollout(st, ocfg, nrm, s0, 4, 1, ref_rs, deterministic)
    for g, r, name in zip(got[:4], ref[:4], ("s", "a", "r", "sp")):
        assert relerr(g, r) < 1e-4, (name, relerr(g, r))
    assert D._same_stream(eng, ref_rs)
    eng.close()


@pytest.mark.parametrize("use_expert_actions", [False, True])
def test_expert_diag_wide(gpu_available, use_expert_actions):
    """The body of test_expert_diag_many_models with 2 wide world models."""
    eng, ocfg, st, buf, nrm, _ = make_pair(act="relu", B=64, seed=71, use_expert=True, normalizers="random", ne=12,
                                           num_models=2, **OBJ)
    S, A, n = ocfg.S, ocfg.A, 300
    r = np.random.RandomState(9)
    s_e = (r.normal(size=(n, S)) * 2).astype(np.float32)
    a_e = r.uniform(-1, 1, (n, A)).astype(np.float32)
    sp_e = (s_e + r.normal(size=(n, S)) * 0.1).astype(np.float32)
    eng.rng_set_state(np.random.RandomState(29).get_state())
    rs = np.random.RandomState(29)
    got = eng.expert_diag(s_e, a_e, sp_e, use_expert_actions=use_expert_actions)
    m_data, m_cf, per_data, per_cf = O.expert_mse_diag(st, ocfg, nrm, s_e, a_e, sp_e, rs, use_expert_actions)
    assert len(got["mse_expert_data_per_model"]) == 2
    assert abs(got["mse_expert_data"] - m_data) <= 1e-4 * abs(m_data)
    assert abs(got["mse_counterfactual"] - m_cf) <= 1e-4 * abs(m_cf)
    assert np.max(np.abs(got["mse_expert_data_per_model"] - per_data) / np.abs(per_data)) < 1e-4
    got_d = eng.expert_diag(s_e, a_e, sp_e, disc=True, use_expert_actions=use_expert_actions)
    ratio, mx, med, tot = O.calc_disc(st, ocfg, nrm, s_e, a_e, rs, use_expert_actions)
    assert abs(got_d["s_disc_total"] - tot) <= 1e-4 * tot
    assert abs(got_d["max_disc"] - mx) <= 1e-4 * mx
    assert relerr(got_d["disc_ratio"], ratio) < 1e-4
    assert D._same_stream(eng, rs)
    eng.close()


@pytest.mark.parametrize("hidden,kernel", [((1024, 1024), "rows"), ((1024, 520, 64), "gemm")])
def test_act_b1_wide(gpu_available, hidden, kernel):
    """The env loop's act on 3 rows, deterministic and sampled: two wide layers without layer norm take
    k_act_rows (its LDS vectors hold 1,024; never run above 512 before), three layers the per-layer
    GEMMs and the wide k_actor_head.  2e-5 of the oracle, the stream bit-exact."""
    eng, ocfg, st, buf, nrm, _ = make_pair(act="tanh", hidden=hidden, B=64, seed=43, normalizers="random")
    S, A = ocfg.S, ocfg.A
    s, _, _ = D._rows(3, S, A, 2)
    rs = np.random.RandomState(31)
    eng.rng_set_state(rs.get_state())
    o, _ = O.actor_forward(st.actor, O._norm(s.astype(np.float64), nrm.s_mean, nrm.s_den), ocfg)
    mu, lraw = O.split_head(o, st.logstd, ocfg)
    det = np.asarray(eng.act_host(s, True)).reshape(3, A)
    assert relerr(det, ocfg.act_limit * np.tanh(mu)) < 2e-5
    assert D._same_stream(eng, rs)                        # a deterministic act draws nothing
    got = np.asarray(eng.act_host(s, False)).reshape(3, A)
    ref_a = O.head_sample(mu, lraw, O.f32_noise(rs.normal(size=mu.shape)), ocfg.act_limit, np.float64)[0]
    assert relerr(got, ref_a) < 2e-5
    assert D._same_stream(eng, rs)
    eng.close()


BC_WIDE = dict(hidden=(520, 1024), model_hidden=(1024, 600), ne=20)


def test_bc_one_update_wide(gpu_available, monkeypatch):
    monkeypatch.setitem(BC.CASES, "wide", BC_WIDE)
    BC.test_bc_one_update(gpu_available, monkeypatch, "wide")


def test_bc_trajectory_wide(gpu_available, monkeypatch):
    """40 graph-replayed BC updates: the MSE series within 1e-4 of its scale, the stream bit-exact (the
    body of test_bc_trajectory)."""
    monkeypatch.setitem(BC.CASES, "wide", BC_WIDE)
    eng, ocfg, st, nrm, mn, expert = BC._pair(monkeypatch, "wide", seed=11)
    nm, A = eng.cfg.num_models, ocfg.A
    rs, gen = np.random.RandomState(123), np.random.default_rng(77)
    eng.rng_set_state(rs.get_state())
    steps = 40
    draws = [BC._draw(rs, gen, expert, nm, A) for _ in range(steps)]
    eng.push_perms(np.stack([p for p, _ in draws]))
    eng.step(steps)
    eng.sync()
    dev = eng.stats(steps)
    ref = np.array([bc_update(st, ocfg, nrm, h, mn)["mse_loss"] for _, h in draws])
    err = L._series_err(dev[:, 5], ref)
    print(f"bc wide: MSE series error {err:.2e}")
    assert err < L.LOSS_TOL, err
    assert np.array_equal(dev[:, 5], dev[:, 2]) and np.array_equal(dev[:, 7], np.arange(steps, dtype=np.float32))
    assert D._same_stream(eng, rs)
    assert eng.ctl()["t_sac"] == steps
    eng.close()


def test_packed_seeds_wide(gpu_available, hidden=(64, 1024)):
    """seeds = 2, hidden (64, 1024): each seed's 10-update statistics, parameters, second moments and
    RNG key bit-identical to the same learner run alone (test_packed_seeds_equal_single's comparison).
    hidden: another caller's widths (tests/test_gpu_ragged.py)."""
    from sac_eo.engine import Engine, EngineConfig
    n, B, N, K = 10, 64, 2000, 2
    learners = [make_learner(hidden=hidden, act="tanh", B=B, N=N, seed=40 + 7 * k) for k in range(K)]

    def cfg(seeds):
        return EngineConfig(s_dim=17, a_dim=6, hidden=hidden, activation="tanh", batch=B, buffer_capacity=N,
                            graph_steps=8, seeds=seeds)

    def drive(eng, k):
        _, st, buf, nrm, ex = learners[k]
        load_learner(eng, st, buf, nrm, ex, 0.1)
        eng.rng_set_state(np.random.RandomState(500 + k).get_state())

    packed = Engine(cfg(K))
    for k in range(K):
        packed.select_seed(k)
        drive(packed, k)
    packed.select_seed(0)
    packed.step(n)
    packed.sync()
    got = []
    for k in range(K):
        packed.select_seed(k)
        got.append((packed.stats(n).copy(), packed.v["params"].cpu().numpy().copy(),
                    packed.v["adam_v"].cpu().numpy().copy(), packed.rng_get_state()[1].copy()))
    packed.close()
    for k in range(K):
        e = Engine(cfg(1))
        drive(e, k)
        e.step(n)
        e.sync()
        ref = (e.stats(n), e.v["params"].cpu().numpy(), e.v["adam_v"].cpu().numpy(), e.rng_get_state()[1])
        e.close()
        for i, (a, b) in enumerate(zip(got[k], ref)):
            assert np.array_equal(a, b), (k, i)
    assert np.all(np.isfinite(got[0][0]))
    assert not np.array_equal(got[0][1], got[1][1])


def test_bf16_trajectory_wide(gpu_available):
    """gemm_bf16 on the all-1,024 handle: 30 updates' Q losses within the 5e-3 bar of
    test_humanoid_bf16_trajectory, the stream bit-exact."""
    B, steps = 64, 30
    eng, ocfg, st, buf, nrm, expert = make_pair(B=B, seed=37, normalizers="random", gemm_bf16=True, **WIDE["all1024"])
    N = buf["r"].shape[0]
    rs = np.random.RandomState(77)
    gen = np.random.default_rng(5)
    eng.rng_set_state(rs.get_state())
    Rs = [O.draw_step_randoms(rs, N, B, ocfg.A, n_expert=eng.cfg.expert_batch, gen=gen, n_models=2)
          for _ in range(steps)]
    eng.push_perms(np.stack([R["perm"] for R in Rs]))
    eng.step(steps)
    eng.sync()
    dev = eng.stats(steps)
    ref = np.array([[o["q1_loss"], o["q2_loss"]] for o in (oracle_step(st, ocfg, nrm, buf, R, expert) for R in Rs)])
    rel = np.abs(dev[:, :2] - ref) / np.abs(ref)
    print("wide bf16 q-loss max rel err", rel.max(), "median", np.median(rel))
    assert rel.max() < 5e-3, rel.max()
    assert D._same_stream(eng, rs)
    eng.close()


@pytest.mark.parametrize("alg,flags", [
    ("sac_imit", ["--model_layers", "1024", "520"]),
    ("sac", ["--critic_layers", "1024", "1024"]),
])
def test_train_loop_wide(gpu_available, alg, flags):
    """The parser -> init_* -> engine path and the training loop at test_gpu_loop's SMALL shape."""
    L.test_train_loop_matches_oracle(gpu_available, alg, flags)


def test_width_limit_launches_nothing(gpu_available):
    """Width 1,025: EngineConfig raises, sacx_create returns an error naming the bound; no handle, no
    arena, no launch."""
    from sac_eo import _native as N
    from sac_eo.engine import Engine, EngineConfig
    with pytest.raises(NotImplementedError):
        Engine(EngineConfig(s_dim=17, a_dim=6, hidden=(1025, 64), buffer_capacity=1000))
    c = EngineConfig(s_dim=17, a_dim=6, hidden=(1024, 64), buffer_capacity=1000).to_c()
    c.net_hidden[0][0] = 1025
    lib = N.lib()
    h = ctypes.c_void_p()
    assert lib.sacx_create(ctypes.byref(c), ctypes.byref(h)) != 0
    assert b"1024" in lib.sacx_last_error(None) and not h.value
