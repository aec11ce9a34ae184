"""alg_type bc on the CPU: the BC update's reference arithmetic and the host side.

* ``bc_oracle.bc_update`` (BC.py:309-363 from the oracle's primitives) against
  ``sac_oracle.sac_update`` with ``Expert.epsilon = 1.0`` -- the committed oracle is BC's parity
  reference: the policy rows carry weight ``1 - epsilon = 0`` -- and against a torch-autograd gradient
  of the BC loss written out directly (fp64);
* ``init_alg('bc')``, ``EngineConfig(bc=True)``, ``sacx_create``'s accepted / rejected combinations;
* the BC loop on the stand-in engine (tests/fake_engine_bc.py): the log's keys and counts, the
  checkpoint, ``sac_eo.train.main`` and the global stream against ``BCLoopOracle``'s.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import sac_oracle as O
from bc_oracle import BCLoopOracle, bc_sections, bc_update
from helpers import make_learner, relerr

CASES = {
    "two_layer": dict(hidden=(32, 24), model_hidden=(40, 40)),
    "ln3": dict(hidden=(24, 32, 16), model_hidden=(40, 24), layer_norm=True),
    "per_state_std": dict(hidden=(24, 24), model_hidden=(32, 32), per_state_std=True, act="elu"),
    "one_model": dict(hidden=(24, 24), model_hidden=(32, 32), num_models=1, ne=11),
}


def _learner(case, seed=5):
    kw = dict(CASES[case])
    kw.setdefault("ne", 12)
    kw.setdefault("act", "relu")
    ocfg, st, buf, nrm, expert = make_learner(S=7, A=3, B=16, N=100, seed=seed, use_expert=True, normalizers="random",
                                              epsilon=1.0, **kw)
    return ocfg, st.astype(np.float64), buf, nrm, expert


def _halves(R, expert):
    noises = [R["noise_e1"]] + ([R["noise_e2"]] if R["noise_e2"] is not None else [])
    return [(expert["s"][sec], expert["sp"][sec], O.f32_noise(u)) for sec, u in zip(R["sections"], noises)]


@pytest.mark.parametrize("case", list(CASES))
def test_bc_update_is_sac_update_at_epsilon_one(case):
    ocfg, st, buf, nrm, expert = _learner(case)
    nm = ocfg.num_models
    rs = np.random.RandomState(3)
    R = O.draw_step_randoms(rs, 100, 16, ocfg.A, n_expert=len(expert["s"]), gen=np.random.default_rng(2), n_models=nm)
    a, b = st.copy(), st.copy()
    halves = _halves(R, expert)
    ex = O.Expert(halves[0][0], halves[0][1], halves[1][0] if nm > 1 else None, halves[1][1] if nm > 1 else None,
                  halves[0][2], halves[1][2] if nm > 1 else None, 1.0)
    ref = O.sac_update(a, ocfg, nrm, O.gather(buf, R["idx"]), O.f32_noise(R["noise_t"]), O.f32_noise(R["noise_pi"]),
                       O.f32_noise(R["noise_alpha"]), expert=ex)
    got = bc_update(b, ocfg, nrm, halves)
    assert abs(got["mse_loss"] - ref["mse_loss"]) <= 1e-12 * abs(ref["mse_loss"])
    assert ref["p_loss"] == ref["mse_loss"]                  # (1 - 1) p + 1 mse
    for x, y in zip(b.actor + [b.logstd] + b.opt_actor.m + b.opt_actor.v,
                    a.actor + [a.logstd] + a.opt_actor.m + a.opt_actor.v):
        assert relerr(x, y) <= 1e-12
    assert b.opt_actor.t == a.opt_actor.t == 1
    # bc_update moves the actor alone
    for x, y in zip(b.q[0] + b.q[1] + b.q_targ[0] + b.q_targ[1] + [b.alpha] + b.models[0],
                    st.q[0] + st.q[1] + st.q_targ[0] + st.q_targ[1] + [st.alpha] + st.models[0]):
        assert np.array_equal(x, y)


def _act_t(x, kind):
    return torch.relu(x) if kind == "relu" else torch.tanh(x) if kind == "tanh" else torch.nn.functional.elu(x)


def _mlp_t(params, x, acts):
    n = len(params) // 2
    for i in range(n):
        x = x @ params[2 * i] + params[2 * i + 1]
        if i < n - 1:
            x = _act_t(x, acts[i] if not isinstance(acts, str) else acts)
    return x


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("clip", [0.0, 0.4])
def test_bc_gradient_is_autograd_of_the_loss(case, clip):
    """BC.py:318-356 written out in torch (fp64) and differentiated by autograd."""
    ocfg, st, buf, nrm, expert = _learner(case, seed=9)
    ocfg.delta_clip_pred = clip
    nm = ocfg.num_models
    rs = np.random.RandomState(8)
    perm = np.arange(len(expert["s"]))
    if nm > 1:
        np.random.default_rng(6).shuffle(perm)
    halves = [(expert["s"][sec], expert["sp"][sec], O.f32_noise(rs.normal(size=(len(sec), ocfg.A))))
              for sec in bc_sections(perm, nm)]
    keep = {}
    got = bc_update(st.copy(), ocfg, nrm, halves, keep=keep)

    T = lambda x, g=False: torch.tensor(np.asarray(x, np.float64), requires_grad=g)
    actor = [T(w, True) for w in st.actor]
    logstd = T(st.logstd, True)
    n64 = nrm.cast(np.float64)
    sq = 0.0
    for k, (se, spe, u) in enumerate(halves):
        se, spe, u = T(se), T(spe), T(u)
        x = (se - T(n64.s_mean)) / T(n64.s_den)
        if ocfg.layer_norm:                                     # Dense -> LayerNorm(1e-3) -> tanh, then the rest
            z = x @ actor[0] + actor[1]
            xh = (z - z.mean(-1, keepdim=True)) / torch.sqrt(z.var(-1, unbiased=False, keepdim=True) + 1e-3)
            out = _mlp_t(actor[4:], torch.tanh(actor[2] * xh + actor[3]), ocfg.aacts[1:])
        else:
            out = _mlp_t(actor, x, ocfg.aacts)
        mu, lraw = (out[:, :ocfg.A], out[:, ocfg.A:]) if ocfg.per_state_std else (out, logstd.expand_as(out))
        a = ocfg.act_limit * torch.tanh(mu + torch.exp(torch.clamp(lraw, -5.0, 2.0)) * u)
        xm = torch.cat([x, (a - T(n64.a_mean)) / T(n64.a_den)], -1)
        dn = _mlp_t([T(w) for w in st.models[k]], xm, ocfg.model_act)[:, :ocfg.S]
        if clip:
            dn = torch.clamp(dn, -clip, clip)
        sq = sq + ((spe - (se + dn * T(n64.d_den) + T(n64.d_mean))) ** 2).sum(-1)
    loss = (0.5 * sq).mean()
    loss.backward()
    assert abs(got["mse_loss"] - loss.item()) <= 1e-12 * abs(loss.item())
    assert any(np.abs(g).max() > 0 for g in keep["actor_grads"])
    for g, p in zip(keep["actor_grads"], actor):
        assert relerr(g.reshape(p.shape), p.grad.numpy()) <= 1e-10
    if ocfg.per_state_std:
        assert logstd.grad is None and not np.any(keep["g_logstd"])
    else:
        assert relerr(keep["g_logstd"], logstd.grad.numpy()) <= 1e-10


# ------------------------------------------------------------------------------ public interface
def test_engine_config_bc_writes_use_expert_2():
    from sac_eo import _native as N
    from sac_eo.engine import EngineConfig
    c = EngineConfig(s_dim=17, a_dim=6, bc=True)
    assert c.use_expert is True                    # bc implies the expert path
    assert c.to_c().use_expert == N.EXPERT_BC == 2
    assert EngineConfig(s_dim=17, a_dim=6, use_expert=True).to_c().use_expert == 1
    assert EngineConfig(s_dim=17, a_dim=6).to_c().use_expert == 0


def _create(**over):
    """sacx_create alone (host only: no arena, no device)."""
    from sac_eo import _native as N
    from sac_eo.engine import EngineConfig
    c = EngineConfig(s_dim=17, a_dim=6, bc=True, buffer_capacity=1000).to_c()
    for k, v in over.items():
        setattr(c, k, v)
    lib = N.lib()
    h = ctypes.c_void_p()
    rc = lib.sacx_create(ctypes.byref(c), ctypes.byref(h))
    msg = lib.sacx_last_error(None)
    if rc == 0:
        lib.sacx_destroy(h)
    return rc, (msg or b"").decode()


def test_sacx_create_accepts_bc_and_rejects_what_it_does_not_run():
    assert _create()[0] == 0
    rc, msg = _create(gemm_bf16=1)
    assert rc != 0 and "bf16" in msg and "BC" in msg
    rc, msg = _create(seeds=2)
    assert rc != 0 and "seeds" in msg and "BC" in msg
    rc, msg = _create(use_expert=3)
    assert rc != 0 and "use_expert" in msg
    assert _create(use_expert=1, seeds=2)[0] == 0            # SAC-EO keeps its packed seeds


# ------------------------------------------------------------------------------ host loop
def _argv(tmp, extra=()):
    return ["--alg_type", "bc", "--env_name", "HalfCheetah-v3", "--actor_layers", "16", "16", "--critic_layers", "16",
            "16", "--model_layers", "16", "16", "--total_timesteps", "700", "--env_batch_size_init", "300",
            "--env_horizon", "200", "--sac_batch_size", "32", "--model_batch_size", "50", "--model_num_epochs", "1",
            "--seed", "3", "--save_path", str(tmp)] + list(extra)


@pytest.mark.parametrize("extra", [(), ("--num_models", "3"), ("--num_models", "1", "--expert_batch_size", "7")])
def test_bc_main_on_the_stand_in_engine(monkeypatch, tmp_path, extra):
    import fake_engine_bc
    fake_engine_bc.install(monkeypatch)
    from sac_eo.common.logger import load_log
    from sac_eo.train import main
    log = load_log(main(_argv(tmp_path, extra)))[0]
    tr = log["train"]
    assert len(tr["BC_MSE_loss"]) == 700 - 300               # one update per env step after the collection
    assert np.all(np.asarray(tr["BC_MSE_loss"]) == np.float32(2.0))
    for k in ("alpha_loss", "p_loss", "epsilon", "q1_loss", "q2_loss"):
        assert k not in tr, k
    for k in ("model_MSE_on_expert_data", "model_MSE_on_expert_counterfactual_action", "model_loss_last",
              "model_updates", "expert_J_tot"):
        assert k in tr, k
    assert len(tr["model_MSE_on_expert_data"]) == 1          # one 1000-step episode: one model fit
    assert "final" in log                                     # the checkpoint's parameter dump


def test_init_alg_bc_and_the_loops_stream(monkeypatch):
    """init_alg('bc') builds a BC whose engine is configured for BC; its loop on the stand-in engine
    leaves the global stream where BCLoopOracle's leaves it (the same draws in the same order: acts,
    model-fit shuffles, counterfactual actions, the expert batch pick and the updates' expert normals;
    a stray randint or policy-noise draw would move it)."""
    import fake_engine_bc
    fake_engine_bc.install(monkeypatch)
    import test_gpu_loop as L
    from sac_eo.algs import BC, SAC_exp
    from sac_eo.common.logger import load_log
    flags = ["--num_models", "3", "--expert_batch_size", "11"]       # sections 4 / 4 / 3: 8 rows used
    alg_obj, d, ak, total, oenvs, rs_state = L._build("bc", flags)
    assert type(alg_obj) is BC and isinstance(alg_obj, SAC_exp)
    assert alg_obj.engine.cfg.bc and alg_obj.engine.cfg.use_expert
    S, A = alg_obj.s_dim, alg_obj.a_dim
    mk = d["model_kwargs"]
    ocfg = O.Config(S=S, A=A, hidden=tuple(d["actor_kwargs"]["actor_layers"]), act="relu", B=L.SMALL["B"],
                    gamma=ak["gamma"], lr_pi=ak["mbpo_actor_lr"], model_hidden=tuple(mk["model_layers"]),
                    num_models=int(mk["num_models"]), model_act="relu", lr_model=ak["model_lr"],
                    critic_hidden=tuple(d["critic_kwargs"]["critic_layers"]))
    st = L._oracle_state(alg_obj, ocfg)
    ex = alg_obj.expert.get_weights()
    expert = ([np.asarray(w, np.float64) for w in ex[:-1]], np.asarray(ex[-1], np.float64))
    name = alg_obj.train(total, d)
    steps = [c for c in alg_obj.engine.calls if isinstance(c, tuple)]
    assert len(steps) == total - L.SMALL["init"] and all(c[1] == 1 for c in steps)
    log = load_log(os.path.join(ak["save_path"], name))
    assert len(log["train"]["BC_MSE_loss"]) == len(steps)
    os.remove(os.path.join(ak["save_path"], name))
    orc = BCLoopOracle(ocfg, st, oenvs[0], oenvs[2], expert, dict(ak, num_models=mk["num_models"]), rs_state,
                       ak["alg_seed"], max_episode_steps=1000).train(total)
    assert len(orc.update_stats) == len(steps)
    assert L._same_stream(alg_obj.engine.rng_get_state(), orc.rs.get_state())
