"""``--alg_type mfrl`` without a GPU: the two softmax-act exports and their refusals on handles that are not
bound, the Discrete space and the discrete synthetic env, ``init_alg('mfrl')``'s dispatch and refusals, the
engine sizing, and ``_update``'s call order against a recording stand-in engine (tests/fake_engine_mbrl.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_ppo_config import KW as PPO_KW
from test_ppo_config import _cfg, _create

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sacx_softmax_act", "sacx_softmax_act_host"]


def test_exports_and_the_unchanged_abi():
    from sac_eo import _native as N
    text = open(os.path.join(ROOT, "include", "sacx.h")).read()
    assert re.search(r"#define SACX_ABI_VERSION 8\b", text) and ctypes.sizeof(N.Config) == 392
    for s in NEW:
        assert s in N.EXPORTS and hasattr(N.lib(), s) and re.search(r"\b%s\(" % s, text), s
    assert len(N.EXPORTS) == len(set(N.EXPORTS)) == 73
    assert "discrete_actors.py:22-42" in text


def test_refusals_on_unbound_and_non_softmax_handles():
    obs, act = (ctypes.c_float * 3)(), (ctypes.c_int32 * 1)()
    calls = lambda lib, h: [lambda: lib.sacx_softmax_act(h, obs, 1, 0, act, None),
                            lambda: lib.sacx_softmax_act_host(h, obs, 1, 0, act)]
    lib, h, rc, msg = _create(_cfg(a_dim=3).to_c())          # a softmax handle, not bound
    assert rc == 0, msg
    assert lib.sacx_softmax_init(h) == 0
    for f in calls(lib, h):
        assert f() != 0 and b"not bound" in lib.sacx_last_error(h)
    lib.sacx_destroy(h)
    for kw in (dict(), dict(actor_gaussian=True), dict(actor_gaussian=False)):     # no sacx_softmax_init
        lib, h, rc, msg = _create(_cfg(a_dim=3, **kw).to_c())
        assert rc == 0, msg
        for f, name in zip(calls(lib, h), NEW):
            assert f() != 0
            err = lib.sacx_last_error(h)
            assert b"not a softmax handle" in err and name.encode() in err, err
        lib.sacx_destroy(h)
    assert lib.sacx_softmax_act(None, obs, 1, 0, act, None) != 0
    assert lib.sacx_softmax_act_host(None, obs, 1, 0, act) != 0
    # the pinned message of the Gaussian-only entry points stays (a bound handle needs a GPU: test_gpu_softmax)
    src = open(os.path.join(ROOT, "sac-expert_amd", "csrc", "sacx.cpp")).read()
    assert src.count("a softmax handle samples on the host from sacx_ppo_dist's logits (discrete_actors.py:22-42)") >= 5


# ------------------------------------------------------------------------------------------ the comparison's premise
def test_u_zero_gives_minus_inf_not_nan():
    """u = 0: g = float32(-log(-log 0)) = -inf and x = -inf, never a NaN (the host arithmetic the kernel restates)."""
    import softmax_act_cases as C
    from sac_eo.actors.discrete_actors import gumbel_argmax
    x = C.perturbed(np.zeros((1, 3), np.float32), np.array([[0.0, 0.5, 0.25]]))
    assert x[0, 0] == -np.inf and not np.isnan(x).any()
    assert gumbel_argmax(np.zeros((1, 3), np.float32), np.array([[0.0, 0.5, 0.25]]))[0] == 1
    assert gumbel_argmax(np.zeros((1, 3), np.float32), np.zeros((1, 3)))[0] == 0        # all -inf: the first index


def test_gpu_cases_premise_holds_on_the_host():
    """tests/test_gpu_softmax_act.py compares actions on rows whose top-two gap of x exceeds 1e-4 and leaves out
    at most 1 % of a case's rows: for its seeded nets, states and streams the host computation (the fp64 oracle's
    logits here) leaves out no more, for the sampled and for the deterministic form."""
    import softmax_act_cases as C
    import softmax_ref as SM
    assert {n for _, n, _, _ in C.CASES} == {1, 7, 16, 17, 1030} and {A for _, _, A, _ in C.CASES} == {2, 5, 32}
    assert {k for _, _, _, k in C.CASES} == set(C.STREAMS)
    for path in (lambda net, n: net == "h64" and n <= 16, lambda net, n: not (net == "h64" and n <= 16)):
        assert {k for net, n, _, k in C.CASES if path(net, n)} == set(C.STREAMS)      # every stream on both paths
    states = {}
    for net, n, A, kind in C.CASES:
        if (net, A) not in states:
            states[(net, A)] = C.make_state(net, A)
        cfg, st, nrm = states[(net, A)]
        logits = np.asarray(SM.forward(st, cfg, nrm, C.states(n, seed=4 + n))[0], np.float32)
        u, after = C.uniforms(C.stream(kind), n, A)
        assert after[3] == C.stream(kind)[3]                     # random_sample keeps the cached gaussian
        for uu in (u, None):
            out = n - int(C.clear_rows(logits, uu).sum())
            assert out <= C.may_leave_out(n), (net, n, A, kind, uu is None, out)
    assert C.stream("pos623")[2] == 623 and C.stream("gauss")[3] == 1 and C.stream("fresh")[2] == 624


# ------------------------------------------------------------------------------------------ the env
def test_discrete_space():
    from sac_eo.envs.synthetic import Discrete
    d = Discrete(3)
    assert d.n == 3 and d.shape == () and not hasattr(d, "low") and not hasattr(d, "high")
    d.seed(5)
    a = [d.sample() for _ in range(50)]
    d.seed(5)
    assert a == [d.sample() for _ in range(50)] and set(a) == {0, 1, 2}
    assert d.contains(0) and d.contains(np.int64(2)) and not d.contains(3) and not d.contains(-1)
    assert not d.contains(1.0) and not d.contains(np.array([1]))


@pytest.mark.parametrize("name,S,n", [("CartPole-v1", 4, 2), ("Acrobot-v1", 6, 3), ("LunarLander-v2", 8, 4)])
def test_discrete_env(name, S, n):
    from sac_eo.actors.discrete_actors import SoftMaxActor
    from sac_eo.actors.init_actor import init_actor
    from sac_eo.envs import init_env
    from sac_eo.envs.synthetic import DISCRETE_ENV_SPECS, ENV_SPECS
    assert DISCRETE_ENV_SPECS[name] == (S, n) and name not in ENV_SPECS
    env = init_env(env_name=name)
    assert env.observation_space.shape == (S,) and env.action_space.n == n and not hasattr(env.action_space, "low")

    def run(seed):
        e = init_env(env_name=name)
        e.seed(seed)
        out = [e.reset()]
        rs = []
        for t in range(6):
            s, r, d, _ = e.step(t % n)
            out.append(s)
            rs.append(r)
            assert r == float(s[0]) and not d and s.dtype == np.float32 and s.shape == (S,)
        return np.stack(out), rs
    a, b, c = run(3), run(3), run(4)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and not np.array_equal(a[0], c[0])
    # the action index selects a fixed row of W_a: two actions from one state differ, noise aside
    e1, e2 = init_env(env_name=name), init_env(env_name=name)
    for e in (e1, e2):
        e.seed(0)
        e.reset()
    assert not np.allclose(e1.step(0)[0], e2.step(n - 1)[0], atol=1e-3)
    with pytest.raises(ValueError):
        env.reset()
        env.step(n)
    kw = dict(actor_layers=[16, 16], actor_activations=["tanh"], actor_gain=0.01, actor_std_mult=1.0,
              actor_init_type="orthogonal", actor_layer_norm=False, actor_weights=None)
    actor = init_actor(env, **kw)
    assert type(actor) is SoftMaxActor and (actor.s_dim, actor.a_dim) == (S, n) and actor.device_sample is False


def test_continuous_env_names_and_message_stay():
    from sac_eo.envs import init_env
    from sac_eo.envs.synthetic import ENV_SPECS
    assert sorted(ENV_SPECS) == ["Ant-v3", "HalfCheetah-v3", "Hopper-v3", "Humanoid-v3", "Pendulum-v1", "Swimmer-v3",
                                 "Walker2d-v3"]
    with pytest.raises(ValueError, match="unknown environment 'Nope-v0'; known: "):
        init_env(env_name="Nope-v0")
    assert hasattr(init_env(env_name="Pendulum-v1").action_space, "low")


# ------------------------------------------------------------------------------------------ init_alg
class _RecEngine:
    """FakeEngineMBRL with a record of the calls an update makes, and the softmax act of a discrete actor."""

    @staticmethod
    def make():
        from fake_engine_mbrl import FakeEngineMBRL

        class Rec(FakeEngineMBRL):
            def _rec(self, name, *a):
                self.calls.append((name,) + a)

            def gae(self, critic, s, r, sp, d, traj, gamma, lam):
                self._rec("gae", int(critic), int(np.shape(r)[0]))
                return super().gae(critic, s, r, sp, d, traj, gamma, lam)

            def vcritic_begin(self, critic, s, rtg):
                self._rec("vcritic_begin", int(critic), int(np.shape(rtg)[0]))
                return super().vcritic_begin(critic, s, rtg)

            def vcritic_steps(self, idx, critic_lr, **kw):
                self._rec("vcritic_steps", np.asarray(idx).shape)
                return super().vcritic_steps(idx, critic_lr, **kw)

            def vcritic_end(self):
                self._rec("vcritic_end")
                return super().vcritic_end()

            def ppo_begin(self, s, a, adv):
                self._rec("ppo_begin", np.shape(s), np.shape(a))
                return super().ppo_begin(s, a, adv)

            def ppo_steps(self, idx, **kw):
                self._rec("ppo_steps", np.asarray(idx).shape)
                return super().ppo_steps(idx, **kw)

            def ppo_end(self, eps):
                self._rec("ppo_end")
                return super().ppo_end(eps)

            def softmax_act_host(self, obs, deterministic=False):
                n = np.asarray(obs).reshape(-1, self.cfg.s_dim).shape[0]
                if not deterministic:
                    self.S["rs"].random_sample((n, self.cfg.a_dim))
                return np.zeros(n, np.int32)
        return Rec


def _install(monkeypatch):
    import sac_eo.algs.mfrl_onpolicy_alg as m
    monkeypatch.setattr(m, "Engine", _RecEngine.make())


LOOP = dict(total=250, init=120, batch=90, horizon=40, a_it=2, a_nmb=3, c_it=3, c_nmb=2)


def _argv(tmp, env="Pendulum-v1", extra=()):
    L = LOOP
    return ["--alg_type", "mfrl", "--mf_algo", "ppo", "--env_name", env, "--actor_layers", "16", "16", "--critic_layers",
            "16", "16", "--model_layers", "16", "16", "--total_timesteps", str(L["total"]), "--env_batch_size_init",
            str(L["init"]), "--env_batch_size", str(L["batch"]), "--env_horizon", str(L["horizon"]), "--actor_update_it",
            str(L["a_it"]), "--actor_nminibatch", str(L["a_nmb"]), "--critic_update_it", str(L["c_it"]),
            "--critic_nminibatch", str(L["c_nmb"]), "--seed", "3", "--save_path", str(tmp)] + list(extra)


def _build(monkeypatch, tmp, env="Pendulum-v1", extra=()):
    import sac_eo.train as T
    from sac_eo.common.train_parser import create_train_parser, gather_inputs
    from sac_eo.common.seeding import derive_seeds
    _install(monkeypatch)
    args = create_train_parser().parse_args(_argv(tmp, env, extra))
    d = gather_inputs(args)
    seeds = derive_seeds(args.seed, 1, 0)
    sk = d["setup_kwargs"]
    sk["idx"] = 0
    for kind, key in (("setup", "setup_seed"), ("sim", "sim_seed"), ("eval", "eval_seed"), ("expert", "expert_seed")):
        sk[key] = int(seeds[kind][0])
    sk["algorithm_seed"] = int(seeds["algorithm"][0])
    return T.build_alg(d), d


def test_init_alg_dispatch_and_refusals(monkeypatch, tmp_path):
    from sac_eo.algs import init_alg
    from sac_eo.algs.mfrl_onpolicy_alg import MFRLOnPolicyAlg
    from sac_eo.algs.model_free.trpo import TRPO
    import sac_eo.algs.model_free as MF
    assert not hasattr(MF, "TRPO")                               # the exports stay: TRPO by module path only
    for bad in ("x", "sac", None):
        with pytest.raises(ValueError, match="mf_algo"):           # before any other argument is touched
            init_alg(0, None, None, None, None, None, None, None, None, {"alg_type": "mfrl", "mf_algo": bad}, PPO_KW,
                     None, None)
    with pytest.raises(NotImplementedError, match="TRPO is not built"):      # the mbrl branch as it was
        init_alg(0, None, None, None, None, None, None, None, None, {"alg_type": "mbrl", "mf_algo": "trpo"}, PPO_KW,
                 None, None)
    alg, _ = _build(monkeypatch, tmp_path)
    assert type(alg) is MFRLOnPolicyAlg and not alg.discrete
    cfg = alg.engine.cfg
    assert cfg.trainable_gaussian and cfg.vcritics == 1 and not cfg.trpo and not cfg.softmax and not cfg.world_models
    assert alg.mf_algo.ent_targ == -1 and alg.B == 1
    alg, _ = _build(monkeypatch, tmp_path, extra=("--mf_algo", "trpo"))
    assert type(alg.mf_algo) is TRPO and alg.engine.cfg.trpo
    alg, _ = _build(monkeypatch, tmp_path, env="Acrobot-v1")
    assert alg.discrete and alg.engine.cfg.softmax and alg.engine.cfg.a_dim == 3 and alg.actor.device_sample is True
    assert alg.mf_algo.ent_targ == -3 and alg.env_data.a_dim == 1
    with pytest.raises(ValueError, match="--critic_ensemble"):
        _build(monkeypatch, tmp_path, extra=("--critic_ensemble", "--num_models", "2"))

    class _Squashed:
        squash, softmax, output_norm = True, False, False

    class _OutputNorm:
        squash, softmax, output_norm = False, False, True
    for actor, word in ((_Squashed(), "--actor_squash"), (_OutputNorm(), "--actor_output_norm")):
        with pytest.raises(ValueError, match=word):
            MFRLOnPolicyAlg(0, alg.env, alg.env, actor, [None], {**_kw(), "mf_algo": "ppo"}, PPO_KW)


def _kw():
    return dict(gamma=0.99, lam=0.95, env_horizon=100, env_batch_type="steps", env_batch_size_init=300,
                env_batch_size=200, critic_lr=1e-3, critic_update_it=2, critic_nminibatch=4, num_mf_updates=1)


def test_train_py_refuses_the_flags_mbrl_refuses(tmp_path):
    from sac_eo.train import main
    with pytest.raises(ValueError, match="--alg_type mfrl.*--actor_squash"):
        main(_argv(tmp_path, extra=("--actor_squash",)))


@pytest.mark.parametrize("kw,mf,cap,batch", [
    (dict(env_batch_type="steps", env_batch_size_init=300, env_batch_size=200, env_horizon=100,
          critic_nminibatch=4, mf_algo_name="ppo"), dict(actor_nminibatch=8), 300, 75),
    (dict(env_batch_type="steps", env_batch_size_init=100, env_batch_size=250, env_horizon=1000,
          critic_nminibatch=4, mf_algo_name="ppo"), dict(actor_nminibatch=2), 250, 125),
    (dict(env_batch_type="traj", env_batch_size_init=3, env_batch_size=2, env_horizon=100,
          critic_nminibatch=7, mf_algo_name="ppo"), dict(actor_nminibatch=32), 300, 42),
    (dict(env_batch_type="traj", env_batch_size_init=2, env_batch_size=5, env_horizon=20,
          critic_nminibatch=4, mf_algo_name="trpo"), dict(actor_nminibatch=1), 100, 25),     # TRPO: the critic's alone
    (dict(env_batch_type="steps", env_batch_size_init=3, env_batch_size=2, env_horizon=20,
          critic_nminibatch=8, mf_algo_name="ppo"), dict(actor_nminibatch=2), 3, 1),
])
def test_capacity_and_batch_arithmetic(kw, mf, cap, batch):
    from sac_eo.algs.mfrl_onpolicy_alg import MFRLOnPolicyAlg
    alg = MFRLOnPolicyAlg.__new__(MFRLOnPolicyAlg)
    for k, v in kw.items():
        setattr(alg, k, v)
    assert alg._capacity() == cap and alg._batch(mf) == batch
    alg.env_batch_size = 1 << 25
    with pytest.raises(NotImplementedError, match="2\\^24"):
        alg._capacity()


# ------------------------------------------------------------------------------------------ the update
@pytest.mark.parametrize("env", ["Pendulum-v1", "CartPole-v1"])
def test_update_call_order_and_reset(monkeypatch, tmp_path, env):
    alg, d = _build(monkeypatch, tmp_path, env=env)
    alg._set_rms()
    n = alg._collect_env_data(0)
    assert n == LOOP["init"] == alg.env_data.current_size
    assert alg.env_data.a_all.shape == (n, 1) and alg.env_data.a_all.dtype == np.float32
    del alg.engine.calls[:]
    alg._update()
    L = LOOP
    acols = (n,) if env == "CartPole-v1" else (n, 1)             # a Discrete action: [n] indices for PPO
    assert alg.engine.calls == [
        ("gae", 0, n),
        ("vcritic_begin", 0, n), ("vcritic_steps", (L["c_it"] * L["c_nmb"], n // L["c_nmb"])), ("vcritic_end",),
        ("ppo_begin", (n, alg.s_dim), acols), ("ppo_steps", (L["a_it"] * L["a_nmb"], n // L["a_nmb"])), ("ppo_end",)]
    assert alg.env_data.current_size == 0 and alg.env_data.steps_total == 0 and alg.env_data.r_all.shape == (0,)
    tr = alg.logger.train_dict
    assert list(tr["steps_update"]) == [n] and {"time_critic", "time_actor", "critic_loss", "kl"} <= set(tr)


TRAIN_KEYS = ["J_tot", "steps", "traj", "time_env_data", "steps_update", "time_actor", "time_critic", "ent", "tv", "kl",
              "alpha", "actor_lr", "outside_clip", "actor_grad_norm_pre", "actor_grad_norm", "critic_loss"]


@pytest.mark.parametrize("env", ["Pendulum-v1", "Acrobot-v1"])
def test_host_loop_on_the_stand_in_engine(monkeypatch, tmp_path, env):
    """The whole loop through the front door: key sets, counts, one update per env batch on that batch's rows,
    and --pack_runs ignored without an error."""
    import sac_eo.train as T
    from sac_eo.common.logger import load_log
    _install(monkeypatch)
    logs = load_log(T.main(_argv(tmp_path, env, ("--runs", "2", "--pack_runs", "--eval_freq", "100", "--eval_num_traj", "1"))))
    assert len(logs) == 2
    for log in logs:
        tr = log["train"]
        assert set(tr) == set(TRAIN_KEYS + ["J_tot_eval", "steps_eval", "time_eval"])
        assert set(log["final"]) == {"actor_weights", "critic_weights", "rms_stats"}
        steps = [int(x) for x in tr["steps"]]
        assert steps == [LOOP["init"], LOOP["batch"], LOOP["batch"]] and sum(steps) >= LOOP["total"]
        assert [int(x) for x in tr["steps_update"]] == steps
        assert np.asarray(tr["critic_loss"]).shape == (3, 1)
        assert log["final"]["rms_stats"]["s_rms"]["t"] == sum(steps)
