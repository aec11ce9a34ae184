"""The world-models handle (use_expert = SACX_EXPERT_MODELS beside a trainable GaussianActor) without a
GPU: the constant and the pinned ABI, sacx_create's accept / refuse with their messages, the layout's
segments, the new exports on unbound and wrong-kind handles, and EngineConfig's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_ppo_config import PPO_SEGMENTS, _cfg, _create, _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sacx_sim_collect", "sacx_model_losses_eval", "sacx_rollout_launches"]


def _mcfg(**kw):
    base = dict(world_models=True, model_hidden=(32, 32), model_batch=16, num_models=2)
    base.update(kw)
    return _cfg(**base)


def test_constant_abi_and_exports():
    from sac_eo import _native as N
    text = open(os.path.join(ROOT, "include", "sacx.h")).read()
    m = re.search(r"^#define\s+SACX_EXPERT_MODELS\s+(\d+)", text, re.M)
    assert m and int(m.group(1)) == N.EXPERT_MODELS == 3
    assert re.search(r"#define SACX_ABI_VERSION 8\b", text) and ctypes.sizeof(N.Config) == 392
    for s in NEW:
        assert s in N.EXPORTS and hasattr(N.lib(), s) and re.search(r"\b%s\(" % s, text), s


@pytest.mark.parametrize("kw", [dict(), dict(num_models=3, model_hidden=(96,)), dict(gaussian_model=True),
                                dict(s_dim=17, a_dim=6, separate_reward_nn=True, reward_hidden=(32, 32))])
def test_models_handle_creates_and_lists_its_segments(kw):
    c = _mcfg(**kw)
    cc = c.to_c()
    assert cc.use_expert == 3 and cc.actor_gaussian == 2 and cc.expert_batch == 0 and cc.expert_capacity == 0
    lib, h, rc, msg = _create(cc)
    assert rc == 0, msg
    segs = _layout(lib, h)
    depth = len(c.model_hidden)
    for k in range(c.num_models):
        for i in range(depth + 1):
            assert f"m{k}.l{i}" in segs, (k, i)
        assert (f"m{k}.logstd" in segs) == bool(c.gaussian_model)
        assert (f"r{k}.l0" in segs) == bool(c.separate_reward_nn)
    assert f"m{c.num_models}.l0" not in segs
    for name in ["mnorm.s_mean", "mnorm.s_den", "mnorm.a_mean", "mnorm.a_den", "mnorm.d_mean", "mnorm.d_den", "mnorm.r",
                 "mfit.idx", "mfit.Xs", "mfit.Ts", "mstats", "roll.X", "roll.Xm", "roll.A", "roll.O", "roll.noise",
                 "roll.idx", "replay"] + PPO_SEGMENTS:
        assert name in segs, name
    assert segs["roll.idx"][1:] == (1, 65536)
    assert segs["m0.l0"][1:] == (c.s_dim + c.a_dim + 1, c.model_hidden[0])
    # the VCritics still go behind everything else
    assert lib.sacx_vcritic_init(h, 2) == 0, lib.sacx_last_error(h)
    more = _layout(lib, h)
    assert {n: v for n, v in more.items() if n in segs} == segs and "v1.l0" in more
    lib.sacx_destroy(h)


def test_existing_handle_kinds_keep_their_layout():
    """roll.idx exists on the new kind only; a trainable handle without world models has no model segment."""
    lib, h, rc, msg = _create(_cfg().to_c())
    assert rc == 0, msg
    plain = _layout(lib, h)
    lib.sacx_destroy(h)
    assert not any(re.match(r"(m\d+\.|mnorm\.|mfit\.|roll\.)", n) for n in plain)
    lib, h, rc, msg = _create(_cfg(actor_gaussian=False, use_expert=True, model_hidden=(32, 32)).to_c())
    assert rc == 0, msg
    eo = _layout(lib, h)
    lib.sacx_destroy(h)
    assert "roll.O" in eo and "roll.idx" not in eo


@pytest.mark.parametrize("ag,ue,word", [
    (0, 3, "use_expert"), (1, 3, "use_expert"),                  # SACX_EXPERT_MODELS: trainable handles only
    (2, 1, "use_expert"), (2, 2, "trains the squashed actor"),   # EO / BC on a trainable handle: as before
    (2, 4, "use_expert"), (0, 4, "use_expert"),
])
def test_sacx_create_refuses_with_a_message(ag, ue, word):
    c = _mcfg(expert_batch=20, expert_capacity=20).to_c()
    c.actor_gaussian, c.use_expert, c.expert_batch, c.expert_capacity = ag, ue, 20, 20
    lib, h, rc, msg = _create(c)
    assert rc != 0 and word in msg, (rc, msg)
    if ue == 3:
        assert "SACX_ACTOR_GAUSSIAN_TRAIN" in msg


def test_models_handle_keeps_the_trainable_handles_refusals():
    for field, word in (("actor_output_norm", "actor_output_norm"), ("gemm_bf16", "gemm_bf16"), ("seeds", "seeds")):
        c = _mcfg().to_c()
        setattr(c, field, 2 if field == "seeds" else 1)
        lib, h, rc, msg = _create(c)
        assert rc != 0 and word in msg, (field, msg)
    lib, h, rc, msg = _create(_mcfg().to_c())
    assert rc == 0, msg
    assert lib.sacx_dp_init_local(h, 2, 0) != 0 and b"plain SAC" in lib.sacx_last_error(h)
    lib.sacx_destroy(h)


def test_new_entry_points_on_unbound_and_null_handles():
    lib, h, rc, msg = _create(_mcfg().to_c())
    assert rc == 0, msg
    calls = [lambda: lib.sacx_sim_collect(h, 0, 4, 2, 0, 0.0, 0.0, None, None, None, None, None),
             lambda: lib.sacx_model_losses_eval(h, 0, None, None, None, None, 4, None),
             lambda: lib.sacx_expert_set(h, None, None, 0, 0.1),
             lambda: lib.sacx_perm_push(h, None, 1),
             lambda: lib.sacx_expert_diag(h, None, None, None, 4, 0, 0.0, None),
             lambda: lib.sacx_rollout(h, 0, None, 4, 2, 0, 0.0, 0.0, None, None, None, None, None),
             lambda: lib.sacx_model_fit(h, None, 1, 0)]
    for i, f in enumerate(calls):
        assert f() != 0, i
        assert b"not bound" in lib.sacx_last_error(h), i
    lib.sacx_destroy(h)
    assert lib.sacx_sim_collect(None, 0, 4, 2, 0, 0.0, 0.0, None, None, None, None, None) != 0
    assert lib.sacx_model_losses_eval(None, 0, None, None, None, None, 4, None) != 0
    assert lib.sacx_rollout_launches(None) == -1
    # (the wrong-kind, empty-ring and bad-size refusals need a bound handle: tests/test_gpu_mbrl.py)


def test_engine_config_refusals():
    from sac_eo.engine import EngineConfig
    for ag in (False, True):
        with pytest.raises(ValueError, match="actor_gaussian='train'"):
            EngineConfig(s_dim=3, a_dim=1, world_models=True, actor_gaussian=ag)
    for kw in (dict(use_expert=True), dict(bc=True)):
        with pytest.raises(ValueError):
            EngineConfig(s_dim=3, a_dim=1, world_models=True, actor_gaussian="train", **kw)
        with pytest.raises(ValueError):                       # without world_models: refused as before
            _cfg(**kw).to_c()
    assert _cfg().to_c().use_expert == 0 and not _cfg().world_models


# ------------------------------------------------------------------------------------------ host side
def test_init_alg_dispatch():
    from sac_eo.algs import init_alg
    from test_ppo_config import KW
    for ak in ({"alg_type": "mbrl"}, {"alg_type": "mbrl", "mf_algo": "trpo"}, {"alg_type": "mbrl", "mf_algo": "x"}):
        with pytest.raises(NotImplementedError, match="TRPO"):       # before any other argument is touched
            init_alg(0, None, None, None, None, None, None, None, None, ak, KW, None, None)


def test_model_classes_have_get_losses_eval():
    from sac_eo.models.continuous_models import GaussianModel, MSEModel
    from test_ppo_config import _Env
    for cls, extra in ((MSEModel, ()), (GaussianModel, (1.0,))):
        m = cls(_Env(), [32, 32], ["relu"], 0.01, [32], ["relu"], 0.01, {}, *extra, rng=np.random.default_rng(0))
        with pytest.raises(RuntimeError, match="not bound"):
            m.get_losses_eval(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 1)), np.zeros(2))


TRAIN_KEYS = ["J_tot", "steps", "traj", "time_env_data", "J_tot_eval", "steps_eval", "time_eval",
              "time_model_fit", "model_ent", "model_loss_epochs", "steps_update", "time_actor", "time_critic",
              "time_sim_data", "ent", "tv", "kl", "alpha", "actor_lr", "outside_clip", "actor_grad_norm_pre",
              "actor_grad_norm", "ent_agg", "kl_agg", "alpha_agg", "time_ac_agg"]
ENSEMBLE_KEYS = ["critic_loss", "model_loss", "model_loss_train", "model_loss_holdout", "model_loss_mse",
                 "model_loss_reward"]

LOOP = dict(total=700, init=300, batch=200, horizon=100, sim=404, sim_h=5, mf=2, a_it=2, a_nmb=4, c_it=3, c_nmb=4,
            mb=50, epochs=4)


def _argv(tmp, extra=()):
    L = LOOP
    return ["--alg_type", "mbrl", "--mf_algo", "ppo", "--env_name", "HalfCheetah-v3", "--actor_layers", "16", "16",
            "--critic_layers", "16", "16", "--model_layers", "16", "16", "--total_timesteps", str(L["total"]),
            "--env_batch_size_init", str(L["init"]), "--env_batch_size", str(L["batch"]), "--env_horizon", str(L["horizon"]),
            "--sim_batch_size", str(L["sim"]), "--sim_horizon", str(L["sim_h"]), "--num_mf_updates", str(L["mf"]),
            "--actor_update_it", str(L["a_it"]), "--actor_nminibatch", str(L["a_nmb"]), "--critic_update_it", str(L["c_it"]),
            "--critic_nminibatch", str(L["c_nmb"]), "--model_batch_size", str(L["mb"]), "--model_num_epochs", str(L["epochs"]),
            "--eval_freq", "400", "--eval_num_traj", "1", "--seed", "3", "--save_path", str(tmp)] + list(extra)


CASES = {"plain": ((), dict(nm=2, critics=1, holdout=0.0, gm=False)),
         "ensemble_holdout_gauss": (("--critic_ensemble", "--num_models", "3", "--model_holdout_ratio", "0.25",
                                     "--model_holdout_epochs", "2", "--gaussian_model"),
                                    dict(nm=3, critics=3, holdout=0.25, gm=True))}


@pytest.mark.parametrize("case", list(CASES))
def test_host_loop_on_the_stand_in_engine(monkeypatch, tmp_path, case):
    """The whole loop on the NumPy stand-in engine: the log's key sets and counts, the fit and sim_collect
    calls, and the global stream bit for bit against mbrl_ref's restatement of the loop's draws."""
    import fake_engine_mbrl
    import mbrl_ref as M
    import sac_eo.train as T
    from sac_eo.common.logger import load_log
    fake_engine_mbrl.install(monkeypatch)
    extra, c = CASES[case]
    L = LOOP
    built = {}
    real_build = T.build_alg

    def build(inputs, pack=None):
        alg = real_build(inputs, pack)
        built["alg"], built["state0"] = alg, alg.engine.rng_get_state()
        return alg
    monkeypatch.setattr(T, "build_alg", build)
    log = load_log(T.main(_argv(tmp_path, extra)))[0]
    alg = built["alg"]
    from sac_eo.algs.mbrl_onpolicy_alg import MBRLOnPolicyAlg
    assert type(alg) is MBRLOnPolicyAlg and alg.engine.cfg.world_models and alg.engine.cfg.vcritics == c["critics"]
    assert not alg.actor.squash
    tr = log["train"]
    assert set(tr) == set(TRAIN_KEYS + ENSEMBLE_KEYS)
    assert set(log["final"]) == {"actor_weights", "critic_weights", "rms_stats", "model_weights", "reward_weights"}
    steps = [int(x) for x in tr["steps"]]
    assert sum(steps) >= L["total"] and len(tr["steps_update"]) == L["mf"] * len(steps)
    assert np.asarray(tr["model_loss"]).shape == (len(steps), c["nm"])
    assert np.all(np.isinf(tr["model_loss_holdout"])) == (c["holdout"] == 0.0)
    # the restatement: the same draws from the state the engine adopted
    rs = np.random.RandomState(0)
    rs.set_state(built["state0"])
    S, A = alg.s_dim, alg.a_dim
    held, fit_calls, epochs, rows_upd = 0, [], [], []
    for n_steps in steps:
        for _ in range(n_steps):
            rs.normal(size=(1, A))                       # actor.sample per env step
        held += n_steps
        ep, calls = M.model_fit_draws(rs, held, c["nm"], L["epochs"], L["mb"], holdout_ratio=c["holdout"],
                                      holdout_epochs=2, holdout_loss=lambda e: 0.5 * c["nm"])
        epochs.append(ep)
        fit_calls += calls
        rows_upd += M.actor_critic_draws(rs, held, c["nm"], S, A, L["sim"], L["sim_h"], L["mf"], c["critics"], L["c_it"],
                                         L["c_nmb"], L["a_it"], L["a_nmb"], gaussian_model=c["gm"])
    assert [int(x) for x in tr["model_loss_epochs"]] == epochs
    assert [n for k, *r in [x for x in alg.engine.calls if isinstance(x, tuple)] if k == "model_fit" for n in r] == fit_calls
    assert [int(x) for x in tr["steps_update"]] == rows_upd
    dev, ref = alg.engine.rng_get_state(), rs.get_state()
    assert np.array_equal(dev[1], ref[1]) and dev[2:5] == ref[2:5]
    # the short last pass of 404 / nm rows per model
    per = int(L["sim"] / c["nm"])
    want = [(n, h) for n, h in M.sim_passes(per, L["sim_h"])]
    got = [(x[2], x[3]) for x in alg.engine.calls if isinstance(x, tuple) and x[0] == "sim_collect"][:len(want)]
    assert got == want and want[-1][1] == per % L["sim_h"] and sum(n * h for n, h in want) == per


@pytest.mark.parametrize("kw,want", [
    (dict(total_timesteps=5000, env_batch_size_init=100, env_batch_size=4000, env_horizon=1000, env_batch_type="steps"), 8100),
    (dict(total_timesteps=700, env_batch_size_init=300, env_batch_size=200, env_horizon=100, env_batch_type="steps"), 700),
    (dict(total_timesteps=500, env_batch_size_init=3, env_batch_size=2, env_horizon=100, env_batch_type="traj"), 700),
])
def test_ring_capacity_covers_every_env_row_the_run_can_collect(kw, want):
    """env_buffer_size=None: the loop collects whole batches while fewer than total_timesteps rows are held, so it
    overshoots by up to a batch (traj batches: by up to batch x horizon rows); the bound must cover `want`, the
    rows such a run really collects at full-length trajectories."""
    from sac_eo.algs.mbrl_onpolicy_alg import MBRLOnPolicyAlg
    alg = MBRLOnPolicyAlg.__new__(MBRLOnPolicyAlg)
    for k, v in kw.items():
        setattr(alg, k, v)
    alg.env_buffer_size, alg.B, alg.sim_batch_size_per_model, alg.sim_batch_type, alg.sim_horizon = None, 2, 20, "steps", 5
    assert alg._env_rows_bound() >= want and alg._capacity() >= want
    alg.env_buffer_size = 30                              # below the 40 simulated rows of an update: refused
    with pytest.raises(NotImplementedError, match="env_buffer_size"):
        alg._capacity()
    alg.env_buffer_size = 64
    assert alg._capacity() == 64
