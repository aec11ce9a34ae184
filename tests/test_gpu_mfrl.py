"""``--alg_type mfrl`` on the device, tiny shapes (S=3 / A=1 and the discrete (4, 2); nets 32 x 2; horizon 20;
batches of 40 rows; two minibatches, two iterations; cg_it 5).

* one ``_update()`` equals its composition on a twin engine with the same weights, normalisers and stream:
  ``Engine.gae``, ``VCriticUpdate.update``, ``PPO.update`` / ``TRPO.update`` by hand on the same batch -- weights
  and stream bit-identical, every logged key but ``time_*`` equal;
* ``sac_eo.train.main`` end to end: the reference's keys, finite values, ``sum(steps) >= total_timesteps``;
* two runs of one seed give equal logs;
* the Gaussian run's log is a valid ``--expert_file``: loaded into a ``sac_imit`` build, the expert's
  deterministic ``sample`` equals the trained actor's to 2e-5 (the project's activation bar).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VARIANTS = {"gauss_ppo": ("Pendulum-v1", "ppo"), "gauss_trpo": ("Pendulum-v1", "trpo"), "discrete_ppo": ("CartPole-v1", "ppo")}
ACTOR_KEYS = {"ppo": ["ent", "tv", "kl", "alpha", "actor_lr", "outside_clip", "actor_grad_norm_pre", "actor_grad_norm"]}
LOOP_KEYS = ["J_tot", "steps", "traj", "time_env_data", "steps_update", "time_critic", "time_actor", "critic_loss"]


def argv(tmp, variant, extra=()):
    env, algo = VARIANTS[variant]
    return ["--alg_type", "mfrl", "--mf_algo", algo, "--env_name", env, "--actor_layers", "32", "32", "--critic_layers",
            "32", "32", "--model_layers", "16", "16", "--total_timesteps", "120", "--env_batch_size_init", "40",
            "--env_batch_size", "40", "--env_horizon", "20", "--actor_update_it", "2", "--actor_nminibatch", "2",
            "--critic_update_it", "2", "--critic_nminibatch", "2", "--cg_it", "5", "--seed", "3",
            "--save_path", str(tmp)] + list(extra)


def build(tmp, variant, extra=()):
    """The construction sequence of run 0 of ``main(argv)`` -> (alg, inputs)."""
    import sac_eo.train as T
    from sac_eo.common.seeding import derive_seeds
    from sac_eo.common.train_parser import create_train_parser, gather_inputs
    args = create_train_parser().parse_args(argv(tmp, variant, extra))
    d = gather_inputs(args)
    seeds = derive_seeds(args.seed, 1, 0)
    sk = d["setup_kwargs"]
    sk["idx"] = 0
    for kind, key in (("setup", "setup_seed"), ("sim", "sim_seed"), ("eval", "eval_seed"), ("expert", "expert_seed")):
        sk[key] = int(seeds[kind][0])
    sk["algorithm_seed"] = int(seeds["algorithm"][0])
    return T.build_alg(d), d


def same_stream(a, b):
    return np.array_equal(a[1], b[1]) and tuple(a[2:5]) == tuple(b[2:5])


def same_weights(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_update_equals_its_composition(gpu_available, tmp_path, variant):
    from sac_eo.algs.model_free import PPO, VCriticUpdate
    from sac_eo.algs.model_free.trpo import TRPO
    alg, d = build(tmp_path, variant)
    twin, _ = build(tmp_path, variant)
    assert same_weights(alg.actor.get_weights(), twin.actor.get_weights())
    assert same_weights(alg.critics[0].get_weights(), twin.critics[0].get_weights())
    w0, c0 = alg.actor.get_weights(), alg.critics[0].get_weights()
    alg._set_rms()
    n = alg._collect_env_data(0)
    assert n == 40 == alg.env_data.current_size
    B = alg.env_data
    s, a, r, sp, dn, idx = (x.copy() for x in (B.s_all, B.a_all, B.r_all, B.sp_all, B.d_all, B.idx_all))
    assert a.shape == (40, 1) and len(np.unique(idx)) == 2
    if alg.discrete:
        assert alg.actor.device_sample and set(np.unique(a)) <= {0.0, 1.0} and len(np.unique(a)) == 2
    # the twin: the same normalisers and stream, the batch fed by hand
    twin.normalizer.set_rms_stats(alg.normalizer.get_rms_stats())
    twin._set_rms()
    twin.engine.rng_set_state(alg.engine.rng_get_state())
    alg._update()
    log = alg.logger.train_dict
    adv, rtg, rtg_sp = (x.cpu().numpy() for x in twin.engine.gae(0, s, r, sp, dn, idx, alg.gamma, alg.lam))
    cu = VCriticUpdate(twin.critics, dict(critic_lr=alg.critic_lr, critic_update_it=alg.critic_update_it,
                                          critic_nminibatch=alg.critic_nminibatch), twin.actor)
    log_c = cu.update(([s], None, None, [rtg], None, None), 1)
    mf = dict(d["mf_update_kwargs"])
    mf["ent_targ"] = -alg.a_dim
    algo = (TRPO if VARIANTS[variant][1] == "trpo" else PPO)(twin.actor, mf)
    log_a = algo.update((s, a.reshape(-1) if alg.discrete else a, adv, rtg, sp, rtg_sp))
    assert algo.engine is twin.engine and cu.engine is twin.engine
    assert same_weights(alg.actor.get_weights(), twin.actor.get_weights())
    assert same_weights(alg.critics[0].get_weights(), twin.critics[0].get_weights())
    assert same_stream(alg.engine.rng_get_state(), twin.engine.rng_get_state())
    assert not same_weights(alg.actor.get_weights(), w0) and not same_weights(alg.critics[0].get_weights(), c0)   # it trained
    want = dict(log_a)
    want.update(steps_update=40, critic_loss=[log_c[0]["critic_loss"]])
    assert set(want) | {"time_critic", "time_actor", "J_tot", "steps", "traj", "time_env_data"} == set(log)
    for k, v in want.items():
        assert len(log[k]) == 1 and np.array_equal(np.asarray(log[k][0]), np.asarray(v), equal_nan=True), k
    assert alg.env_data.current_size == 0 and alg.env_data.traj_total == 0
    alg.engine.close()
    twin.engine.close()


def run(tmp, variant, capture=None, extra=()):
    import sac_eo.train as T
    from sac_eo.common.logger import load_log
    real = T.build_alg

    def build_and_keep(inputs, pack=None):
        alg = real(inputs, pack)
        if capture is not None:
            capture.append(alg)
        return alg
    T.build_alg = build_and_keep
    try:
        path = T.main(argv(tmp, variant, extra))
    finally:
        T.build_alg = real
    return path, load_log(path)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_train_end_to_end_and_deterministic(gpu_available, tmp_path, variant):
    path, logs = run(tmp_path / "a", variant)
    assert len(logs) == 1
    tr = logs[0]["train"]
    keys = set(LOOP_KEYS)
    if VARIANTS[variant][1] == "ppo":
        keys |= set(ACTOR_KEYS["ppo"])
        assert keys == set(tr)
    else:
        assert keys <= set(tr) and {"kl", "ent"} <= set(tr)
    assert set(logs[0]["final"]) == {"actor_weights", "critic_weights", "rms_stats"}
    steps = [int(x) for x in tr["steps"]]
    assert steps == [40, 40, 40] and sum(steps) >= 120 and [int(x) for x in tr["steps_update"]] == steps
    for k, v in tr.items():
        assert np.all(np.isfinite(np.asarray(v, np.float64))), k
    for w in logs[0]["final"]["actor_weights"] + logs[0]["final"]["critic_weights"][0]:
        assert np.all(np.isfinite(w))
    _, again = run(tmp_path / "b", variant)
    for k in tr:
        if not k.startswith("time_"):
            assert np.array_equal(np.asarray(tr[k]), np.asarray(again[0]["train"][k])), k
    assert same_weights(logs[0]["final"]["actor_weights"], again[0]["final"]["actor_weights"])


def test_expert_round_trip(gpu_available, tmp_path):
    """The Gaussian mfrl log as the --expert_file of a sac_imit build: the expert acts as the trained actor does."""
    import sac_eo.train as T
    from sac_eo.actors import GaussianActor
    from sac_eo.common.train_parser import create_train_parser, gather_inputs
    from sac_eo.common.seeding import derive_seeds
    kept = []
    path, logs = run(tmp_path, "gauss_ppo", capture=kept)
    trained = kept[0]
    s = np.random.RandomState(7).normal(size=(8, 3)).astype(np.float32)
    want = np.asarray(trained.actor.sample(s, deterministic=True))
    args = create_train_parser().parse_args(
        ["--alg_type", "sac_imit", "--env_name", "Pendulum-v1", "--actor_layers", "32", "32", "--critic_layers", "32", "32",
         "--model_layers", "16", "16", "--total_timesteps", "100", "--env_batch_size_init", "40", "--env_horizon", "20",
         "--sac_batch_size", "16", "--model_batch_size", "16", "--seed", "5", "--save_path", str(tmp_path),
         "--expert_path", os.path.dirname(path), "--expert_file", os.path.basename(path)])
    d = gather_inputs(args)
    d["actor_kwargs"]["actor_squash"] = True
    seeds = derive_seeds(args.seed, 1, 0)
    sk = d["setup_kwargs"]
    sk["idx"] = 0
    for kind, key in (("setup", "setup_seed"), ("sim", "sim_seed"), ("eval", "eval_seed"), ("expert", "expert_seed")):
        sk[key] = int(seeds[kind][0])
    sk["algorithm_seed"] = int(seeds["algorithm"][0])
    imit = T.build_alg(d)
    assert type(imit.expert) is GaussianActor
    assert same_weights(imit.expert.get_weights(), logs[0]["final"]["actor_weights"])
    imit.expert.set_rms(imit.expert_normalizer)
    imit._expert_engine_for()
    got = np.asarray(imit.expert.sample(s, deterministic=True))
    err = float(np.max(np.abs(got - want)))
    print(f"expert round trip: max |expert - trained| = {err:.3e} over {want.shape} actions (|a| up to {np.abs(want).max():.3f})")
    assert got.shape == want.shape == (8, 1) and err <= 2e-5
