"""The model-based on-policy data path on a world-models handle (EngineConfig(world_models=True):
SACX_EXPERT_MODELS) against tests/mbrl_ref.py.

* ``sim_collect``: the index draw, the ring rows in logical order (a wrapped ring: 50 rows into capacity
  40) and the rollout under GaussianActor.sample -- start states and the stream afterwards exact, rows
  within the rollout bar of tests/test_gpu_ref_fixtures.py (1e-4 of the tensor's max);
* the clip: with a wide policy the stored action is raw and the model steps on clip(a);
* ``sim_collect`` == host-drawn indices + ``Engine.rollout`` on the same handle, and graph replay ==
  eager over two calls, bit for bit;
* the model fit on a world-models handle == the same steps on an SAC-EO handle, bit for bit;
* ``model_losses_eval`` against fp64 at the 2e-5 loss bar;
* the calls that need expert rows, an empty ring and bad sizes fail with messages.
* the host loop: ``python -m sac_eo.train --alg_type mbrl --mf_algo ppo``; CUDA rows into the updates == NumPy
  rows; one whole ``MBRLOnPolicyAlg._update()`` against ``mbrl_ref.UpdateRef`` (fp64; the fp32 envelope under
  ``sac_oracle.MATMUL_ORDERS``): the stream bit-exact, every logged loss and the final weights within
  max(2e-5 / 1e-6, envelope), envelope < 1e-2.
"""
import numpy as np
import pytest

import mbrl_ref as M
import sac_oracle as O
from helpers import nontrivial_normalizers, relerr

pytestmark = pytest.mark.gpu

CAP, APPENDED = 40, 50
SHAPES = {
    "pendulum": dict(S=3, A=1, model_hidden=(32, 32), nm=2),
    "halfcheetah": dict(S=17, A=6, model_hidden=(96,), nm=3),
    "gauss": dict(S=3, A=1, model_hidden=(32, 32), nm=2, gaussian_model=True),
    # the advertised maximum; sim_collect rolls out its last model
    "eight": dict(S=3, A=1, model_hidden=(32, 32), nm=8, collect_model=7),
}


def _same_stream(eng, rs):
    dev, ref = eng.rng_get_state(), rs.get_state()
    return np.array_equal(dev[1], ref[1]) and dev[2] == ref[2] and dev[3] == ref[3] and dev[4] == ref[4]


def make_case(shape, seed=3, logstd=None, std_mult=1.0, capacity=CAP, appended=APPENDED, expert=False):
    """(engine, oracle cfg, fp64 state, normaliser, the ring's rows oldest first)."""
    from sac_eo.engine import Engine, EngineConfig
    c = SHAPES[shape]
    S, A, nm = c["S"], c["A"], c["nm"]
    gm = c.get("gaussian_model", False)
    ocfg = O.Config(S=S, A=A, hidden=(64, 64), act="tanh", model_hidden=c["model_hidden"], num_models=nm,
                    gaussian_model=gm)
    st = O.init_state(ocfg, seed=seed, with_models=True, bias_scale=0.05, actor_gain=0.5, model_gain=0.3,
                      model_std_mult=0.7)
    rs = np.random.RandomState(seed + 100)
    st.logstd = (np.full((1, A), -0.5) + 0.1 * rs.normal(size=(1, A))).astype(np.float32) if logstd is None \
        else np.full((1, A), logstd, np.float32)
    nrm = nontrivial_normalizers(rs, S, A)
    nrm.r_mean, nrm.r_den = np.float32(0.3), np.float32(1.7)
    kw = dict(s_dim=S, a_dim=A, hidden=(64, 64), activation="tanh", batch=16, buffer_capacity=capacity,
              model_hidden=c["model_hidden"], num_models=nm, model_batch=16, gaussian_model=gm, graph_steps=1)
    if expert:
        eng = Engine(EngineConfig(use_expert=True, expert_batch=2 * nm, expert_capacity=2 * nm, **kw))
    else:
        eng = Engine(EngineConfig(actor_gaussian="train", actor_std_mult=std_mult, world_models=True, **kw))
        eng.set_net("actor", st.actor)
        eng.set_logstd(st.logstd)
    for k in range(nm):
        eng.set_net(f"m{k}", st.models[k])
        if gm:
            eng.set_model_logstd(k, st.model_logstd[k])
    eng.set_normalizers(nrm.s_mean, nrm.s_den, nrm.a_mean, nrm.a_den, nrm.d_mean, nrm.d_den, nrm.r_mean, nrm.r_den,
                        nrm.ret_den)
    rows = dict(s=(rs.normal(size=(appended, S)) * 1.5).astype(np.float32),
                a=rs.uniform(-1, 1, (appended, A)).astype(np.float32),
                r=rs.normal(size=appended).astype(np.float32),
                sp=(rs.normal(size=(appended, S)) * 1.5).astype(np.float32),
                d=np.zeros(appended, np.float32))
    cut = 30 if appended > 30 else appended           # two appends: the second wraps the ring
    for lo, hi in ((0, cut), (cut, appended)):
        if hi > lo:
            eng.append(*[rows[k][lo:hi] for k in ("s", "a", "r", "sp", "d")])
    held = {k: M.ring_rows(v, capacity) for k, v in rows.items()}
    return eng, ocfg, st.astype(np.float64), nrm, held


COLLECT = [("pendulum", 1, 1, False), ("pendulum", 5, 5, False), ("halfcheetah", 5, 5, False),
           ("halfcheetah", 1, 5, True), ("halfcheetah", 4097, 2, False), ("gauss", 5, 5, False),
           ("eight", 5, 5, False), ("eight", 1, 5, True)]


@pytest.mark.parametrize("shape,n,H,det", COLLECT)
def test_sim_collect_against_the_restatement(gpu_available, shape, n, H, det):
    eng, ocfg, st, nrm, held = make_case(shape)
    assert held["s"].shape[0] == CAP and not np.array_equal(held["s"], eng.v["replay"][:, :ocfg.S].cpu().numpy())
    rs = np.random.RandomState(77)
    eng.rng_set_state(rs.get_state())
    k = SHAPES[shape].get("collect_model", 1)
    got = [t.cpu().numpy() for t in eng.sim_collect(k, n, H, deterministic=det, delta_clip=0.8, reward_clip=2.0)]
    idx, ref = M.sim_collect(st, ocfg, nrm, held["s"], n, H, k, rs, deterministic=det, delta_clip=0.8, reward_clip=2.0)
    S = ocfg.S
    errs = {k: relerr(g, r) for k, g, r in zip(("s", "a", "r", "sp"), got, ref)}
    print(f"{shape} n={n} H={H} det={det}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for g, r in zip(got, ref):
        assert g.shape == r.shape
    assert np.array_equal(got[0].reshape(n, H, S)[:, 0], held["s"][idx])      # the drawn ring rows, exactly
    assert _same_stream(eng, rs)
    assert not got[4].any() and np.array_equal(got[5], ref[5])
    assert max(errs.values()) < 1e-4, errs
    eng.close()


def test_the_model_steps_on_the_clipped_action(gpu_available):
    """std = 3 at act_limit 1: most |a| > act_limit.  a_out is the raw sample; sp follows the clipped
    restatement and misses an unclipped one by more than the bar."""
    eng, ocfg, st, nrm, held = make_case("halfcheetah", logstd=float(np.log(3.0)))
    n, H = 64, 3
    state = np.random.RandomState(5).get_state()
    eng.rng_set_state(state)
    got = [t.cpu().numpy() for t in eng.sim_collect(0, n, H)]
    outs = {}
    for clip in (True, False):
        rs = np.random.RandomState(0)
        rs.set_state(state)
        outs[clip] = M.sim_collect(st, ocfg, nrm, held["s"], n, H, 0, rs, clip_action=clip)[1]
    frac = float(np.mean(np.abs(got[1]) > ocfg.act_limit))
    e_clip, e_raw = relerr(got[3], outs[True][3]), relerr(got[3], outs[False][3])
    print(f"|a| > lim: {frac:.2f}; sp vs clipped {e_clip:.2e}, vs unclipped {e_raw:.2e}; a {relerr(got[1], outs[True][1]):.2e}")
    assert frac > 0.5
    # the first step's actions do not depend on the clip: raw in both restatements
    a0 = got[1].reshape(n, H, -1)[:, 0]
    assert relerr(a0, outs[False][1].reshape(n, H, -1)[:, 0]) < 1e-4
    assert e_clip < 1e-4 and e_raw > 1e-4
    assert relerr(got[1], outs[True][1]) < 1e-4
    eng.close()


@pytest.mark.parametrize("shape,n,H", [("pendulum", 5, 5), ("halfcheetah", 4097, 2)])
def test_sim_collect_equals_host_indices_plus_rollout(gpu_available, shape, n, H):
    eng, ocfg, st, nrm, held = make_case(shape)
    state = np.random.RandomState(11).get_state()
    eng.rng_set_state(state)
    a = [t.cpu().numpy() for t in eng.sim_collect(1, n, H, delta_clip=0.8)]
    end_a = eng.rng_get_state()
    rs = np.random.RandomState(0)
    rs.set_state(state)
    idx = M.draw_indices(rs, CAP, n)
    eng.rng_set_state(rs.get_state())
    b = [t.cpu().numpy() for t in eng.rollout(1, held["s"][idx], H, delta_clip=0.8)]
    end_b = eng.rng_get_state()
    S, A = ocfg.S, ocfg.A
    for x, y, w in zip(a[:4], b[:4], (S, A, 0, S)):
        assert np.array_equal(x, y.reshape(-1, w) if w else y.reshape(-1))
    assert np.array_equal(end_a[1], end_b[1]) and end_a[2:5] == end_b[2:5]
    eng.close()


def test_graph_replay_equals_eager(gpu_available, monkeypatch):
    outs = {}
    for mode in ("graph", "eager"):
        if mode == "eager":
            monkeypatch.setenv("SACX_ROLL_GRAPH", "0")
        eng, ocfg, st, nrm, held = make_case("halfcheetah")
        eng.rng_set_state(np.random.RandomState(19).get_state())
        calls = [[t.cpu().numpy() for t in eng.sim_collect(2, 7, 3)] for _ in range(2)]      # capture, then replay
        outs[mode] = calls + [eng.rng_get_state()]
        eng.close()
    for c in range(2):
        for x, y in zip(outs["graph"][c], outs["eager"][c]):
            assert np.array_equal(x, y)
    assert not np.array_equal(outs["graph"][0][0], outs["graph"][1][0])               # the second call drew anew
    assert np.array_equal(outs["graph"][2][1], outs["eager"][2][1]) and outs["graph"][2][2:5] == outs["eager"][2][2:5]


def _fit_on_both_handle_kinds(shape, steps=3):
    nm = SHAPES[shape]["nm"]
    idx = np.random.RandomState(13).randint(CAP, size=(steps, nm, 16))
    res = []
    for expert in (False, True):
        eng, ocfg, st, nrm, held = make_case(shape, expert=expert)
        eng.model_fit(idx)
        eng.sync()
        res.append(([w for k in range(nm) for w in eng.get_net(f"m{k}")], eng.model_stats(steps).copy()))
        if not expert:
            init = [np.asarray(w, np.float32) for k in range(nm) for w in st.models[k]]
            assert not any(np.array_equal(a, b) for a, b in zip(res[0][0], init))      # trained
        eng.close()
    assert len(res[0][0]) == len(res[1][0]) == nm * (2 * len(SHAPES[shape]["model_hidden"]) + 2)
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(res[0][1], res[1][1]) and np.all(np.isfinite(res[0][1]))


def test_model_fit_equals_an_eo_handle(gpu_available):
    """3 steps of model_fit (2 models, minibatch 16) on the world-models handle and on an SAC-EO handle
    with the same weights, normaliser and ring: the same launches and arithmetic, bit for bit."""
    _fit_on_both_handle_kinds("pendulum")


def test_model_fit_equals_an_eo_handle_eight_models(gpu_available):
    """The same at 8 models: 24 dW problems, three model.adam launches on either handle kind."""
    _fit_on_both_handle_kinds("eight")


def _losses_eval(shape, n, models):
    eng, ocfg, st, nrm, held = make_case(shape)
    r = np.random.RandomState(n)
    s = (r.normal(size=(n, ocfg.S)) * 1.5).astype(np.float32)
    a = r.uniform(-1, 1, (n, ocfg.A)).astype(np.float32)
    sp = (s + r.normal(size=(n, ocfg.S)) * 0.3).astype(np.float32)
    rr = r.normal(size=n).astype(np.float32)
    for k in models:
        got = eng.model_losses_eval(k, s, sp, a, rr)
        ref = M.losses_eval(st, ocfg, nrm, k, s, sp, a, rr)
        print(f"{shape} n={n} model {k}: mse {got[0]:.6g} / {ref[0]:.6g}  r {got[1]:.6g} / {ref[1]:.6g}")
        assert abs(got[0] - ref[0]) <= 2e-5 * abs(ref[0]) and abs(got[1] - ref[1]) <= 2e-5 * abs(ref[1]), (got, ref)
    eng.close()


@pytest.mark.parametrize("shape", ["halfcheetah", "gauss"])
@pytest.mark.parametrize("n", [1, 17, 1025, 4100])
def test_model_losses_eval(gpu_available, shape, n):
    _losses_eval(shape, n, range(2))


@pytest.mark.parametrize("n", [1, 1025])
def test_model_losses_eval_eight_models(gpu_available, n):
    _losses_eval("eight", n, (0, 5, 7))


def test_refusals_on_the_device(gpu_available):
    from sac_eo._native import SacxError
    eng, ocfg, st, nrm, held = make_case("gauss", appended=0)
    with pytest.raises(SacxError, match="ring is empty"):
        eng.sim_collect(0, 4, 2)
    z = np.zeros((4, ocfg.S), np.float32)
    eng.append(z, np.zeros((4, ocfg.A), np.float32), np.zeros(4, np.float32), z, np.zeros(4, np.float32))
    for n, H in ((-1, 2), (2, -1)):
        with pytest.raises(SacxError, match="must be >= 0"):
            eng.sim_collect(0, n, H)
    with pytest.raises(SacxError, match="at most 4096 trajectories"):       # GaussianModel: as sacx_rollout
        eng.sim_collect(0, 4097, 1)
    with pytest.raises(SacxError, match="model index"):
        eng.sim_collect(2, 4, 2)
    before = eng.rng_get_state()
    assert [int(t.shape[0]) for t in eng.sim_collect(0, 0, 3)] == [0] * 6 and eng.rng_get_state()[2] == before[2]
    with pytest.raises(SacxError, match="no expert rows"):
        eng.set_expert(z[:2], z[:2], 0.1)
    with pytest.raises(SacxError, match="sacx_perm_push"):
        eng.push_perms(np.zeros((1, 2), np.int32))
    with pytest.raises(SacxError, match="sacx_expert_diag"):
        eng.expert_diag(z, np.zeros((4, ocfg.A), np.float32), z)
    eng.close()
    eo, *_ = make_case("pendulum", expert=True)
    with pytest.raises(SacxError, match="SACX_EXPERT_MODELS handle only"):
        eo.sim_collect(0, 4, 2)
    eo.close()


# ------------------------------------------------------------------------------------------ host loop
TRAIN_KEYS = ["J_tot", "steps", "traj", "time_env_data", "J_tot_eval", "steps_eval", "time_eval",
              "time_model_fit", "model_ent", "model_loss_epochs", "steps_update", "time_actor", "time_critic",
              "time_sim_data", "ent", "tv", "kl", "alpha", "actor_lr", "outside_clip", "actor_grad_norm_pre",
              "actor_grad_norm", "ent_agg", "kl_agg", "alpha_agg", "time_ac_agg"]
ENSEMBLE_KEYS = ["critic_loss", "model_loss", "model_loss_train", "model_loss_holdout", "model_loss_mse",
                 "model_loss_reward"]
FINAL_KEYS = {"actor_weights", "critic_weights", "rms_stats", "model_weights", "reward_weights"}


def _argv(tmp, extra=()):
    return ["--alg_type", "mbrl", "--mf_algo", "ppo", "--env_name", "HalfCheetah-v3", "--actor_layers", "64", "64",
            "--critic_layers", "64", "64", "--model_layers", "32", "32", "--total_timesteps", "700",
            "--env_batch_size_init", "300", "--env_batch_size", "200", "--env_horizon", "100", "--sim_batch_size", "400",
            "--sim_horizon", "5", "--num_mf_updates", "2", "--actor_update_it", "2", "--actor_nminibatch", "4",
            "--critic_update_it", "2", "--critic_nminibatch", "4", "--model_batch_size", "50", "--model_num_epochs", "2",
            "--eval_freq", "400", "--eval_num_traj", "1", "--seed", "3", "--save_path", str(tmp)] + list(extra)


@pytest.mark.parametrize("extra", [(), ("--critic_ensemble", "--model_holdout_ratio", "0.25", "--num_models", "3",
                                        "--sim_batch_size", "404")])
def test_train_entry_point_mbrl(gpu_available, tmp_path, extra):
    """``python -m sac_eo.train --alg_type mbrl --mf_algo ppo`` on a synthetic env: it finishes, the pickled
    log has the reference's keys, every value is finite (model_loss_holdout is inf without holdout)."""
    from sac_eo.common.logger import load_log
    from sac_eo.train import main
    log = load_log(main(_argv(tmp_path, extra)))[0]
    tr = log["train"]
    for k in TRAIN_KEYS + ENSEMBLE_KEYS:
        assert k in tr, k
    nm = 3 if extra else 2
    iters = len(tr["model_loss_epochs"])                   # env batches: 300, then 200 each up to >= 700
    assert iters == 3 and len(tr["steps_update"]) == 2 * iters and len(tr["ent_agg"]) == iters
    assert np.asarray(tr["model_loss"]).shape == (iters, nm) and np.asarray(tr["model_ent"]).shape == (iters, nm)
    assert np.asarray(tr["critic_loss"]).shape == (2 * iters, nm if extra else 1)
    # the short last pass: 404 / 3 = 134 rows per model = 26 trajectories of 5 + one of 4
    assert set(np.asarray(tr["steps_update"]).tolist()) == ({3 * 134} if extra else {400})
    for k, v in tr.items():
        if k == "model_loss_holdout" and not extra:
            assert np.all(np.isinf(np.asarray(v)))
        else:
            assert np.all(np.isfinite(np.asarray(v, np.float64))), k
    assert set(log["final"]) == FINAL_KEYS
    assert len(log["final"]["model_weights"]) == nm and len(log["final"]["critic_weights"]) == (nm if extra else 1)
    assert all(np.all(np.isfinite(w)) for w in log["final"]["actor_weights"])
    assert np.all(np.asarray(tr["kl_agg"]) >= 0) and np.any(np.asarray(tr["kl_agg"]) > 0)      # the policy moved


def test_updates_take_device_rows_as_numpy_rows(gpu_available):
    """PPO.update / VCriticUpdate.update on CUDA tensors == the same rows as NumPy arrays, bit for bit."""
    import torch
    from test_ppo_config import KW, _Env
    from sac_eo.actors.continuous_actors import GaussianActor
    from sac_eo.algs.model_free import PPO, VCriticUpdate
    from sac_eo.critics.critics import VCritic
    res = []
    for dev in (False, True):
        np.random.seed(4)
        actor = GaussianActor(_Env(), [64, 64], ["tanh"], 0.5, "orthogonal", False, rng=np.random.default_rng(0))
        ppo = PPO(actor, dict(KW, vcritics=2, rollout_capacity=128))
        r = np.random.RandomState(9)
        s = r.normal(size=(120, 3)).astype(np.float32)
        a = r.normal(size=(120, 1)).astype(np.float32)
        adv = r.normal(size=120).astype(np.float32)
        rtg = [r.normal(size=60).astype(np.float32) for _ in range(2)]
        to = (lambda x: torch.as_tensor(x, device="cuda")) if dev else (lambda x: x)
        log_a = ppo.update((to(s), to(a), to(adv), None, None, None))
        crit = [VCritic(_Env(), [64, 64], ["tanh"], 1.0, rng=np.random.default_rng(k)) for k in range(2)]
        vu = VCriticUpdate(crit, dict(critic_lr=1e-3, critic_update_it=2, critic_nminibatch=4), actor)
        data = ([to(s[:60]), to(s[60:])], None, None, [to(x) for x in rtg], None, None)
        log_c = vu.update(data, 2)
        res.append((actor.get_weights(), [c.get_weights() for c in crit], log_a, log_c, ppo.engine.rng_get_state()))
        ppo.engine.close()
    for x, y in zip(res[0][0], res[1][0]):
        assert np.array_equal(x, y)
    for cx, cy in zip(res[0][1], res[1][1]):
        for x, y in zip(cx, cy):
            assert np.array_equal(x, y)
    assert res[0][2] == res[1][2] and res[0][3] == res[1][3]
    assert np.array_equal(res[0][4][1], res[1][4][1]) and res[0][4][2:5] == res[1][4][2:5]


# ------------------------------------------------------------------------------------------ one whole _update()
UPD = dict(S=3, A=1, rows=60, sim=40, horizon=5, nm=2, mf=2, its=2, nmb=4, epochs=2, mb=16)
UPD_SEEDS = {(1, 0.0): 1, (2, 0.0): 1, (1, 0.25): 1, (2, 0.25): 1}      # (critics, holdout) -> seed, checked on the CPU:
#                                                    the restatement's own fp32 envelope stays below 1e-2 for them
PPO_KW = dict(actor_lr=3e-4, actor_update_it=UPD["its"], actor_nminibatch=UPD["nmb"], adv_center=True, adv_scale=True,
              eps_ppo=0.2, max_grad_norm=0.5, adaptlr=True, adapt_factor=0.03, adapt_minthresh=0.0, adapt_maxthresh=1.0,
              ent_reg=False, ent_targ=-float(UPD["A"]), alpha_lr=3e-4)
PPO_LOG = ("ent", "tv", "kl", "alpha", "actor_lr", "outside_clip", "actor_grad_norm_pre", "actor_grad_norm")
MODEL_LOG = ("model_loss", "model_loss_train", "model_loss_holdout", "model_loss_mse", "model_loss_reward")


class _UBox:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, np.float32), np.ones(n, np.float32)


class _UEnv:
    observation_space, action_space = _UBox(UPD["S"]), _UBox(UPD["A"])


def alg_kwargs(nc, holdout):
    return dict(gamma=0.99, lam=0.95, env_buffer_size=None, mf_algo="ppo", total_timesteps=UPD["rows"], env_horizon=30,
                env_batch_type="steps", env_batch_size_init=UPD["rows"], env_batch_size=30, critic_lr=1e-3,
                critic_update_it=UPD["its"], critic_nminibatch=UPD["nmb"], num_mf_updates=UPD["mf"], sim_buffer_size=None,
                sim_horizon=UPD["horizon"], sim_batch_type="steps", sim_batch_size=UPD["sim"], model_lr=1e-3,
                reset_model_optimizer=False, model_num_epochs=UPD["epochs"], model_batch_size=UPD["mb"],
                model_batch_shuffle=True, model_max_updates=1e5, model_max_grad_norm=None, model_holdout_ratio=holdout,
                model_holdout_epochs=5)


def update_case(nc, holdout, seed):
    """The host objects of one learner (unbound: their weights are NumPy), the env rows, the normaliser the
    loop would hold after them, and the restatement's states built from the same weights."""
    import ppo_ref as R
    import vcritic_ref as V
    from sac_eo.actors.continuous_actors import GaussianActor
    from sac_eo.common.normalizer import RunningNormalizers
    from sac_eo.critics.critics import VCritic
    from sac_eo.models.continuous_models import MSEModel
    S, A, n = UPD["S"], UPD["A"], UPD["rows"]
    g = lambda k: np.random.default_rng(1000 * seed + k)
    actor = GaussianActor(_UEnv(), [64, 64], ["tanh"], 0.5, "orthogonal", False, rng=g(0))
    rs = np.random.RandomState(seed)
    w = actor.get_weights()
    w[-1] = (0.1 * rs.normal(size=(1, A)) - 0.5).astype(np.float32)
    actor.set_weights(w)
    critics = [VCritic(_UEnv(), [64, 64], ["tanh"], 1.0, rng=g(10 + k)) for k in range(nc)]
    models = [MSEModel(_UEnv(), [32, 32], ["relu"], 0.3, [32, 32], ["relu"], 0.3, {}, rng=g(20 + k)) for k in range(UPD["nm"])]
    s = (rs.normal(size=(n, S)) * 1.5).astype(np.float32)
    rows = dict(s=s, a=rs.uniform(-1, 1, (n, A)).astype(np.float32), r=rs.normal(size=n).astype(np.float32),
                sp=(s + 0.3 * rs.normal(size=(n, S))).astype(np.float32), d=np.zeros(n))
    norm = RunningNormalizers(S, A, 0.99, None)
    for lo in (0, n // 2):                                # two trajectories, as the env loop would add them
        norm.update_rms(*[rows[k][lo:lo + n // 2] for k in ("s", "a", "r", "sp")])
    f = lambda x, m: np.broadcast_to(np.asarray(x, np.float32), (m,)).copy()
    one = lambda x: np.float32(np.asarray(x).reshape(-1)[0])
    nrm = O.Normalizers(f(norm.s_rms.mean, S), f(norm.s_rms.den(), S), f(norm.a_rms.mean, A), f(norm.a_rms.den(), A),
                        f(norm.delta_rms.mean, S), f(norm.delta_rms.den(), S), one(norm.r_rms.mean), one(norm.r_rms.den()),
                        one(norm.ret_rms.den()))
    cfg = O.Config(S=S, A=A, hidden=(64, 64), actor_acts=("tanh", "tanh"), model_hidden=(32, 32), model_act="relu",
                   num_models=UPD["nm"], lr_model=1e-3, act_limit=1.0)
    sac = O.init_state(cfg, seed=1, with_models=True)
    sac.models = [[np.asarray(x, np.float32) for x in m.get_weights()] for m in models]
    sac.opt_model = O.AdamState.zeros_like(sac.model_all_vars())
    alpha = np.zeros((), np.float32)
    ppo = R.PPOState([x.copy() for x in w[:-1]], w[-1].copy(), None, alpha, O.AdamState.zeros_like([alpha]), 1.0)
    ppo.opt_actor = O.AdamState.zeros_like(ppo.trainables(cfg))
    vst = V.VState([[np.asarray(x, np.float32) for x in c.get_weights()] for c in critics], None)
    vst.opt = O.AdamState.zeros_like(vst.trainables())
    return dict(actor=actor, critics=critics, models=models, rows=rows, norm=norm, nrm=nrm, cfg=cfg, sac=sac, ppo=ppo,
                vst=vst)


def run_restatement(case, nc, holdout, dt, order="default", stream_seed=31):
    """One _update() of the restatement in dtype dt -> (its logs, its states, the stream afterwards)."""
    rows = case["rows"]
    ref = M.UpdateRef(case["sac"].astype(dt), case["ppo"].astype(dt), case["vst"].astype(dt), case["cfg"],
                      ("tanh", "tanh"), case["nrm"], (rows["s"], rows["a"], rows["sp"], rows["r"]), alg_kwargs(nc, holdout),
                      PPO_KW, np.random.RandomState(stream_seed))
    O.MATMUL_ORDER = order
    try:
        logs = ref.update()
    finally:
        O.MATMUL_ORDER = "default"
    return logs, ref, ref.rs.get_state()


def flat_figures(logs, ref, cfg):
    """{name: value} of every logged loss (relative bar 2e-5) and {name: array} of the final weights (1e-6)."""
    vals = {}
    for k, m in enumerate(logs["models"]):
        for key in MODEL_LOG:
            if np.isfinite(m[key]):
                vals[f"{key}[{k}]"] = float(m[key])
    for u, upd in enumerate(logs["updates"]):
        for key in PPO_LOG:
            vals[f"update {u} {key}"] = float(upd[key])
        for c, x in enumerate(upd["critic_loss"]):
            vals[f"update {u} critic_loss[{c}]"] = float(x)
    for key, x in logs["agg"].items():
        vals[key] = float(x)
    ws = {f"actor {i}": np.asarray(x, np.float64) for i, x in enumerate(ref.ppo.trainables(cfg))}
    for c, w in enumerate(ref.vst.critics):
        ws.update({f"critic {c} {i}": np.asarray(x, np.float64) for i, x in enumerate(w)})
    for k, w in enumerate(ref.sac.models):
        ws.update({f"model {k} {i}": np.asarray(x, np.float64) for i, x in enumerate(w)})
    return vals, ws


def envelopes(case, nc, holdout):
    """The fp64 restatement, and its fp32 runs under every summation order against it."""
    l64, r64, stream = run_restatement(case, nc, holdout, np.float64)
    v64, w64 = flat_figures(l64, r64, case["cfg"])
    env_v, env_w = {k: 0.0 for k in v64}, {k: 0.0 for k in w64}
    for order in O.MATMUL_ORDERS:
        l32, r32, s32 = run_restatement(case, nc, holdout, np.float32, order)
        assert np.array_equal(s32[1], stream[1]) and s32[2:5] == stream[2:5]
        v32, w32 = flat_figures(l32, r32, case["cfg"])
        for k in v64:
            env_v[k] = max(env_v[k], abs(v32[k] - v64[k]) / max(abs(v64[k]), 1e-30))
        for k in w64:
            env_w[k] = max(env_w[k], float(np.max(np.abs(w32[k] - w64[k]))))
    return l64, v64, w64, env_v, env_w, stream


@pytest.mark.parametrize("nc,holdout", list(UPD_SEEDS))
def test_one_update_against_the_restatement(gpu_available, nc, holdout):
    """MBRLOnPolicyAlg._update() (model fit on the ring's rows, holdout, the five losses; two policy updates:
    sim_collect per model, gae with the per-model critic, the critic update, PPO on the aggregate) against
    mbrl_ref.UpdateRef in fp64: the global stream bit-exact; every logged loss and the final weights within
    max(single-step bar, fp32 envelope), bars 2e-5 (losses, relative) and 1e-6 (weights, absolute), the
    envelope itself below 1e-2."""
    from sac_eo.algs.mbrl_onpolicy_alg import MBRLOnPolicyAlg
    case = update_case(nc, holdout, UPD_SEEDS[(nc, holdout)])
    l64, v64, w64, env_v, env_w, stream = envelopes(case, nc, holdout)
    alg = MBRLOnPolicyAlg(0, _UEnv(), _UEnv(), case["actor"], case["critics"], case["models"], alg_kwargs(nc, holdout),
                          dict(PPO_KW))
    alg.normalizer = case["norm"]
    alg._set_rms()
    rows, n = case["rows"], UPD["rows"]
    for lo in (0, n // 2):
        part = [rows[k][lo:lo + n // 2] for k in ("s", "a", "r", "sp", "d")]
        alg.env_data.add(*part)
        alg.engine.append(*part[:4], part[4].astype(np.float32))
    alg.engine.rng_set_state(np.random.RandomState(31).get_state())
    alg._update()
    tr = alg.logger.train_dict
    dev = {}
    for k in range(UPD["nm"]):
        for key in MODEL_LOG:
            if f"{key}[{k}]" in v64:
                dev[f"{key}[{k}]"] = float(np.asarray(tr[key][0])[k])
    for u in range(UPD["mf"]):
        for key in PPO_LOG:
            dev[f"update {u} {key}"] = float(tr[key][u])
        for c in range(nc):
            dev[f"update {u} critic_loss[{c}]"] = float(np.asarray(tr["critic_loss"][u])[c])
    for key in ("ent_agg", "kl_agg", "alpha_agg"):
        dev[key] = float(tr[key][0])
    dw = {f"actor {i}": x for i, x in enumerate(alg.actor.get_weights())}
    for c, cr in enumerate(alg.critics):
        dw.update({f"critic {c} {i}": x for i, x in enumerate(cr.get_weights())})
    for k, m in enumerate(alg.models):
        dw.update({f"model {k} {i}": x for i, x in enumerate(m.get_weights())})
    figures = []
    for k, want in v64.items():
        err = abs(dev[k] - want) / max(abs(want), 1e-30)
        print(f"{k}: device {dev[k]:.7g} ref {want:.7g} error {err:.2e} fp32 envelope {env_v[k]:.2e}")
        figures.append((k, err, env_v[k], 2e-5))
    for k, want in w64.items():
        err = float(np.max(np.abs(np.asarray(dw[k], np.float64).reshape(want.shape) - want)))
        print(f"final {k} {want.shape}: device error {err:.2e} fp32 envelope {env_w[k]:.2e}")
        figures.append((f"final {k}", err, env_w[k], 1e-6))
    got = alg.engine.rng_get_state()
    same = np.array_equal(got[1], stream[1]) and got[2:5] == stream[2:5]
    print(f"stream bit-exact: {same}; epochs {tr['model_loss_epochs']} / {l64['fit']['model_loss_epochs']}; "
          f"steps_update {tr['steps_update']}")
    assert same                                           # (every figure is printed before the first assertion)
    assert int(tr["model_loss_epochs"][0]) == l64["fit"]["model_loss_epochs"]
    assert [int(x) for x in tr["steps_update"]] == [u["steps_update"] for u in l64["updates"]]
    assert np.all(np.isinf(tr["model_loss_holdout"][0])) == (holdout == 0.0)
    for what, err, env, bar in figures:
        assert env < 1e-2, (what, env)
        assert err <= max(bar, env), (what, err, env)
    alg.engine.close()
