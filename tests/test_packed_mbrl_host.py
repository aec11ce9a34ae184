"""``--pack_runs`` on the CPU stand-in engine (tests/fake_engine_packed.py): ``python -m sac_eo.train --alg_type
mbrl --mf_algo ppo --runs 2 --pack_runs`` against the same command without the flag, at the loop sizes of
tests/test_mbrl_config.py -- both runs' logs key by key (all but ``time_*``), each run's stream at the end,
every steps call each learner saw, one packed steps call per critic round and per actor round, and the
divergences that must raise."""
import numpy as np
import pytest

from test_mbrl_config import ENSEMBLE_KEYS, LOOP, TRAIN_KEYS, _argv


def _same(a, b, path):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            if not str(k).startswith("time_"):
                _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        x, y = np.asarray(a), np.asarray(b)
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), path
    else:
        assert type(a) is type(b) and (a == b or (a != a and b != b)), (path, a, b)


def _run(monkeypatch, tmp, extra, hook=None):
    """One command on the stand-in -> (the runs' logs, the engines built, the algorithms built)."""
    import fake_engine_packed as F
    import sac_eo.train as T
    from sac_eo.common.logger import load_log
    F.install(monkeypatch)
    algs = []
    real_build = T.build_alg

    def build(inputs, pack=None):
        alg = real_build(inputs, pack)
        algs.append(alg)
        if hook:
            hook(len(algs) - 1, alg)
        return alg
    monkeypatch.setattr(T, "build_alg", build)
    try:
        logs = load_log(T.main(_argv(tmp, ("--runs", "2") + tuple(extra))))
    finally:
        monkeypatch.setattr(T, "build_alg", real_build)
    return logs, list(F.ENGINES), algs


def _streams(engines):
    out = []
    for e in engines:
        for k in range(e.seeds):
            e.select_seed(k)
            out.append((e.rng_get_state(), list(e.S["steps_log"])))
    return out


@pytest.mark.parametrize("extra", [(), ("--critic_ensemble", "--num_models", "3", "--model_holdout_ratio", "0.25",
                                        "--model_holdout_epochs", "2")])
def test_packed_runs_log_what_the_serial_runs_log(monkeypatch, tmp_path, extra):
    from sac_eo.engine import SeedView
    serial, s_eng, s_algs = _run(monkeypatch, tmp_path, extra)
    packed, p_eng, p_algs = _run(monkeypatch, tmp_path, extra + ("--pack_runs",))
    assert len(serial) == len(packed) == 2
    # serial: one engine per run; packed: both runs on the learners of ONE engine
    assert [e.seeds for e in s_eng] == [1, 1] and [e.seeds for e in p_eng] == [2]
    assert p_eng[0].cfg.learners == 2 and s_eng[0].cfg.learners == 0
    assert all(isinstance(a.engine, SeedView) and a.engine._eng is p_eng[0] for a in p_algs)
    assert [a.engine.seed_index for a in p_algs] == [0, 1]
    for r in range(2):
        assert set(packed[r]["train"]) == set(TRAIN_KEYS + ENSEMBLE_KEYS)
        _same(serial[r]["train"], packed[r]["train"], f"run{r}.train")
        _same(serial[r]["final"], packed[r]["final"], f"run{r}.final")
        assert set(serial[r]) == set(packed[r])
        _same(serial[r]["param"], packed[r]["param"], f"run{r}.param")
    assert not np.array_equal(np.asarray(serial[0]["train"]["tv"]), np.asarray(serial[1]["train"]["tv"]))   # two runs
    lr = [np.asarray(serial[r]["train"]["actor_lr"]) for r in range(2)]
    assert len(set(lr[0].tolist())) > 1 and not np.array_equal(lr[0], lr[1])       # adaptlr moved each its own way
    # each run's stream at the end, and every steps call it saw (shape, indices, rate), bit for bit
    for r, ((st_s, log_s), (st_p, log_p)) in enumerate(zip(_streams(s_eng), _streams(p_eng))):
        assert np.array_equal(st_s[1], st_p[1]) and st_s[2:5] == st_p[2:5], r
        assert log_s == log_p and len(log_s) > 0, r
    # exactly one packed steps call per critic round and per actor round, none on a single learner
    L = LOOP
    iters = len(serial[0]["train"]["steps"])
    rounds = L["mf"] * iters
    pk = [c for c in p_eng[0].calls if isinstance(c, tuple) and c[0].endswith("_packed")]
    assert [c[0] for c in pk] == ["vcritic_steps_packed", "ppo_steps_packed"] * rounds
    assert all(c[1] == 2 for c in pk)
    nm = 3 if extra else 2
    rows = int(L["sim"] / nm) * nm
    assert {c[2:] for c in pk if c[0] == "ppo_steps_packed"} == {(L["a_it"] * L["a_nmb"], int(rows / L["a_nmb"]))}
    per = int(L["sim"] / nm) if extra else rows
    assert {c[2:] for c in pk if c[0] == "vcritic_steps_packed"} == {(L["c_it"] * L["c_nmb"], int(per / L["c_nmb"]))}
    assert not any(isinstance(c, tuple) and c[0].endswith("_packed") for e in s_eng for c in e.calls)


def test_pack_runs_is_off_by_default_and_needs_mbrl_ppo():
    import sac_eo.train as T
    from sac_eo.common.train_parser import create_train_parser
    p = create_train_parser()
    a = p.parse_args(["--alg_type", "mbrl", "--mf_algo", "ppo"])
    assert not hasattr(a, "pack_runs") and not T.pack_runs_ok(a, 4)       # absent: the namespace is what it was
    a = p.parse_args(["--alg_type", "mbrl", "--mf_algo", "ppo", "--pack_runs"])
    assert a.pack_runs is True
    assert T.pack_runs_ok(a, 4) and T.pack_runs_ok(a, 64) and not T.pack_runs_ok(a, 1) and not T.pack_runs_ok(a, 65)
    assert not T.pack_runs_ok(p.parse_args(["--alg_type", "mbrl", "--mf_algo", "ppo", "--pack_runs", "--serial_runs"]), 4)
    assert not T.pack_runs_ok(p.parse_args(["--alg_type", "mbrl", "--mf_algo", "trpo", "--pack_runs"]), 4)
    assert not T.pack_runs_ok(p.parse_args(["--alg_type", "sac", "--pack_runs"]), 4)
    from sac_eo.common.train_parser import all_kwargs
    assert not any("pack_runs" in v for v in all_kwargs.values())          # no logged kwarg: the params stay the reference's


@pytest.mark.parametrize("what", ["n_steps", "minibatch", "finishes_early"])
def test_a_divergence_raises(monkeypatch, tmp_path, what):
    def hook(i, alg):
        if i != 1:
            return
        if what == "n_steps":
            alg.critic_update.critic_update_it += 1
        elif what == "minibatch":
            alg.mf_algo.actor_nminibatch *= 2
        else:
            loop = alg._train_loop
            alg._train_loop = lambda total, params: loop(LOOP["init"], params)   # stops after its first env batch
    with pytest.raises(RuntimeError, match="packed runs diverged.*--serial_runs or drop --pack_runs"):
        _run(monkeypatch, tmp_path, ("--pack_runs",), hook)


def test_different_requests_in_one_round_raise():
    from sac_eo.algs.lockstep import run_lockstep_onpolicy

    class _Alg:
        def __init__(self, kinds):
            self.kinds = kinds

        def _train_loop(self, total, params):
            for k in self.kinds:
                yield (k, None, 1)
            return "name"

    class _Eng:
        seeds = 2
    with pytest.raises(RuntimeError, match="ask for different updates.*--serial_runs or drop --pack_runs"):
        run_lockstep_onpolicy([_Alg(["critic_update"]), _Alg(["actor_update"])], _Eng(), 1, [None, None])
    with pytest.raises(ValueError, match="one learner per learner"):
        run_lockstep_onpolicy([_Alg([])], _Eng(), 1, [None])


def test_update_packed_refuses_what_is_not_one_packed_engine(monkeypatch):
    from sac_eo.algs.model_free.packed import update_packed

    with pytest.raises(ValueError, match="one rollout per updater"):
        update_packed([], [])
    with pytest.raises(ValueError, match="list of PPO objects, or a list of VCriticUpdate"):
        update_packed([object()], [None])
