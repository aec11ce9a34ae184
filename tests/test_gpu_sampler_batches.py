"""The grown sampler batches of long graphs (sampler_sched.h: 1, 4, 16, 64 updates per k_rng +
k_gather launch on the 128-slot ring of the HalfCheetah-class handles) change when the randoms are
drawn, never which: the MT19937 stream is consumed in update order whatever the batching.

Small learners (S=17, A=6, hidden (64, 64), B=64, N=5000) at graph_steps = 256:
* step(300) (a 256-update graph: batches 1, 4, 16, 43, 64, 64, 64; then a 44-update one) == eager
  launches, bit for bit: statistics, params, Adam moments, the RNG state;
* two step(256) calls == 512 eager updates (the 128-slot ring wraps four times);
* the default growth == SACX_NBATCH=8 (the fixed schedule) on the same seeds;
* SAC-EO (20 expert rows): the expert permutation of an update follows pseq[slot] while the
  sampler runs 64 updates ahead;
* 2 packed seeds, 150 updates (one 150-update graph) == two one-seed engines run eagerly.
"""
import numpy as np
import pytest

from helpers import load_learner, make_learner, make_pair

pytestmark = pytest.mark.gpu

KW = dict(act="relu", hidden=(64, 64), B=64, N=5000, graph_steps=256)
_REF = {}


def _state(eng, n):
    key = eng.rng_get_state()
    return (eng.stats(n).copy(), eng.v["params"].cpu().numpy().copy(), eng.v["adam_m"].cpu().numpy().copy(),
            eng.v["adam_v"].cpu().numpy().copy(), np.asarray(key[1]).copy(), np.array([key[2], key[3]]),
            np.array([key[4]], np.float64))


def _run(calls, eager, seed=71, use_expert=False):
    """`calls` step() calls on a fresh learner; -> (stats, params, adam_m, adam_v, RNG key, pos / has_gauss, gauss)"""
    n = sum(calls)
    eng, *_ = make_pair(seed=seed, use_expert=use_expert, ne=20, model_hidden=(64, 64), **KW)
    eng.rng_set_state(np.random.RandomState(seed + 1).get_state())
    if use_expert:
        rs = np.random.RandomState(seed + 2)
        eng.push_perms(np.stack([rs.permutation(eng.cfg.expert_batch) for _ in range(n)]))
    done = 0
    for c in calls:
        eng.step(c, num_timesteps=done, ts_increment=1, eager=eager)
        done += c
    eng.sync()
    out = _state(eng, n)
    eng.close()
    return out


def _eager300():
    if "e300" not in _REF:          # computed once, shared, never modified
        _REF["e300"] = _run((300,), True)
    return _REF["e300"]


def _graph300():
    if "g300" not in _REF:
        _REF["g300"] = _run((300,), False)
    return _REF["g300"]


def _same(got, ref):
    for i, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(a, b), i


def test_grown_graph_equals_eager(gpu_available, monkeypatch):
    monkeypatch.delenv("SACX_NBATCH", raising=False)
    monkeypatch.delenv("SACX_NSLOT", raising=False)
    ref, got = _eager300(), _graph300()
    assert np.all(np.isfinite(got[0])) and np.array_equal(got[0][:, 7], np.arange(300, dtype=np.float32))
    _same(got, ref)


def test_ring_wraps_across_two_graphs(gpu_available):
    _same(_run((256, 256), False), _run((512,), True))


def test_growth_draws_the_fixed_schedules_stream(gpu_available, monkeypatch):
    grown = _graph300()
    monkeypatch.setenv("SACX_NBATCH", "8")
    _same(_run((300,), False), grown)


def test_expert_permutations_follow_the_ring(gpu_available):
    _same(_run((300,), False, seed=83, use_expert=True), _run((300,), True, seed=83, use_expert=True))


def test_two_packed_seeds_equal_single_engines(gpu_available):
    from sac_eo.engine import Engine, EngineConfig
    K, n, B, N = 2, 150, 64, 5000
    learners = [make_learner(act="relu", hidden=(64, 64), B=B, N=N, seed=90 + 3 * k) for k in range(K)]

    def cfg(seeds):
        return EngineConfig(s_dim=17, a_dim=6, hidden=(64, 64), activation="relu", batch=B, buffer_capacity=N,
                            graph_steps=256, seeds=seeds)

    def drive(eng, k):
        _, st, buf, nrm, ex = learners[k]
        load_learner(eng, st, buf, nrm, ex, 0.1)
        eng.rng_set_state(np.random.RandomState(300 + k).get_state())

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
        got.append(_state(packed, n))
    packed.close()
    for k in range(K):
        e = Engine(cfg(1))
        drive(e, k)
        e.step(n, eager=True)
        e.sync()
        ref = _state(e, n)
        e.close()
        _same(got[k], ref)
    assert not np.array_equal(got[0][1], got[1][1])     # the seeds are different learners
