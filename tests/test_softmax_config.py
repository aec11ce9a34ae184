"""SoftMaxActor on the trainable handle without a GPU: ``init_actor``'s dispatch, ``sacx_softmax_init``'s
refusals with their messages, the unchanged layout (with and without the call, and composed with the
VCritic and TRPO inits in any order), the host class's unbound errors, ``EngineConfig(softmax=True)``'s
requirements and ``MBRLOnPolicyAlg``'s refusal."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from test_ppo_config import _cfg, _create, _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Obs:
    def __init__(self, n):
        self.shape = (n,)


class _Discrete:
    def __init__(self, n):
        self.n = n
        self.shape = ()


class _Env:
    def __init__(self, S=4, n=3):
        self.observation_space, self.action_space = _Obs(S), _Discrete(n)


KW = dict(actor_layers=[64, 32], actor_activations=["tanh"], actor_gain=0.01, actor_std_mult=0.7,
          actor_init_type="orthogonal", actor_layer_norm=False, actor_weights=None)


def test_init_actor_returns_a_softmax_actor_for_a_discrete_space():
    from sac_eo.actors.discrete_actors import SoftMaxActor
    from sac_eo.actors.init_actor import init_actor
    # the continuous flags are ignored, as the reference ignores them
    actor = init_actor(_Env(4, 3), actor_squash=True, actor_per_state_std=True, actor_output_norm=True, **KW)
    assert type(actor) is SoftMaxActor and actor.a_dim == 3 and actor.s_dim == 4
    w = actor.get_weights()
    assert [x.shape for x in w] == [(4, 64), (64,), (64, 32), (32,), (32, 3), (3,)]
    assert actor.d == sum(x.size for x in w) == 4 * 64 + 64 + 64 * 32 + 32 + 32 * 3 + 3
    assert len(actor.trainable) == 6 and actor.get_weights(flat=True).shape == (actor.d,)
    assert actor.clip(2) == 2
    ln = init_actor(_Env(4, 3), **{**KW, "actor_layer_norm": True})
    assert ln.d == actor.d + 2 * 64 and len(ln.get_weights()) == 8
    given = init_actor(_Env(4, 3), **{**KW, "actor_weights": [x + 1 for x in w]})
    assert all(np.array_equal(x, y + 1) for x, y in zip(given.get_weights(), w))

    class _Other:
        shape = (2,)
    env = _Env()
    env.action_space = _Other()
    with pytest.raises(TypeError):
        init_actor(env, **KW)
    with pytest.raises(NotImplementedError, match="32"):
        init_actor(_Env(4, 33), **KW)


def test_set_weights_flat_and_increment_floor_nothing():
    from sac_eo.actors.discrete_actors import SoftMaxActor
    actor = SoftMaxActor(_Env(4, 3), [8], ["tanh"], 0.01, rng=np.random.default_rng(0))
    flat = actor.get_weights(flat=True)
    actor.set_weights(np.full(actor.d, -20.0, np.float32), from_flat=True)
    assert all((x == -20).all() for x in actor.get_weights())
    actor.set_weights(flat + 20, from_flat=True, increment=True)
    assert np.allclose(actor.get_weights(flat=True), flat, atol=1e-5)
    with pytest.raises(ValueError):
        actor.set_weights(np.zeros(actor.d + 1), from_flat=True)


def test_unbound_methods_raise():
    from sac_eo.actors.discrete_actors import SoftMaxActor
    actor = SoftMaxActor(_Env(4, 3), [8], ["tanh"], 0.01, rng=np.random.default_rng(0))
    s = np.zeros((2, 4))
    for call in (lambda: actor.neglogp(s, [0, 1]), lambda: actor.entropy(s), lambda: actor.kl(s, np.zeros((2, 3))),
                 lambda: actor.get_kl_info(s), lambda: actor.sample(s)):
        with pytest.raises(RuntimeError, match="not bound"):
            call()


def test_the_export_and_the_unchanged_config():
    from sac_eo import _native as N
    text = open(os.path.join(ROOT, "include", "sacx.h")).read()
    assert re.search(r"#define SACX_ABI_VERSION 8\b", text) and ctypes.sizeof(N.Config) == 392
    assert "sacx_softmax_init" in N.EXPORTS and hasattr(N.lib(), "sacx_softmax_init")
    assert re.search(r"\bsacx_softmax_init\(", text) and "discrete_actors.py:8-117" in text
    assert sorted(N.EXPORTS) == sorted(set(re.findall(r"\b(sacx_[a-z_]+)\s*\(", text)))


def test_refusals_with_their_messages():
    lib, h, rc, msg = _create(_cfg(a_dim=3).to_c())
    assert rc == 0, msg
    assert lib.sacx_softmax_init(h) == 0, lib.sacx_last_error(h)
    assert lib.sacx_softmax_init(h) != 0 and b"already called" in lib.sacx_last_error(h)
    lib.sacx_destroy(h)
    for ag in (False, True):                               # not a train handle
        lib, h, rc, msg = _create(_cfg(a_dim=3, actor_gaussian=ag).to_c())
        assert rc == 0, msg
        assert lib.sacx_softmax_init(h) != 0 and b"not a trainable GaussianActor handle" in lib.sacx_last_error(h)
        lib.sacx_destroy(h)
    lib, h, rc, msg = _create(_cfg(a_dim=3, per_state_std=True).to_c())
    assert rc == 0, msg
    assert lib.sacx_softmax_init(h) != 0 and b"per_state_std" in lib.sacx_last_error(h)
    lib.sacx_destroy(h)
    lib, h, rc, msg = _create(_cfg(a_dim=3, world_models=True, model_hidden=(16, 16), model_batch=8).to_c())
    assert rc == 0, msg
    assert lib.sacx_softmax_init(h) != 0 and b"continuous actions" in lib.sacx_last_error(h)
    lib.sacx_destroy(h)
    src = open(os.path.join(ROOT, "sac-expert_amd", "csrc", "sacx.cpp")).read()
    assert "sacx_softmax_init must precede sacx_bind" in src          # (a bound handle needs a GPU: test_gpu_softmax)


def test_the_layout_is_unchanged_and_the_inits_compose_in_any_order():
    lib, h0, rc, msg = _create(_cfg(a_dim=3).to_c())
    plain, bytes0 = _layout(lib, h0), lib.sacx_arena_bytes(h0)
    lib.sacx_destroy(h0)
    lib, h, rc, msg = _create(_cfg(a_dim=3).to_c())
    assert lib.sacx_softmax_init(h) == 0
    assert _layout(lib, h) == plain and lib.sacx_arena_bytes(h) == bytes0
    lib.sacx_destroy(h)
    lib, h0, rc, msg = _create(_cfg(a_dim=3).to_c())
    assert lib.sacx_vcritic_init(h0, 2) == 0 and lib.sacx_trpo_init(h0) == 0
    both, bytes_both = _layout(lib, h0), lib.sacx_arena_bytes(h0)
    lib.sacx_destroy(h0)
    calls = {"s": lambda l, h: l.sacx_softmax_init(h), "v": lambda l, h: l.sacx_vcritic_init(h, 2),
             "t": lambda l, h: l.sacx_trpo_init(h)}
    for order in itertools.permutations("svt"):
        lib, h, rc, msg = _create(_cfg(a_dim=3).to_c())
        for k in order:
            assert calls[k](lib, h) == 0, (order, k, lib.sacx_last_error(h))
        segs = _layout(lib, h)
        assert {n: v for n, v in segs.items() if n in plain} == plain, order
        assert set(segs) == set(both) and lib.sacx_arena_bytes(h) <= bytes_both, order
        for n in both:                                     # the flat vectors may be the shorter net-only ones
            assert segs[n][1] == both[n][1] and segs[n][2] <= both[n][2], (order, n)
        # they hold the net only: actor.l0 up to where actor.logstd begins
        nv = (plain["actor.logstd"][0] - plain["actor.l0"][0]) // 4
        assert nv <= segs["trpo.vec"][2], order
        lib.sacx_destroy(h)


def test_engine_config_requirements():
    from sac_eo.engine import EngineConfig
    for ag in (False, True):
        with pytest.raises(ValueError, match="actor_gaussian='train'"):
            EngineConfig(s_dim=3, a_dim=2, softmax=True, actor_gaussian=ag)
    with pytest.raises(ValueError, match="per_state_std"):
        EngineConfig(s_dim=3, a_dim=2, softmax=True, actor_gaussian="train", per_state_std=True)
    with pytest.raises(ValueError, match="world_models"):
        EngineConfig(s_dim=3, a_dim=2, softmax=True, actor_gaussian="train", world_models=True)
    assert EngineConfig(s_dim=3, a_dim=2, softmax=True, actor_gaussian="train").softmax is True
    assert EngineConfig(s_dim=3, a_dim=2).softmax is False


def test_algorithms_accept_or_refuse_a_softmax_actor():
    from sac_eo.actors.discrete_actors import SoftMaxActor
    from sac_eo.algs.mbrl_onpolicy_alg import MBRLOnPolicyAlg
    from sac_eo.algs.model_free import PPO
    from sac_eo.algs.model_free.trpo import TRPO
    from test_ppo_config import KW as PPO_KW
    from test_trpo_config import KW as TRPO_KW
    actor = SoftMaxActor(_Env(4, 3), [8], ["tanh"], 0.01, rng=np.random.default_rng(0))
    assert PPO(actor, PPO_KW).actor is actor and TRPO(actor, TRPO_KW).actor is actor
    with pytest.raises(ValueError, match="continuous actions"):
        MBRLOnPolicyAlg(0, _Env(), _Env(), actor, [], [], None, None)
