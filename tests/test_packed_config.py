"""Packed on-policy learners without a GPU: ``sacx_learners_init``'s refusals with their messages, the
per-learner layout against the one-learner handle's (with and without VCritics, softmax and the world
models), ``sacx_arena_bytes == K * sacx_seed_stride``, the three entry points on an unbound handle,
``EngineConfig(learners=...)``'s refusals, and the exports."""
import ctypes
import os
import re

import pytest

from test_ppo_config import _cfg, _create, _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sacx_learners_init", "sacx_ppo_steps_packed", "sacx_vcritic_steps_packed"]


def _inits(lib, h, vc, softmax):
    if vc:
        assert lib.sacx_vcritic_init(h, vc) == 0, lib.sacx_last_error(h)
    if softmax:
        assert lib.sacx_softmax_init(h) == 0, lib.sacx_last_error(h)


def test_exports_and_the_unchanged_config():
    from sac_eo import _native as N
    text = open(os.path.join(ROOT, "include", "sacx.h")).read()
    assert re.search(r"#define SACX_ABI_VERSION 8\b", text) and ctypes.sizeof(N.Config) == 392
    for s in NEW:
        assert s in N.EXPORTS and hasattr(N.lib(), s) and re.search(r"\b%s\(" % s, text), s
    m = re.search(r"^#define\s+SACX_MAX_LEARNERS\s+(\d+)", text, re.M)
    assert m and int(m.group(1)) == N.MAX_LEARNERS == 64
    # each carries the header comment citing what it restates
    for s in NEW:
        head = text[:text.index("int %s(" % s)]
        head = head[head.rindex("/*"):]
        for cite in ("train.py:148-152", "ppo.py:55-83", "base_onpolicy_alg.py:219-283"):
            assert cite in head, (s, cite)


@pytest.mark.parametrize("kw,vc,softmax", [
    (dict(), 0, False), (dict(), 2, False), (dict(a_dim=3), 1, True), (dict(world_models=True, num_models=2), 2, False),
    (dict(per_state_std=True, actor_layer_norm=True), 1, False)])
@pytest.mark.parametrize("K", [2, 5])
def test_the_learners_layout_is_the_one_learner_handles(kw, vc, softmax, K):
    lib, h0, rc, msg = _create(_cfg(**kw).to_c())
    assert rc == 0, msg
    _inits(lib, h0, vc, softmax)
    plain, bytes0, stride0 = _layout(lib, h0), lib.sacx_arena_bytes(h0), lib.sacx_seed_stride(h0)
    lib.sacx_destroy(h0)
    assert stride0 == bytes0                                 # one learner: one block, no rounding
    lib, h, rc, msg = _create(_cfg(**kw).to_c())
    assert rc == 0, msg
    _inits(lib, h, vc, softmax)
    assert lib.sacx_learners_init(h, K) == 0, lib.sacx_last_error(h)
    assert _layout(lib, h) == plain                          # byte for byte: names, offsets, shapes
    stride = lib.sacx_seed_stride(h)
    assert stride == (bytes0 + 65535) // 65536 * 65536       # rounded up to 64 KiB, as packed SAC handles
    assert lib.sacx_arena_bytes(h) == K * stride
    lib.sacx_destroy(h)


def test_refusals_with_their_messages():
    err = lambda lib, h: lib.sacx_last_error(h)
    for ag in (False, True):                                # a non-trainable handle
        lib, h, rc, msg = _create(_cfg(actor_gaussian=ag).to_c())
        assert rc == 0, msg
        assert lib.sacx_learners_init(h, 2) != 0 and b"not a trainable GaussianActor handle" in err(lib, h)
        lib.sacx_destroy(h)
    lib, h, rc, msg = _create(_cfg().to_c())
    for K in (-1, 0, 1, 65, 1000):                          # K out of range (and the handle stays as it was)
        assert lib.sacx_learners_init(h, K) != 0 and b"outside [2, SACX_MAX_LEARNERS = 64]" in err(lib, h), K
    assert lib.sacx_seed_stride(h) == lib.sacx_arena_bytes(h)
    assert lib.sacx_learners_init(h, 64) == 0
    assert lib.sacx_learners_init(h, 2) != 0 and b"already called" in err(lib, h)      # a second call
    assert lib.sacx_trpo_init(h) != 0 and b"sacx_learners_init" in err(lib, h) and b"TRPO" in err(lib, h)
    assert lib.sacx_vcritic_init(h, 1) != 0 and b"must precede sacx_learners_init" in err(lib, h)
    lib.sacx_destroy(h)
    lib, h, rc, msg = _create(_cfg().to_c())               # a handle that had sacx_trpo_init
    assert lib.sacx_trpo_init(h) == 0
    assert lib.sacx_learners_init(h, 2) != 0 and b"sacx_trpo_init" in err(lib, h) and b"one learner" in err(lib, h)
    lib.sacx_destroy(h)
    src = open(os.path.join(ROOT, "sac-expert_amd", "csrc", "sacx.cpp")).read()
    assert "sacx_learners_init must precede sacx_bind" in src           # (a bound handle needs a GPU: test_gpu_packed_onpolicy)
    assert "use sacx_ppo_steps_packed" in src and "use sacx_vcritic_steps_packed" in src


def test_sacx_config_seeds_stays_refused_on_a_trainable_handle():
    c = _cfg().to_c()
    c.seeds = 2
    lib, h, rc, msg = _create(c)
    assert rc != 0 and "seeds" in msg


def test_entry_points_on_an_unbound_handle_return_an_error():
    from sac_eo import _native as N
    for K in (0, 3):
        lib, h, rc, msg = _create(_cfg().to_c())
        assert rc == 0, msg
        assert lib.sacx_vcritic_init(h, 1) == 0
        if K:
            assert lib.sacx_learners_init(h, K) == 0
        par = (N.PpoParams * 3)()
        lrs = (ctypes.c_float * 3)(1e-3, 1e-3, 1e-3)
        idx = (ctypes.c_int32 * 12)()
        for i, f in enumerate([lambda: lib.sacx_ppo_steps_packed(h, idx, 1, 4, par, 0),
                               lambda: lib.sacx_vcritic_steps_packed(h, idx, 1, 4, lrs, 0)]):
            assert f() != 0, i
            assert b"not bound" in lib.sacx_last_error(h), i
        lib.sacx_destroy(h)


def test_engine_config_learners_refusals():
    from sac_eo.engine import EngineConfig
    assert EngineConfig(s_dim=3, a_dim=1).learners == 0
    assert EngineConfig(s_dim=3, a_dim=1, actor_gaussian="train", learners=4, vcritics=2).learners == 4
    for ag in (False, True):
        with pytest.raises(ValueError, match="actor_gaussian='train'"):
            EngineConfig(s_dim=3, a_dim=1, learners=2, actor_gaussian=ag)
    with pytest.raises(ValueError, match="trpo"):
        EngineConfig(s_dim=3, a_dim=1, learners=2, actor_gaussian="train", trpo=True)
    with pytest.raises(ValueError, match="seeds left at 1"):
        EngineConfig(s_dim=3, a_dim=1, learners=2, actor_gaussian="train", seeds=2)
    for K in (1, -2, 65):
        with pytest.raises(ValueError, match=r"in \[2, 64\]"):
            EngineConfig(s_dim=3, a_dim=1, learners=K, actor_gaussian="train")
    # host-only: sacx_config does not carry it
    assert EngineConfig(s_dim=3, a_dim=1, actor_gaussian="train", learners=4).to_c().seeds == 1
