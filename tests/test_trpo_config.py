"""The TRPO update on the trainable GaussianActor handle without a GPU: ``sacx_trpo_init``'s refusals, the
unchanged layout without it, every earlier segment's offset with it (with and without VCritics, in either
order), the entry points on an unbound handle, ``EngineConfig(trpo=True)``'s requirement, and the host
class's import path and refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_ppo_config import _Env, _cfg, _create, _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sacx_trpo_init", "sacx_trpo_begin", "sacx_trpo_grad", "sacx_trpo_fvp", "sacx_trpo_step", "sacx_trpo_plan_info"]
KW = dict(adv_center=True, adv_scale=True, delta_trpo=0.02, cg_it=20, trust_sub=1, trust_damp=0.01, kl_maxfactor=1.5,
          ent_reg=False, ent_targ=0.0, alpha_lr=1e-3)


def test_exports_and_the_unchanged_config():
    from sac_eo import _native as N
    text = open(os.path.join(ROOT, "include", "sacx.h")).read()
    assert re.search(r"#define SACX_ABI_VERSION 8\b", text) and ctypes.sizeof(N.Config) == 392
    for s in NEW:
        assert s in N.EXPORTS and hasattr(N.lib(), s) and re.search(r"\b%s\(" % s, text), s
    assert ctypes.sizeof(N.TrpoParams) == 40
    src = open(os.path.join(ROOT, "sac-expert_amd", "csrc", "trpo.h")).read()
    assert int(re.search(r"#define TRPO_CHUNK (\d+)", src).group(1)) == 4096


def test_without_the_init_call_the_layout_is_the_parents():
    lib, h0, rc, msg = _create(_cfg().to_c())
    assert rc == 0, msg
    plain = _layout(lib, h0)
    bytes0 = lib.sacx_arena_bytes(h0)
    lib.sacx_destroy(h0)
    assert not any(n.startswith("trpo.") for n in plain)
    lib, h, rc, msg = _create(_cfg().to_c())
    assert lib.sacx_trpo_init(h) == 0, lib.sacx_last_error(h)
    segs = _layout(lib, h)
    assert {n: v for n, v in segs.items() if not n.startswith("trpo.")} == plain
    new = {n: v for n, v in segs.items() if n.startswith("trpo.")}
    assert min(v[0] for v in new.values()) >= bytes0
    for name in ("trpo.par", "trpo.sc", "trpo.vec", "trpo.rr", "trpo.pz", "trpo.done", "trpo.adv", "trpo.ev", "trpo.X",
                 "trpo.H0", "trpo.T0", "trpo.D0", "trpo.H1", "trpo.T1", "trpo.D1", "trpo.G", "trpo.O", "trpo.D3", "trpo.E"):
        assert name in new, name
    # the flat vectors span the actor's contiguous trainable range, actor.l0 .. actor.logstd
    nv = (plain["actor.logstd"][0] + 4 * plain["actor.logstd"][2] - plain["actor.l0"][0]) // 4
    assert new["trpo.vec"][1] == 7 and nv <= new["trpo.vec"][2] < nv + 4
    assert new["trpo.X"][1] == 4096 and new["trpo.adv"][1:] == (2, 10000)
    lib.sacx_destroy(h)
    # a rollout bound below the chunk: the chunk is the bound
    lib, h, rc, msg = _create(_cfg(buffer_capacity=500).to_c())
    assert lib.sacx_trpo_init(h) == 0
    assert _layout(lib, h)["trpo.X"][1] == 500
    lib.sacx_destroy(h)


def test_the_odd_shapes_flat_range_is_no_whole_number_of_float4s():
    """tests/test_gpu_trpo.py's "odd" shape (S = 3, A = 2, hidden (23, 41)): the flat range actor.l0 ..
    actor.logstd is 1,282 floats, so trpo.vec's rows are padded (k_trpo_cg / k_trpo_acc walk them by float4)."""
    lib, h, rc, msg = _create(_cfg(s_dim=3, a_dim=2, hidden=(23, 41), actor_activations=("tanh", "elu"), batch=16,
                                   buffer_capacity=100).to_c())
    assert rc == 0, msg
    assert lib.sacx_trpo_init(h) == 0, lib.sacx_last_error(h)
    segs = _layout(lib, h)
    nv = (segs["actor.logstd"][0] + 4 * segs["actor.logstd"][2] - segs["actor.l0"][0]) // 4
    assert nv % 4 != 0 and segs["trpo.vec"][2] == nv + 4 - nv % 4, (nv, segs["trpo.vec"])
    lib.sacx_destroy(h)


@pytest.mark.parametrize("order", ["trpo_first", "vcritic_first"])
def test_with_vcritics_in_either_order_every_earlier_segment_keeps_its_offset(order):
    lib, h0, rc, msg = _create(_cfg().to_c())
    assert lib.sacx_vcritic_init(h0, 2) == 0
    with_vc = _layout(lib, h0)
    lib.sacx_destroy(h0)
    lib, h0, rc, msg = _create(_cfg().to_c())
    plain = _layout(lib, h0)
    lib.sacx_destroy(h0)
    lib, h, rc, msg = _create(_cfg().to_c())
    if order == "trpo_first":
        assert lib.sacx_trpo_init(h) == 0 and lib.sacx_vcritic_init(h, 2) == 0, lib.sacx_last_error(h)
    else:
        assert lib.sacx_vcritic_init(h, 2) == 0 and lib.sacx_trpo_init(h) == 0, lib.sacx_last_error(h)
    segs = _layout(lib, h)
    assert {n: v for n, v in segs.items() if n in plain} == plain
    if order == "vcritic_first":
        assert {n: v for n, v in segs.items() if n in with_vc} == with_vc
    for n in with_vc:
        assert n in segs and segs[n][1:] == with_vc[n][1:], n
    assert "trpo.vec" in segs and "vc.grad" in segs
    # no two segments overlap
    spans = sorted((v[0], v[0] + v[1] * v[2] * 4) for n, v in segs.items()
                   if n.startswith(("trpo.", "vc.", "v0.", "v1.")) and n not in ("trpo.sc", "trpo.rr", "trpo.pz", "vc.ctl",
                                                                                    "vc.gagg"))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    lib.sacx_destroy(h)


def test_refusals_with_their_messages():
    lib, h, rc, msg = _create(_cfg().to_c())
    assert rc == 0, msg
    assert lib.sacx_trpo_init(h) == 0
    assert lib.sacx_trpo_init(h) != 0 and b"already called" in lib.sacx_last_error(h)
    lib.sacx_destroy(h)
    for ag in (False, True):                               # another handle kind
        lib, h, rc, msg = _create(_cfg(actor_gaussian=ag).to_c())
        assert rc == 0, msg
        assert lib.sacx_trpo_init(h) != 0 and b"not a trainable GaussianActor handle" in lib.sacx_last_error(h)
        lib.sacx_destroy(h)
    src = open(os.path.join(ROOT, "sac-expert_amd", "csrc", "sacx.cpp")).read()
    assert "sacx_trpo_init must precede sacx_bind" in src             # (a bound handle needs a GPU: test_gpu_trpo)


def test_entry_points_on_an_unbound_handle_return_an_error():
    from sac_eo import _native as N
    for init in (False, True):
        lib, h, rc, msg = _create(_cfg().to_c())
        assert rc == 0, msg
        if init:
            assert lib.sacx_trpo_init(h) == 0
        par = N.TrpoParams(delta=0.02, trust_damp=0.01, kl_maxfactor=1.5, cg_it=5, trust_sub=1)
        out = (ctypes.c_double * 8)()
        n = ctypes.c_int32()
        calls = [lambda: lib.sacx_trpo_begin(h, None, None, None, 4, ctypes.byref(par)),
                 lambda: lib.sacx_trpo_grad(h, None),
                 lambda: lib.sacx_trpo_fvp(h, None, None, 0),
                 lambda: lib.sacx_trpo_step(h, ctypes.byref(par), 0, out),
                 lambda: lib.sacx_trpo_plan_info(h, 16, None, 0, ctypes.byref(n))]
        for i, f in enumerate(calls):
            assert f() != 0, i
            assert b"not bound" in lib.sacx_last_error(h), i
        lib.sacx_destroy(h)


def test_engine_config_needs_the_trainable_actor():
    from sac_eo.engine import EngineConfig
    for ag in (False, True):
        with pytest.raises(ValueError, match="actor_gaussian='train'"):
            EngineConfig(s_dim=3, a_dim=1, trpo=True, actor_gaussian=ag)
    assert EngineConfig(s_dim=3, a_dim=1, trpo=True, actor_gaussian="train").trpo is True
    assert EngineConfig(s_dim=3, a_dim=1).trpo is False


def test_trpo_class_imports_by_path_and_refuses_what_is_not_built():
    from sac_eo.actors.continuous_actors import GaussianActor, SquashedGaussianActor
    from sac_eo.algs.model_free.trpo import TRPO
    import sac_eo.algs.model_free as mf
    assert not hasattr(mf, "TRPO") and "TRPO" not in mf.__all__      # the front door stays shut
    actor = GaussianActor(_Env(), [64, 64], ["tanh"], 0.01, "orthogonal", False, rng=np.random.default_rng(0))
    t = TRPO(actor, KW)
    assert t.alpha == 0.0 and t.delta == 0.02 and t.cg_it == 20 and t.trust_sub == 1 and t.kl_maxfactor == 1.5
    data = (np.zeros((8, 3)), np.zeros((8, 1)), np.zeros(8), None, None, None)
    with pytest.raises(NotImplementedError, match="expert_reg"):
        t.update(data, expert_reg=())
    sq = SquashedGaussianActor(_Env(), [64, 64], ["tanh"], 0.01, "orthogonal", False, rng=np.random.default_rng(0))
    with pytest.raises(ValueError, match="plain GaussianActor"):
        TRPO(sq, KW)
    with pytest.raises(KeyError):
        TRPO(actor, {k: v for k, v in KW.items() if k != "delta_trpo"})


def test_init_alg_still_refuses_trpo():
    from sac_eo.algs.init_alg import init_alg
    import inspect
    assert "TRPO is not built" in inspect.getsource(init_alg)
