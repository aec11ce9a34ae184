"""The trainable GaussianActor handle (actor_gaussian = SACX_ACTOR_GAUSSIAN_TRAIN) without a GPU: the
constants, sacx_create's accept / reject, the layout's new segments (and their absence elsewhere), the
entry points on an unbound handle, and the host class ``sac_eo.algs.model_free.PPO``."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PPO_SEGMENTS = ["ppo.ctl", "ppo.par", "ppo.alpha", "ppo.acc", "ppo.log", "ppo.stats", "ppo.idx", "ppo.s", "ppo.a",
                "ppo.adv", "ppo.nlp_old", "ppo.mean_ref", "ppo.ls_ref", "ppo.tmp", "ppo.X", "ppo.A", "ppo.advn",
                "ppo.nlpo", "ppo.rl", "ppo.O", "ppo.gnorm"]


def _create(c):
    from sac_eo import _native as N
    lib = N.lib()
    h = ctypes.c_void_p()
    rc = lib.sacx_create(ctypes.byref(c), ctypes.byref(h))
    msg = (lib.sacx_last_error(None) or b"").decode()
    return lib, h, rc, msg


def _layout(lib, h):
    from sac_eo import _native as N
    n = ctypes.c_int32()
    lib.sacx_layout(h, None, 0, ctypes.byref(n))
    segs = (N.Segment * n.value)()
    lib.sacx_layout(h, segs, n.value, ctypes.byref(n))
    return {s.name.decode(): (int(s.offset), int(s.rows), int(s.cols)) for s in segs}


def _cfg(**kw):
    from sac_eo.engine import EngineConfig
    base = dict(s_dim=3, a_dim=1, hidden=(64, 64), activation="tanh", batch=312, buffer_capacity=10000,
                actor_gaussian="train")
    base.update(kw)
    return EngineConfig(**base)


def test_constants_match_header():
    from sac_eo import _native as N
    text = open(os.path.join(ROOT, "include", "sacx.h")).read()
    for name, val in (("SACX_ACTOR_SQUASHED", N.ACTOR_SQUASHED), ("SACX_ACTOR_GAUSSIAN", N.ACTOR_GAUSSIAN),
                      ("SACX_ACTOR_GAUSSIAN_TRAIN", N.ACTOR_GAUSSIAN_TRAIN)):
        m = re.search(r"^#define\s+%s\s+(\d+)" % name, text, re.M)
        assert m and int(m.group(1)) == val, name
    assert N.ACTOR_GAUSSIAN_TRAIN == 2
    assert re.search(r"#define SACX_ABI_VERSION 8\b", text)          # new entry points, no bump
    assert ctypes.sizeof(N.PpoParams) == 32
    for s in ("sacx_ppo_neglogp", "sacx_ppo_dist", "sacx_ppo_kl", "sacx_ppo_begin", "sacx_ppo_steps", "sacx_ppo_end",
              "sacx_ppo_plan_info"):
        assert s in N.EXPORTS and hasattr(N.lib(), s)


@pytest.mark.parametrize("kw", [dict(), dict(per_state_std=True, a_dim=17, s_dim=17), dict(actor_layer_norm=True),
                                dict(hidden=(32, 48, 40), actor_activations=("relu", "tanh", "elu")),
                                dict(hidden=(520,))])
def test_trainable_handle_creates_and_lists_its_segments(kw):
    c = _cfg(**kw)
    assert c.trainable_gaussian and c.to_c().actor_gaussian == 2
    lib, h, rc, msg = _create(c.to_c())
    assert rc == 0, msg
    segs = _layout(lib, h)
    for name in PPO_SEGMENTS:
        assert name in segs, name
    A = c.a_dim
    assert segs["ppo.s"][1:] == (10000, c.s_dim) and segs["ppo.a"][1:] == (10000, A)
    assert segs["ppo.nlp_old"][1:] == (1, 10000) and segs["ppo.mean_ref"][1:] == (10000, A)
    assert segs["ppo.X"][1] == 312 and segs["ppo.idx"][2] == 312
    assert segs["ppo.O"][2] == (2 * A if c.per_state_std else A)
    lib.sacx_destroy(h)


def test_other_handles_keep_their_layout():
    """The new segments exist on the trainable handle only, behind everything else: an inference-only
    GaussianActor handle of the same shapes has the same segments at the same offsets without them."""
    lib, h2, rc, msg = _create(_cfg().to_c())
    assert rc == 0, msg
    train = _layout(lib, h2)
    lib.sacx_destroy(h2)
    for ag in (False, True):
        lib, h, rc, msg = _create(_cfg(actor_gaussian=ag).to_c())
        assert rc == 0, msg
        segs = _layout(lib, h)
        assert not any(n.startswith("ppo.") for n in segs)
        assert segs == {n: v for n, v in train.items() if not n.startswith("ppo.")}
        assert lib.sacx_arena_bytes(h) <= min(v[0] for n, v in train.items() if n.startswith("ppo."))
        lib.sacx_destroy(h)


@pytest.mark.parametrize("field,value,word", [
    ("actor_output_norm", 1, "actor_output_norm"),
    ("gemm_bf16", 1, "gemm_bf16"),
    ("seeds", 2, "seeds"),
    ("use_expert", 1, "use_expert"),
    ("use_expert", 2, "trains the squashed actor"),
    ("actor_gaussian", 3, "actor_gaussian"),
])
def test_sacx_create_refuses_with_a_message(field, value, word):
    c = _cfg(expert_batch=20, expert_capacity=20).to_c()
    setattr(c, field, value)
    lib, h, rc, msg = _create(c)
    assert rc != 0 and word in msg, (rc, msg)


@pytest.mark.parametrize("kw", [dict(actor_output_norm=True), dict(gemm_bf16=True), dict(seeds=2), dict(use_expert=True),
                                dict(bc=True), dict(actor_gaussian="yes")])
def test_engine_config_refuses(kw):
    with pytest.raises(ValueError):
        _cfg(**kw).to_c()


def test_data_parallel_modes_refuse_the_trainable_handle():
    lib, h, rc, msg = _create(_cfg().to_c())
    assert rc == 0, msg
    assert lib.sacx_dp_init_local(h, 2, 0) != 0
    assert b"trainable GaussianActor" in lib.sacx_last_error(h)
    buf = ctypes.create_string_buffer(256)
    assert lib.sacx_dp_init(h, buf, 2, 0) != 0
    assert b"trainable GaussianActor" in lib.sacx_last_error(h)
    lib.sacx_destroy(h)


def test_entry_points_on_an_unbound_handle_return_an_error():
    from sac_eo import _native as N
    lib, h, rc, msg = _create(_cfg().to_c())
    assert rc == 0, msg
    idx = np.zeros((1, 16), np.int32)
    par = N.PpoParams(eps_ppo=0.2, actor_lr=1e-3)
    out = (ctypes.c_double * 8)()
    n = ctypes.c_int32()
    assert lib.sacx_ppo_steps(h, idx.ctypes.data, 1, 16, ctypes.byref(par), 0) != 0
    assert b"not bound" in lib.sacx_last_error(h)
    assert lib.sacx_ppo_begin(h, None, None, None, 4) != 0
    assert lib.sacx_ppo_end(h, 0.2, out) != 0
    assert lib.sacx_ppo_neglogp(h, None, None, 0, None) != 0
    assert lib.sacx_ppo_dist(h, None, 0, None, None, None) != 0
    assert lib.sacx_ppo_kl(h, None, None, None, 0, None) != 0
    assert lib.sacx_ppo_plan_info(h, 16, None, 0, ctypes.byref(n)) != 0
    lib.sacx_destroy(h)


class _Box:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, np.float32), np.ones(n, np.float32)


class _Env:
    observation_space, action_space = _Box(3), _Box(1)


KW = dict(actor_lr=3e-4, actor_update_it=3, actor_nminibatch=4, adv_center=True, adv_scale=True, eps_ppo=0.2,
          max_grad_norm=0.5, adaptlr=True, adapt_factor=0.03, adapt_minthresh=0.0, adapt_maxthresh=1.0, ent_reg=False,
          ent_targ=0.0, alpha_lr=1e-3)


def test_ppo_class_imports_and_refuses_what_is_not_built():
    from sac_eo.actors.continuous_actors import GaussianActor, SquashedGaussianActor
    from sac_eo.algs.model_free import PPO
    import sac_eo.algs.model_free as mf
    assert not hasattr(mf, "TRPO")
    actor = GaussianActor(_Env(), [64, 64], ["tanh"], 0.01, "orthogonal", False, rng=np.random.default_rng(0))
    ppo = PPO(actor, KW)
    assert ppo.actor_lr == float(np.float32(3e-4)) and ppo.actor_optimizer.learning_rate.numpy() == np.float32(3e-4)
    assert ppo.alpha == 0.0 and ppo.eps == 0.2 and ppo.actor_nminibatch == 4
    data = (np.zeros((8, 3)), np.zeros((8, 1)), np.zeros(8), None, None, None)
    with pytest.raises(NotImplementedError):
        ppo.update(data, expert_reg=())
    with pytest.raises(ValueError):                       # n < actor_nminibatch: n_batch = 0
        ppo.update((np.zeros((3, 3)), np.zeros((3, 1)), np.zeros(3), None, None, None))
    with pytest.raises(KeyError):
        PPO(actor, {k: v for k, v in KW.items() if k != "eps_ppo"})
    sq = SquashedGaussianActor(_Env(), [64, 64], ["tanh"], 0.01, "orthogonal", False, rng=np.random.default_rng(0))
    with pytest.raises(ValueError):
        PPO(sq, KW)
    for name in ("neglogp", "entropy", "kl", "get_kl_info"):
        with pytest.raises(NotImplementedError):
            getattr(sq, name)(np.zeros((2, 3)))
        with pytest.raises(RuntimeError):                 # unbound: no device engine, no CPU path
            getattr(actor, name)(*([np.zeros((2, 3))] * (2 if name in ("neglogp", "kl") else 1)))
    with pytest.raises(NotImplementedError):
        actor.kl(np.zeros((2, 3)), np.zeros((2, 1, 2)), direction="reverse")


def test_init_alg_mbrl_still_raises():
    from sac_eo.algs import init_alg
    with pytest.raises(NotImplementedError):             # the MBRLOnPolicyAlg loop is not part of this
        init_alg(0, None, None, None, None, None, None, None, None, {"alg_type": "mbrl"}, KW, None, None)
