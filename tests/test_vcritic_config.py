"""VCritics on the trainable GaussianActor handle without a GPU: the init call's segments behind the
``ppo.*`` ones (and the unchanged layout without it), the layer shapes, every refusal with its message,
the new entry points on an unbound handle, and the host classes' unbound errors."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_ppo_config import KW, _Env, _cfg, _create, _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sacx_vcritic_init", "sacx_vcritic_value", "sacx_gae_values", "sacx_gae", "sacx_vcritic_loss", "sacx_vcritic_begin",
       "sacx_vcritic_steps", "sacx_vcritic_end", "sacx_vcritic_plan_info"]
VC_STATE = ["vc.adam_m", "vc.adam_v", "vc.grad", "vc.ctl", "vc.par", "vc.s", "vc.rtg", "vc.stats", "vc.idx"]
VC_WORK = ["vc.X", "vc.T", "vc.O", "vc.G", "vc.sq", "vc.tmp", "vc.gv", "vc.gagg"]


def _is_new(name):
    return name.startswith("vc.") or re.fullmatch(r"v\d+\.l\d+", name) is not None


def test_constants_and_exports():
    from sac_eo import _native as N
    text = open(os.path.join(ROOT, "include", "sacx.h")).read()
    assert re.search(r"#define SACX_ABI_VERSION 8\b", text) and ctypes.sizeof(N.Config) == 392
    for s in NEW:
        assert s in N.EXPORTS and hasattr(N.lib(), s) and re.search(r"\b%s\(" % s, text), s
    src = open(os.path.join(ROOT, "sac-expert_amd", "csrc", "vcritic.h")).read()
    assert int(re.search(r"#define GAE_TILE (\d+)", src).group(1)) == N.GAE_TILE
    assert len(N.VC_STAT_NAMES) == N.MAX_MODELS + 2


def test_without_the_init_call_the_layout_is_the_parents():
    """A trainable handle on which sacx_vcritic_init was not made has no new segment, and a handle with
    it keeps every earlier segment's offset; the new ones lie behind the last ppo.* one."""
    lib, h0, rc, msg = _create(_cfg().to_c())
    assert rc == 0, msg
    plain = _layout(lib, h0)
    bytes0 = lib.sacx_arena_bytes(h0)
    lib.sacx_destroy(h0)
    assert not any(_is_new(n) for n in plain)
    lib, h, rc, msg = _create(_cfg().to_c())
    assert lib.sacx_vcritic_init(h, 2) == 0, lib.sacx_last_error(h)
    segs = _layout(lib, h)
    assert {n: v for n, v in segs.items() if not _is_new(n)} == plain
    ppo_end = max(v[0] + 4 * v[1] * v[2] for n, v in plain.items() if n.startswith("ppo."))
    new = {n: v for n, v in segs.items() if _is_new(n)}
    assert min(v[0] for v in new.values()) >= ppo_end and min(v[0] for v in new.values()) >= bytes0
    for name in VC_STATE + VC_WORK + ["vc.H0", "vc.D0", "vc.H1", "vc.D1"]:
        assert name in new, name
    assert lib.sacx_arena_bytes(h) > bytes0
    # the moments and gradients sit one parameter-range length behind each other
    stride = new["vc.adam_m"][0] - new["v0.l0"][0]
    assert new["vc.adam_v"][0] - new["vc.adam_m"][0] == stride and new["vc.grad"][0] - new["vc.adam_v"][0] == stride
    assert new["vc.adam_m"][1:] == (1, stride // 4) and new["v1.l2"][0] + 4 * 65 <= new["vc.adam_m"][0]
    assert new["vc.s"][1:] == (2 * 10000, 3) and new["vc.rtg"][1:] == (2, 10000)
    assert new["vc.X"][1] == 2 * 312 and new["vc.idx"][2] == 312 and new["vc.stats"][2] == 10
    lib.sacx_destroy(h)


@pytest.mark.parametrize("kw,shapes", [
    (dict(), [(4, 64), (65, 64), (65, 1)]),
    (dict(critic_hidden=(32, 48, 40), critic_activations=("relu", "tanh", "elu")), [(4, 32), (33, 48), (49, 40), (41, 1)]),
    (dict(critic_hidden=(520,)), [(4, 520), (521, 1)]),
])
def test_layer_shapes(kw, shapes):
    lib, h, rc, msg = _create(_cfg(**kw).to_c())
    assert rc == 0, msg
    assert lib.sacx_vcritic_init(h, 3) == 0, lib.sacx_last_error(h)
    segs = _layout(lib, h)
    for k in range(3):
        for i, sh in enumerate(shapes):
            assert segs[f"v{k}.l{i}"][1:] == sh, (k, i)
        assert f"v{k}.l{len(shapes)}" not in segs
    assert "v3.l0" not in segs
    # one contiguous parameter range, in critic then layer order
    offs = [segs[f"v{k}.l{i}"][0] for k in range(3) for i in range(len(shapes))]
    assert offs == sorted(offs)
    lib.sacx_destroy(h)


def test_refusals_with_their_messages():
    lib, h, rc, msg = _create(_cfg().to_c())
    assert rc == 0, msg
    for n in (0, -1, 9):
        assert lib.sacx_vcritic_init(h, n) != 0 and b"outside [1, SACX_MAX_MODELS = 8]" in lib.sacx_last_error(h)
    assert lib.sacx_vcritic_init(h, 8) == 0
    assert lib.sacx_vcritic_init(h, 1) != 0 and b"already called" in lib.sacx_last_error(h)
    lib.sacx_destroy(h)
    for ag in (False, True):                               # another handle kind
        lib, h, rc, msg = _create(_cfg(actor_gaussian=ag).to_c())
        assert rc == 0, msg
        assert lib.sacx_vcritic_init(h, 1) != 0 and b"not a trainable GaussianActor handle" in lib.sacx_last_error(h)
        lib.sacx_destroy(h)
    src = open(os.path.join(ROOT, "sac-expert_amd", "csrc", "sacx.cpp")).read()
    assert "sacx_vcritic_init must precede sacx_bind" in src          # (a bound handle needs a GPU: test_gpu_vcritic)


def test_entry_points_on_an_unbound_handle_return_an_error():
    for init in (False, True):
        lib, h, rc, msg = _create(_cfg().to_c())
        assert rc == 0, msg
        if init:
            assert lib.sacx_vcritic_init(h, 2) == 0
        idx = np.zeros((1, 16), np.int32)
        out = (ctypes.c_double * 9)()
        n = ctypes.c_int32()
        calls = [lambda: lib.sacx_vcritic_value(h, 0, None, 0, 1, None),
                 lambda: lib.sacx_gae_values(h, None, None, None, None, None, 4, 0.99, 0.95, None, None, None),
                 lambda: lib.sacx_gae(h, 0, None, None, None, None, None, 4, 0.99, 0.95, None, None, None),
                 lambda: lib.sacx_vcritic_loss(h, 0, None, None, 4, None),
                 lambda: lib.sacx_vcritic_begin(h, 0, None, None, 4),
                 lambda: lib.sacx_vcritic_steps(h, idx.ctypes.data, 1, 16, 1e-3, 0),
                 lambda: lib.sacx_vcritic_end(h, out),
                 lambda: lib.sacx_vcritic_plan_info(h, 16, None, 0, ctypes.byref(n))]
        for i, f in enumerate(calls):
            assert f() != 0, i
            assert b"not bound" in lib.sacx_last_error(h), i
        lib.sacx_destroy(h)


def test_scratch_guard_reads_the_new_kernels():
    """libsacx.so holds one offload bundle per translation unit with kernels: the guard walks them all."""
    import sys
    so = os.path.join(ROOT, "sac-expert_amd", "lib", "libsacx.so")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler") or not os.path.exists(so):
        pytest.skip("ROCm LLVM tools or libsacx.so absent")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_scratch
    sizes = check_scratch.kernel_scratch(so)
    assert check_scratch.kernel_scratch.bundles >= 2
    for name in ("k_vc_gather", "k_vc_head", "k_vc_final", "k_vc_adam", "k_vc_set", "k_vc_rows", "k_vc_reduce",
                 "k_gae_tiles", "k_gae_apply", "k_gemm"):
        hit = [k for k in sizes if name in k]
        assert hit and all(sizes[k] <= 256 for k in hit), name          # (the guard's bound)
    assert all(r in " ".join(sizes) for r in check_scratch.REQUIRED)


def test_engine_config_field_is_host_only():
    from sac_eo import _native as N
    c = _cfg(vcritics=2)
    assert c.vcritics == 2 and ctypes.sizeof(c.to_c()) == 392
    assert bytes(c.to_c()) == bytes(_cfg().to_c())                # no config field carries it
    assert N.GAE_TILE >= 256 and N.GAE_TILE % 256 == 0


def test_vcritic_unbound_errors_and_bind_checks():
    from sac_eo.critics.critics import VCritic
    c = VCritic(_Env(), [64, 64], ["tanh"], 1.0, rng=np.random.default_rng(0))
    s = np.zeros((2, 3), np.float32)
    for call in (lambda: c._forward(s), lambda: c.value(s), lambda: c.get_loss(s, np.zeros(2, np.float32))):
        with pytest.raises(RuntimeError, match="not bound to a device engine"):
            call()
    assert len(c.get_weights()) == 6                      # weights without an engine, as before

    class _E:
        class cfg:
            vcritics = 0
    with pytest.raises(RuntimeError, match="vcritics"):
        c._bind(_E(), "v0")
    _E.cfg.vcritics = 2
    with pytest.raises(ValueError):
        c._bind(_E(), "v2")
    with pytest.raises(ValueError):
        c._bind(_E(), "q0")


def test_critic_update_class_and_ppo_option():
    from sac_eo.actors.continuous_actors import GaussianActor
    from sac_eo.algs.model_free import PPO, VCriticUpdate
    from sac_eo.critics.critics import VCritic
    cs = [VCritic(_Env(), [64, 64], ["tanh"], 1.0, rng=np.random.default_rng(k)) for k in range(2)]
    kw = dict(critic_lr=1e-3, critic_update_it=3, critic_nminibatch=4)
    u = VCriticUpdate(cs, kw)
    assert u.critic_lr == float(np.float32(1e-3)) and u.critic_update_it == 3 and u.critic_nminibatch == 4
    with pytest.raises(KeyError):
        VCriticUpdate(cs, dict(critic_lr=1e-3))
    with pytest.raises(ValueError):
        VCriticUpdate([], kw)
    data = ([np.zeros((3, 3))], None, None, [np.zeros(3)], None, None)
    with pytest.raises(ValueError):                       # 3 rows, 4 minibatches: n_batch = 0
        u.update(data, 1)
    with pytest.raises(ValueError):                       # two tables asked for (B == the critics), one given
        u.update(([np.zeros((8, 3))], None, None, [np.zeros(8)], None, None), 2)
    actor = GaussianActor(_Env(), [64, 64], ["tanh"], 0.01, "orthogonal", False, rng=np.random.default_rng(0))
    assert PPO(actor, KW)._vcritics == 0 and PPO(actor, dict(KW, vcritics=2))._vcritics == 2


def test_init_alg_mbrl_still_raises():
    from sac_eo.algs import init_alg
    with pytest.raises(NotImplementedError):             # the MBRLOnPolicyAlg loop is not part of this
        init_alg(0, None, None, None, None, None, None, None, None, {"alg_type": "mbrl"}, KW, None, None)
