"""The hidden-layer width bound (SACX_MAX_WIDTH = 1,024) without a GPU: the constant in the header and
its Python mirror, EngineConfig's error, and sacx_create's accept / reject (host only: no arena, no
device, nothing launched)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_define(name):
    text = open(os.path.join(ROOT, "include", "sacx.h")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def test_max_width_constant_matches_header():
    from sac_eo import _native as N
    assert N.MAX_WIDTH == 1024
    assert N.MAX_WIDTH == _header_define("SACX_MAX_WIDTH")
    assert N.MAX_DEPTH == _header_define("SACX_MAX_DEPTH")


@pytest.mark.parametrize("kw,named", [
    (dict(hidden=(1025, 64)), "[1025, 64]"),
    (dict(critic_hidden=(64, 2048)), "[64, 2048]"),
    (dict(use_expert=True, model_hidden=(1024, 1025, 8)), "[1024, 1025, 8]"),
    (dict(hidden=(0, 64)), "[0, 64]"),
])
def test_engine_config_rejects_wider_than_max(kw, named):
    from sac_eo.engine import EngineConfig
    with pytest.raises(NotImplementedError) as e:
        EngineConfig(s_dim=17, a_dim=6, buffer_capacity=1000, **kw).to_c()
    assert named in str(e.value) and "1024" in str(e.value)


def _create(c):
    from sac_eo import _native as N
    lib = N.lib()
    h = ctypes.c_void_p()
    rc = lib.sacx_create(ctypes.byref(c), ctypes.byref(h))
    msg = (lib.sacx_last_error(None) or b"").decode()
    return lib, h, rc, msg


@pytest.mark.parametrize("net", [0, 1, 2, 3])
def test_sacx_create_rejects_1025_and_names_the_bound(net):
    """Width 1,025 in any used net, past EngineConfig's own check: an error return whose message names
    the bound."""
    from sac_eo.engine import EngineConfig
    c = EngineConfig(s_dim=17, a_dim=6, buffer_capacity=1000, use_expert=True, separate_reward_nn=True,
                     expert_batch=20, expert_capacity=20).to_c()
    c.net_hidden[net][c.net_depth[net] - 1] = 1025
    lib, h, rc, msg = _create(c)
    assert rc != 0 and "1024" in msg and "SACX_MAX_WIDTH" in msg, (rc, msg)


def test_sacx_create_ignores_unused_nets_width():
    """The world-model and reward lists of a plain SAC handle are not built: their widths are not checked."""
    from sac_eo.engine import EngineConfig
    c = EngineConfig(s_dim=17, a_dim=6, buffer_capacity=1000).to_c()
    c.net_hidden[2][0] = 4096
    lib, h, rc, msg = _create(c)
    assert rc == 0, msg
    lib.sacx_destroy(h)


@pytest.mark.parametrize("kw", [
    dict(hidden=(1024, 1024)),
    dict(hidden=(64, 64), critic_hidden=(520,)),
    dict(hidden=(64, 64), use_expert=True, model_hidden=(1024, 600), expert_batch=12, expert_capacity=12),
    dict(hidden=(600, 64), use_expert=True, bc=True, model_hidden=(64, 1000), expert_batch=12, expert_capacity=12),
])
def test_sacx_create_accepts_up_to_1024(kw):
    """Widths in (512, 1,024] construct and lay out (the parent commit refused them here)."""
    from sac_eo import _native as N
    from sac_eo.engine import EngineConfig
    lib, h, rc, msg = _create(EngineConfig(s_dim=17, a_dim=6, buffer_capacity=1000, **kw).to_c())
    assert rc == 0, msg
    n = ctypes.c_int32()
    lib.sacx_layout(h, None, 0, ctypes.byref(n))
    segs = (N.Segment * n.value)()
    lib.sacx_layout(h, segs, n.value, ctypes.byref(n))
    widest = max(max(v) for v in kw.values() if isinstance(v, tuple))
    assert any(s.cols == widest for s in segs)
    lib.sacx_destroy(h)
