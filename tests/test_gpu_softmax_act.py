"""``sacx_softmax_act`` / ``sacx_softmax_act_host`` (SoftMaxActor.sample on the device, discrete_actors.py:22-42)
against NumPy: the cases, nets and starting streams of tests/softmax_act_cases.py.

* ``u_out`` equals ``RandomState.random_sample((n, A))`` bit for bit, and the device stream afterwards equals
  NumPy's -- key, pos, has_gauss, gauss (the cached gaussian is preserved);
* the actions equal ``gumbel_argmax(eng.dist(s)[0], u)`` on every row whose host top-two gap of x exceeds 1e-4
  (the device's f64 log and its summation order may differ from the host's in the last place; near ties are the
  only rows where that can show), with at most 1 % of a case's rows left out -- asserted of the host
  computation before the comparison;
* the deterministic form is the argmax of the logits and leaves the stream bit-identical;
* the ``_host`` form gives the same actions and stream as the device form;
* ``SoftMaxActor.sample`` with ``device_sample = True`` equals the host draw on the same state, same shapes;
* on an ``EngineConfig(learners=K)`` engine the call acts for the selected learner;
* refusals leave the arena byte-identical.
"""
import numpy as np
import pytest

import softmax_act_cases as C

pytestmark = pytest.mark.gpu


def make_engine(net, A, softmax=True):
    from sac_eo.engine import Engine, EngineConfig
    c = C.NETS[net]
    return Engine(EngineConfig(s_dim=C.S, a_dim=A, hidden=c["hidden"], actor_activations=c["acts"], batch=16,
                               buffer_capacity=64, actor_gaussian="train", actor_layer_norm=c.get("layer_norm", False),
                               graph_steps=1, softmax=softmax))


@pytest.fixture(scope="module")
def engines():
    """One loaded engine per (net, A), shared by the cases (nothing here changes the weights)."""
    cache = {}

    def get(net, A):
        if (net, A) not in cache:
            cfg, st, nrm = C.make_state(net, A)
            eng = make_engine(net, A)
            eng.set_net("actor", [np.asarray(w, np.float32) for w in st.actor])
            eng.set_normalizers(nrm.s_mean, nrm.s_den, nrm.a_mean, nrm.a_den)
            cache[(net, A)] = eng
        return cache[(net, A)]
    yield get
    for eng in cache.values():
        eng.close()


def same_stream(a, b):
    return np.array_equal(a[1], b[1]) and tuple(a[2:5]) == tuple(b[2:5])


def compare(tag, got, logits, u, n):
    """got == gumbel_argmax(logits, u) on the clear rows; the host computation leaves out no more than the cap."""
    from sac_eo.actors.discrete_actors import gumbel_argmax
    clear = C.clear_rows(logits, u)
    out = int(n - clear.sum())
    want = gumbel_argmax(logits, u)
    diff = int(np.sum(np.asarray(got) != want))
    print(f"{tag}: rows {n} left out {out} (cap {C.may_leave_out(n)}) differing {diff}, on clear rows "
          f"{int(np.sum((np.asarray(got) != want) & clear))}")
    assert out <= C.may_leave_out(n), (tag, out)
    assert np.array_equal(np.asarray(got)[clear], want[clear]), tag


@pytest.mark.parametrize("net,n,A,kind", C.CASES)
def test_softmax_act(gpu_available, engines, net, n, A, kind):
    eng = engines(net, A)
    s = C.states(n, seed=4 + n)
    logits = eng.dist(s)[0].cpu().numpy()
    state0 = C.stream(kind)
    u_ref, state1 = C.uniforms(state0, n, A)
    # ---- the device form
    eng.rng_set_state(state0)
    act, u = eng.softmax_act(s, return_u=True)
    after = eng.rng_get_state()
    act, u = act.cpu().numpy(), u.cpu().numpy()
    assert act.shape == (n,) and act.dtype == np.int32 and u.shape == (n, A) and u.dtype == np.float64
    assert np.array_equal(u.view(np.uint64), u_ref.view(np.uint64)), "u_out differs from RandomState.random_sample"
    assert same_stream(after, state1), (after[2:5], state1[2:5])
    assert np.all((act >= 0) & (act < A))
    compare(f"{net} n={n} A={A} {kind} device", act, logits, u_ref, n)
    # ---- the _host form: the same actions, the same stream
    eng.rng_set_state(state0)
    act_h = eng.softmax_act_host(s)
    assert act_h.shape == (n,) and act_h.dtype == np.int32
    assert np.array_equal(act_h, act) and same_stream(eng.rng_get_state(), state1)
    # ---- deterministic: the argmax of the logits, no draw
    eng.rng_set_state(state0)
    det, none = eng.softmax_act(s, deterministic=True, return_u=True)
    assert none is None
    det = det.cpu().numpy()
    det_h = eng.softmax_act_host(s, deterministic=True)
    assert same_stream(eng.rng_get_state(), state0)
    assert np.array_equal(det, det_h)
    compare(f"{net} n={n} A={A} deterministic", det, logits, None, n)
    # one row: 0-d results
    one = eng.softmax_act(s[0], deterministic=True)
    assert one.shape == () and int(one) == int(det[0]) and np.shape(eng.softmax_act_host(s[0], True)) == ()


@pytest.mark.parametrize("net,n,A", [("h64", 1, 5), ("h64", 16, 2), ("h64", 17, 32), ("ln64", 7, 5), ("one32", 1030, 32)])
def test_device_sample_equals_the_host_draw(gpu_available, engines, net, n, A):
    from sac_eo.actors.discrete_actors import SoftMaxActor

    class _Space:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    class _Env:
        observation_space, action_space = _Space(shape=(C.S,)), _Space(n=A, shape=())
    eng = engines(net, A)
    c = C.NETS[net]
    actor = SoftMaxActor(_Env(), list(c["hidden"]), list(c["acts"]), 0.01, layer_norm=c.get("layer_norm", False),
                         rng=np.random.default_rng(0))
    assert actor.device_sample is False
    actor._engine, actor._net = eng, "actor"                 # serve the engine's loaded weights as they are
    s = C.states(n, seed=40 + n)
    s_in = s[0] if n == 1 else s
    state0 = C.stream("gauss", seed=5)
    logits = eng.dist(s)[0].cpu().numpy()
    u_ref, state1 = C.uniforms(state0, n, A)
    clear, clear_det = C.clear_rows(logits, u_ref), C.clear_rows(logits, None)
    assert n - clear.sum() <= C.may_leave_out(n) and n - clear_det.sum() <= C.may_leave_out(n)
    out = {}
    for dev in (False, True):
        actor.device_sample = dev
        eng.rng_set_state(state0)
        a = actor.sample(s_in)
        assert same_stream(eng.rng_get_state(), state1), dev
        d = actor.sample(s_in, deterministic=True)
        assert same_stream(eng.rng_get_state(), state1), dev
        out[dev] = (a, d)
    for k, rows in ((0, clear), (1, clear_det)):
        h, d = out[False][k], out[True][k]
        assert type(h) is type(d) and h.shape == d.shape == (() if n == 1 else (n,)) and h.dtype == d.dtype
        assert np.array_equal(np.asarray(h).reshape(-1)[rows], np.asarray(d).reshape(-1)[rows])


@pytest.mark.parametrize("n", [7, 17])
def test_packed_learners_engine_acts_for_the_selected_learner(gpu_available, engines, n):
    """EngineConfig(learners=2): each learner's call uses its own weights, normaliser and stream -- the results
    of a one-learner engine bit for bit -- and leaves the other learner's stream as it was."""
    import dataclasses
    from sac_eo.engine import Engine
    A = 5
    one = engines("h64", A)
    eng = Engine(dataclasses.replace(one.cfg, learners=2))
    states = [C.make_state("h64", A, seed=2), C.make_state("h64", A, seed=9)]
    streams = [C.stream("gauss", seed=21), C.stream("pos623", seed=22)]
    for k, (cfg, st, nrm) in enumerate(states):
        v = eng.seed_view(k)
        v.set_net("actor", [np.asarray(w, np.float32) for w in st.actor])
        v.set_normalizers(nrm.s_mean, nrm.s_den, nrm.a_mean, nrm.a_den)
        v.rng_set_state(streams[k])
    s = C.states(n, seed=60)
    cfg, st, nrm = states[1]
    ref = make_engine("h64", A)
    ref.set_net("actor", [np.asarray(w, np.float32) for w in st.actor])
    ref.set_normalizers(nrm.s_mean, nrm.s_den, nrm.a_mean, nrm.a_den)
    ref.rng_set_state(streams[1])
    want, u_want = ref.softmax_act(s, return_u=True)
    got, u_got = eng.seed_view(1).softmax_act(s, return_u=True)
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()) and np.array_equal(u_got.cpu().numpy(), u_want.cpu().numpy())
    assert same_stream(eng.seed_view(1).rng_get_state(), ref.rng_get_state())
    assert same_stream(eng.seed_view(0).rng_get_state(), streams[0])
    ref.rng_set_state(streams[1])
    eng.seed_view(1).rng_set_state(streams[1])
    assert np.array_equal(eng.seed_view(1).softmax_act_host(s), ref.softmax_act_host(s))
    # learner 0: the shared one-learner engine's weights
    one.rng_set_state(streams[0])
    assert np.array_equal(eng.seed_view(0).softmax_act_host(s), one.softmax_act_host(s))
    assert same_stream(eng.seed_view(0).rng_get_state(), one.rng_get_state())
    ref.close()
    eng.close()


def test_refusals_leave_the_arena_untouched(gpu_available, engines):
    import ctypes
    import torch
    from sac_eo import _native as N
    eng = engines("h64", 5)
    eng.rng_set_state(C.stream("fresh"))
    s = torch.as_tensor(C.states(4, 1)).cuda()
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    host_s, host_a = C.states(4, 1), np.zeros(4, np.int32)
    eng.sync()
    before = eng.arena_all.cpu().numpy().copy()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib, h = eng.lib, eng.h
    bad = [lambda: lib.sacx_softmax_act(h, p(s), -1, 0, p(out), None),
           lambda: lib.sacx_softmax_act(h, None, 4, 0, p(out), None),
           lambda: lib.sacx_softmax_act(h, p(s), 4, 0, None, None),
           lambda: lib.sacx_softmax_act_host(h, host_s.ctypes.data, -1, 0, host_a.ctypes.data),
           lambda: lib.sacx_softmax_act_host(h, None, 4, 0, host_a.ctypes.data),
           lambda: lib.sacx_softmax_act_host(h, host_s.ctypes.data, 4, 0, None)]
    for i, f in enumerate(bad):
        assert f() != 0, i
        assert b"bad arguments" in lib.sacx_last_error(h), i
    eng.sync()
    assert np.array_equal(eng.arena_all.cpu().numpy(), before)
    assert lib.sacx_softmax_act(h, p(s), 0, 0, p(out), None) == 0            # n = 0: nothing to do
    # a bound Gaussian handle: the new calls refuse it, the Gaussian calls keep refusing a softmax handle
    g = make_engine("h64", 5, softmax=False)
    g.sync()
    gb = g.arena_all.cpu().numpy().copy()
    with pytest.raises(N.SacxError, match="not a softmax handle"):
        g.softmax_act(C.states(4, 1))
    with pytest.raises(N.SacxError, match="not a softmax handle"):
        g.softmax_act_host(C.states(4, 1))
    g.sync()
    assert np.array_equal(g.arena_all.cpu().numpy(), gb)
    g.close()
    for call in (lambda: eng.act(C.states(4, 1)), lambda: eng.act_host(C.states(4, 1))):
        with pytest.raises(N.SacxError, match="samples on the host from sacx_ppo_dist's logits"):
            call()
    eng.sync()
    assert np.array_equal(eng.arena_all.cpu().numpy(), before)
