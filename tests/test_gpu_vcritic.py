"""VCritics on the device against tests/vcritic_ref.py: value, GAE and the critic update.

* ``value`` / ``get_loss`` rows at 2e-5 of the tensor's max (the bar tests/test_gpu_ppo.py uses for rows);
* ``gae_values`` on the reference's fixture and on generated cases whose trajectory lengths sit on the scan's
  tile boundaries.  Bar per element: ``|dev - ref| <= spacing(f32 |ref|) + 1e-9 max|delta|`` -- derived: both
  sides round the same f64 number to f32 (one f32 spacing when a last-bit difference of the f64 scans flips
  the rounding), and an f64 scan's own error is ~1e-14 max|delta|.  An f32 scan misses it by 6x .. 350x from
  n = 64 upwards at (0.99, 0.95), so the bar also proves that the scan runs in f64;
* ``gae`` end to end: the device's own values fed to the fp64 loop meet that bar; against the all-fp64
  restatement the result lies inside the fp32 envelope (the restatement's value pass in fp32 under each of
  ``sac_oracle.MATMUL_ORDERS`` against its fp64 run);
* one critic step at the bars of tests/test_gpu_bc.py / test_gpu_ppo.py: loss 2e-5, gradients (through Adam's
  first moment after step 1) 2e-4, weights after Adam 1e-6;
* ``VCriticUpdate.update`` end to end, graph == eager == single steps bit for bit, the tie-up with
  ``TrajectoryBuffer`` and ``PPO`` on one engine, and the PPO step on a handle without / with critics.
"""
import os

import numpy as np
import pytest

import sac_oracle as O
import vcritic_ref as V
from helpers import B1, nontrivial_normalizers, relerr

pytestmark = pytest.mark.gpu

SHAPES = {
    "two": dict(hidden=(64, 64), acts=("tanh", "tanh")),
    "three": dict(hidden=(32, 48, 40), acts=("relu", "tanh", "elu")),
    "wide1": dict(hidden=(520,), acts=("tanh",)),
    "odd": dict(hidden=(23, 41), acts=("tanh", "elu")),      # widths off the 4-grid
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gae_ref.npz")


def make_engine(S, shape, nc, batch, capacity, **kw):
    from sac_eo.engine import Engine, EngineConfig
    c = SHAPES[shape]
    return Engine(EngineConfig(s_dim=S, a_dim=2, hidden=(64, 64), activation="tanh", critic_hidden=c["hidden"],
                               critic_activations=c["acts"], batch=batch, buffer_capacity=capacity,
                               actor_gaussian="train", graph_steps=1, vcritics=nc, **kw))


def make_state(S, shape, nc, seed, ret_den=2.7):
    rng = np.random.RandomState(seed + 70)
    nrm = nontrivial_normalizers(rng, S, 2)
    nrm.ret_den = np.float32(ret_den)
    return V.init_state(S, SHAPES[shape]["hidden"], nc, seed=seed, gain=1.0, bias_scale=0.1), nrm


def load(eng, st, nrm):
    for k, w in enumerate(st.critics):
        eng.set_net(f"v{k}", [np.asarray(x, np.float32) for x in w])
    eng.set_normalizers(nrm.s_mean, nrm.s_den, nrm.a_mean, nrm.a_den, ret_den=float(nrm.ret_den))


def states(S, n, seed):
    rng = np.random.RandomState(seed + 900)
    return (rng.normal(size=(n, S)) * rng.uniform(0.3, 2.0, S)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- value / loss
VALUE = [(3, "two", 1, 1), (3, "two", 1, 17), (17, "two", 3, 1025), (17, "three", 3, 17), (3, "wide1", 1, 1025),
         (17, "wide1", 3, 1)]


@pytest.mark.parametrize("S,shape,nc,n", VALUE)
def test_value_and_loss_rows(gpu_available, S, shape, nc, n):
    st, nrm = make_state(S, shape, nc, seed=2)
    eng = make_engine(S, shape, nc, batch=16, capacity=max(n, 16))
    load(eng, st, nrm)
    s = states(S, n, 4)
    rtg = (np.random.RandomState(8).normal(size=n) * 4 + 1).astype(np.float32)
    acts = SHAPES[shape]["acts"]
    for k in range(nc):
        out = eng.vcritic_value(k, s, value=False).cpu().numpy()
        val = eng.vcritic_value(k, s, value=True).cpu().numpy()
        ref = V.forward(st.critics[k], acts, nrm, s, np.float64)[0]
        loss = float(eng.vcritic_loss(k, s, rtg).cpu().numpy()[0])
        lref = float(V.loss_and_grads(st.critics[k], acts, nrm, s, rtg)[0])
        errs = (relerr(out, ref), relerr(val, ref * np.float64(nrm.ret_den)), abs(loss - lref) / lref)
        print(f"S={S} {shape} critic {k} n={n}: output {errs[0]:.2e} value {errs[1]:.2e} loss {errs[2]:.2e}")
        assert out.shape == (n,) and max(errs) < 2e-5, errs
    if nc > 1:                                          # the critics are different nets
        assert relerr(eng.vcritic_value(0, s).cpu().numpy(), eng.vcritic_value(1, s).cpu().numpy()) > 1e-2
    eng.close()


# ---------------------------------------------------------------------------------------------- GAE
def gae_bar(ref, delta):
    return np.spacing(np.abs(np.asarray(ref, np.float32))).astype(np.float64) + 1e-9 * np.max(np.abs(delta))


def check_gae(got, v_s, v_sp, r, d, traj, gamma, lam, what):
    adv, rtg, rtg_sp, delta = V.gae_batch_loop(v_s, v_sp, r, d, traj, gamma, lam, f64=True)
    worst = 0.0
    for name, g, ref in zip(("adv", "rtg", "rtg_sp"), got, (adv, rtg, rtg_sp)):
        g = g.cpu().numpy()
        assert g.dtype == np.float32 and g.shape == ref.shape
        ratio = np.abs(g.astype(np.float64) - ref.astype(np.float32).astype(np.float64)) / gae_bar(ref, delta)
        worst = max(worst, float(ratio.max()))
    print(f"{what} gamma={gamma} lam={lam} n={len(r)}: worst error / bar {worst:.3f}")
    assert worst <= 1.0, (what, worst)
    return worst


def gae_case(lens, seed, done_p=0.05):
    rng = np.random.RandomState(seed)
    n = int(sum(lens))
    v_s, v_sp = [(rng.normal(size=n) * 3).astype(np.float32) for _ in range(2)]
    r = (rng.normal(size=n) + 0.5).astype(np.float32)
    d = (rng.uniform(size=n) < done_p).astype(np.float64)            # dones inside trajectories ...
    ends = np.cumsum(lens) - 1
    d[ends[::2]] = 1.0                                               # ... and at the ends of every other one
    traj = np.concatenate([np.full(l, 3 + i, np.float64) for i, l in enumerate(lens)])
    return v_s, v_sp, r, d, traj


@pytest.fixture(scope="module")
def gae_engine(gpu_available):
    from sac_eo import _native as N
    eng = make_engine(3, "two", 1, batch=16, capacity=7 * N.GAE_TILE)
    yield eng
    eng.close()


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.99, 0.0)])
def test_gae_values(gae_engine, gamma, lam):
    from sac_eo import _native as N
    T = N.GAE_TILE
    eng = gae_engine
    g = np.load(GOLDEN)
    if (gamma, lam) == (float(g["gamma"]), float(g["lam"])):         # the reference's own results
        got = eng.gae_values(g["v_s"], g["v_sp"], g["r"], g["d"], g["idx_all"], gamma, lam)
        check_gae(got, g["v_s"], g["v_sp"], g["r"], g["d"], g["idx_all"], gamma, lam, "fixture")
    lens = [1, 1, 5, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1, 2]
    c = gae_case(lens, seed=12)
    check_gae(eng.gae_values(*c, gamma, lam), *c, gamma, lam, "tiles")
    one = gae_case([1], seed=13)
    check_gae(eng.gae_values(*one, gamma, lam), *one, gamma, lam, "one row")
    long = gae_case([3 * T + 7], seed=14, done_p=0.0)                # one trajectory over four tiles, no done inside
    check_gae(eng.gae_values(*long, gamma, lam), *long, gamma, lam, "one trajectory")


def test_any_change_of_the_trajectory_index_restarts(gae_engine):
    """The reference restarts wherever neighbouring indices differ at all (buffer_utils.py:63): fractional
    indices, and indices 2^31 or 2^32 apart, are different trajectories."""
    v_s, v_sp, r, d, _ = gae_case([12], seed=3, done_p=0.0)
    traj = np.array([0.0, 0.0, 0.25, 0.25, 0.5, 2.0 ** 31 + 0.5, 2.0 ** 31 + 0.5, 2.0 ** 32 + 0.5, 7.0, 7.0, -7.0, -7.0])
    got = gae_engine.gae_values(v_s, v_sp, r, d, traj, 0.99, 0.95)
    check_gae(got, v_s, v_sp, r, d, traj, 0.99, 0.95, "odd indices")
    cuts = np.flatnonzero(traj[1:] != traj[:-1]) + 1
    assert list(cuts) == [2, 4, 5, 7, 8, 10]
    delta = r + 0.99 * (1 - d) * v_sp - v_s                  # a trajectory's last row: adv = delta
    assert np.array_equal(got[0].cpu().numpy()[cuts - 1], delta[cuts - 1].astype(np.float32))


def test_a_failed_init_call_raises_and_leaves_no_handle(gpu_available):
    from sac_eo._native import SacxError
    from sac_eo.engine import Engine, EngineConfig
    with pytest.raises(SacxError, match="not a trainable GaussianActor handle"):
        Engine(EngineConfig(s_dim=3, a_dim=1, hidden=(64, 64), batch=16, buffer_capacity=64, graph_steps=1, vcritics=1))
    with pytest.raises(SacxError, match="outside"):
        make_engine(3, "two", 9, batch=16, capacity=32)


def test_gae_values_refusals(gae_engine):
    from sac_eo._native import SacxError
    from sac_eo import _native as N
    c = gae_case([5], seed=1)
    with pytest.raises(SacxError, match="gamma must be positive"):
        gae_engine.gae_values(*c, 0.0, 0.9)
    big = gae_case([7 * N.GAE_TILE + 1], seed=1)
    with pytest.raises(SacxError, match="buffer_capacity"):
        gae_engine.gae_values(*big, 0.99, 0.95)


def test_gae_end_to_end(gpu_available):
    S, shape = 17, "two"
    acts = SHAPES[shape]["acts"]
    st, nrm = make_state(S, shape, 2, seed=5)
    lens = [1, 40, 1030, 2, 2100, 7]
    n = sum(lens)
    eng = make_engine(S, shape, 2, batch=16, capacity=n)
    load(eng, st, nrm)
    _, _, r, d, traj = gae_case(lens, seed=21)
    s, sp = states(S, n, 6), states(S, n, 7)
    gamma, lam = 0.99, 0.95
    got = eng.gae(1, s, r, sp, d, traj, gamma, lam)
    # (a) the device's own values through the fp64 loop: the scan bar
    v_s, v_sp = eng.vcritic_value(1, s).cpu().numpy(), eng.vcritic_value(1, sp).cpu().numpy()
    check_gae(got, v_s, v_sp, r, d, traj, gamma, lam, "gae (device values)")
    # (b) against the all-fp64 restatement: inside the envelope of a faithful fp32 value pass -- the same
    # restatement with the value pass in fp32 under each summation order and the outputs rounded to f32 as
    # the device's are, against the fp64 run
    w = st.critics[1]
    v64, vp64 = V.value(w, acts, nrm, s), V.value(w, acts, nrm, sp)
    ref = V.gae_batch_loop(v64, vp64, r, d, traj, gamma, lam, f64=True)
    env = [0.0, 0.0, 0.0]
    w32 = [np.asarray(x, np.float32) for x in w]
    for order in O.MATMUL_ORDERS:
        O.MATMUL_ORDER = order
        try:
            a32 = V.gae_batch_loop(V.value(w32, acts, nrm, s, np.float32), V.value(w32, acts, nrm, sp, np.float32), r, d,
                                   traj, gamma, lam)
        finally:
            O.MATMUL_ORDER = "default"
        env = [max(e, float(np.max(np.abs(x.astype(np.float64) - y)))) for e, x, y in zip(env, a32, ref)]
    figs = []
    for name, g, y, e in zip(("adv", "rtg", "rtg_sp"), got, ref, env):
        err = float(np.max(np.abs(g.cpu().numpy().astype(np.float64) - y)))
        print(f"gae end to end {name}: device error {err:.3e} fp32 envelope {e:.3e} ratio {err / e:.3f}")
        figs.append((name, err, e))
    for name, err, e in figs:                            # every figure is printed before the first assertion
        assert err <= e, (name, err, e)
    # the host gae_batch with a bound critic is this one call
    from sac_eo.common.buffer_utils import gae_batch
    from sac_eo.critics.critics import VCritic
    c = VCritic(_Env(S), list(SHAPES[shape]["hidden"]), list(acts), 1.0, rng=np.random.default_rng(0))
    c._w = [np.asarray(x, np.float32) for x in w]
    c._bind(eng, "v1")
    hb = gae_batch(c, gamma, lam, s, r, sp, d, traj)
    for x, y in zip(hb, got):
        assert x.dtype == np.float32 and np.array_equal(x, y.cpu().numpy())
    assert np.array_equal(np.asarray(c.value(s)), v_s) and np.asarray(c._forward(s)).shape == (n, 1)
    eng.close()


# ---------------------------------------------------------------------------------------------- one step
STEP_CASES = {
    # name: S, shape, critics, minibatch rows, table rows per critic
    "two_1_312": dict(S=3, shape="two", nc=1, mb=312, n=[400]),
    "two_2_33": dict(S=17, shape="two", nc=2, mb=33, n=[64, 50]),
    "two_3_16": dict(S=3, shape="two", nc=3, mb=16, n=[20, 16, 31]),           # 9 dW problems: two v.grad launches
    "two_8_17": dict(S=3, shape="two", nc=8, mb=17, n=[17, 20, 18, 25, 19, 17, 30, 21]),   # 24: three
    "three_3_17": dict(S=17, shape="three", nc=3, mb=17, n=[40, 64, 33]),
    "wide_2_16": dict(S=7, shape="wide1", nc=2, mb=16, n=[16, 30]),
    "odd_2_17": dict(S=17, shape="odd", nc=2, mb=17, n=[40, 33]),
}


def _moment(eng, name):
    seg = eng.segments[name]
    off = (seg["offset"] - eng.segments["v0.l0"]["offset"]) // 4
    n = seg["rows"] * seg["cols"]
    return eng.v["vc.adam_m"][0][off: off + n].cpu().numpy().reshape(seg["rows"], seg["cols"]) / B1


def tables(c, seed):
    rng = np.random.RandomState(seed + 40)
    s = [states(c["S"], n, seed + k) for k, n in enumerate(c["n"])]
    rtg = [(rng.normal(size=n) * 4 + 1).astype(np.float32) for n in c["n"]]
    return s, rtg


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_one_critic_step(gpu_available, case):
    from sac_eo._native import SacxError
    c = STEP_CASES[case]
    acts = SHAPES[c["shape"]]["acts"]
    st, nrm = make_state(c["S"], c["shape"], c["nc"], seed=3)
    s, rtg = tables(c, 9)
    nmin = min(c["n"])
    idx = np.stack([np.random.RandomState(31 + j).permutation(nmin)[:c["mb"]] for j in range(2)]).astype(np.int32)
    eng = make_engine(c["S"], c["shape"], c["nc"], batch=c["mb"], capacity=max(c["n"]))
    load(eng, st, nrm)
    eng.v["vc.grad"].fill_(3.0)                         # a reused arena: vcritic_begin clears the gradient words
    for k in range(c["nc"]):
        eng.vcritic_begin(k, s[k], rtg[k])
    if c["nc"] > 1:                                     # an index >= the shortest table: refused, nothing touched
        eng.sync()
        before = eng.arena_all.clone()
        bad = idx[:1].copy()
        bad[0, 0] = nmin
        with pytest.raises(SacxError, match="shortest critic table"):
            eng.vcritic_steps(bad, critic_lr=1e-4)
        eng.sync()
        assert bool((eng.arena_all == before).all())
    ref = st.copy()
    for j in range(2):
        keep = {}
        o = V.critic_step(ref, acts, nrm, [x[idx[j]] for x in s], [x[idx[j]] for x in rtg], 1e-4, keep)
        eng.vcritic_steps(idx[j:j + 1], critic_lr=1e-4)       # (the rate of test_gpu_ppo's step cases)
        eng.sync()
        row = eng.vcritic_stats(1)[0]
        print(f"{case} step {j}: {[l['name'] for l in eng.vcritic_plan_info(c['mb'])] if j == 0 else ''} loss {row[0]:.6g} "
              f"vs {o['loss']:.6g}")
        assert abs(row[0] - o["loss"]) <= 2e-5 * abs(o["loss"]) and row[9] == j + 1
        for k in range(8):                              # each critic's slot at its own loss's bar; the rest hold 0
            if k < c["nc"]:
                assert abs(row[1 + k] - o["losses"][k]) <= 2e-5 * abs(o["losses"][k]), k
            else:
                assert row[1 + k] == 0.0, k
        if j == 0:                                      # the plan: 2 D + 5 launches around the dW launches, which
            D, probs = len(acts), c["nc"] * (len(acts) + 1)      # take 8 problems (GEMM_MAXP) each
            assert len(eng.vcritic_plan_info(c["mb"])) == 5 + 2 * D + (probs + 7) // 8
        if j == 0:                                      # gradients, through Adam's first moment
            gi = iter(keep["grads"])
            for k in range(c["nc"]):
                for i in range(len(acts) + 1):
                    m = _moment(eng, f"v{k}.l{i}")
                    gw, gb = next(gi), next(gi)
                    assert relerr(m[:-1], gw) < 2e-4 and relerr(m[-1], gb) < 2e-4, (k, i)
    werr = max(float(np.max(np.abs(x - y))) for k in range(c["nc"]) for x, y in zip(eng.get_net(f"v{k}"), ref.critics[k]))
    print(f"{case}: weights after Adam max abs error {werr:.2e}")
    assert werr < 1e-6
    ctl = eng.v["vc.ctl"][0].cpu().numpy()
    assert ctl[0] == ctl[1] == 2 and list(ctl[2:2 + c["nc"]]) == c["n"]
    out = eng.vcritic_end()                             # every critic's loss over its whole table
    for k in range(c["nc"]):
        lref = float(V.loss_and_grads(ref.critics[k], acts, nrm, s[k], rtg[k])[0])
        assert abs(float(out["critic_loss"][k]) - lref) <= 2e-5 * lref
    assert out["n_steps"] == 2
    eng.close()


def test_steps_need_every_table_and_a_bound_handle_refuses_init(gpu_available):
    from sac_eo._native import SacxError
    eng = make_engine(3, "two", 2, batch=16, capacity=32)
    s, rtg = states(3, 20, 1), np.ones(20, np.float32)
    eng.vcritic_begin(0, s, rtg)
    with pytest.raises(SacxError, match="critic 1 has no table"):
        eng.vcritic_steps(np.arange(16, dtype=np.int32)[None], critic_lr=1e-3)
    with pytest.raises(SacxError, match="critic 1 has no table"):
        eng.vcritic_end()
    with pytest.raises(SacxError, match="critic 2 outside"):
        eng.vcritic_value(2, s)
    assert eng.lib.sacx_vcritic_init(eng.h, 1) != 0 and b"must precede sacx_bind" in eng.lib.sacx_last_error(eng.h)
    eng.close()
    plain = make_engine(3, "two", 0, batch=16, capacity=32)             # a trainable handle without critics
    with pytest.raises(SacxError, match="has no VCritics"):
        plain.vcritic_value(0, s)
    plain.close()


# ---------------------------------------------------------------------------------------------- forms
@pytest.mark.parametrize("steps,mb", [(12, 33), (72, 16)])
def test_graph_eager_and_single_steps_bit_identical(gpu_available, steps, mb):
    """12 steps replay as graphs of 8, 1, 1, 1, 1; 72 steps as one graph of 64 and one of 8."""
    c = dict(S=17, shape="two", nc=2, n=[80, 70])
    st, nrm = make_state(17, "two", 2, seed=1)
    s, rtg = tables(c, 2)
    idx = np.stack([np.random.RandomState(5 + j).permutation(70)[:mb] for j in range(steps)]).astype(np.int32)
    got = []
    for mode in ("graph", "eager", "single"):
        eng = make_engine(17, "two", 2, batch=40, capacity=80)
        load(eng, st, nrm)
        for k in range(2):
            eng.vcritic_begin(k, s[k], rtg[k])
        if mode == "single":
            for j in range(steps):
                eng.vcritic_steps(idx[j:j + 1], critic_lr=3e-4)
        else:
            eng.vcritic_steps(idx, critic_lr=3e-4, eager=mode == "eager")
        eng.sync()
        out = {n: eng.v[n].cpu().numpy().copy() for n in eng.segments
               if n[:1] == "v" and (n[1:2].isdigit() or n in ("vc.adam_m", "vc.adam_v", "vc.ctl"))}
        out["stats"] = eng.vcritic_stats(steps)
        out["end"] = np.array([float(x) for x in eng.vcritic_end()["critic_loss"]])
        got.append(out)
        eng.close()
    assert np.array_equal(got[0]["stats"][:, 9], np.arange(1, steps + 1, dtype=np.float32))
    for other in got[1:]:
        for key in got[0]:
            assert np.array_equal(got[0][key], other[key]), key


# ---------------------------------------------------------------------------------------------- the host classes
class _Box:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, np.float32), np.ones(n, np.float32)


class _Env:
    def __init__(self, S, A=2):
        self.observation_space, self.action_space = _Box(S), _Box(A)


class _Rms:
    def __init__(self, mean, den):
        self.mean, self._den = mean, den

    def den(self):
        return self._den


UPD_KW = dict(critic_lr=1e-3, critic_update_it=3, critic_nminibatch=4)


def test_vcritic_update_end_to_end(gpu_available):
    """n = 200, 4 minibatches, 3 iterations, twice, 2 critics (B = 2: a table each)."""
    from sac_eo.algs.model_free import VCriticUpdate
    from sac_eo.critics.critics import VCritic
    S, acts = 17, ("tanh", "tanh")
    st, nrm = make_state(S, "two", 2, seed=4)
    critics = []
    for k in range(2):
        c = VCritic(_Env(S), [64, 64], ["tanh"], 1.0, rng=np.random.default_rng(k))
        c.set_weights([np.asarray(x, np.float32) for x in st.critics[k]])
        c.s_rms, c.ret_rms = _Rms(nrm.s_mean, nrm.s_den), _Rms(None, np.float32(nrm.ret_den))
        critics.append(c)
    data = [tables(dict(S=S, n=[200, 200]), 50 + 10 * u) for u in range(2)]
    refs = {}
    for key in ("f64",) + tuple(O.MATMUL_ORDERS):
        rs = np.random.RandomState(11)
        ref = V.VCriticUpdateRef(st.astype(np.float64 if key == "f64" else np.float32), acts, nrm, UPD_KW, rs)
        O.MATMUL_ORDER = "default" if key == "f64" else key
        try:
            logs = [(ref.update(s, rtg, 2), rs.get_state()) for s, rtg in data]
        finally:
            O.MATMUL_ORDER = "default"
        refs[key] = (ref, logs)
    ref, logs = refs["f64"]
    np.random.set_state(np.random.RandomState(11).get_state())
    upd = VCriticUpdate(critics, UPD_KW)
    figures = []                                         # (what, device error, fp32 envelope, single-step bar)
    for u, (s, rtg) in enumerate(data):
        log = upd.update((s, None, None, rtg, None, None), 2)
        dev, want = upd.engine.rng_get_state(), logs[u][1]
        assert np.array_equal(dev[1], want[1]) and dev[2] == want[2]         # the host stream, bit for bit
        assert len(log) == 2 and all(sorted(x) == ["critic_loss"] for x in log)
        (l64, steps64), _ = logs[u]
        assert len(steps64) == 12
        for k in range(2):
            y = l64[k]["critic_loss"]
            env = max(abs(refs[o][1][u][0][0][k]["critic_loss"] - y) for o in O.MATMUL_ORDERS) / abs(y)
            err = abs(float(log[k]["critic_loss"]) - y) / abs(y)
            print(f"update {u} critic {k} critic_loss: device {float(log[k]['critic_loss']):.7g} ref {y:.7g} error {err:.2e} "
                  f"fp32 envelope {env:.2e}")
            figures.append((f"update {u} critic_loss {k}", err, env, 2e-5))
        rows = upd.engine.vcritic_stats(12)
        assert np.array_equal(rows[:, 9], 12 * u + np.arange(1, 13, dtype=np.float32))
    assert upd.engine.v["vc.ctl"][0, 1].item() == 24
    for k in range(2):
        for i, (x, y) in enumerate(zip(critics[k].get_weights(), ref.st.critics[k])):
            env = max(float(np.max(np.abs(np.asarray(refs[o][0].st.critics[k][i], np.float64) - y))) for o in O.MATMUL_ORDERS)
            err = float(np.max(np.abs(np.asarray(x, np.float64).reshape(y.shape) - y)))
            print(f"final weights critic {k} {y.shape}: device error {err:.2e} fp32 envelope {env:.2e}")
            figures.append((f"final weights {k}.{i}", err, env, 1e-6))
    for what, err, env, bar in figures:                  # every figure is printed before the first assertion
        assert env < 1e-2, (what, env)
        assert err <= max(bar, env), (what, err, env)
    upd.engine.close()


def test_buffer_critic_update_and_ppo_on_one_engine(gpu_available):
    """TrajectoryBuffer.add x 3 -> get_update_info(critic) -> VCriticUpdate.update -> PPO.update on the engine
    PPO builds (update_kwargs['vcritics']); the global stream afterwards equals the restatement's draws."""
    import ppo_ref as R
    import test_gpu_ppo as P
    from sac_eo.algs.model_free import PPO, VCriticUpdate
    from sac_eo.common.buffers import TrajectoryBuffer
    from sac_eo.critics.critics import VCritic
    actor, cfg, pst, nrm, _ = P.update_case(seed=3, n=8)
    S, A = cfg.S, cfg.A
    actor.s_rms = _Rms(nrm.s_mean, nrm.s_den)
    vst, _ = make_state(S, "two", 1, seed=6)
    critic = VCritic(_Env(S, A), [64, 64], ["tanh"], 1.0, rng=np.random.default_rng(1))
    critic.set_weights([np.asarray(x, np.float32) for x in vst.critics[0]])
    critic.s_rms, critic.ret_rms = _Rms(nrm.s_mean, nrm.s_den), _Rms(None, np.float32(1.0))
    buf = TrajectoryBuffer(S, A, 0.99, 0.95)
    rng = np.random.RandomState(2)
    for n in (50, 90, 60):
        s = states(S, n + 1, n)
        d = np.zeros(n)
        d[-1] = n == 90
        buf.add(s[:-1], rng.normal(size=(n, A)).astype(np.float32), rng.normal(size=n).astype(np.float32), s[1:], d)
    assert buf.current_size == 200 and buf.traj_total == 3
    np.random.set_state(np.random.RandomState(17).get_state())
    ppo = PPO(actor, dict(P.UPD_KW, vcritics=1, rollout_capacity=200))
    ppo._ensure_engine(200, 50)                          # the engine, with the critic's segments
    eng = ppo.engine
    assert eng.cfg.vcritics == 1 and "v0.l0" in eng.segments
    upd = VCriticUpdate([critic], UPD_KW, actor=actor)
    with pytest.raises(RuntimeError, match="not bound"):   # an unbound critic has no value(): no CPU path
        buf.get_update_info(critic)
    upd._ensure_engine(200, 50)                          # the actor's engine has a critic: bound to it as v0
    assert upd.engine is eng and critic._net == "v0"
    s_all, a_all, adv, rtg, sp_all, rtg_sp = buf.get_update_info(critic)
    assert adv.dtype == np.float32 and adv.shape == (200,) and np.isfinite(adv).all()
    v_s, v_sp = np.asarray(critic.value(s_all)), np.asarray(critic.value(sp_all))
    a64 = V.gae_batch_loop(v_s, v_sp, buf.r_all, buf.d_all, buf.idx_all, 0.99, 0.95, f64=True)
    assert np.max(np.abs(adv - a64[0]) / gae_bar(a64[0], a64[3])) <= 1.0
    log_c = upd.update(([s_all], None, None, [rtg], None, None), 1)
    log_a = ppo.update((s_all, a_all, adv, rtg, sp_all, rtg_sp))
    assert np.isfinite(float(log_c[0]["critic_loss"])) and sorted(log_a) == sorted(P.LOG_KEYS)
    rs = np.random.RandomState(17)                       # 3 critic shuffles, then 3 actor shuffles, of 200 rows
    for _ in range(6):
        rs.shuffle(np.arange(200))
    dev, want = eng.rng_get_state(), rs.get_state()
    assert np.array_equal(dev[1], want[1]) and dev[2] == want[2]
    assert eng.v["vc.ctl"][0, 1].item() == 12 and eng.v["ppo.ctl"][0, 1].item() == 12
    eng.close()


def test_critics_of_another_shape_get_their_own_engine(gpu_available):
    """PPO's vcritics option builds critics of the actor's description; VCriticUpdate adopts the actor's engine
    only for critics that fit it (layers and activations), and builds one otherwise."""
    import test_gpu_ppo as P
    from sac_eo.algs.model_free import PPO, VCriticUpdate
    from sac_eo.critics.critics import VCritic
    actor, cfg, _, _, _ = P.update_case(seed=3, n=8)
    ppo = PPO(actor, dict(P.UPD_KW, vcritics=1, rollout_capacity=64))
    ppo._ensure_engine(64, 16)
    s, rtg = tables(dict(S=cfg.S, n=[64]), 3)
    engines = []
    for layers, acts in (([64, 64], ["tanh"]), ([32, 48], ["tanh"]), ([64, 64], ["relu"])):
        c = VCritic(_Env(cfg.S, cfg.A), layers, acts, 1.0, rng=np.random.default_rng(1))
        upd = VCriticUpdate([c], UPD_KW, actor=actor)
        log = upd.update((s, None, None, rtg, None, None), 1)
        assert np.isfinite(float(log[0]["critic_loss"]))
        engines.append(upd.engine)
    assert engines[0] is ppo.engine and engines[1] is not ppo.engine and engines[2] is not ppo.engine
    assert [tuple(t.shape) for t in engines[1]._layers("v0")] == [(cfg.S + 1, 32), (33, 48), (49, 1)]
    for e in engines:
        e.close()


@pytest.mark.parametrize("vcritics", [0, 2])
def test_ppo_step_is_left_alone(gpu_available, monkeypatch, vcritics):
    """test_gpu_ppo's single-step case on a trainable handle without critics, and on one with them."""
    import test_gpu_ppo as P
    if vcritics:
        orig = P.make_engine
        monkeypatch.setattr(P, "make_engine", lambda *a, **kw: orig(*a, vcritics=vcritics, **kw))
    P.test_one_minibatch_step(True, "pendulum_312")
    P.test_one_minibatch_step(True, "hc_33_floor")
