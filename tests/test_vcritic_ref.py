"""tests/vcritic_ref.py (the fp64 restatement of the critic side of the on-policy loop) pinned to
independent computations, and the host ``TrajectoryBuffer`` / ``gae_batch`` pinned bit for bit to what
the reference's own NumPy modules returned (tests/golden/gae_ref.npz, made by
tests/golden/make_gae_fixtures.py).  No GPU."""
import os

import numpy as np
import pytest

import sac_oracle as O
import vcritic_ref as V
from helpers import nontrivial_normalizers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gae_ref.npz")

CASES = [dict(S=3, hidden=(64, 64), acts=("tanh", "tanh"), nc=1), dict(S=17, hidden=(32, 48, 40), acts=("relu", "tanh", "elu"), nc=3),
         dict(S=7, hidden=(520,), acts=("tanh",), nc=2)]


def _setup(c, seed=3):
    rng = np.random.RandomState(seed)
    nrm = nontrivial_normalizers(rng, c["S"], 1)
    nrm.ret_den = np.float32(2.7)
    st = V.init_state(c["S"], c["hidden"], c["nc"], seed=seed)
    n = 37
    s = [(rng.normal(size=(n, c["S"])) * 1.5).astype(np.float32) for _ in range(c["nc"])]
    rtg = [(rng.normal(size=n) * 4.0 + 1.0).astype(np.float32) for _ in range(c["nc"])]
    return st, nrm, s, rtg


def _torch_loss(ws, acts, nrm, s, rtg):
    import torch
    x = (torch.as_tensor(np.asarray(s, np.float64)) - torch.as_tensor(np.asarray(nrm.s_mean, np.float64))) / \
        torch.as_tensor(np.asarray(nrm.s_den, np.float64))
    h = x
    nl = len(ws) // 2
    for l in range(nl):
        z = h @ ws[2 * l] + ws[2 * l + 1]
        if l < nl - 1:
            h = {"relu": torch.relu, "tanh": torch.tanh, "elu": torch.nn.functional.elu}[acts[l]](z)
    rden = float(nrm.ret_den)
    value = z[:, 0] * rden
    return 0.5 * torch.mean((torch.as_tensor(np.asarray(rtg, np.float64)) / rden - value / rden) ** 2)


@pytest.mark.parametrize("c", CASES, ids=lambda c: "x".join(map(str, c["hidden"])))
def test_loss_and_gradients_match_torch_autograd(c):
    import torch
    st, nrm, s, rtg = _setup(c)
    tw = [[torch.tensor(np.asarray(w, np.float64), requires_grad=True) for w in cw] for cw in st.critics]
    total = sum(_torch_loss(tw[k], c["acts"], nrm, s[k], rtg[k]) for k in range(c["nc"]))
    total.backward()
    total = total.detach()
    ref = [w.grad.numpy() for cw in tw for w in cw]
    keep = {}
    before = [w.copy() for w in st.trainables()]
    out = V.critic_step(st, c["acts"], nrm, s, rtg, 1e-3, keep)
    assert abs(out["loss"] - float(total)) <= 1e-10 * max(1.0, abs(float(total)))
    assert abs(sum(out["losses"]) - out["loss"]) <= 1e-12 * max(1.0, abs(out["loss"]))
    for g, r in zip(keep["grads"], ref):
        assert np.max(np.abs(g - r)) <= 1e-10 * max(1.0, np.max(np.abs(r)))
    # the summed-loss Adam step: ONE iteration count over all critics, moments per variable; Keras Adam's
    # first step written out independently
    assert st.opt.t == 1 and len(st.opt.m) == len(before)
    lr_t = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    for w0, w1, g in zip(before, st.trainables(), ref):
        step = lr_t * (g * (1 - 0.9)) / (np.sqrt(g * g * (1 - 0.999)) + 1e-7)
        assert np.max(np.abs((w0 - w1) - step)) <= 1e-12


def test_value_is_the_output_times_ret_den():
    c = CASES[0]
    st, nrm, s, _ = _setup(c)
    out = V.forward(st.critics[0], c["acts"], nrm, s[0], np.float64)[0]
    assert np.array_equal(V.value(st.critics[0], c["acts"], nrm, s[0]), out * np.float64(nrm.ret_den))


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.99, 0.0)])
def test_gae_loop_equals_lfilter(gamma, lam):
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.RandomState(5)
    for n in (1, 2, 63, 64, 65, 1000):
        v_s, v_sp, r = [rng.normal(size=n).astype(np.float32) * 3 for _ in range(3)]
        d = (rng.uniform(size=n) < 0.1).astype(np.float64)
        adv, rtg, rtg_sp, delta = V.gae_loop(v_s, v_sp, r, d, gamma, lam)
        dref = r + gamma * (1 - d) * v_sp - v_s
        aref = sig.lfilter([1], [1, float(-gamma * lam)], dref[::-1], axis=0)[::-1]
        assert np.array_equal(delta, dref)
        assert np.array_equal(adv, aref.astype("float32"))
        assert np.array_equal(rtg, (aref + v_s).astype("float32"))
        assert np.array_equal(rtg_sp, (((aref + v_s) - r) / gamma).astype("float32"))


def test_gae_batch_loop_restarts_at_every_trajectory():
    rng = np.random.RandomState(6)
    lens = [1, 4, 1, 9]
    n = sum(lens)
    v_s, v_sp, r = [rng.normal(size=n).astype(np.float32) for _ in range(3)]
    d = np.zeros(n)
    traj = np.concatenate([np.full(l, 7 + i) for i, l in enumerate(lens)])
    got = V.gae_batch_loop(v_s, v_sp, r, d, traj, 0.99, 0.95)
    o = 0
    for l in lens:
        one = V.gae_loop(v_s[o:o + l], v_sp[o:o + l], r[o:o + l], d[o:o + l], 0.99, 0.95)
        for a, b in zip(got, one):
            assert np.array_equal(a[o:o + l], b)
        o += l


# ---------------------------------------------------------------------------------------------- the fixture
class LookupCritic:
    """The fixture's duck critic from its recorded arrays: value(s).numpy() by state row."""

    class _Out(np.ndarray):
        def numpy(self):
            return np.asarray(self)

    def __init__(self, pairs):
        self.table = {}
        for s, v in pairs:
            for row, x in zip(np.asarray(s, np.float32), v):
                self.table[row.tobytes()] = x
        self.calls = 0

    def value(self, s):
        self.calls += 1
        return np.array([self.table[row.tobytes()] for row in np.asarray(s, np.float32)], np.float32).view(self._Out)


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def test_fixture_is_small(gold):
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_host_gae_batch_reproduces_the_reference(gold):
    from sac_eo.common.buffer_utils import gae_batch
    g = gold
    critic = LookupCritic([(g["s"], g["v_s"]), (g["sp"], g["v_sp"])])
    adv, rtg, rtg_sp = gae_batch(critic, float(g["gamma"]), float(g["lam"]), g["s"], g["r"], g["sp"], g["d"], g["idx_all"])
    for name, x in (("adv", adv), ("rtg", rtg), ("rtg_sp", rtg_sp)):
        assert x.dtype == np.float32 and np.array_equal(x, g[name]), name
    # and the restatement's plain loop on the recorded values
    a2, r2, p2, _ = V.gae_batch_loop(g["v_s"], g["v_sp"], g["r"], g["d"], g["idx_all"], float(g["gamma"]), float(g["lam"]))
    assert np.array_equal(a2, g["adv"]) and np.array_equal(r2, g["rtg"]) and np.array_equal(p2, g["rtg_sp"])


def test_host_trajectory_buffer_reproduces_the_reference(gold):
    from sac_eo.common.buffers import TrajectoryBuffer
    g = gold
    buf = TrajectoryBuffer(3, 2, float(g["gamma"]), float(g["lam"]), buffer_size=100)
    for i in range(4):
        buf.add(*[g[f"t_in{i}_{k}"] for k in ("s", "a", "r", "sp", "d")])
        assert [buf.traj_total, buf.steps_total, buf.current_size] == list(g["t_counters"][i])
    for name in ("s_all", "a_all", "r_all", "sp_all", "d_all", "idx_all"):
        x = getattr(buf, name)
        assert x.dtype == g["t_" + name].dtype and np.array_equal(x, g["t_" + name]), name
    critic = LookupCritic([(g["t_s_all"], g["t_v_s"]), (g["t_sp_all"], g["t_v_sp"])])
    whole = buf.get_update_info(critic)
    for name, x in zip(("s", "a", "adv", "rtg", "sp", "rtg_sp"), whole):
        assert np.array_equal(x, g["t_whole_" + name]), name
    np.random.seed(77)
    sub = buf.get_update_info(critic, batch_size=16)
    for name, x in zip(("s", "a", "adv", "rtg", "sp", "rtg_sp"), sub):
        assert np.array_equal(x, g["t_sub_" + name]), name
    assert np.array_equal(np.random.randint(1 << 30, size=2), g["t_sub_next_draw"])      # one randint draw, no more


def test_add_batch_keeps_the_reference_indexing():
    """add_batch with a 1-d batch is add; with trajectories that terminate it indexes ONE row
    ([term_idx], as written), which np.concatenate then refuses -- the reference's behaviour."""
    from sac_eo.common.buffers import TrajectoryBuffer
    buf = TrajectoryBuffer(3, 2, 0.99, 0.95)
    rng = np.random.RandomState(1)
    s, a, r, sp = rng.normal(size=(5, 3)), rng.normal(size=(5, 2)), rng.normal(size=5), rng.normal(size=(5, 3))
    buf.add_batch(*[np.asarray(x, np.float32) for x in (s, a, r, sp)], np.zeros(5))
    assert buf.current_size == 5 and buf.traj_total == 1
    S, Ab, R, SP = [np.stack([np.asarray(x, np.float32)] * 2) for x in (s, a, r, sp)]
    buf.add_batch(S, Ab, R, SP, np.zeros((2, 5)))                      # no terminal: whole trajectories
    assert buf.current_size == 15 and buf.traj_total == 3
    D = np.zeros((2, 5))
    D[0, 1] = 1
    with pytest.raises(ValueError):
        buf.add_batch(S, Ab, R, SP, D)


def test_model_info_draws_one_randint():
    from sac_eo.common.buffers import TrajectoryBuffer
    buf = TrajectoryBuffer(3, 2, 0.99, 0.95)
    rng = np.random.RandomState(2)
    buf.add(*[np.asarray(x, np.float32) for x in (rng.normal(size=(9, 3)), rng.normal(size=(9, 2)), rng.normal(size=9),
                                                   rng.normal(size=(9, 3)))], np.zeros(9))
    np.random.seed(5)
    s, a, sp, r = buf.get_model_info(4)
    ref = np.random.RandomState(5).randint(9, size=4)
    assert np.array_equal(s, buf.s_all[ref]) and np.array_equal(r, buf.r_all[ref])
    assert buf.get_states() is buf.s_all and len(buf.get_offmodel_info()) == 5
