"""The cases of tests/test_gpu_softmax_act.py and their seeded inputs, shared with the CPU check of the
comparison's premise (tests/test_mfrl_config.py): nets, states, starting streams, and the rows a comparison
of Gumbel-argmax picks may leave out.

Rows n in {1, 7, 16, 17, 1030} x actions A in {2, 5, 32}, S = 17.  The (64, 64) net takes the few-rows path
up to 16 rows and the generic chain above; (32,) and (64, 64) + layer norm take the chain at every n.
n = 1030 crosses a chunk of 1,024 rows."""
import numpy as np

import sac_oracle as O
import softmax_ref as SM
from helpers import nontrivial_normalizers

S = 17
GAP = 1e-4              # rows whose top-two gap of x is below this are left out of the action comparison
MAX_OUT = 0.01          # ... at most this share of a case's rows

NETS = {
    "h64": dict(hidden=(64, 64), acts=("tanh", "tanh")),
    "one32": dict(hidden=(32,), acts=("tanh",)),
    "ln64": dict(hidden=(64, 64), acts=("tanh", "tanh"), layer_norm=True),
}
STREAMS = ("fresh", "pos623", "gauss")

CASES = [("h64", n, A) for n in (1, 7, 16, 17, 1030) for A in (2, 5, 32)]
CASES += [("one32", n, A) for n, A in ((1, 2), (7, 32), (16, 5), (17, 5), (1030, 32))]
CASES += [("ln64", n, A) for n, A in ((1, 32), (7, 5), (16, 2), (1030, 5))]
# every case with one starting stream, in rotation: each stream meets both paths and every A
CASES = [(net, n, A, STREAMS[i % 3]) for i, (net, n, A) in enumerate(CASES)]


def make_state(net, A, seed=2, span=4.0):
    """(oracle cfg, state, normaliser): the last layer scaled so that the logits of 64 probe rows span about
    +-span around their row mean (argmax rows of the deterministic form then have gaps of the logits' order)."""
    c = NETS[net]
    cfg = O.Config(S=S, A=A, hidden=c["hidden"], actor_acts=c["acts"], layer_norm=c.get("layer_norm", False))
    st = SM.init_state(cfg, seed=seed, bias_scale=0.1, gain=0.5)
    nrm = nontrivial_normalizers(np.random.RandomState(seed + 50), S, A)
    lg = SM.forward(st, cfg, nrm, states(64, seed))[0]
    k = np.float32(span / np.abs(lg - lg.mean(-1, keepdims=True)).max())
    st.actor[-2] = np.asarray(np.asarray(st.actor[-2] * k, np.float32), np.float64)
    st.actor[-1] = np.asarray(np.asarray(st.actor[-1] * k, np.float32), np.float64)
    return cfg, st, nrm


def states(n, seed):
    rng = np.random.RandomState(seed + 900)
    return (rng.normal(size=(n, S)) * rng.uniform(0.3, 2.0, S)).astype(np.float32)


def stream(kind, seed=11):
    """A starting state of the global stream: fresh from a seed; position 623, so that the first double
    straddles the 624-word block; with a cached gaussian (has_gauss = 1)."""
    rs = np.random.RandomState(seed)
    if kind == "pos623":
        rs.random_sample(40)
        st = rs.get_state()
        return (st[0], st[1], 623, 0, 0.0)
    if kind == "gauss":
        rs.normal()
        assert rs.get_state()[3] == 1
    return rs.get_state()


def uniforms(state, n, A):
    """np.random.random(size=(n, A)) from `state` -> (u, the state afterwards)."""
    rs = np.random.RandomState(0)
    rs.set_state(state)
    u = rs.random_sample((n, A))
    return u, rs.get_state()


def perturbed(logits, u):
    """x of gumbel_argmax: the f32 (logits - rowmax) + float32(-log(-log u)); u = None: the logits."""
    x = np.asarray(logits, np.float32)
    if u is None:
        return x
    x = x - x.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return x + (-np.log(-np.log(np.asarray(u, np.float64)))).astype(np.float32)


def clear_rows(logits, u):
    """Rows whose top-two gap of x exceeds GAP (one action: every row)."""
    x = perturbed(logits, u)
    if x.shape[-1] < 2:
        return np.ones(x.shape[0], bool)
    top = np.sort(x, axis=-1)[:, -2:]
    return (top[:, 1] - top[:, 0]) > GAP


def may_leave_out(n):
    """The cap on rows left out: 1 % of the rows of a case (none below 100 rows)."""
    return int(MAX_OUT * n)
