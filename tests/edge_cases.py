"""Edge states of the squashed-Gaussian head and of min(Q1, Q2), shared by the CPU and the device tests.

Each mutator changes an oracle state in place, after ``helpers.make_learner`` built it and before it is
loaded into an engine, so the oracle and the device start from the same edge.  ``mutating`` wraps
``helpers.make_learner`` for ``monkeypatch.setattr(helpers, "make_learner", ...)``: ``helpers.make_pair``
resolves the name through its module, so the one-update bodies of test_gpu_depth.py run on the edge state
as they are.

  lsvar      the state-independent log-std at (-6, -5, 2, 2.5, 0, 1.9): two coordinates outside the clip
             [-5, 2] (mask 0), two exactly on its bounds (TF clip_by_value passes the gradient there: mask 1),
             two inside, one of them near the top.  At std = e^2 the pre-squash x = mu + std u reaches +-20:
             tanh rounds to +-1 in fp32 and softplus(-2x) takes both of its outer branches (|x| > 6.97:
             |-2x| beyond SOFTPLUS_THR = 13.94).
  pss_edges  per_state_std: the log-std half of the actor's output layer scaled by 12 around the same six
             biases, the weight columns of coordinates 1 and 2 zeroed: those two are exactly -5.0 and exactly
             2.0 on every row, the other four fall on both sides of each bound from row to row.
  SAT        make_learner / make_pair keywords: an actor output layer of gain 8 under tanh hidden layers,
             max |mu| about 15, so the mean alone saturates tanh.
  tie        critic 1 and its target are copies of critic 0: Q1 == Q2 bit for bit on every row.
"""
import inspect

import numpy as np

LOGSTD_EDGES = (-6.0, -5.0, 2.0, 2.5, 0.0, 1.9)
SAT = dict(actor_gain=8.0, act="tanh")


def lsvar(st, ocfg):
    st.logstd[0] = np.resize(np.asarray(LOGSTD_EDGES, st.logstd.dtype), ocfg.A)


def pss_edges(st, ocfg):
    assert ocfg.per_state_std
    A = ocfg.A
    W, b = st.actor[-2], st.actor[-1]
    W[:, A:] *= W.dtype.type(12)
    b[A:] = np.resize(np.asarray(LOGSTD_EDGES, b.dtype), A)
    W[:, A + 1] = 0          # exactly -5.0 on every row
    W[:, A + 2] = 0          # exactly 2.0 on every row


def tie(st, ocfg):
    st.q[1] = [w.copy() for w in st.q[0]]
    st.q_targ[1] = [w.copy() for w in st.q_targ[0]]


MUTATORS = {"lsvar": lsvar, "pss_edges": pss_edges, "tie": tie}


def split(edge):
    """'lsvar+sat' -> ((lsvar,), SAT): the mutators of an edge name and the keywords it adds."""
    parts = edge.split("+")
    kw = dict(SAT) if "sat" in parts else {}
    if "pss_edges" in parts:
        kw["per_state_std"] = True
    return tuple(MUTATORS[p] for p in parts if p != "sat"), kw


def mutating(make_learner, mutators):
    """make_learner followed by the mutators on its state (same signature, same return)."""
    sig = inspect.signature(make_learner)

    def wrapped(*args, **kwargs):
        sig.bind(*args, **kwargs)
        out = make_learner(*args, **kwargs)
        for m in mutators:
            m(out[1], out[0])
        return out
    return wrapped


def clip_mask(lraw):
    """d clip / d lraw of TF clip_by_value on [-5, 2]: 1 inside and at the bounds, 0 outside."""
    return ((lraw >= -5.0) & (lraw <= 2.0)).astype(np.float64)
