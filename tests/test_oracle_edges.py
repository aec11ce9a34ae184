"""The oracle's edge semantics against autograd, before the device is held to them (tests/test_gpu_edges.py).

The closed-form backward of oracle/sac_oracle.py on the states of tests/edge_cases.py -- the log-std below,
exactly at, inside and above the clip bounds [-5, 2] (state-independent and per state), pre-squash values
past both outer softplus branches, and Q1 == Q2 on every row -- against torch.autograd in fp64 on the
torch restatement of tests/test_oracle.py.  torch.clamp passes the gradient at the bounds and torch.minimum
splits a tie evenly, as TF's clip_by_value and reduce_min do (the reference: continuous_actors.py:250-379,
SAC_expert.py:262-296).
"""
import numpy as np
import pytest

import edge_cases as EC
import sac_oracle as O
import test_oracle as TO

torch = pytest.importorskip("torch")
_t, _mlp, _head_eval = TO._t, TO._mlp, TO._head_eval


@pytest.mark.parametrize("edge,use_expert", [("lsvar", False), ("lsvar", True), ("pss_edges", False),
                                             ("pss_edges", True), ("tie", False)])
def test_oracle_edge_gradients_match_autograd(edge, use_expert):
    act = "tanh"
    pss = edge == "pss_edges"
    cfg = O.Config(S=5, A=6, hidden=(16, 12), act=act, B=32, model_hidden=(20, 18), per_state_std=pss)
    A, S = cfg.A, cfg.S
    st0, batch, noises, nrm, ex = TO._make(cfg)
    for m in EC.split(edge)[0]:
        m(st0, cfg)
    ls0 = st0.logstd.copy()
    st1 = st0.copy()
    keep = {}
    O.sac_update(st1, cfg, nrm, batch, *noises, expert=ex if use_expert else None, keep=keep)

    # the edges are there
    mask = np.concatenate([keep["head_p"].mask] + [h.mask for h in keep["head_e"]], 0)
    lraw = np.asarray(keep["ls_p"]) if pss else np.broadcast_to(ls0, keep["mu_p"].shape)
    if edge != "tie":
        assert (mask == 0).any() and (lraw == -5).any() and (lraw == 2).any() and (lraw < -5).any() and (lraw > 2).any()
        assert np.array_equal(keep["head_p"].mask, EC.clip_mask(lraw))
        y = -2 * keep["head_p"].x
        thr = -(np.log(np.finfo(np.float32).eps) + 2.0)      # where an fp32 run leaves the middle branch
        print(f"{edge}: mask zeros {int((mask == 0).sum())} of {mask.size}, softplus outer branches "
              f"{int((y > thr).sum())} / {int((y < -thr).sum())}, max |x| {np.max(np.abs(keep['head_p'].x)):.1f}")
        if edge == "lsvar":      # std = e^2: x past the threshold on both sides, where -2 tanh(x) is the whole slope
            assert (y > thr).any() and (y < -thr).any()
    else:
        assert np.array_equal(keep["q1p"], keep["q2p"])

    s, a, sp, r, d = [_t(x) for x in batch]
    nm = lambda x, m, dd: (x - _t(m)) / _t(dd)
    y = _t(keep["y"])
    for k in range(2):
        P = [_t(w).requires_grad_() for w in st0.q[k]]
        q = _mlp(P, torch.cat([nm(s, nrm.s_mean, nrm.s_den), nm(a, nrm.a_mean, nrm.a_den)], 1), act)
        g = torch.autograd.grad(torch.mean(0.5 * ((q - y[:, None]) ** 2).sum(-1)), P)
        for gg, mine in zip(g, keep["q%d_grads" % k]):
            np.testing.assert_allclose(mine, gg.numpy(), rtol=1e-9, atol=1e-12)

    PA = [_t(w).requires_grad_() for w in st0.actor]
    LS = _t(st0.logstd).requires_grad_()
    Q = [[_t(w) for w in net] for net in st1.q]

    def head(x):
        out = _mlp(PA, x, act)
        return (out[:, :A], out[:, A:]) if pss else (out, LS.expand_as(out))

    s_n = nm(s, nrm.s_mean, nrm.s_den)
    pi, nlp = _head_eval(*head(s_n), _t(noises[1]))
    xq = torch.cat([s_n, nm(pi, nrm.a_mean, nrm.a_den)], 1)
    minq = torch.minimum(_mlp(Q[0], xq, act), _mlp(Q[1], xq, act))
    p = torch.mean(-float(st0.alpha) * nlp[:, None] - minq)
    if use_expert:
        M = [[_t(w) for w in net] for net in st0.models]
        sq = []
        for k, (se, spe, ne) in enumerate([(ex.s1, ex.sp1, ex.noise1), (ex.s2, ex.sp2, ex.noise2)]):
            se_n = nm(_t(se), nrm.s_mean, nrm.s_den)
            mue, le = head(se_n)
            ca = torch.tanh(mue + torch.exp(torch.clamp(le, -5.0, 2.0)) * _t(ne))
            om = _mlp(M[k], torch.cat([se_n, nm(ca, nrm.a_mean, nrm.a_den)], 1), cfg.model_act)
            sp_hat = _t(se) + (om[:, :S] * _t(nrm.d_den) + _t(nrm.d_mean))
            sq.append(((_t(spe) - sp_hat) ** 2).sum(-1))
        p = (1 - ex.epsilon) * p + ex.epsilon * torch.mean(0.5 * (sq[0] + sq[1]))
    g = torch.autograd.grad(p, PA + ([] if pss else [LS]))
    for gg, mine in zip(g[:len(PA)], keep["actor_grads"]):
        np.testing.assert_allclose(mine, gg.numpy(), rtol=1e-7, atol=1e-10)
    if pss:
        assert not keep["g_logstd"].any()
    else:
        gl = g[-1].numpy()
        np.testing.assert_allclose(keep["g_logstd"], gl, rtol=1e-7, atol=1e-10)
        if edge == "lsvar":      # 0 outside the bounds, passed at them
            masked = EC.clip_mask(ls0[0]) == 0
            assert np.all(gl[0][masked] == 0) and np.all(keep["g_logstd"][0][masked] == 0)
            assert np.all(gl[0][~masked] != 0)
