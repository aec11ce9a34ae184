"""The oracle's operand-rounding mode (sac_oracle.GEMM_OPERANDS = "bf16") pinned
on the CPU before tests/test_gpu_bf16.py trusts it:

* bf16_rne equals torch's float32 -> bfloat16 conversion bit for bit;
* the closed-form backward under "bf16" equals torch autograd (fp64) of the same forward with each
  rounding straight-through and each backward GEMM taking its rounded delta;
* the envelope: for every case of the device test the rounding oracle in fp32 under each of
  MATMUL_ORDERS stays inside the bars the device test uses (bf16_parity.bars), the cap on outliers
  included with half of it to spare, and no bar exceeds 10 x the fp32 path's;
* sensitivity: the fp64 oracle with exact operands, with truncated operands and with the dW GEMMs left
  unrounded each miss those bars, through the comparison the device test calls.

Measured envelopes (largest error of the three fp32 executions against the fp64 one; stages after
leaving out flip_cap elements, none of which lay beyond a bar):

  case      stages    losses   gradients  targets   widest bar / the fp32 path's
  odd       4.0e-07   1.9e-07  1.5e-04    5.1e-08   2.9  (grad.q1.0)
  narrow    2.7e-07   2.9e-07  2.4e-04    5.0e-08   4.8  (grad.q0.2)
  hc        3.0e-07   2.5e-07  1.4e-04    3.0e-08   2.7  (grad.actor.0)
  pss_ln    2.7e-07   2.7e-07  8.3e-08    5.0e-08   1.0
  generic   3.4e-07   2.3e-07  3.6e-04    2.0e-08   7.1  (grad.q0.0)
  wide_k0   2.3e-07   2.6e-07  2.0e-05    5.0e-08   1.0
  off4_bf16 2.8e-07   2.6e-07  1.9e-05    5.3e-08   1.0  (hidden (63, 65): tests/test_gpu_ragged.py)
  hc, Q1 / Q2 over 30 updates: 3.8e-05 (bar 1.5e-04)
  world-model fit: first-step gradients 1.9e-04 (3.9, grad.m0.2), three losses 6.5e-07; object calls on
  64 rows <= 3e-07 (nothing left out); one rollout step <= 1.1e-07 (no element beyond a bar)

The forward stages and the losses of the fp32 executions sit at fp32 rounding.  The gradients do not:
a delta that the fp32 run computes within 1e-7 of the fp64 one can round to the other neighbouring
bf16 as a dW or dX operand, which moves one term of a sum over B rows by up to 2^-8 of it -- 1e-4 of
the gradient's largest element at B = 37 .. 128.  Whether one of the three orders meets such a flip
depends on the seed (2e-7 .. 7e-4 over eight seeds per case), so the gradient bars are 2e-4 where none
did and up to 1.4e-3 where one did.
"""
import numpy as np
import pytest

import bf16_parity as P
import sac_oracle as O

torch = pytest.importorskip("torch")


# ----------------------------------------------------------------- bf16_rne
def _bits(f):
    return np.asarray(f, np.float32).view(np.uint32)


def test_bf16_rne_matches_torch():
    rs = np.random.RandomState(0)
    x = np.concatenate([
        rs.normal(size=20000).astype(np.float32) * np.float32(10.0) ** rs.randint(-30, 30, 20000).astype(np.float32),
        # exact ties: the low half 0x8000 under an even and under an odd kept mantissa, both signs
        np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F7F8000, 0x00018000, 0x7F7F8000],
                 np.uint32).view(np.float32),
        # just below and just above a tie
        np.array([0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001], np.uint32).view(np.float32),
        np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, np.finfo(np.float32).tiny, np.finfo(np.float32).max,
                  -np.finfo(np.float32).max, np.inf, -np.inf], np.float32)])
    ref = torch.tensor(x).to(torch.bfloat16).float().numpy()
    got = O.bf16_rne(x)
    assert got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(ref))
    assert np.array_equal(_bits(got) & 0xFFFF, np.zeros_like(_bits(got)))
    nan = O.bf16_rne(np.array([np.nan, -np.nan], np.float32))
    assert np.all(np.isnan(nan)) and np.all(np.isnan(torch.tensor([float("nan")]).to(torch.bfloat16).float().numpy()))
    # the caller's dtype and shape; fp64 values round through their float32 image
    x64 = rs.normal(size=(7, 5))
    got64 = O.bf16_rne(x64)
    assert got64.dtype == np.float64 and got64.shape == (7, 5)
    assert np.array_equal(got64, torch.tensor(x64.astype(np.float32)).to(torch.bfloat16).double().numpy())
    # off: the identity, the same object
    assert O.GEMM_OPERANDS == "exact" and O._rb(x64) is x64


# ----------------------------------------------------------------- backward vs autograd
def _t(x):
    return torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)


def _rb(t):
    return torch.from_numpy(O.bf16_rne(t.detach().numpy()))


class _Dense(torch.autograd.Function):
    """y = a w + b as the device runs it.  fwd: the product is an MFMA GEMM (operands rounded, straight
    through); dx: so is its dX (rounded delta and weights).  dW is always a GEMM: rounded input and delta,
    the bias gradient the column sums of the rounded delta."""
    @staticmethod
    def forward(ctx, a, w, b, fwd, dx):
        ctx.save_for_backward(a, w)
        ctx.dx = dx
        return (_rb(a) @ _rb(w) if fwd else a @ w) + b

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        ga = _rb(g) @ _rb(w).T if ctx.dx else g @ w.T
        return ga, _rb(a).T @ _rb(g), _rb(g).sum(0), None, None


class _ColSum(torch.autograd.Function):
    """x + p with p one row per column (logstd, beta): p's gradient sums the rounded rows (an all-ones-row
    problem of actor.adam)."""
    @staticmethod
    def forward(ctx, x, p):
        return x + p

    @staticmethod
    def backward(ctx, g):
        return g, _rb(g).sum(0, keepdim=True).reshape(-1)


class _Scale(torch.autograd.Function):
    """gamma * xhat: gamma's gradient sums the rounded rows of dY * xhat."""
    @staticmethod
    def forward(ctx, xh, gamma):
        ctx.save_for_backward(xh, gamma)
        return xh * gamma

    @staticmethod
    def backward(ctx, g):
        xh, gamma = ctx.saved_tensors
        return g * gamma, _rb(g * xh).sum(0)


_ACT = {"relu": torch.relu, "tanh": torch.tanh, "elu": torch.nn.functional.elu}


def _net(params, x, act, head, ln=None):
    """head "rows": the output layer on a row kernel (forward and dX unrounded); "gemm": a GEMM."""
    n = len(params) // 2
    h = x
    for l in range(n):
        last = l == n - 1
        fwd = not (last and head == "rows")
        z = _Dense.apply(h, params[2 * l], params[2 * l + 1], fwd, fwd and l > 0)
        if l == 0 and ln is not None:
            d = z - z.mean(-1, keepdim=True)
            xh = d / torch.sqrt((d * d).mean(-1, keepdim=True) + O.LN_EPS)
            h = torch.tanh(_ColSum.apply(_Scale.apply(xh, ln[0]), ln[1]))
        else:
            h = z if last else _ACT[act](z)
    return h


def _head_eval(mu, lraw, u):
    l = torch.clamp(lraw, -5.0, 2.0)
    x = mu + torch.exp(l) * u
    z = (x - mu) / torch.exp(l)
    nlp = 0.5 * (z * z + 2 * l + np.log(2 * np.pi)).sum(-1)
    return torch.tanh(x), nlp + (2.0 * (np.log(2.0) - x - torch.nn.functional.softplus(-2.0 * x))).sum(-1)


@pytest.mark.parametrize("act,use_expert,layer_norm", [("relu", False, False), ("tanh", True, False), ("elu", True, False),
                                                       ("relu", True, True)])
def test_bf16_backward_matches_autograd(act, use_expert, layer_norm):
    """The scaled-delta form (BF16_UNIT_DELTAS False) is autograd's chain rule term by term; the unit form
    is checked against it below."""
    from test_oracle import _make
    cfg = O.Config(S=5, A=3, hidden=(16, 12), act=act, B=32, model_hidden=(20, 18), layer_norm=layer_norm)
    st0, batch, noises, nrm, ex = _make(cfg)
    st1 = st0.copy()
    keep = {}
    with P.oracle_mode("bf16", unit=False):
        O.sac_update(st1, cfg, nrm, batch, *noises, expert=ex if use_expert else None, keep=keep)
    s, a, sp, r, d = [_t(x) for x in batch]
    S = cfg.S
    nm = lambda x, m, dd: (x - _t(m)) / _t(dd)
    y = _t(keep["y"])
    for k in range(2):
        Pq = [_t(w).requires_grad_() for w in st0.q[k]]
        q = _net(Pq, torch.cat([nm(s, nrm.s_mean, nrm.s_den), nm(a, nrm.a_mean, nrm.a_den)], 1), act, "rows")
        g = torch.autograd.grad(torch.mean(0.5 * ((q - y[:, None]) ** 2).sum(-1)), Pq)
        for gg, mine in zip(g, keep["q%d_grads" % k]):
            np.testing.assert_allclose(mine, gg.numpy(), rtol=1e-9, atol=1e-12)

    PA = [_t(w).requires_grad_() for w in st0.actor]
    LS = _t(st0.logstd[0]).requires_grad_()
    Q = [[_t(w) for w in net] for net in st1.q]

    def actor(x):
        if layer_norm:
            return _net(PA[:2] + PA[4:], x, act, "rows", ln=(PA[2], PA[3]))
        return _net(PA, x, act, "rows")

    s_n = nm(s, nrm.s_mean, nrm.s_den)
    mu = actor(s_n)
    pi, nlp = _head_eval(mu, _ColSum.apply(torch.zeros_like(mu), LS), _t(noises[1]))
    xq = torch.cat([s_n, nm(pi, nrm.a_mean, nrm.a_den)], 1)
    minq = torch.minimum(_net(Q[0], xq, act, "rows"), _net(Q[1], xq, act, "rows"))
    alpha = float(st0.alpha)
    p = torch.mean(-alpha * nlp[:, None] - minq)
    if use_expert:
        M = [[_t(w) for w in net] for net in st0.models]
        sq = []
        for k, (se, spe, ne) in enumerate([(ex.s1, ex.sp1, ex.noise1), (ex.s2, ex.sp2, ex.noise2)]):
            se_n = nm(_t(se), nrm.s_mean, nrm.s_den)
            mue = actor(se_n)
            ca = torch.tanh(mue + torch.exp(torch.clamp(_ColSum.apply(torch.zeros_like(mue), LS), -5, 2)) * _t(ne))
            om = _net(M[k], torch.cat([se_n, nm(ca, nrm.a_mean, nrm.a_den)], 1), cfg.model_act, "gemm")
            sp_hat = _t(se) + (om[:, :S] * _t(nrm.d_den) + _t(nrm.d_mean))
            sq.append(((_t(spe) - sp_hat) ** 2).sum(-1))
        p = (1 - ex.epsilon) * p + ex.epsilon * torch.mean(0.5 * (sq[0] + sq[1]))
    g = torch.autograd.grad(p, PA + [LS])
    for i, (gg, mine) in enumerate(zip(g[:-1], keep["actor_grads"])):
        np.testing.assert_allclose(mine, gg.numpy(), rtol=1e-7, atol=1e-10, err_msg=str(i))
    np.testing.assert_allclose(keep["g_logstd"][0], g[-1].numpy(), rtol=1e-7, atol=1e-10)


def test_unit_deltas_equal_scaled_ones():
    """The fused plan's form (the per-row loss gradient g apart from the dX chain, on the dW operand): the
    same gradients as the scaled form bit for bit when every g is a power of two (rounding commutes with
    the scale), and within two bf16 roundings of a sum's terms otherwise."""
    rs = np.random.RandomState(3)
    params = [rs.normal(size=s) * 0.3 for s in ((7, 24), (24,), (24, 20), (20,), (20, 1), (1,))]
    x = rs.normal(size=(33, 7))
    with P.oracle_mode("bf16"):
        out, hs = O.mlp_forward(params, x, "tanh", rows_head=True)
        for pow2 in (True, False):
            g = rs.normal(size=33)
            if pow2:
                g = np.sign(g) * 2.0 ** np.round(np.log2(np.abs(g)))
            unit, dxu = O.mlp_backward(params, x, hs, np.ones((33, 1)), "tanh", need_dx=True, rows_head=True, row_scale=g)
            scaled, dxs = O.mlp_backward(params, x, hs, g[:, None], "tanh", need_dx=True, rows_head=True)
            for a, b in zip(unit + [dxu * g[:, None]], scaled + [dxs]):
                if pow2:
                    assert np.array_equal(a, b)
                else:
                    assert not np.array_equal(unit[0], scaled[0])
                    assert np.max(np.abs(a - b)) <= 2.0 ** -7 * np.max(np.abs(b))
    # and in the exact mode sac_update does not take the unit form at all (its arithmetic stays as it was)
    assert O.GEMM_OPERANDS == "exact"


# ----------------------------------------------------------------- envelope and sensitivity
@pytest.mark.parametrize("name", list(P.CASES))
def test_envelope(name):
    """The reference alone meets the bars: the three fp32 executions of the rounding oracle pass the
    device test's comparison, with no stage element beyond its bar where one is allowed and at most half
    the cap elsewhere; no bar above BAR_CAP x the fp32 path's."""
    ref, loose = P.reference(name)
    bars, env = P.bars(name), P.envelope(name)
    for k, b in bars.items():
        print(f"{name} {k}: envelope {env[k]:.2e} bar {b:.2e}")
        assert b <= P.BAR_CAP * P.FP32_BARS[P.kind(k)], (k, b)
        assert b == max(P.FP32_BARS[P.kind(k)], P.ENVELOPE_FACTOR * env[k])
    for order in O.MATMUL_ORDERS:
        rep = P.compare(P.oracle_run(name, np.float32, order)[0], ref, bars, loose)
        for k, (e, b, beyond) in rep.items():
            assert beyond <= P.flip_cap(ref[k].size) // 2, (order, k, beyond)


def test_trajectory_envelope():
    """hc over 30 updates: Q1 / Q2 of the fp32 executions within 3.8e-5 of the fp64 one (measured), so the
    device's bar (4 x: 1.5e-4) is a thirtieth of the 5e-3 the exact-oracle trajectory tests allow."""
    ref, env = P.trajectory_envelope("hc", 30)
    print(f"hc trajectory envelope {env:.2e}")
    assert np.all(np.isfinite(ref)) and ref.shape == (30, 2)
    assert 0 < P.ENVELOPE_FACTOR * env < 5e-3 / 10, env


@pytest.mark.parametrize("name", list(P.CASES))
@pytest.mark.parametrize("wrong", ["exact", "truncated", "exact_dw"])
def test_bars_catch_a_wrong_kernel(name, wrong):
    """(a) no operand rounding at all, (b) truncation in place of RNE, (c) rounding left out of the dW GEMMs
    only: each misses the device test's bars against the RNE oracle."""
    kw = {"exact": dict(operands="exact"), "truncated": dict(_trunc_operands=True), "exact_dw": dict(_exact_dw=True)}[wrong]
    ref, loose = P.reference(name)
    got = P.oracle_run(name, np.float64, "default", **kw)[0]
    with pytest.raises(AssertionError) as e:
        P.compare(got, ref, P.bars(name), loose)
    missed = [m[0] for m in e.value.args[0]]
    assert any(k.startswith("grad.") for k in missed), missed
    if wrong == "exact":            # and a NaN in one element of a stage is refused, not left out as a flip
        bad = dict(ref, Ha1=ref["Ha1"].copy())
        bad["Ha1"][0, 0] = np.nan
        with pytest.raises(AssertionError) as e:
            P.compare(bad, ref, P.bars(name), loose)
        assert ("Ha1", "not finite") in e.value.args[0]
    if wrong != "exact_dw":
        assert "Ha1" in missed and "Hq2" in missed, missed


@pytest.mark.parametrize("which", ["fit", "obj", "roll"])
def test_other_plans_envelope_and_sensitivity(which):
    """The world-model fit (first-step gradients, three losses), the object calls on 64 rows and one
    rollout step: the fp32 executions of the rounding oracle meet the device test's bars through the
    device test's comparison -- the object calls with no element left out, the rollout with no element
    beyond a bar (half its cap of one) and every element within the loose bound -- no bar above 10 x the
    fp32 path's, and the exact oracle misses them; so does a NaN in one element."""
    run = {"fit": lambda *a: (P.fit_oracle(*a),), "obj": P.obj_oracle, "roll": P.roll_oracle}[which]
    ref, env, bars, fp32 = P.plan_envelope(which)
    for k in ref:
        print(f"{which} {k}: envelope {env[k]:.2e} bar {bars[k]:.2e}")
        assert bars[k] <= P.BAR_CAP * fp32[k], (k, bars[k])
    for order in O.MATMUL_ORDERS:
        rep = P.plan_compare(which, run(np.float32, order)[0], ref, bars)
        assert all(beyond == 0 for _, beyond in rep.values()), (order, rep)
    with pytest.raises(AssertionError):
        P.plan_compare(which, run(np.float64, "default", "exact")[0], ref, bars)
    bad = {k: np.array(v, np.float64) for k, v in ref.items()}
    k0 = sorted(bad)[0]
    bad[k0].reshape(-1)[0] = np.nan
    with pytest.raises(AssertionError):
        P.plan_compare(which, bad, ref, bars)
