"""Shared by tests/test_oracle_bf16.py (CPU) and tests/test_gpu_bf16.py (device): the cases of the
bf16 stage-level parity check, the operand-rounding oracle runs they compare against, the envelope
of the fp32 executions of that oracle, the bars made from it, and the one comparison both call.

The reference of every case is sac_oracle with GEMM_OPERANDS = "bf16" in fp64 (DESIGN.md section
6.6: the rounding contract).  The bars come from the oracle alone:

    bar(quantity) = max(the fp32 path's bar, ENVELOPE_FACTOR x envelope(quantity))

where the envelope is the largest distance of the same oracle run in fp32 under each of
sac_oracle.MATMUL_ORDERS from the fp64 run.  The device is a fourth summation order that the three
only sample, hence the factor 4.  No bar may exceed BAR_CAP x the fp32 path's (test_envelope).

Rounding flips.  A value within fp32 rounding of the reference can still round to the other
neighbouring bf16 when it is next loaded as an operand, which moves one term of one row's sum by one
bf16 spacing.  The element-wise stage comparisons therefore have two tiers: at most
max(1, FLIP_SHARE x elements) elements of an array beyond the tight bar, and every element within
the loose bound of `loose_bounds` (2^-8 x the row's largest term, carried through the layers).
"""
import contextlib
import functools

import numpy as np

import sac_oracle as O
from helpers import B1, make_learner, net_grads, oracle_step

ENVELOPE_FACTOR = 4.0
BAR_CAP = 10.0
FLIP_SHARE = 1e-4
NE = 20                      # expert rows of the SAC-EO cases

# the fp32 path's bars (tests/test_gpu_engine.py::_one_step_compare)
FP32_BARS = dict(Xa=1e-6, stage=2e-5, loss=2e-5, alpha=1e-6, grad=2e-4, target=1e-5)
STAGES = ("Ha1", "Ha2", "Hq2", "nlp_t", "nlp_p")
LOSSES = ("q1_loss", "q2_loss", "p_loss", "alpha_loss", "mse_loss")

# make_learner's arguments per case (+ "unit": the fused plan's unit critic deltas,
# sac_oracle.BF16_UNIT_DELTAS; "env": the plan variables of the device run).  N is kept small: the
# replay rows only feed the gather.
CASES = {
    "odd": dict(S=3, A=1, B=37, hidden=(40, 40), act="tanh", seed=7, N=600),
    "narrow": dict(S=17, A=6, B=37, hidden=(100, 60), act="elu", seed=9, N=600),
    "hc": dict(S=17, A=6, B=128, hidden=(256, 256), act="relu", seed=5, N=2000, use_expert=True, ne=NE,
               normalizers="random"),
    "pss_ln": dict(S=17, A=6, B=64, hidden=(64, 48), act="relu", seed=23, N=600, per_state_std=True, layer_norm=True),
    "generic": dict(S=17, A=6, B=64, hidden=(520, 64), act="relu", seed=31, N=600),
    "wide_k0": dict(S=376, A=17, B=64, hidden=(64, 64), act="relu", seed=42, N=300),
    # widths off the 4-grid: element-wise operand loads, a half-filled last bf16 pair (tests/test_gpu_ragged.py)
    "off4_bf16": dict(S=17, A=6, B=37, hidden=(63, 65), act="elu", seed=9, N=600),
}
UNIT_DELTAS = {"generic": False}           # every other case takes the fused plan
DONE_P = 0.05


def learner(name):
    return make_learner(done_p=DONE_P, **CASES[name])


def randoms(name, buf, A, steps=1):
    c = CASES[name]
    rs = np.random.RandomState(c["seed"] + 5)
    gen = np.random.default_rng(c["seed"] + 6)
    state0 = rs.get_state()
    Rs = [O.draw_step_randoms(rs, buf["r"].shape[0], c["B"], A, n_expert=NE if c.get("use_expert") else 0, gen=gen)
          for _ in range(steps)]
    return state0, Rs, rs


def _trunc(x):
    """bf16 by truncation (what a conversion that drops the low half would give): the sensitivity test's."""
    a = np.asarray(x)
    f = np.ascontiguousarray(a, dtype=np.float32)
    return (f.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(a.dtype).reshape(a.shape)


@contextlib.contextmanager
def oracle_mode(operands="bf16", order="default", unit=True, _trunc_operands=False, _exact_dw=False):
    saved = (O.GEMM_OPERANDS, O.MATMUL_ORDER, O.BF16_UNIT_DELTAS, O.bf16_rne, O._rb_dw)
    O.GEMM_OPERANDS, O.MATMUL_ORDER, O.BF16_UNIT_DELTAS = operands, order, unit
    if _trunc_operands:
        O.bf16_rne = _trunc
    if _exact_dw:
        O._rb_dw = lambda x: x
    try:
        yield
    finally:
        O.GEMM_OPERANDS, O.MATMUL_ORDER, O.BF16_UNIT_DELTAS, O.bf16_rne, O._rb_dw = saved


def quantities(keep, stats, st, B):
    """The compared quantities of one update, by name."""
    q = {"Xa": keep["sp_n"], "Ha1": keep["actor_h_t"][0], "Ha2": keep["actor_h_p"][1], "Hq2": keep["q0_h"][1],
         "nlp_t": keep["nlp_t"], "nlp_p": keep["nlp_p"], "alpha": stats["alpha"]}
    for k in LOSSES:
        if k in stats:
            q[k] = stats[k]
    for k in range(2):
        for i, g in enumerate(keep[f"q{k}_grads"]):
            q[f"grad.q{k}.{i}"] = g
        for i, w in enumerate(st.q_targ[k]):
            q[f"target.t{k}.{i}"] = w
    for i, g in enumerate(keep["actor_grads"]):
        q[f"grad.actor.{i}"] = g
    if "g_logstd" in keep and np.any(keep["g_logstd"]):
        q["grad.logstd"] = keep["g_logstd"][0]
    return {k: np.asarray(v, np.float64) for k, v in q.items()}


def oracle_run(name, dtype=np.float64, order="default", operands="bf16", **private):
    """One update of the case under the given oracle mode: (quantities, keep, oracle cfg, post-update state)."""
    ocfg, st, buf, nrm, expert = learner(name)
    st = st.astype(dtype)
    _, Rs, _ = randoms(name, buf, ocfg.A)
    keep = {}
    with oracle_mode(operands, order, UNIT_DELTAS.get(name, True), **private):
        stats = oracle_step(st, ocfg, nrm, buf, Rs[0], expert, keep)
    return quantities(keep, stats, st, ocfg.B), keep, ocfg, st


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 rounding oracle's update of the case, computed once per process and left unchanged."""
    q, keep, ocfg, st = oracle_run(name)
    return q, loose_bounds(name, keep, ocfg)


def kind(key):
    return ("Xa" if key == "Xa" else "stage" if key in STAGES else "loss" if key in LOSSES else
            "alpha" if key == "alpha" else "grad" if key.startswith("grad.") else "target")


def flip_cap(n):
    return max(1, int(FLIP_SHARE * n))


def error(key, got, ref):
    """The figure the bar of `key` bounds.  Arrays: max |got - ref| / max |ref| (targets: absolute); a
    stage leaves out its flip_cap largest elements (the second tier bounds those)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    k = kind(key)
    if k in ("loss", "alpha"):
        return float(abs(got - ref) / max(abs(ref), 1e-30))
    e = np.abs(got - ref).ravel()
    if k == "target":
        return float(e.max())
    scale = max(float(np.max(np.abs(ref))), 1e-30)
    if k == "stage":
        e = np.sort(e)[:e.size - flip_cap(e.size)]
    return float(e.max() / scale)


@functools.lru_cache(maxsize=None)
def envelope(name):
    """Per quantity, the largest error of the fp32 rounding oracle under MATMUL_ORDERS against the fp64 one."""
    ref = reference(name)[0]
    env = {k: 0.0 for k in ref}
    for order in O.MATMUL_ORDERS:
        got = oracle_run(name, np.float32, order)[0]
        for k in ref:
            env[k] = max(env[k], error(k, got[k], ref[k]))
    return env


def bars(name):
    return {k: max(FP32_BARS[kind(k)], ENVELOPE_FACTOR * e) for k, e in envelope(name).items()}


def _terms(X, W):
    """Per row of X, the largest |x_ik w_kj| over k, j of the product X W."""
    return np.max(np.abs(X) * np.max(np.abs(W), axis=1)[None, :], axis=1)


def _chain(X, hs, Ws, prev=None, ln=None):
    """lb_l[i] = 2^-8 T_l[i] + lb_{l-1}[i] max |W_l| over the GEMM layers Ws on the rows X (hs: the hidden
    activations feeding layers 1, 2, ...); `prev`: the bound on a moved input element."""
    lb, prev = [], np.zeros(X.shape[0]) if prev is None else prev
    for l, (inp, w) in enumerate(zip([X] + list(hs), Ws)):
        cur = 2.0 ** -8 * _terms(inp, w) + prev * np.max(np.abs(w))
        if l == 0 and ln is not None:
            cur = cur * 2.0 * np.max(np.abs(ln[0])) * ln[1][:, 0]
        lb.append(cur)
        prev = cur
    return lb


def loose_bounds(name, keep, ocfg):
    """The second tier, per row of each stage: one operand element of the row moved to the neighbouring
    bf16 changes one term of the row's sums by at most 2^-8 of it (the issue's figure for a flip), so an
    output of the layer moves by at most 2^-8 x the row's largest term T_l (relu, tanh and elu are
    1-Lipschitz), and by at most lb_{l-1} x max |W_l| for a moved element of the layer below:
        lb_l[i] = 2^-8 T_l[i] + lb_{l-1}[i] max |W_l|,   lb_{-1} = 0.
    Layer norm (pss_ln): z -> tanh(gamma xhat + beta) moves by at most 2 max |gamma| rstd_i per unit of
    one z element (the element itself and the row's mean / variance).  neglogp: the output layer runs in
    fp32, so output j of row i moves by at most lb_1[i] m_j, m_j = max_k |W3[k, j]|; d nlp / d mu_j =
    -2 tanh x_j (at most 2) and, with a per-state std, d nlp / d logstd_j = 1 - 2 tanh(x_j) std_ij u_ij (at
    most 1 + 2 std_ij |u_ij|, the row's own std and noise), so
        lb_nlp[i] = lb_1[i] (2 sum_j m_j + sum_j (1 + 2 std_ij |u_ij|) m_{A + j})."""
    c = CASES[name]
    W = ocfg_weights(name)
    out = {}
    Bn, A = c["B"], ocfg.A
    aW = W["actor"]
    ln_t = ln_p = None
    if c.get("layer_norm"):
        ln_t = (W["gamma"], keep["actor_h_t"][-1])
        ln_p = (W["gamma"], keep["actor_h_p"][-1][:Bn])
    lt = _chain(keep["sp_n"], keep["actor_h_t"][:1], aW[:2], ln=ln_t)
    lp = _chain(keep["s_n"], [keep["actor_h_p"][0][:Bn]], aW[:2], ln=ln_p)
    lq = _chain(keep["xq"], keep["q0_h"][:1], W["q0"])
    out["Ha1"], out["Ha2"], out["Hq2"] = lt[0], lp[1], lq[1]
    m3 = np.max(np.abs(aW[2]), axis=0)
    noise = np.abs(keep["noise"]).reshape(2, Bn, A)
    for key, lb1, ls, u in (("nlp_t", lt[1], keep["ls_t"], noise[0]), ("nlp_p", lp[1], keep["ls_p"], noise[1])):
        f = 2.0 * np.sum(m3[:A]) * np.ones(Bn)
        if c.get("per_state_std"):
            std = np.exp(np.clip(np.asarray(ls, np.float64), O.LOG_STD_MIN, O.LOG_STD_MAX))
            f = f + ((1.0 + 2.0 * std * u) * m3[A:][None, :]).sum(axis=1)
        out[key] = f * lb1
    return out


def ocfg_weights(name):
    """The pre-update weight matrices the loose bounds need."""
    ocfg, st, *_ = learner(name)
    a = st.actor
    Wa = [a[0], a[4], a[6]] if ocfg.layer_norm else [a[0], a[2], a[4]]
    return {"actor": [w.astype(np.float64) for w in Wa], "gamma": a[2].astype(np.float64) if ocfg.layer_norm else None,
            "q0": [st.q[0][0].astype(np.float64), st.q[0][2].astype(np.float64)]}


def _tiers(k, g, r, bar_k, lb, miss):
    """The two tiers of an element-wise comparison: the elements beyond the bar counted against flip_cap,
    every element within bar + its row's loose bound.  Returns the count."""
    scale = max(float(np.max(np.abs(r))), 1e-30)
    d = np.abs(g - r)
    beyond = int(np.sum(d > bar_k * scale))
    if beyond > flip_cap(r.size):
        miss.append((k, "elements beyond the bar", beyond, flip_cap(r.size)))
    if lb is not None:
        lim = np.asarray(lb, np.float64).reshape((-1,) + (1,) * (r.ndim - 1)) + bar_k * scale
        if np.any(d > lim):
            miss.append((k, "beyond the loose bound", float(np.max(d / lim))))
    return beyond


def compare(got, ref, bar, loose=None):
    """The check of the device test, and of the sensitivity test on the oracle's wrong variants: every
    quantity of `ref` finite and within its bar; a stage's elements beyond the bar at most flip_cap and all
    of them within bar + the loose bound.  Returns {key: (error, bar, elements beyond the bar)}; raises
    AssertionError naming every quantity that misses."""
    report, miss = {}, []
    for k, r in ref.items():
        g = np.asarray(got[k], np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if not np.all(np.isfinite(g)):
            miss.append((k, "not finite"))
            report[k] = (float("nan"), bar[k], 0)
            continue
        e = error(k, g, r)
        beyond = _tiers(k, g, r, bar[k], None if loose is None else loose[k], miss) if kind(k) == "stage" else 0
        tol = 1e-7 / max(abs(float(r)), 1e-30) if kind(k) == "loss" else 0.0      # the fp32 test's absolute term
        if not e <= bar[k] + tol:
            miss.append((k, e, bar[k]))
        report[k] = (e, bar[k], beyond)
    assert not miss, miss
    return report


def oracle_trajectory(name, steps, dtype=np.float64, order="default"):
    """Q1 / Q2 losses over `steps` updates of the case under the rounding oracle."""
    ocfg, st, buf, nrm, expert = learner(name)
    st = st.astype(dtype)
    _, Rs, _ = randoms(name, buf, ocfg.A, steps)
    out = []
    with oracle_mode("bf16", order, UNIT_DELTAS.get(name, True)):
        for R in Rs:
            o = oracle_step(st, ocfg, nrm, buf, R, expert)
            out.append([o["q1_loss"], o["q2_loss"]])
    return np.array(out)


@functools.lru_cache(maxsize=None)
def trajectory_envelope(name, steps):
    """(the fp64 rounding oracle's Q-loss trajectory, the largest relative error of its fp32 executions)."""
    ref = oracle_trajectory(name, steps)
    env = max(float(np.max(np.abs(oracle_trajectory(name, steps, np.float32, o) - ref) / np.abs(ref)))
              for o in O.MATMUL_ORDERS)
    return ref, env


def device_quantities(eng, ocfg):
    """The same quantities read from an engine after one eager update (the views and the Adam first
    moments tests/test_gpu_engine.py::_one_step_compare reads)."""
    B, S, A = ocfg.B, ocfg.S, ocfg.A
    v = eng.v
    f = lambda t: t.cpu().numpy().astype(np.float64)
    q = {"Xa": f(v["slot0.Xa"])[:B, :S], "Ha1": f(v["ws.Ha1"])[:B], "Ha2": f(v["ws.Ha2"])[B:2 * B],
         "Hq2": f(v["ws.Hq2"])[2 * B:3 * B], "nlp_t": f(v["ws.nlp_t"])[0], "nlp_p": f(v["ws.nlp_p"])[0]}
    row = eng.stats(1)[0]
    for i, k in enumerate(("q1_loss", "q2_loss", "p_loss", "alpha_loss", "alpha")):
        q[k] = np.float64(row[i])
    if eng.cfg.use_expert:
        q["mse_loss"] = np.float64(row[5])
    m = f(v["adam_m"][0])

    def moment(seg_name, rows=None):
        seg = eng.segments[seg_name]
        off = seg["offset"] // 4
        n = seg["rows"] * seg["cols"] if rows is None else rows * seg["cols"]
        return m[off: off + n].reshape(-1, seg["cols"]) / np.float64(B1)

    for net in ("q0", "q1", "actor"):           # the fp32 test's reader (helpers.net_grads)
        g = net_grads(eng, net)
        if net == "actor" and ocfg.layer_norm:  # gamma / beta behind b0, the oracle's order
            gb = moment("actor.ln", 2)
            g = g[:2] + [gb[0], gb[1]] + g[2:]
        for i, w in enumerate(g):
            q[f"grad.{net}.{i}"] = np.asarray(w, np.float64)
    if not ocfg.per_state_std:
        seg = eng.segments["actor.logstd"]
        q["grad.logstd"] = m[seg["offset"] // 4: seg["offset"] // 4 + A] / np.float64(B1)
    for k in range(2):
        for i, w in enumerate(eng.get_net(f"t{k}")):
            q[f"target.t{k}.{i}"] = np.asarray(w, np.float64)
    return q


# ------------------------------------------------------------------ the other plans of a gemm_bf16 handle
# Which of them run bf16 GEMMs: model_fit (every layer, forward, dX and dW),
# evaluate / act above ACT_ROWS_MAX rows / rollout (the actor's hidden layers; the head is a row kernel),
# critic_forward (every layer: its head is a GEMM problem), model_forward / rollout (every layer of the
# model).  act on at most 16 rows of a two-layer actor runs k_act_rows: fp32 throughout.
FIT = dict(act="relu", B=64, seed=31, N=800, use_expert=True, normalizers="random")
FIT_STEPS, FIT_MB = 3, 200
FIT_BARS = dict(loss=1e-4, grad=2e-4)        # tests/test_gpu_engine.py: test_model_fit_matches_oracle, _one_step_compare
OBJ = dict(act="tanh", hidden=(64, 48), B=64, seed=41, N=600, normalizers="random", use_expert=True, ne=12,
           model_hidden=(96, 80))
OBJ_ROWS = 64
OBJ_BAR = 2e-5                              # tests/test_gpu_depth.py::test_objects_any_depth
# one model step: at two the fp32 executions of the oracle are themselves 4e-4 apart in the actions (a
# flipped operand of step 0 moves step 1's whole row), 16 x what a bar may be
# (stream 24: the first seed after test_rollout_matches_oracle's 23 at which none of the oracle's fp32
# executions meets a flip -- at 23 one moves a reward by 4e-4)
ROLL = dict(n=37, horizon=1, model=1, stream=24)
ROLL_BAR = 1e-4                             # tests/test_gpu_engine.py::test_rollout_matches_oracle


def relmax(got, ref, discard=0):
    e = np.sort(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).ravel())
    return float(e[:e.size - discard].max() / max(float(np.max(np.abs(ref))), 1e-30))


def fit_indices(N):
    return np.random.RandomState(9).randint(N, size=(FIT_STEPS, 2, FIT_MB))


def fit_oracle(dtype=np.float64, order="default", operands="bf16"):
    """{"loss": [steps], "grad.m<k>.<i>": the first step's gradients (Adam's first moment / (1 - beta_1))}
    of the world-model fit.  The weights after the steps are no check of a bf16 kernel: Adam's m / sqrt(v)
    turns a flip-sized difference in a near-zero gradient element into an lr-sized step, and the fp32
    executions of the oracle end 1.5e-3 apart (30 x the fp32 path's 5e-5) after three steps."""
    ocfg, st, buf, nrm, _ = make_learner(**FIT)
    st = st.astype(dtype)
    idx = fit_indices(buf["r"].shape[0])
    loss, out = [], {}
    with oracle_mode(operands, order):
        for j in range(FIT_STEPS):
            loss.append(O.model_fit_step(st, ocfg, nrm, [(buf["s"][idx[j, k]], buf["a"][idx[j, k]], buf["sp"][idx[j, k]],
                                                          buf["r"][idx[j, k]]) for k in range(2)]))
            if j == 0:
                b1 = dtype(1) - dtype(0.9)
                n = len(st.models[0])
                for k in range(2):
                    for i in range(n):
                        out[f"grad.m{k}.{i}"] = np.asarray(st.opt_model.m[k * n + i] / b1, np.float64)
    out["loss"] = np.array(loss)
    return out


def fit_error(key, got, ref):
    if key == "loss":
        return float(np.max(np.abs(got - ref) / np.abs(ref)))
    return relmax(got, ref)


def obj_rows():
    r = np.random.RandomState(1)
    S, A = 17, 6
    s = (r.normal(size=(OBJ_ROWS, S)) * 1.5).astype(np.float32)
    return s, r.uniform(-1, 1, (OBJ_ROWS, A)).astype(np.float32)


def obj_oracle(dtype=np.float64, order="default", operands="bf16"):
    """The object calls' outputs on OBJ_ROWS rows, the draws in the device test's order; returns (outputs,
    the stream after them)."""
    ocfg, st, buf, nrm, _ = make_learner(**OBJ)
    st = st.astype(dtype)
    s, a = obj_rows()
    rs = np.random.RandomState(19)
    out = {}
    with oracle_mode(operands, order):
        out["evaluate.pi"], out["evaluate.nlp"] = O.actor_evaluate(st, ocfg, nrm, s, rs)
        out["act"] = O._actor_sample(st, ocfg, nrm.cast(dtype), s.astype(dtype), rs)
        for net, params in (("q0", st.q[0]), ("t1", st.q_targ[1])):
            out[f"critic.{net}"] = O.critic_forward(params, ocfg, nrm, s, a)
            out[f"value.{net}"] = O.critic_forward(params, ocfg, nrm, s, a, value=True)
        for k in range(2):
            out[f"model{k}.pred"], out[f"model{k}.sp"], out[f"model{k}.r"] = O.model_forward(st, ocfg, nrm, k, s, a)
    return {k: np.asarray(v, np.float64) for k, v in out.items()}, rs


def roll_oracle(dtype=np.float64, order="default", operands="bf16"):
    ocfg, st, buf, nrm, _ = make_learner(**OBJ)
    st = st.astype(dtype)
    s0 = (np.random.RandomState(5).normal(size=(ROLL["n"], ocfg.S)) * 1.5).astype(np.float32)
    rs = np.random.RandomState(ROLL["stream"])
    with oracle_mode(operands, order):
        ref = O.rollout(st, ocfg, nrm, s0, ROLL["horizon"], ROLL["model"], rs, False)
    return {k: np.asarray(v, np.float64) for k, v in zip(("s", "a", "r", "sp"), ref[:4])}, rs, s0


@functools.lru_cache(maxsize=None)
def roll_loose():
    """The second tier of the one-step rollout, per row, as loose_bounds carries it through the stages: lb_1
    of the actor's two hidden GEMMs; its fp32 head and the 1-Lipschitz tanh give |d a| <= lim lb_1 max |W3|,
    the model's input |d a| / min a_den; then lb through the model's three GEMM layers from that input
    bound; sp = s + d_den dn + d_mean and r = r_den rn + r_mean scale it by max d_den and r_den.  s is the
    caller's rows: no bound."""
    ocfg, st, buf, nrm, _ = make_learner(**OBJ)
    st, nrm = st.astype(np.float64), nrm.cast(np.float64)
    s0 = roll_oracle()[2].astype(np.float64)
    rs = np.random.RandomState(ROLL["stream"])
    with oracle_mode("bf16"):
        x = O._norm(s0, nrm.s_mean, nrm.s_den)
        o, hs = O.actor_forward(st.actor, x, ocfg)
        a = O.head_sample(*O.split_head(o, st.logstd, ocfg), O.f32_noise(rs.normal(size=o.shape)), ocfg.act_limit,
                          np.float64)[0]
        xm = np.concatenate([x, O._norm(a, nrm.a_mean, nrm.a_den)], 1)
        _, mhs = O.mlp_forward(st.models[ROLL["model"]], xm, ocfg.model_act)
    lb1 = _chain(x, hs[:1], st.actor[0:4:2])[1]
    da = ocfg.act_limit * lb1 * np.max(np.abs(st.actor[4]))
    lm = _chain(xm, mhs, st.models[ROLL["model"]][0::2], prev=da / np.min(nrm.a_den))[-1]
    return {"s": np.zeros(ROLL["n"]), "a": da, "sp": lm * np.max(nrm.d_den), "r": lm * float(nrm.r_den)}


@functools.lru_cache(maxsize=None)
def plan_envelope(which):
    """(the fp64 rounding oracle's outputs, their envelope over the fp32 executions, the bars, the fp32
    path's bars) of "fit", "obj" or "roll"."""
    run = {"fit": lambda *a: (fit_oracle(*a),), "obj": obj_oracle, "roll": roll_oracle}[which]
    ref = run()[0]
    err = plan_error(which)
    env = {k: 0.0 for k in ref}
    for order in O.MATMUL_ORDERS:
        got = run(np.float32, order)[0]
        for k in ref:
            env[k] = max(env[k], err(k, got[k], ref[k]))
    fp32 = (lambda k: FIT_BARS["loss" if k == "loss" else "grad"]) if which == "fit" else \
        (lambda k: OBJ_BAR if which == "obj" else ROLL_BAR)
    return ref, env, {k: max(fp32(k), ENVELOPE_FACTOR * env[k]) for k in ref}, {k: fp32(k) for k in ref}


def plan_error(which):
    """The figure a bar bounds: fit's as fit_error; an object call's the plain max-norm error (nothing left
    out); the rollout's, as a stage's, without its flip_cap largest elements (plan_compare counts and
    bounds those)."""
    if which == "fit":
        return fit_error
    if which == "obj":
        return lambda k, got, ref: relmax(got, ref)
    return lambda k, got, ref: relmax(got, ref, flip_cap(np.asarray(ref).size))


def plan_compare(which, got, ref, bars):
    """Every output finite and within its bar; the rollout's outputs with the stages' two tiers (at most
    flip_cap elements beyond the bar, every element within bar + roll_loose's bound).  Raises
    AssertionError naming the outputs that miss; returns {key: (error, elements beyond the bar)}."""
    err, rep, miss = plan_error(which), {}, []
    for k, r in ref.items():
        r = np.asarray(r, np.float64)
        g = np.asarray(got[k], np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if not np.all(np.isfinite(g)):
            miss.append((k, "not finite"))
            rep[k] = (float("nan"), 0)
            continue
        e = err(k, g, r)
        beyond = _tiers(k, g, r, bars[k], roll_loose()[k], miss) if which == "roll" else 0
        if not e <= bars[k]:
            miss.append((k, e, bars[k]))
        rep[k] = (e, beyond)
    assert not miss, miss
    return rep
