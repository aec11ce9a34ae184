"""Config C5 (gemm_bf16) against the operand-rounding oracle, stage by stage (-m gpu).

One eager update of a gemm_bf16 engine against sac_oracle with GEMM_OPERANDS = "bf16" in fp64 (the
rounding contract of DESIGN.md section 6.6) at the stages tests/test_gpu_engine.py::_one_step_compare
checks on the fp32 path: the sampler and the stream bit-exact; slot0.Xa, ws.Ha1, ws.Ha2, ws.Hq2,
ws.nlp_t, ws.nlp_p; the losses (SAC-EO: the MSE term too) and alpha; every critic, actor and logstd
gradient through adam_m / (1 - beta_1); the Polyak targets.  The cases, the bars (max(the fp32 path's,
4 x the CPU envelope), none above 10 x the fp32 path's), the two tiers of the element-wise comparisons
and the comparison itself are tests/bf16_parity.py's; tests/test_oracle_bf16.py shows on the CPU that
the oracle's own fp32 executions meet these bars and that the exact oracle, truncated operands and an
unrounded dW GEMM each miss them.

k slabs: a GEMM's reduction runs in 16-wide slabs, two per v_mfma_f32_16x16x32_bf16; an odd count
leaves a half-filled pair, K % 16 != 0 a ragged last slab.  Slab counts below are ceil(K / 16) as
forward layer 0 / layer 1 (actor; critics), dX (layer 1's, K = its output width), dW (K = the rows
reduced).
"""
import numpy as np
import pytest

import bf16_parity as P
import sac_oracle as O
from helpers import make_pair

pytestmark = pytest.mark.gpu


def _noise(R):
    parts = [R["noise_t"], R["noise_pi"]]
    if "noise_e1" in R:
        parts += [R["noise_e1"]] + ([R["noise_e2"]] if R["noise_e2"] is not None else [])
    parts.append(R["noise_alpha"])
    return np.concatenate([p.ravel() for p in parts]).astype(np.float32)


def _one_update(name, monkeypatch, env=None, expect=(), absent=(), views=()):
    for k, v in (env or {}).items():            # plan variables: before the engine is built
        monkeypatch.setenv(k, v)
    c = P.CASES[name]
    eng, ocfg, st, buf, nrm, expert = make_pair(done_p=P.DONE_P, gemm_bf16=True, **c)
    state0, Rs, rs = P.randoms(name, buf, ocfg.A)
    eng.rng_set_state(state0)
    if expert is not None:
        eng.push_perms(Rs[0]["perm"][None, :])
    eng.step(1, eager=True)
    eng.sync()
    plan = eng.plan_info()
    names = [L["name"] for L in plan]
    print(name, "launches:", [(L["name"], L["kernel"]) for L in plan])
    got = P.device_quantities(eng, ocfg)
    idx = eng.v["slot0.idx"][0].cpu().numpy()
    noise = eng.v["slot0.noise"][0].cpu().numpy()
    stream = eng.rng_get_state()
    have = set(eng.v)
    eng.close()
    for n in views:                             # the shadows / images the plan variables ask for exist
        assert n in have, (n, sorted(have))
    for n in expect:
        assert n in names, (n, names)
    for n in absent:
        assert n not in names, (n, names)
    # the sampler and the stream: bit-exact
    assert np.array_equal(idx, Rs[0]["idx"])
    assert np.array_equal(noise[:_noise(Rs[0]).size], _noise(Rs[0]))
    exp = rs.get_state()
    assert np.array_equal(stream[1], exp[1]) and stream[2] == exp[2] and stream[3] == exp[3] and stream[4] == exp[4]
    ref, loose = P.reference(name)
    bars, env = P.bars(name), P.envelope(name)
    for k in ref:                               # each figure before the assertion
        print(f"{name} {k}: device {P.error(k, got[k], ref[k]):.2e} bar {bars[k]:.2e} envelope {env[k]:.2e}")
    return P.compare(got, ref, bars, loose), plan


def test_bf16_update_odd(gpu_available, monkeypatch):
    """S=3, A=1, B=37, hidden (40, 40), tanh.  The fused plan on 16x16 tiles (q.head+critic.bwd1, unit
    critic deltas) with actor.head and actor.head.bwd as launches of their own (H1 % 16 != 0; hc and
    pss_ln reach the head folded into q.fwd0).
    Slabs: forward 1 (K = 3 and 4: ragged, a lone slab in its pair) / 3 (K = 40: odd, ragged); dX 3;
    dW 3 (37 rows: odd, ragged)."""
    _one_update("odd", monkeypatch, expect=("actor.head", "q.head+critic.bwd1", "critic.adam", "actor.head.bwd"))


def test_bf16_update_narrow(gpu_available, monkeypatch):
    """S=17, A=6, B=37, hidden (100, 60), elu: widths that are multiples of 4 but not of 16 (ragged k slabs;
    off the 4-grid, where the operands load scalar by scalar, is tests/test_gpu_ragged.py's off4_bf16), and
    H1 % 16 != 0, so the head keeps its own launch (actor.head, actor.head.bwd).
    Slabs: forward 2 (K = 17, 23: even, ragged) / 7 (K = 100: odd, ragged); dX 4 (K = 60: even,
    ragged); dW 3 (37 rows)."""
    _one_update("narrow", monkeypatch, expect=("actor.head", "actor.head.bwd", "actor.bwd1", "critic.adam"),
                absent=("q.fwd0+actor.head",))


def test_bf16_update_hc(gpu_available, monkeypatch):
    """The default plan at HalfCheetah shapes: S=17, A=6, B=128, hidden (256, 256), relu, SAC-EO with 20
    expert rows (world models 512 x 512, the MSE head as GEMM problems of pi.q.fwd1+model.head, model.bwd1)
    and random normalisers.  Slabs: forward 2 (ragged) / 16 (actor, critics), 32 (models); dX 16, 32 and
    2 (the model head's, K = 17: ragged); dW 8 (critics: 128 rows) and 9 (actor: 148 rows, odd, ragged)."""
    _one_update("hc", monkeypatch, expect=("q.fwd0+actor.head", "pi.q.fwd1+model.head", "model.bwd1", "actor.adam"))


def test_bf16_update_hc_t32(gpu_available, monkeypatch):
    """The hc learner on 32x32 tiles (SACX_T32=1) with the weight and activation shadows (SACX_WBF=1:
    wbf.* / abf.*) and the transposed X^T images of critic.adam (SACX_XBF=2; B % 128 == 0); once more
    with k_dwl's dW + Adam tiles (SACX_DWL=2, and SACX_FUSE_HEAD=0 as in tests/test_gpu_dw.py: k_dwl takes
    critic.adam only without the policy head's rows riding along, so this run also has the actor head as
    its own launch at the hc shapes).  The same reference and bars as hc: a shadow, an image or another
    tiling changes no operand value.  That the variables engage at B = 128: the weight shadows, the
    layer-0 output shadow and the slots' X^T images exist, and the forward launches' grids shrink against
    the 16x16 plan's.  k_dwl's launches report the k_gemm family; they show in the grid (32x16 tiles against
    32x32)."""
    eng, *_ = make_pair(done_p=P.DONE_P, gemm_bf16=True, **P.CASES["hc"])
    plan16 = eng.plan_info()
    eng.close()
    env = {"SACX_T32": "1", "SACX_WBF": "1", "SACX_XBF": "2"}
    views = ("wbf.q0.l0", "wbf.actor.l1", "abf.ws.Hq1", "slot0.xbfq")
    _, plan = _one_update("hc", monkeypatch, env=env, expect=("critic.adam+actor.head",), views=views)
    _, plan_dwl = _one_update("hc", monkeypatch, env=dict(env, SACX_DWL="2", SACX_FUSE_HEAD="0"),
                              expect=("critic.adam", "actor.head"), views=views)
    grid = lambda pl, n: [L["grid"] for L in pl if L["name"] == n][0]
    for n in ("actor.fwd1", "q.fwd1", "pi.q.fwd0"):
        assert grid(plan, n) < grid(plan16, n), (n, grid(plan, n), grid(plan16, n))
    assert grid(plan_dwl, "actor.adam") > grid(plan, "actor.adam"), (grid(plan_dwl, "actor.adam"), grid(plan, "actor.adam"))


def test_bf16_update_pss_ln(gpu_available, monkeypatch):
    """Per-state std and the actor's layer norm: S=17, A=6, B=64, hidden (64, 48).  actor.fwd0 stores
    the pre-norm rows, k_ln norms them in fp32, gamma / beta's gradients are all-ones-row problems of
    actor.adam.  Slabs: forward 2 (ragged) / 4; dX 3 (K = 48: odd); dW 4 (64 rows)."""
    _one_update("pss_ln", monkeypatch, expect=("actor.ln", "actor.ln.bwd", "actor.adam"))


def test_bf16_update_generic(gpu_available, monkeypatch):
    """Hidden (520, 64), B=64: a layer above 512 takes the generic per-layer plan (q.head, critic.bwd1,
    pi.q.bwd1, actor.head.bwd as launches of their own; loss-scaled deltas, sac_oracle.BF16_UNIT_DELTAS
    False) with bf16 GEMMs.  Slabs: forward 2 (ragged) / 33 (K = 520: odd, ragged); dX 4; dW 4."""
    assert P.UNIT_DELTAS["generic"] is False
    _one_update("generic", monkeypatch, expect=("q.head", "critic.bwd1", "pi.q.bwd1", "actor.head.bwd"),
                absent=("q.head+critic.bwd1",))


def test_bf16_update_wide_k0(gpu_available, monkeypatch):
    """Humanoid's layer-0 K at a small batch: S=376, A=17, B=64, hidden (64, 64).  S + A > 64 keeps the
    actor head out of q.fwd0.  Slabs: forward 24 (K = 376: ragged) and 25 (K = 393: odd, ragged) / 4;
    dX 4; dW 4."""
    _one_update("wide_k0", monkeypatch, expect=("actor.head",), absent=("q.fwd0+actor.head",))


def test_bf16_trajectory_hc(gpu_available):
    """30 graph-replayed updates of hc (graph_steps = 8: three 8-update graphs and remainders): Q1 / Q2
    against the rounding oracle within 4 x the largest relative error its own fp32 executions reach over
    the same 30 updates (tests/test_oracle_bf16.py records the figure); the stream bit-exact."""
    steps = 30
    c = P.CASES["hc"]
    eng, ocfg, st, buf, nrm, expert = make_pair(done_p=P.DONE_P, gemm_bf16=True, graph_steps=8, **c)
    state0, Rs, rs = P.randoms("hc", buf, ocfg.A, steps)
    eng.rng_set_state(state0)
    eng.push_perms(np.stack([R["perm"] for R in Rs]))
    eng.step(steps)
    eng.sync()
    dev = eng.stats(steps)[:, :2].astype(np.float64)
    stream = eng.rng_get_state()
    eng.close()
    ref, env = P.trajectory_envelope("hc", steps)
    rel = np.abs(dev - ref) / np.abs(ref)
    bar = P.ENVELOPE_FACTOR * env
    print(f"hc trajectory: device {rel.max():.2e} bar {bar:.2e} envelope {env:.2e}")
    assert rel.max() <= bar, (rel.max(), bar)
    exp = rs.get_state()
    assert np.array_equal(stream[1], exp[1]) and stream[2] == exp[2] and stream[3] == exp[3] and stream[4] == exp[4]


# ------------------------------------------------------------------ the other plans of a gemm_bf16 handle
def _same_stream(eng, rs):
    got, exp = eng.rng_get_state(), rs.get_state()
    return np.array_equal(got[1], exp[1]) and got[2] == exp[2] and got[3] == exp[3] and got[4] == exp[4]


def _report(which, got):
    ref, env, bars, _ = P.plan_envelope(which)
    err = P.plan_error(which)
    for k in ref:
        print(f"{which} {k}: device {err(k, np.asarray(got[k], np.float64), np.asarray(ref[k])):.2e} bar {bars[k]:.2e} envelope {env[k]:.2e}")
    return P.plan_compare(which, got, ref, bars)


@pytest.mark.parametrize("mfuse", [None, "3"])
def test_bf16_model_fit(gpu_available, monkeypatch, mfuse):
    """Three world-model fitting steps (B = 64, models 512 x 512, minibatches of 200 rows) of a gemm_bf16
    handle: every launch of its chain with a GEMM is a bf16 one (forward with the loss epilogue, dX, dW +
    Adam), so the first step's gradients (through Adam's first moment) and the three losses are held to the
    rounding oracle.  model.bwd2 is a GEMM launch of its own also under SACX_MFUSE=3: that fold of it into
    model.bwd1 generates the head's dX with fp32 MFMAs, which would leave a GEMM's operands unrounded in
    one variant only, and is not taken under config C5."""
    if mfuse:
        monkeypatch.setenv("SACX_MFUSE", mfuse)
    eng, ocfg, st, buf, nrm, _ = make_pair(gemm_bf16=True, **P.FIT)
    assert eng.cfg.model_batch == P.FIT_MB
    idx = P.fit_indices(buf["r"].shape[0])
    eng.model_fit(idx[:1], eager=True)
    eng.sync()
    names = [L["name"] for L in eng.model_plan_info()]
    kernels = {L["name"]: L["kernel"] for L in eng.model_plan_info()}
    print("fit launches:", kernels)
    m = eng.v["adam_m"][0].cpu().numpy().astype(np.float64)
    got = {}
    for k in range(2):
        for l in range(3):
            seg = eng.segments[f"m{k}.l{l}"]
            off, n = seg["offset"] // 4, seg["rows"] * seg["cols"]
            w = m[off: off + n].reshape(seg["rows"], seg["cols"]) / np.float64(P.B1)
            got[f"grad.m{k}.{2 * l}"], got[f"grad.m{k}.{2 * l + 1}"] = w[:-1], w[-1]
    eng.model_fit(idx[1:])
    eng.sync()
    got["loss"] = eng.model_stats(P.FIT_STEPS).astype(np.float64)
    steps = eng.ctl()["t_model"]
    eng.close()
    assert steps == P.FIT_STEPS
    assert "model.bwd2+bwd1+final" not in names and any(n.startswith("model.bwd2") for n in names), names
    # (the kernel family is k_gemm for fp32 and bf16 launches alike: that the GEMMs round their operands
    # shows in the comparison -- the exact oracle is 1e-1 away in these gradients)
    _report("fit", got)


def test_bf16_objects(gpu_available):
    """The object calls on 64 rows of a gemm_bf16 handle against the rounding oracle: evaluate and act (the
    actor's hidden layers are bf16 GEMMs, the head a row kernel), critic_forward / value (every layer a
    GEMM, the head too), model_forward (every layer).  act on 3 rows runs k_act_rows, fp32 throughout: it
    is held to the EXACT oracle, which the rounding one is 1e-3 away from, so that a change of either
    path's mode shows.  The stream bit-exact."""
    eng, ocfg, st, buf, nrm, _ = make_pair(gemm_bf16=True, **P.OBJ)
    s, a = P.obj_rows()
    eng.rng_set_state(np.random.RandomState(19).get_state())
    got = {}
    got["evaluate.pi"], got["evaluate.nlp"] = [t.cpu().numpy() for t in eng.evaluate(s)]
    got["act"] = eng.act(s, False).cpu().numpy().reshape(P.OBJ_ROWS, ocfg.A)
    for net in ("q0", "t1"):
        got[f"critic.{net}"] = eng.critic_forward(net, s, a).cpu().numpy().reshape(P.OBJ_ROWS, 1)
        got[f"value.{net}"] = eng.critic_forward(net, s, a, value=True).cpu().numpy().reshape(P.OBJ_ROWS)
    for k in range(2):
        got[f"model{k}.pred"], got[f"model{k}.sp"], got[f"model{k}.r"] = [t.cpu().numpy() for t in eng.model_forward(k, s, a)]
    _, rs = P.obj_oracle()
    assert _same_stream(eng, rs)
    # three rows: the fp32 row kernel
    st64 = st
    few = np.asarray(eng.act_host(s[:3], False)).reshape(3, ocfg.A)
    u = rs.get_state()
    exact = O.head_sample(*O.split_head(O.actor_forward(st64.actor, O._norm(s[:3].astype(np.float64), nrm.s_mean, nrm.s_den),
                                                        ocfg)[0], st64.logstd, ocfg),
                          O.f32_noise(rs.normal(size=(3, ocfg.A))), ocfg.act_limit, np.float64)[0]
    rs.set_state(u)
    with P.oracle_mode("bf16"):
        rounded = O.head_sample(*O.split_head(O.actor_forward(st64.actor, O._norm(s[:3].astype(np.float64), nrm.s_mean,
                                                                                    nrm.s_den), ocfg)[0], st64.logstd, ocfg),
                                O.f32_noise(rs.normal(size=(3, ocfg.A))), ocfg.act_limit, np.float64)[0]
    assert _same_stream(eng, rs)
    eng.close()
    print(f"obj act3: device vs exact {P.relmax(few, exact):.2e}, rounded vs exact {P.relmax(rounded, exact):.2e}")
    assert P.relmax(few, exact) < P.OBJ_BAR and P.relmax(rounded, exact) > 10 * P.OBJ_BAR
    _report("obj", got)


def test_bf16_rollout(gpu_available):
    """One step of the world-model rollout on 37 rows (the actor's hidden layers and every layer of the
    model are bf16 GEMMs) against the rounding oracle, with the stages' two tiers (bf16_parity.roll_loose);
    the stream bit-exact."""
    eng, ocfg, st, buf, nrm, _ = make_pair(gemm_bf16=True, **P.OBJ)
    ref, rs, s0 = P.roll_oracle()
    eng.rng_set_state(np.random.RandomState(P.ROLL["stream"]).get_state())
    out = [t.cpu().numpy() for t in eng.rollout(P.ROLL["model"], s0, P.ROLL["horizon"], False)]
    ok = _same_stream(eng, rs)
    eng.close()
    assert ok and not out[4].any()
    _report("roll", dict(zip(("s", "a", "r", "sp"), out[:4])))
