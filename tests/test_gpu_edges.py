"""The squashed-Gaussian head at its clip bounds, in saturation, and min(Q1, Q2) on ties, on the device
against the oracle.

The head's branchy arithmetic -- the clip of the raw log-std to [-5, 2] with its pass-through mask (TF
clip_by_value: gradient 1 inside and AT the bounds, 0 outside), tanh where it rounds to +-1 in fp32, the three
branches of softplus(-2x) split at |x| = 6.97, and the 1 / 0 / 0.5-0.5 split of the min's gradient -- lives in
several copies in k_sac.hip (head_pre_finish, k_actor_head, head_bwd_prologue, k_actor_bwd, k_actor_bwd_wide,
k_act_rows / k_act_rng, k_roll, qhead_block, k_qhead_wide), and the plan picks the copy.  The learners of the
other test files leave every copy on its smooth middle (log-std 0, max |mu| about 2, no tie).  Here the states
of tests/edge_cases.py put each copy on its edges: `lsvar`, `lsvar+sat`, `pss_edges` and `tie`, on the shapes
whose plans reach the copies (the plan's launch names are asserted per shape, so that a changed fold shows
before the coverage moves to another copy):

  h64x64          the whole fused plan: the folded head prologues, head_bwd_prologue
  h63x65          the stand-alone k_actor_head / k_actor_bwd
  h64x61x64       the generic plan
  h520x64         k_actor_bwd_wide (the critics' layer 0 above 512)
  h64x520         the wide k_actor_head, k_qhead_wide and k_actor_bwd_wide's other axis (last layers above 512)
  a32             Aout = 32
  eo              SAC-EO: head_sample rows, where the mask applies with no entropy term
  h64x64x64_elu   per_state_std on three layers (pss_edges only)

Every one-update case runs the body of test_gpu_depth.py::test_one_update_any_depth as it is (losses 2e-5,
Dense gradients 2e-4 of the tensor's max, stream bit-exact) on the edge state and adds: ws.c_mask equal to the
oracle's mask exactly; the state-independent log-std gradient (Adam's first moment) within 2e-4 and exactly 0
on the masked coordinates; ws.nlp_t / ws.nlp_p within 2e-5 of the rows' max; ws.c_t equal to +-1 exactly
wherever the fp32 oracle's tanh is; actor.logstd after the step within 1e-6, a masked coordinate unmoved bit
for bit.

The reference alone (test_premise_of_the_edge_cases_on_the_cpu, no device): the oracle in fp32 against fp64
stays inside a quarter of each bar (losses 5e-6, gradients 5e-5, nlp rows 5e-6) on every case, the edges are
present in the shares asserted there, and both precisions take the same mask.  Measured: losses 4e-8 .. 2.0e-7,
gradients 2.3e-7 .. 4.5e-6, nlp rows 1.4e-7 .. 1.4e-6; at B = 1 the one neglogp row differs 5.1e-5 through
cancellation in the reference alone, so the B = 1 case compares losses and gradients only.

Ties: identical critics give identical dQ/da, so a 0.5 + 0.5 split and a 1 + 0 split give the same actor
gradient and this test cannot tell them apart.  What it catches is a split that does not sum to 1 (`<=` on
both sides doubles the gradient, `<` on both zeroes it): the actor gradients at 2e-4 and g0 + g1 == gmin on
every row of ws.gp.
"""
import numpy as np
import pytest

import edge_cases as EC
import helpers
import sac_oracle as O
import test_gpu_depth as D
from helpers import B1, make_learner, make_pair, oracle_step, relerr

N = 2000
SHAPES = {
    "h64x64": dict(hidden=(64, 64)),
    "h63x65": dict(hidden=(63, 65)),
    "h64x61x64": dict(hidden=(64, 61, 64)),
    "h520x64": dict(hidden=(520, 64)),
    "h64x520": dict(hidden=(64, 520)),
    "a32": dict(S=1, A=32, hidden=(64, 64)),
    "eo": dict(hidden=(64, 64), use_expert=True, model_hidden=(96, 96), ne=12),
    "h64x64x64_elu": dict(hidden=(64, 64, 64), act="elu"),
    "h64x96x48": dict(hidden=(64, 96, 48)),
}
SIX = ("h64x64", "h63x65", "h64x61x64", "h520x64", "a32", "eo")
UPDATE = ([(s, e) for s in SIX for e in ("lsvar", "lsvar+sat")] +
          [(s, "pss_edges") for s in ("h64x64", "h63x65", "h64x64x64_elu")] + [("h64x520", "lsvar+sat")])
BATCHES = (1, 15, 17)                    # lsvar on h64x64
TIES = ("h64x64", "h63x65", "h64x520")
TRAJ = (("h64x64", "lsvar"), ("h63x65", "pss_edges"))
TRAJ_STEPS = 20
# launch names a shape's plan must have / must not have ("+": no fused launch name at all)
PLAN = {
    "h64x64": (("q.fwd01+actor.head", "actor.head.bwd+actor.bwd1"), ("actor.head",)),
    "h63x65": (("actor.head", "actor.head.bwd", "q.head+critic.bwd1"), ("actor.fwd01", "q.fwd01+actor.head")),
    "h64x61x64": (("actor.head", "q.head", "pi.q.head", "actor.head.bwd"), ("+",)),
    "h520x64": (("actor.head", "q.head", "pi.q.head", "actor.head.bwd"), ("+",)),
    "h64x520": (("actor.head", "q.head", "pi.q.head", "actor.head.bwd"), ("+",)),
    "a32": (("actor.head", "actor.fwd01", "actor.head.bwd"), ("q.fwd01+actor.head",)),
    # the head forward folded (the policy rows' as critic.adam's prologue), the head backward a launch of its own
    "eo": (("q.fwd0+actor.head", "critic.adam+actor.head", "pi.q.fwd1+model.head", "actor.head.bwd"),
           ("actor.head", "actor.head.bwd+actor.bwd1")),
    "h64x64:pss_edges": (("q.fwd0+actor.head", "critic.adam+actor.head", "actor.head.bwd"),
                         ("actor.head", "actor.head.bwd+actor.bwd1")),
    "h64x64x64_elu": (("actor.head", "q.head", "pi.q.head", "actor.head.bwd"), ("+",)),
}
THR32 = -(np.log(np.finfo(np.float32).eps) + 2.0)      # softplus_f's outer branches: |-2x| > 13.94


def _kw(shape, edge):
    kw = dict(SHAPES[shape])
    kw.update(EC.split(edge)[1])
    kw.setdefault("ne", 12)
    kw.setdefault("act", "relu")
    return kw


def _check_plan(eng, shape, edge=""):
    names = [p["name"] for p in eng.plan_info()]
    have, lack = PLAN.get(f"{shape}:{edge}", PLAN[shape])
    for n in have:
        assert n in names, (shape, n, names)
    for n in lack:
        assert not any(n in m for m in names) if n == "+" else n not in names, (shape, n, names)


# ---------------------------------------------------------------------------------------------- the reference alone
def _oracle_updates(shape, edge, B, dtype, seed, draws, steps):
    """`steps` oracle updates of the edge state in `dtype`: per step (stats, keep, the log-std variable before
    the step).  `draws`: the seeds of the RandomState / Generator the randoms come from, as the device body
    draws them."""
    kw = _kw(shape, edge)
    ocfg, st, buf, nrm, expert = make_learner(B=B, seed=seed, N=N, normalizers="random", **kw)
    for m in EC.split(edge)[0]:
        m(st, ocfg)
    st = st.astype(dtype)
    eo = expert is not None
    rs, gen = np.random.RandomState(draws[0]), np.random.default_rng(draws[1])
    out = []
    for _ in range(steps):
        R = O.draw_step_randoms(rs, N, B, ocfg.A, n_expert=kw["ne"] if eo else 0, gen=gen, n_models=2)
        keep = {}
        ls0 = st.logstd.copy()
        ref = oracle_step(st, ocfg, nrm, buf, R, expert, keep)
        out.append((ref, keep, ls0))
    return ocfg, out, st


def _compared(ref, keep, ocfg, eo):
    losses = [ref[k] for k in ("q1_loss", "q2_loss", "p_loss", "alpha_loss")] + ([ref["mse_loss"]] if eo else [])
    grads = list(keep["q0_grads"]) + list(keep["q1_grads"]) + list(keep["actor_grads"])
    if not ocfg.per_state_std:
        grads.append(keep["g_logstd"])
    return np.array(losses, np.float64), [np.asarray(g, np.float64) for g in grads]


def _masks(keep):
    return np.concatenate([keep["head_p"].mask] + [h.mask for h in keep["head_e"]], 0)


PREMISE = ([(s, e, 64) for s, e in UPDATE] + [("h64x64", "lsvar", B) for B in BATCHES] +
           [(s, "tie", 64) for s in TIES])


@pytest.mark.parametrize("shape,edge,B", PREMISE)
def test_premise_of_the_edge_cases_on_the_cpu(shape, edge, B):
    """No device.  The oracle's one update of every case in fp32 against fp64 (the learner and the draws of
    test_one_update_any_depth) stays inside a quarter of each device bar, and the conditions that keep the
    device tests from passing vacuously hold: the edges are present, both precisions take the same mask, the
    log-std gradient is non-zero on the unmasked coordinates (the at-bound ones included) and exactly 0 on
    the masked ones, every row of a tie case ties."""
    runs = {}
    for dt in (np.float64, np.float32):
        ocfg, out, _ = _oracle_updates(shape, edge, B, dt, 3, (17, 4), 1)
        runs[dt] = out[0]
    (r64, k64, ls0), (r32, k32, _) = runs[np.float64], runs[np.float32]
    eo = "mse_loss" in r64
    l64, g64 = _compared(r64, k64, ocfg, eo)
    l32, g32 = _compared(r32, k32, ocfg, eo)
    loss = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
    grad = max(relerr(a, b) for a, b in zip(g32, g64))
    nlp = max(relerr(k32[k], k64[k]) for k in ("nlp_p", "nlp_t"))
    h64, h32 = k64["head_p"], k32["head_p"]
    m64, m32 = _masks(k64), _masks(k32)
    lraw = np.asarray(k64["ls_p"] if ocfg.per_state_std else np.broadcast_to(ls0, h64.mask.shape), np.float64)
    lo, at_lo, at_hi, hi = [float(np.mean(c)) for c in (lraw < -5, lraw == -5, lraw == 2, lraw > 2)]
    sat = float(np.mean(np.abs(h32.t) == 1))
    x2 = np.float32(-2) * h32.x
    print(f"premise {shape} {edge} B={B}: loss {loss:.2e} (quarter bar 5e-6) gradient {grad:.2e} (5e-5) nlp rows "
          f"{nlp:.2e} (5e-6); raw log-std below {lo:.3f} at -5 {at_lo:.3f} at 2 {at_hi:.3f} above {hi:.3f}, mask 0 "
          f"{float(np.mean(m64 == 0)):.3f}; |tanh| == 1 in fp32 {sat:.3f}, max |mu| {float(np.max(np.abs(k64['mu_p']))):.1f}, "
          f"softplus outer branches {int((x2 > THR32).sum())} / {int((x2 < -THR32).sum())} of {x2.size}; "
          f"ties {int(np.sum(k64['q1p'] == k64['q2p']))} of {B}")
    assert loss < 5e-6, loss
    assert grad < 5e-5, grad
    if B > 1:
        assert nlp < 5e-6, nlp
    assert np.array_equal(m64, m32)
    parts = edge.split("+")
    if "lsvar" in parts or "pss_edges" in parts:
        assert np.mean(m64 == 0) >= 0.10 and np.mean(m64 == 1) >= 0.10
        assert at_lo > 0 and at_hi > 0
        assert np.array_equal(h64.mask, EC.clip_mask(lraw))
    if "lsvar" in parts or "sat" in parts:
        # 5 % of the 64-row cases' 384 actions and more.  The small-batch cases are about the batch: of their 6,
        # 90 and 102 actions 1, 5 and 5 saturate (4.9 % at B = 17: a share of so few draws cannot be held to
        # 5 %) and B = 1 has one action beyond the softplus threshold, so they ask for one of each
        assert sat >= 0.05 if B == 64 else sat > 0, sat
        assert ((x2 > THR32).any() and (x2 < -THR32).any()) if B > 1 else (np.abs(x2) > THR32).any()
    if "pss_edges" in parts:
        for k in (k64, k32):
            d = np.minimum(np.abs(np.asarray(k["ls_p"], np.float64) + 5), np.abs(np.asarray(k["ls_p"], np.float64) - 2))
            assert np.all((d == 0) | (d > 1e-4)), float(np.min(d[d > 0]))
    if "lsvar" in parts:
        gl, mk = k64["g_logstd"][0], EC.clip_mask(ls0[0])
        print(f"premise {shape} {edge} B={B}: g_logstd {np.array2string(gl[:6], precision=2)}")
        assert np.all(gl[mk == 0] == 0.0) and np.all(gl[mk == 1] != 0.0), gl
        assert np.all(k32["g_logstd"][0][mk == 0] == 0.0)
    if edge == "tie":
        assert np.array_equal(k64["q1p"], k64["q2p"]) and np.array_equal(k32["q1p"], k32["q2p"])


@pytest.mark.parametrize("shape,edge", TRAJ)
def test_premise_of_the_edge_trajectories_on_the_cpu(shape, edge):
    """No device.  20 oracle updates of the trajectory cases in both precisions: the losses inside a quarter
    of the device bar (2.5e-5), the final log-std variable within 1.25e-6, the same mask at every step, the
    masked coordinates of the variable never moved, and from step 1 on no coordinate of the variable closer
    than 5e-5 to a clip bound (the at-bound coordinates leave the bound by one Adam step of 1e-4), so that
    the fp32 device and the fp64 oracle cannot disagree about a coordinate's side."""
    runs = {dt: _oracle_updates(shape, edge, 64, dt, 11, (123, 77), TRAJ_STEPS) for dt in (np.float64, np.float32)}
    (ocfg, o64, st64), (_, o32, st32) = runs[np.float64], runs[np.float32]
    L = lambda o: np.array([[r["q1_loss"], r["q2_loss"], r["p_loss"]] for r, _, _ in o])
    rel = float(np.max(np.abs(L(o32) - L(o64)) / np.abs(L(o64))))
    dls = float(np.max(np.abs(st32.logstd - st64.logstd)))
    ls = np.array([l[0] for _, _, l in o64[1:]] + [st64.logstd[0]])
    dist = float(np.min(np.minimum(np.abs(ls + 5), np.abs(ls - 2))))
    print(f"premise trajectory {shape} {edge}: losses {rel:.2e} (quarter bar 2.5e-5) final log-std {dls:.2e} "
          f"(1.25e-6) closest to a bound after step 1 {dist:.2e}")
    assert rel < 2.5e-5 and dls < 1.25e-6
    for (_, k64, _), (_, k32, _) in zip(o64, o32):
        assert np.array_equal(_masks(k64), _masks(k32))
    if not ocfg.per_state_std:
        masked = EC.clip_mask(o64[0][2][0]) == 0
        assert masked.any() and dist >= 5e-5, dist
        for st, o in ((st64, o64), (st32, o32)):
            assert np.array_equal(st.logstd[0][masked], o[0][2][0][masked])


# ---------------------------------------------------------------------------------------------------- the device
def _run_body(monkeypatch, shape, edge, B=64):
    """test_one_update_any_depth on the edge state, as it is; its engine is handed back open (the caller
    closes it) with the oracle's keep of the fp64 update, of the same update in fp32, and the log-std
    variable as it was before the step (keep["ls_p"] is a view that Adam moves)."""
    cap = {}
    monkeypatch.setattr(helpers, "make_learner", EC.mutating(helpers.make_learner, EC.split(edge)[0]))
    real_pair, real_step = D.make_pair, D.oracle_step

    def pair(*a, **k):
        out = real_pair(*a, **k)
        cap.update(eng=out[0], close=out[0].close)
        out[0].close = lambda: None
        return out

    def step(st, ocfg, nrm, buf, R, expert=None, keep=None):
        cap.update(ls0=st.logstd.copy(), keep32={}, ocfg=ocfg, st=st)
        oracle_step(st.astype(np.float32), ocfg, nrm, buf, R, expert, cap["keep32"])
        cap["keep"] = keep
        return real_step(st, ocfg, nrm, buf, R, expert, keep)

    monkeypatch.setattr(D, "make_pair", pair)
    monkeypatch.setattr(D, "oracle_step", step)
    name = f"{shape}:{edge}"
    monkeypatch.setitem(D.CASES, name, dict(_kw(shape, edge), N=N))
    try:
        D.test_one_update_any_depth(True, monkeypatch, name, B=B)
    except BaseException:
        if "close" in cap:
            cap["close"]()
        raise
    return cap


def _check_head(cap, shape, edge, B, rows_nlp=True):
    """What the body does not compare: the mask, the saturated tanh, the neglogp rows, the log-std variable's
    gradient and step."""
    eng, keep, keep32, ocfg, st, ls0 = (cap[k] for k in ("eng", "keep", "keep32", "ocfg", "st", "ls0"))
    A = ocfg.A
    v = lambda n: eng.v[n].cpu().numpy()
    mask = _masks(keep)
    rows = mask.shape[0]
    assert np.array_equal(mask, _masks(keep32))
    assert np.array_equal(v("ws.c_mask")[:rows], mask), np.argwhere(v("ws.c_mask")[:rows] != mask)[:8]
    t32 = np.concatenate([keep32["head_p"].t] + [h.t for h in keep32["head_e"]], 0)
    one = np.abs(t32) == 1
    ct = v("ws.c_t")[:rows]
    assert np.array_equal(ct[one], t32[one]), (int(one.sum()), int((ct[one] != t32[one]).sum()))
    err_t = relerr(ct, np.concatenate([keep["head_p"].t] + [h.t for h in keep["head_e"]], 0))
    assert err_t < 2e-5, err_t
    msg = f"edges {shape} {edge} B={B}: mask rows {rows} zeros {int((mask == 0).sum())}, tanh == +-1 {int(one.sum())} of {one.size}"
    if rows_nlp:
        e_t, e_p = relerr(v("ws.nlp_t")[0][:B], keep["nlp_t"]), relerr(v("ws.nlp_p")[0][:B], keep["nlp_p"])
        msg += f", nlp_t {e_t:.2e} nlp_p {e_p:.2e} (bar 2e-5)"
        assert e_t < 2e-5 and e_p < 2e-5, (e_t, e_p)
    if not ocfg.per_state_std:
        seg = eng.segments["actor.logstd"]
        gl = eng.v["adam_m"][0][seg["offset"] // 4: seg["offset"] // 4 + A].cpu().numpy() / B1
        masked = EC.clip_mask(ls0[0]) == 0
        ls = v("actor.logstd").reshape(-1)
        e_g, e_l = relerr(gl, keep["g_logstd"][0]), float(np.max(np.abs(ls - st.logstd[0])))
        msg += f", g_logstd {e_g:.2e} (bar 2e-4) logstd after {e_l:.2e} (bar 1e-6)"
        assert e_g < 2e-4, (gl, keep["g_logstd"][0])
        assert np.all(gl[masked] == 0.0), gl
        assert e_l < 1e-6, e_l
        assert np.array_equal(ls[masked], ls0[0][masked].astype(np.float32)), (ls, ls0)
    print(msg)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,edge", UPDATE)
def test_one_update_edges(gpu_available, monkeypatch, shape, edge):
    cap = _run_body(monkeypatch, shape, edge)
    try:
        _check_head(cap, shape, edge, 64)
        _check_plan(cap["eng"], shape, edge)
    finally:
        cap["close"]()


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
def test_one_update_edges_small_batches(gpu_available, monkeypatch, B):
    """lsvar on the fused plan at 1, 15 and 17 rows.  At B = 1 the losses and the gradients only: the reference
    alone differs 5.1e-5 on the one neglogp row there, through cancellation."""
    cap = _run_body(monkeypatch, "h64x64", "lsvar", B=B)
    try:
        _check_head(cap, "h64x64", "lsvar", B, rows_nlp=B > 1)
        _check_plan(cap["eng"], "h64x64")
    finally:
        cap["close"]()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TIES)
def test_min_ties(gpu_available, monkeypatch, shape):
    """Critic 1 a copy of critic 0: every policy row ties.  Identical critics give identical dQ/da, so a
    0.5 + 0.5 split and a 1 + 0 split give the same actor gradient: this test cannot tell those apart.  It
    catches a split that does not sum to 1: the body's actor gradients at 2e-4, and g0 + g1 == gmin on
    every row of ws.gp (qhead_block on the narrow shapes, k_qhead_wide on h64x520)."""
    cap = _run_body(monkeypatch, shape, "tie")
    try:
        eng, B = cap["eng"], 64
        gp = eng.v["ws.gp"].cpu().numpy().reshape(2, -1)[:, :B]
        gmin = -(np.float32(1) / np.float32(B))
        ties = int(np.sum(gp[0] == gp[1]))
        print(f"ties {shape}: {ties} of {B} rows bitwise ties on the device, {int(np.sum(cap['keep']['q1p'] == cap['keep']['q2p']))} in the oracle")
        assert np.array_equal(gp[0] + gp[1], np.full(B, gmin, np.float32)), (gp, gmin)
        assert ties > 0
        _check_plan(eng, shape)
    finally:
        cap["close"]()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,edge", TRAJ)
def test_trajectory_edges(gpu_available, monkeypatch, shape, edge):
    """20 graph-replayed updates: the Q losses and the policy loss within 1e-4 at every step, the final log-std
    variable within 5e-6, its masked coordinates bit-identical to their initial values (zero gradient: Adam
    must not move them), the stream bit-exact.  Under per_state_std the variable is not used at all, so for
    pss_edges that last check only shows that an unused variable stays untouched; what holds the per-state mask
    over the 20 steps there is the loss comparison."""
    B, steps = 64, TRAJ_STEPS
    monkeypatch.setattr(helpers, "make_learner", EC.mutating(helpers.make_learner, EC.split(edge)[0]))
    eng, ocfg, st, buf, nrm, expert = make_pair(B=B, seed=11, N=N, normalizers="random", **_kw(shape, edge))
    try:
        ls0 = st.logstd.copy()
        rs, gen = np.random.RandomState(123), np.random.default_rng(77)
        eng.rng_set_state(rs.get_state())
        Rs = [O.draw_step_randoms(rs, N, B, ocfg.A, gen=gen) for _ in range(steps)]
        eng.step(steps)
        eng.sync()
        dev = eng.stats(steps)
        ref = np.array([[o["q1_loss"], o["q2_loss"], o["p_loss"]] for o in (oracle_step(st, ocfg, nrm, buf, R) for R in Rs)])
        rel = float(np.max(np.abs(dev[:, :3] - ref) / np.abs(ref)))
        ls = eng.v["actor.logstd"].cpu().numpy().reshape(-1)
        dls = float(np.max(np.abs(ls - st.logstd[0])))
        print(f"trajectory {shape} {edge}: losses {rel:.2e} (bar 1e-4) final log-std {dls:.2e} (bar 5e-6)")
        assert rel < 1e-4, rel
        assert dls < 5e-6, dls
        masked = np.ones(ocfg.A, bool) if ocfg.per_state_std else EC.clip_mask(ls0[0]) == 0
        assert masked.any() and np.array_equal(ls[masked], ls0[0][masked].astype(np.float32)), (ls, ls0)
        assert D._same_stream(eng, rs)
        _check_plan(eng, shape)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["h63x65", "h64x64", "h64x96x48"])
def test_objects_edges(gpu_available, monkeypatch, shape):
    """The lsvar+sat state through the object calls: evaluate on 300 rows, act / act_host on 3 rows (k_act_rows)
    and 40 (the GEMMs and k_actor_head), stochastic and deterministic, and a rollout of horizon 4 (k_roll), at
    the bars of test_objects_any_depth / test_rollout_any_depth, the stream bit-exact."""
    monkeypatch.setattr(helpers, "make_learner", EC.mutating(helpers.make_learner, (EC.lsvar,)))
    eng, ocfg, st, buf, nrm, _ = make_pair(B=64, seed=41, N=N, normalizers="random", use_expert=True, ne=12,
                                           model_hidden=(64, 64), **dict(SHAPES[shape], **EC.SAT))
    try:
        S, A = ocfg.S, ocfg.A
        s, _, _ = D._rows(300, S, A, 1)
        rs = np.random.RandomState(19)
        eng.rng_set_state(rs.get_state())
        pi, nlp = [t.cpu().numpy() for t in eng.evaluate(s)]
        rpi, rnlp = O.actor_evaluate(st, ocfg, nrm, s, rs)
        sat = float(np.mean(np.abs(rpi.astype(np.float32)) == 1))
        print(f"objects {shape}: evaluate pi {relerr(pi, rpi):.2e} nlp {relerr(nlp, rnlp):.2e} (bar 2e-5), |pi| == 1 {sat:.3f}")
        assert sat >= 0.05
        assert relerr(pi, rpi) < 2e-5 and relerr(nlp, rnlp) < 2e-5
        for host in (True, False):
            for det in (False, True):
                for rows in (3, 40):
                    got = eng.act_host(s[:rows], det) if host else eng.act(s[:rows], det).cpu().numpy()
                    o, _ = O.actor_forward(st.actor, O._norm(s[:rows].astype(np.float64), nrm.s_mean, nrm.s_den), ocfg)
                    mu, lraw = O.split_head(o, st.logstd, ocfg)
                    u = np.zeros_like(mu) if det else O.f32_noise(rs.normal(size=mu.shape))
                    ref_a = O.head_sample(mu, lraw, u, ocfg.act_limit, np.float64)[0]
                    err = relerr(np.asarray(got).reshape(rows, A), ref_a)
                    assert err < 2e-5, (host, det, rows, err)
        assert D._same_stream(eng, rs)
        s0 = (np.random.RandomState(5).normal(size=(300, S)) * 1.5).astype(np.float32)
        for det in (False, True):
            got = [t.cpu().numpy() for t in eng.rollout(1, s0, 4, det)]
            ref = O.rollout(st, ocfg, nrm, s0, 4, 1, rs, det)
            print(f"objects {shape}: rollout det={det} " + " ".join(
                f"{name} {relerr(g, r):.2e}" for g, r, name in zip(got[:4], ref[:4], ("s", "a", "r", "sp"))) + " (bar 1e-4)")
            for g, r, name in zip(got[:4], ref[:4], ("s", "a", "r", "sp")):
                assert relerr(g, r) < 1e-4, (name, det, relerr(g, r))
            assert D._same_stream(eng, rs)
    finally:
        eng.close()


@pytest.mark.gpu
def test_dropin_act_edges(gpu_available, monkeypatch):
    """One drop-in call through k_act_rng on the lsvar+sat state: after an update of one, a deterministic
    act_host carries the next update's draw in its launch (tests/test_gpu_dropin.py).  The saturated action
    within 2e-5 of the oracle's, and the update that follows, run on that draw, within the one-update bars."""
    monkeypatch.setenv("SACX_SPEC", "1")
    monkeypatch.setattr(helpers, "make_learner", EC.mutating(helpers.make_learner, (EC.lsvar,)))
    B = 64
    eng, ocfg, st, buf, nrm, _ = make_pair(B=B, seed=5, N=N, normalizers="random", graph_steps=1,
                                           **dict(SHAPES["h64x64"], **EC.SAT))
    try:
        rs = np.random.RandomState(12)
        eng.rng_set_state(rs.get_state())
        obs = (np.random.RandomState(3).normal(size=(3, ocfg.S)) * 1.5).astype(np.float32)
        for j in range(2):
            ref = oracle_step(st, ocfg, nrm, buf, O.draw_step_randoms(rs, N, B, ocfg.A))
            eng.step(1, num_timesteps=j, ts_increment=1)
            row = eng.stats(1)[0]
            for i, k in enumerate(("q1_loss", "q2_loss", "p_loss", "alpha_loss")):
                assert abs(row[i] - ref[k]) <= 2e-5 * abs(ref[k]) + 1e-7, (j, k, row[i], ref[k])
            if j == 0:
                got = np.asarray(eng.act_host(obs, True)).reshape(3, ocfg.A)
                o, _ = O.actor_forward(st.actor, O._norm(obs.astype(np.float64), nrm.s_mean, nrm.s_den), ocfg)
                mu, lraw = O.split_head(o, st.logstd, ocfg)
                ref_a = O.head_sample(mu, lraw, np.zeros_like(mu), ocfg.act_limit, np.float64)[0]
                assert np.mean(np.abs(ref_a.astype(np.float32)) == 1) >= 0.05
                assert relerr(got, ref_a) < 2e-5, relerr(got, ref_a)
        assert eng.spec_hits() >= 1, eng.spec_hits()
        assert D._same_stream(eng, rs)
    finally:
        eng.close()
