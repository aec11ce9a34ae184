"""Packed on-policy learners on the device: ``Engine.ppo_steps_packed`` / ``vcritic_steps_packed`` on an
``EngineConfig(learners=3)`` engine against the one-learner path, which tests/test_gpu_ppo.py and
tests/test_gpu_vcritic.py hold to the fp64 restatements.

The packed call runs the same kernels in the same reduction orders at grid z = learner, so each learner must
end BIT FOR BIT where a fresh one-learner engine given the same weights, table, indices and parameters ends:
every PARAM and STATE segment of its arena block (weights, Adam m / v / t, logstd, ``ppo.alpha``, the control
blocks, the statistics rings, the tables with ``neglogp_old`` and the reference distribution) and the outputs of
``ppo_end`` / ``vcritic_end``.

Shapes, the smallest that reach each boundary: S = 3, A = 2 (softmax: 3), hidden (16, 8), tanh; learner k with
its own weights, tables of 37 / 41 / 29 rows, its own indices and its own rate; mb = 5 and 9 (no multiples of
the head's 4 rows per workgroup); 11 steps (graphs of 8 + 1 + 1 + 1), 75 (64 + 8 + three singles) and one case
of 1,100 at mb = 5, which wraps the 1,024-step index ring.
"""
import numpy as np
import pytest
import torch

import ppo_ref as R
import sac_oracle as O
import vcritic_ref as V
from helpers import nontrivial_normalizers

pytestmark = pytest.mark.gpu

S, HID, ACTS, K = 3, (16, 8), ("tanh", "tanh"), 3
ROWS = (37, 41, 29)
CAP, BATCH = 41, 9
PPO_LR = (1e-4, 3e-4, 2e-4)          # each learner's own rate (adaptlr makes them differ)
VC_LR = (1e-3, 5e-4, 2e-3)


def make_engine(learners=0, vcritics=0, hidden=HID, acts=None, **kw):
    from sac_eo.engine import Engine, EngineConfig
    A = 3 if kw.get("softmax") else 2
    return Engine(EngineConfig(s_dim=S, a_dim=A, hidden=hidden, activation="tanh", actor_activations=acts, critic_hidden=hidden,
                               batch=BATCH, buffer_capacity=CAP, actor_gaussian="train", graph_steps=1, vcritics=vcritics,
                               learners=learners, **kw))


def learner(k, n_steps, mb, nc=0, softmax=False, per_state_std=False, layer_norm=False, hidden=HID, acts=ACTS):
    """Everything learner k brings, decided on the CPU from its own seed."""
    A = 3 if softmax else 2
    cfg = O.Config(S=S, A=A, hidden=hidden, actor_acts=acts, per_state_std=per_state_std, layer_norm=layer_norm)
    rng = np.random.RandomState(100 + 7 * k)
    st0 = R.init_state(cfg, seed=20 + k, logstd=(0.2 * rng.normal(size=A) - 0.3), gain=0.5, dt=np.float32)
    st = st0.copy()                                       # the policy a few updates after the rollout: r leaves 1
    for w in st.actor:
        w += (0.05 * rng.normal(size=w.shape)).astype(np.float32)
    st.logstd += (0.03 * rng.normal(size=st.logstd.shape)).astype(np.float32)
    n = ROWS[k]
    s = (rng.normal(size=(n, S)) * rng.uniform(0.3, 2.0, S)).astype(np.float32)
    a = rng.randint(0, A, n).astype(np.float32) if softmax else rng.normal(size=(n, A)).astype(np.float32)
    adv = (rng.normal(size=n) * 1.5 + 0.4).astype(np.float32)
    nrm = nontrivial_normalizers(rng, S, A)
    nrm.ret_den = np.float32(2.7 + k)
    crit = V.init_state(S, hidden, max(nc, 1), seed=40 + k, dt=np.float32)
    vn = [n - 2 * c for c in range(nc)]                   # the critics' tables differ in length too
    vs = [(rng.normal(size=(m, S)) * 1.3).astype(np.float32) for m in vn]
    vrtg = [(rng.normal(size=m) * 4 + 1).astype(np.float32) for m in vn]
    idx = np.stack([rng.permutation(n)[:mb] for _ in range(n_steps)]).astype(np.int32)
    vidx = np.stack([rng.permutation(min(vn) if vn else n)[:mb] for _ in range(n_steps)]).astype(np.int32)
    return dict(cfg=cfg, st0=st0, st=st, s=s, a=a, adv=adv, nrm=nrm, crit=crit, vs=vs, vrtg=vrtg, idx=idx, vidx=vidx,
                nc=nc, softmax=softmax)


def give(eng, L, st):
    eng.set_net("actor", [np.asarray(w, np.float32) for w in st.actor])
    eng.set_logstd(np.asarray(st.logstd, np.float32))
    eng.set_normalizers(L["nrm"].s_mean, L["nrm"].s_den, L["nrm"].a_mean, L["nrm"].a_den, ret_den=float(L["nrm"].ret_den))
    for c in range(L["nc"]):
        eng.set_net(f"v{c}", [np.asarray(x, np.float32) for x in L["crit"].critics[c]])


def ppo_prepare(eng, L):
    give(eng, L, L["st0"])
    eng.ppo_begin(L["s"], L["a"], L["adv"])
    give(eng, L, L["st"])


def vc_prepare(eng, L):
    give(eng, L, L["st0"])
    for c in range(L["nc"]):
        eng.vcritic_begin(c, L["vs"][c], L["vrtg"][c])


def same_state(pk, k, one, what):
    """Learner k's block of the packed engine == the one-learner engine's arena, every PARAM / STATE segment."""
    from sac_eo import _native as N
    pk.sync()
    one.sync()
    names = []
    for name, d in pk.segments.items():
        if d["role"] not in (N.ROLE_PARAM, N.ROLE_STATE):
            continue
        assert one.segments[name] == d, name
        nb = d["rows"] * d["cols"] * (8 if d["dtype"] in ("i64", "f64") else 4)
        x, y = pk._arenas[k][d["offset"]: d["offset"] + nb], one.arena[d["offset"]: d["offset"] + nb]
        assert torch.equal(x, y), (what, k, name, int((x != y).sum().item()))
        names.append(name)
    return names


def _eq(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (key, a[key], b[key])


PPO_CASES = {
    # name: (flags of the engine and the learners, mb, n_steps, parameters)
    "gaussian": (dict(), 5, 11, dict(max_grad_norm=None)),
    "per_state_std": (dict(per_state_std=True), 9, 11, dict(max_grad_norm=None, adv_center=False)),
    "layer_norm": (dict(layer_norm=True), 9, 75, dict(max_grad_norm=None, adv_scale=False)),
    "softmax": (dict(softmax=True), 5, 75, dict(max_grad_norm=None)),
    "ent_reg": (dict(), 9, 11, dict(max_grad_norm=None, ent_reg=True, alpha_lr=0.02, ent_targ=4.0)),
    "grad_clip": (dict(), 5, 11, dict(max_grad_norm=0.05)),
    "ring_wrap": (dict(), 5, 1100, dict(max_grad_norm=0.5)),
    # two learners off the 4-grid: every row stride odd, the learners' blocks apart by the arena's own stride
    "odd": (dict(hidden=(23, 41), acts=("tanh", "elu"), K=2), 5, 11, dict(max_grad_norm=None)),
}


def _eng_flags(flags):
    f = dict(flags)
    f.pop("K", None)                                       # (the case's learner count: K unless it says so)
    if f.pop("layer_norm", False):
        f["actor_layer_norm"] = True
    return f


def _run_packed_ppo(Ls, flags, par, eager=False):
    nk = len(Ls)
    pk = make_engine(learners=nk, **_eng_flags(flags))
    assert pk.seeds == nk and pk.arena_all.numel() == nk * pk.seed_stride
    for k in reversed(range(nk)):                          # (any order: each call addresses the selected learner)
        pk.select_seed(k)
        ppo_prepare(pk, Ls[k])
    pk.ppo_steps_packed(np.stack([L["idx"] for L in Ls]), actor_lr=PPO_LR[:nk], eps_ppo=0.2, eager=eager, **par)
    ends = []
    for k in range(nk):
        pk.select_seed(k)
        ends.append(pk.ppo_end(0.2))
    return pk, ends


@pytest.mark.parametrize("case", list(PPO_CASES))
def test_packed_ppo_steps_equal_the_one_learner_steps(gpu_available, case):
    flags, mb, n_steps, par = PPO_CASES[case]
    nk = flags.get("K", K)
    Ls = [learner(k, n_steps, mb, **{a: b for a, b in flags.items() if a != "K"}) for k in range(nk)]
    pk, ends = _run_packed_ppo(Ls, flags, par)
    for k in range(nk):
        one = make_engine(**_eng_flags(flags))
        ppo_prepare(one, Ls[k])
        one.ppo_steps(Ls[k]["idx"], actor_lr=PPO_LR[k], eps_ppo=0.2, **par)
        end = one.ppo_end(0.2)
        names = same_state(pk, k, one, case)
        for need in ("actor.l0", "actor.l2", "actor.logstd", "adam_m", "adam_v", "ppo.alpha", "ppo.ctl", "ppo.stats",
                     "ppo.acc", "ppo.log"):
            assert need in names, need
        _eq(ends[k], end)
        assert end["n_steps"] == n_steps
        ctl = one.v["ppo.ctl"][0].cpu().numpy()
        assert ctl[0] == ctl[1] == n_steps and ctl[4] == ROWS[k]
        moved = max(float(np.max(np.abs(x - np.asarray(y, np.float32)))) for x, y in zip(one.get_net("actor"), Ls[k]["st"].actor))
        assert moved > 1e-5                                # the steps trained something
        st = one.ppo_stats(min(n_steps, 8))
        if case == "grad_clip":                            # the bound binds: both norms differ on every step
            assert np.all(st[:, 2] > 0.05) and np.all(st[:, 3] < st[:, 2])
        if case == "ent_reg":
            assert ctl[2] == n_steps and end["alpha"] > 0
        one.close()
    # the learners are different runs
    assert not torch.equal(pk._views[0]["actor.l0"], pk._views[1]["actor.l0"])
    pk.close()


VC_CASES = {"one_critic": (1, 5, 75), "two_critics": (2, 9, 11)}


def _run_packed_vc(Ls, nc, eager=False):
    pk = make_engine(learners=K, vcritics=nc)
    for k in range(K):
        pk.select_seed(k)
        vc_prepare(pk, Ls[k])
    pk.vcritic_steps_packed(np.stack([L["vidx"] for L in Ls]), critic_lr=VC_LR, eager=eager)
    ends = []
    for k in range(K):
        pk.select_seed(k)
        ends.append(pk.vcritic_end())
    return pk, ends


@pytest.mark.parametrize("case", list(VC_CASES))
def test_packed_critic_steps_equal_the_one_learner_steps(gpu_available, case):
    nc, mb, n_steps = VC_CASES[case]
    Ls = [learner(k, n_steps, mb, nc=nc) for k in range(K)]
    pk, ends = _run_packed_vc(Ls, nc)
    for k in range(K):
        one = make_engine(vcritics=nc)
        vc_prepare(one, Ls[k])
        one.vcritic_steps(Ls[k]["vidx"], critic_lr=VC_LR[k])
        end = one.vcritic_end()
        names = same_state(pk, k, one, case)
        for need in ("v0.l0", f"v{nc - 1}.l2", "vc.adam_m", "vc.adam_v", "vc.ctl", "vc.stats"):
            assert need in names, need
        assert end["n_steps"] == n_steps and len(end["critic_loss"]) == nc
        assert np.array_equal(np.asarray(ends[k]["critic_loss"]), np.asarray(end["critic_loss"])) and ends[k]["n_steps"] == n_steps
        ctl = one.v["vc.ctl"][0].cpu().numpy()
        assert ctl[0] == ctl[1] == n_steps and list(ctl[2:2 + nc]) == [ROWS[k] - 2 * c for c in range(nc)]
        one.close()
    pk.close()


def test_graph_replay_equals_eager_bit_for_bit(gpu_available):
    flags, mb, n_steps, par = PPO_CASES["grad_clip"]
    Ls = [learner(k, 75, mb, nc=2) for k in range(K)]
    a, ends_a = _run_packed_ppo(Ls, flags, par)
    b, ends_b = _run_packed_ppo(Ls, flags, par, eager=True)
    a.sync(), b.sync()
    for k in range(K):
        _eq(ends_a[k], ends_b[k])
    assert torch.equal(a.arena_all, b.arena_all)            # every byte of every learner, work areas included
    a.close(), b.close()
    a, ends_a = _run_packed_vc(Ls, 2)
    b, ends_b = _run_packed_vc(Ls, 2, eager=True)
    a.sync(), b.sync()
    assert torch.equal(a.arena_all, b.arena_all)
    assert [e["critic_loss"] for e in ends_a] == [e["critic_loss"] for e in ends_b]
    a.close(), b.close()


def test_learner_1_against_the_fp64_restatements(gpu_available):
    """One packed step, learner 1 read directly against tests/ppo_ref.py and tests/vcritic_ref.py at the bars
    tests/test_gpu_ppo.py and tests/test_gpu_vcritic.py use for the same quantities: loss, entropy, both norms
    and alpha 2e-5 relative, the weights after Adam 1e-6 absolute."""
    mb, nc = 9, 2
    par = dict(max_grad_norm=0.5, ent_reg=True, alpha_lr=0.02, ent_targ=4.0, adv_center=False)
    Ls = [learner(k, 1, mb, nc=nc) for k in range(K)]
    L = Ls[1]
    ref = L["st"].astype(np.float64)
    b = L["idx"][0]
    nlp_old = R.neglogp(L["st0"].astype(np.float64), L["cfg"], L["nrm"], L["s"], L["a"])
    o = R.ppo_step(ref, L["cfg"], L["nrm"], L["s"][b], L["a"][b], L["adv"][b], nlp_old[b],
                   {**R.DEFAULTS, "actor_lr": PPO_LR[1], "eps_ppo": 0.2, **par})
    assert abs(o["loss"]) >= 0.05, o                        # (a relative bar needs a loss that is no near-cancellation)
    pk, _ = _run_packed_ppo(Ls, dict(), par)
    pk.select_seed(1)
    row = pk.ppo_stats(1)[0]
    print(f"packed learner 1: loss {row[0]:.6g} vs {o['loss']:.6g}, ent {row[1]:.6g} vs {o['ent']:.6g}, norms {row[2]:.6g} / "
          f"{row[3]:.6g} vs {o['grad_norm_pre']:.6g} / {o['grad_norm_post']:.6g}, alpha {row[4]:.6g} vs {o['alpha']:.6g}")
    werr = max(float(np.max(np.abs(x - y))) for x, y in zip(pk.get_net("actor"), ref.actor))
    werr = max(werr, float(np.max(np.abs(pk.v["actor.logstd"].cpu().numpy() - ref.logstd))))
    print(f"packed learner 1: actor weights after Adam max abs error {werr:.2e}")
    for got, key in ((row[0], "loss"), (row[1], "ent"), (row[2], "grad_norm_pre"), (row[3], "grad_norm_post"), (row[4], "alpha")):
        assert abs(got - o[key]) <= 2e-5 * abs(o[key]), (key, got, o[key])
    assert werr < 1e-6 and row[7] == 1
    pk.close()
    # the critic step
    vref = V.VState([[np.asarray(x, np.float64) for x in w] for w in L["crit"].critics[:nc]], None)
    vref.opt = O.AdamState.zeros_like(vref.trainables())
    vb = L["vidx"][0]
    vo = V.critic_step(vref, ACTS, L["nrm"], [x[vb] for x in L["vs"]], [x[vb] for x in L["vrtg"]], VC_LR[1])
    pk, _ = _run_packed_vc(Ls, nc)
    pk.select_seed(1)
    vrow = pk.vcritic_stats(1)[0]
    verr = max(float(np.max(np.abs(x - y))) for c in range(nc) for x, y in zip(pk.get_net(f"v{c}"), vref.critics[c]))
    print(f"packed learner 1: critic loss {vrow[0]:.6g} vs {vo['loss']:.6g}, weights after Adam max abs error {verr:.2e}")
    assert abs(vrow[0] - vo["loss"]) <= 2e-5 * abs(vo["loss"]) and vrow[9] == 1
    for c in range(nc):
        assert abs(vrow[1 + c] - vo["losses"][c]) <= 2e-5 * abs(vo["losses"][c]), c
    assert verr < 1e-6
    pk.close()


def _wm_engine(learners):
    from sac_eo.engine import Engine, EngineConfig
    return Engine(EngineConfig(s_dim=S, a_dim=2, hidden=HID, activation="tanh", critic_hidden=HID, batch=BATCH,
                               buffer_capacity=CAP, actor_gaussian="train", graph_steps=1, vcritics=1, learners=learners,
                               world_models=True, model_hidden=(16, 16), num_models=2, model_batch=8))


def _wm_pass(eng, L, models, rows, midx, seed):
    """The per-learner passes of one policy-update iteration on the selected learner."""
    give(eng, L, L["st"])
    for m, w in enumerate(models):
        eng.set_net(f"m{m}", w)
    eng.set_normalizers(L["nrm"].s_mean, L["nrm"].s_den, L["nrm"].a_mean, L["nrm"].a_den, L["nrm"].d_mean, L["nrm"].d_den,
                        0.3, 1.7, float(L["nrm"].ret_den))
    eng.rng_seed(seed)
    eng.append(*rows)
    out = {}
    sim = eng.sim_collect(0, 5, 2)
    out["sim"] = [t.cpu().numpy() for t in sim]
    s, a, r, sp, d, traj = sim
    out["gae"] = [t.cpu().numpy() for t in eng.gae(0, s, r, sp, d.float(), traj, 0.99, 0.95)]
    eng.ppo_begin(s, a, torch.as_tensor(out["gae"][0]))
    out["end"] = eng.ppo_end(0.2)
    eng.model_fit(midx)
    eng.sync()
    out["mstats"] = eng.model_stats(1)
    out["models"] = [w for m in range(2) for w in eng.get_net(f"m{m}")]
    out["rng"] = eng.rng_get_state()
    return out


def test_per_learner_passes_on_a_packed_world_models_engine(gpu_available):
    """ppo_begin / ppo_end, gae, sim_collect(0, 5, 2) and one model_fit step on learner 2 of a packed engine
    == the same calls on a one-learner engine holding learner 2's state, bit for bit."""
    Ls = [learner(k, 1, 5, nc=1) for k in range(K)]
    rng = np.random.RandomState(77)
    models = [[O.init_mlp(np.random.RandomState(60 + 5 * k + m), S + 2, S + 1, (16, 16), 0.3, 0.05) for m in range(2)]
              for k in range(K)]
    rows = [((rng.normal(size=(30, S)) * 1.5).astype(np.float32), rng.uniform(-1, 1, (30, 2)).astype(np.float32),
             rng.normal(size=30).astype(np.float32), (rng.normal(size=(30, S)) * 1.5).astype(np.float32),
             np.zeros(30, np.float32)) for _ in range(K)]
    midx = rng.randint(0, 30, (1, 2, 8)).astype(np.int32)
    pk = _wm_engine(K)
    outs = []
    for k in (1, 2):                                       # learner 1 first: its calls must leave learner 2 alone
        pk.select_seed(k)
        outs.append(_wm_pass(pk, Ls[k], models[k], rows[k], midx, seed=5 + k))
    one = _wm_engine(0)
    ref = _wm_pass(one, Ls[2], models[2], rows[2], midx, seed=7)
    got = outs[1]
    for x, y in zip(got["sim"] + got["gae"] + got["models"], ref["sim"] + ref["gae"] + ref["models"]):
        assert np.array_equal(x, y)
    _eq(got["end"], ref["end"])
    assert np.array_equal(got["mstats"], ref["mstats"])
    assert np.array_equal(got["rng"][1], ref["rng"][1]) and got["rng"][2:] == ref["rng"][2:]
    same_state(pk, 2, one, "world models")
    assert not np.array_equal(outs[0]["sim"][0], got["sim"][0])
    pk.close(), one.close()


def test_refusals_on_the_device(gpu_available):
    from sac_eo._native import SacxError
    Ls = [learner(k, 2, 5, nc=1) for k in range(K)]
    pk = make_engine(learners=K, vcritics=1)
    assert pk.lib.sacx_learners_init(pk.h, 2) != 0 and b"must precede sacx_bind" in pk.lib.sacx_last_error(pk.h)
    pidx, vidx = np.stack([L["idx"] for L in Ls]), np.stack([L["vidx"] for L in Ls])
    for k in (0, 1):
        pk.select_seed(k)
        ppo_prepare(pk, Ls[k])
        vc_prepare(pk, Ls[k])
    with pytest.raises(SacxError, match="learner 2 has no rollout table"):
        pk.ppo_steps_packed(pidx, actor_lr=1e-4, eps_ppo=0.2)
    with pytest.raises(SacxError, match="learner 2: critic 0 has no table"):
        pk.vcritic_steps_packed(vidx, critic_lr=1e-3)
    pk.select_seed(2)
    ppo_prepare(pk, Ls[2])
    vc_prepare(pk, Ls[2])
    # the one-learner calls on a packed engine raise, naming the packed call
    with pytest.raises(SacxError, match="sacx_ppo_steps_packed"):
        pk.ppo_steps(Ls[2]["idx"], actor_lr=1e-4, eps_ppo=0.2)
    with pytest.raises(SacxError, match="sacx_vcritic_steps_packed"):
        pk.vcritic_steps(Ls[2]["vidx"], critic_lr=1e-3)
    # each learner's indices are checked against ITS table: row 36 exists for learner 0 (37 rows), not for learner 2 (29)
    pk.sync()
    before = pk.arena_all.clone()
    bad = pidx.copy()
    bad[0, 0, 0] = 36
    bad[2, 1, 0] = 29
    with pytest.raises(SacxError, match="learner 2: minibatch index outside its rollout table"):
        pk.ppo_steps_packed(bad, actor_lr=1e-4, eps_ppo=0.2)
    vbad = vidx.copy()
    vbad[2, 0, 0] = 29
    with pytest.raises(SacxError, match="learner 2: minibatch index outside its shortest critic table"):
        pk.vcritic_steps_packed(vbad, critic_lr=1e-3)
    with pytest.raises(ValueError, match="learners = 3"):
        pk.ppo_steps_packed(pidx[:2], actor_lr=1e-4, eps_ppo=0.2)
    pk.sync()
    assert torch.equal(pk.arena_all, before)                # a refused call touches nothing
    ok = pidx.copy()
    ok[0, 0, 0] = 36
    pk.ppo_steps_packed(ok, actor_lr=1e-4, eps_ppo=0.2)
    pk.close()
    one = make_engine(vcritics=1)                           # the packed calls on a one-learner engine
    ppo_prepare(one, Ls[0])
    vc_prepare(one, Ls[0])
    with pytest.raises(SacxError, match="holds one learner"):
        one.ppo_steps_packed(pidx[:1], actor_lr=1e-4, eps_ppo=0.2)
    with pytest.raises(SacxError, match="holds one learner"):
        one.vcritic_steps_packed(vidx[:1], critic_lr=1e-3)
    one.close()
