"""alg_type bc on the device (``sacx_config.use_expert = SACX_EXPERT_BC``) against the oracle.

The BC update (reference ``sac_eo/algs/BC.py:309-363``) through ``Engine.step``: its generic plan
(any depth, layer norm; ``SACX_GENERIC=1`` at two layers) and its folded plan (two-layer nets), fp32
device against the fp64 ``bc_oracle.bc_update`` -- which tests/test_bc_oracle.py pins to the committed
oracle's ``sac_update`` at epsilon 1 -- at the project's bars (test_gpu_depth.py:94-112): the loss
within 2e-5, every actor gradient (through Adam's first moment) within 2e-4 of the tensor's max, the
weights after Adam within 1e-6, the device stream bit-equal to NumPy's after the update's draws (the
expert normals alone), and everything that is not the actor untouched bit for bit.  Then 60
graph-replayed updates, graph == eager == one update at a time, ``BC.train`` against
``BCLoopOracle``, and the plan's structure at the HalfCheetah shapes.

The device keeps ONE step counter (``ctl.t_sac``) for the critic / actor / alpha optimiser groups; under
BC it counts the actor's Adam steps (the only ones there are), so "the critics' step counters" have no
separate device value to compare: their weights and both moment ranges are compared byte for byte."""
import os

import numpy as np
import pytest

import edge_cases as EC
import helpers
import sac_oracle as O
import test_gpu_loop as L
from bc_oracle import BCLoopOracle, bc_sections, bc_update
from helpers import B1, make_pair, nontrivial_normalizers, relerr
from test_gpu_depth import _adam_grads, _same_stream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = {
    # halves of 6: a partial 16-row tile
    "base": dict(hidden=(64, 64), model_hidden=(96, 96), ne=12),
    # 17-row halves: one row past a tile
    "rows17": dict(hidden=(64, 64), model_hidden=(96, 96), ne=34),
    # odd row count, no permutation
    "one_model": dict(hidden=(64, 64), model_hidden=(96, 96), num_models=1, ne=11),
    # sections 7 / 7 / 6: 14 rows used, 14 A normals
    "three_models": dict(hidden=(64, 64), model_hidden=(96, 96), num_models=3, ne=20),
    # the advertised maximum: eight sections of 2 rows, every world model a problem of the model launches
    "eight_models": dict(hidden=(64, 64), model_hidden=(96, 96), num_models=8, ne=16),
    "deep": dict(hidden=(48, 64, 48), model_hidden=(64, 96, 64), ne=12),
    "layer_norm": dict(hidden=(64, 80, 48), model_hidden=(96, 96), ne=12, layer_norm=True),
    "pss_elu": dict(hidden=(64, 64, 64), model_hidden=(96, 96), ne=12, per_state_std=True, act="elu"),
    # a bound that clips some but not all of the models' delta columns (checked below)
    "delta_clip": dict(hidden=(64, 64), model_hidden=(96, 96), ne=12, delta_clip_pred=0.25),
    "model_normalizer": dict(hidden=(64, 64), model_hidden=(96, 96), ne=12, mnorm=True),
    "generic2": dict(hidden=(64, 64), model_hidden=(96, 96), ne=12, generic=True),
    # the folded plan with every fold (k_fwd2 pairs, folded head backward, folded finalisation)
    "hc": dict(hidden=(256, 256), model_hidden=(512, 512), ne=20, B=256),
    "hc_generic": dict(hidden=(256, 256), model_hidden=(512, 512), ne=20, B=256, generic=True),
    # the log-std variable below, at, inside and above its clip bounds [-5, 2] (tests/edge_cases.py): the
    # mask of the sample rows, with no entropy term beside it
    "lsvar": dict(hidden=(64, 64), model_hidden=(96, 96), ne=12, edge="lsvar"),
}


def _pair(monkeypatch, case, seed=0, **over):
    kw = dict(CASES[case])
    kw.update(over)
    generic = kw.pop("generic", False)
    mnorm = kw.pop("mnorm", False)
    edge = kw.pop("edge", None)
    if edge:                               # make_pair resolves make_learner through its module
        monkeypatch.setattr(helpers, "make_learner", EC.mutating(helpers.make_learner, EC.split(edge)[0]))
    kw.setdefault("act", "relu")
    kw.setdefault("B", 64)
    if generic:
        monkeypatch.setenv("SACX_GENERIC", "1")
    eng, ocfg, st, buf, nrm, expert = make_pair(seed=seed, use_expert=True, bc=True, epsilon=1.0, normalizers="random",
                                                **kw)
    monkeypatch.delenv("SACX_GENERIC", raising=False)
    ocfg.delta_clip_pred = kw.get("delta_clip_pred", 0.0)
    mn = None
    if mnorm:                              # --only_model_normalizer: the models on their own statistics
        mn = nontrivial_normalizers(np.random.RandomState(seed + 300), ocfg.S, ocfg.A)
        eng.set_normalizers(mn.s_mean, mn.s_den, mn.a_mean, mn.a_den, mn.d_mean, mn.d_den, mn.r_mean, mn.r_den,
                            which="model")
    return eng, ocfg, st, nrm, mn, expert


def _draw(rs, gen, expert, nm, A):
    """One update's randoms in the reference's order: the permutation (Generator; 2+ models), then the
    sections' normals from the global stream.  Returns (perm, halves)."""
    perm = np.arange(len(expert["s"]))
    if nm > 1:
        gen.shuffle(perm)
    halves = [(expert["s"][sec], expert["sp"][sec], O.f32_noise(rs.normal(size=(len(sec), A))))
              for sec in bc_sections(perm, nm)]
    return perm, halves


def _others(eng):
    """Bytes of everything trainable that is not the actor: weights and both Adam moment ranges of the
    critics, targets, alpha and the world models."""
    out = []
    for name, seg in eng.segments.items():
        if seg["role"] not in (1, 2) or name.startswith("actor") or name == "params":
            continue
        off, n = seg["offset"] // 4, seg["rows"] * seg["cols"]
        for blk in ("params", "adam_m", "adam_v"):
            out.append((f"{blk}:{name}", eng.v[blk][0][off: off + n].cpu().numpy().copy()))
    return out


def _moment(eng, name):
    seg = eng.segments[name]
    off, n = seg["offset"] // 4, seg["rows"] * seg["cols"]
    return eng.v["adam_m"][0][off: off + n].cpu().numpy().reshape(seg["rows"], seg["cols"]) / B1


def _chain(eng):
    return [l for l in eng.plan_info() if l["name"] not in ("rng", "gather")]


@pytest.mark.parametrize("case", list(CASES))
def test_bc_one_update(gpu_available, monkeypatch, case):
    eng, ocfg, st, nrm, mn, expert = _pair(monkeypatch, case, seed=3)
    nm, A = eng.cfg.num_models, ocfg.A
    rs, gen = np.random.RandomState(17), np.random.default_rng(4)
    eng.rng_set_state(rs.get_state())
    perm, halves = _draw(rs, gen, expert, nm, A)
    if nm > 1:
        eng.push_perms(perm[None])
    before = _others(eng)
    ctl0 = eng.ctl()
    alpha0 = eng.alpha()
    keep = {}
    ls0 = st.logstd.copy()
    edge = "edge" in CASES[case]
    if edge:                               # the update must write its rows of the mask: none of them holds 7
        eng.v["ws.c_mask"].fill_(7.0)
        torch.cuda.synchronize()           # the fill runs on torch's stream, the update on the engine's
    ref = bc_update(st, ocfg, nrm, halves, mn, keep=keep)
    if ocfg.delta_clip_pred:               # the case's premise: some columns clipped, not all
        frac = _clip_fraction(st, ocfg, nrm, halves)
        assert 0.05 < frac < 0.95, frac
    eng.step(1, eager=True)
    eng.sync()
    row = eng.stats(1)[0]
    print(f"{case}: {[l['name'] for l in _chain(eng)]}; mse {row[5]:.6g} vs {ref['mse_loss']:.6g}")
    for col in (5, 2):                      # SACX_STAT_MSE_LOSS, SACX_STAT_P_LOSS
        assert abs(row[col] - ref["mse_loss"]) <= 2e-5 * abs(ref["mse_loss"]), (col, row[col], ref["mse_loss"])
    assert row[0] == row[1] == row[3] == row[6] == 0.0
    assert row[4] == np.float32(alpha0) and row[7] == float(ctl0["step_seq"])
    assert _same_stream(eng, rs)
    ctl1 = eng.ctl()
    assert ctl1["step_seq"] == ctl0["step_seq"] + 1 and ctl1["t_sac"] == ctl0["t_sac"] + 1
    assert ctl1["num_timesteps"] == 1 and ctl1["t_model"] == ctl0["t_model"]
    # gradients, read back through Adam's first moment
    ga = _adam_grads(eng, "actor", None)
    go = list(keep["actor_grads"])
    if ocfg.layer_norm:                    # the oracle's list carries gamma / beta after b0
        gb = _moment(eng, "actor.ln")
        for i in range(2):
            assert relerr(gb[i], go[2 + i]) < 2e-4, ("actor.ln", i, relerr(gb[i], go[2 + i]))
        go = go[:2] + go[4:]
    assert len(ga) == len(go)
    for i, (gd, gr) in enumerate(zip(ga, go)):
        assert relerr(gd, gr) < 2e-4, ("actor", i, relerr(gd, gr))
    if not ocfg.per_state_std:
        assert relerr(_moment(eng, "actor.logstd"), keep["g_logstd"]) < 2e-4
    # weights after Adam
    for a_, b_ in zip(eng.get_net("actor"), st.actor):
        assert np.max(np.abs(a_ - b_)) < 1e-6
    assert np.max(np.abs(eng.v["actor.logstd"].cpu().numpy() - st.logstd)) < 1e-6
    if edge:
        # the sample rows' clip mask (the update's rows of ws.c_mask, wherever the plan keeps them) equal to the
        # oracle's; the masked coordinates of the log-std variable: gradient exactly 0, not moved by Adam
        mask = np.concatenate([h.mask for h in keep["heads"]], 0)
        masked = EC.clip_mask(ls0[0]) == 0
        assert (mask == 0).any() and (mask == 1).any() and masked.any() and not masked.all()
        dev = eng.v["ws.c_mask"].cpu().numpy()
        rows = np.where((dev != 7.0).any(axis=1))[0]
        assert len(rows) == len(mask) and np.array_equal(rows, rows[0] + np.arange(len(mask))), rows
        assert np.array_equal(dev[rows], mask), (dev[rows], mask)
        gl = _moment(eng, "actor.logstd")[0]
        assert np.all(gl[masked] == 0.0) and np.all(keep["g_logstd"][0][masked] == 0.0), gl
        assert np.all(gl[~masked] != 0.0), gl
        ls = eng.v["actor.logstd"].cpu().numpy().reshape(-1)
        assert np.array_equal(ls[masked], ls0[0][masked].astype(np.float32)), (ls, ls0)
        print(f"{case}: mask rows {rows[0]}..{rows[-1]}, zeros {int((mask == 0).sum())} of {mask.size}; g_logstd {gl} "
              f"error {relerr(gl, keep['g_logstd'][0]):.2e} (held to 2e-4 by the comparison above)")
    # critics, targets, alpha, world models: weights and moments byte for byte
    for (name, x), (_, y) in zip(before, _others(eng)):
        assert np.array_equal(x, y), name
    eng.close()


def _clip_fraction(st, ocfg, nrm, halves):
    """Fraction of the models' delta columns outside [-c, c] at the state the update starts from
    (recomputed from the post-update actor: one Adam step of 1e-4 does not move it)."""
    n, tot = 0, 0
    for k, (se, spe, u) in enumerate(halves):
        nn = nrm.cast(np.float64)
        x = (se - nn.s_mean) / nn.s_den
        out, _ = O.actor_forward(st.actor, x, ocfg)
        mu, ls = O.split_head(out, st.logstd, ocfg)
        a, _ = O.head_sample(mu, ls, np.asarray(u, np.float64), ocfg.act_limit, np.float64)
        om, _ = O.mlp_forward(st.models[k], np.concatenate([x, (a - nn.a_mean) / nn.a_den], 1), ocfg.model_act)
        n += int((np.abs(om[:, :ocfg.S]) > ocfg.delta_clip_pred).sum())
        tot += om[:, :ocfg.S].size
    return n / tot


@pytest.mark.parametrize("case", ["base", "deep"])
def test_bc_trajectory(gpu_available, monkeypatch, case):
    """60 graph-replayed updates (graphs of 8, the sampler forked ahead, the permutations pushed ahead)
    against 60 oracle updates: the MSE series within 1e-4 of its scale, the stream bit-exact at the end."""
    eng, ocfg, st, nrm, mn, expert = _pair(monkeypatch, case, seed=11)
    nm, A = eng.cfg.num_models, ocfg.A
    rs, gen = np.random.RandomState(123), np.random.default_rng(77)
    eng.rng_set_state(rs.get_state())
    steps = 60
    draws = [_draw(rs, gen, expert, nm, A) for _ in range(steps)]
    eng.push_perms(np.stack([p for p, _ in draws]))
    eng.step(steps)
    eng.sync()
    dev = eng.stats(steps)
    ref = np.array([bc_update(st, ocfg, nrm, h, mn)["mse_loss"] for _, h in draws])
    err = L._series_err(dev[:, 5], ref)
    print(f"{case}: MSE series error {err:.2e}")
    assert err < L.LOSS_TOL, err
    assert np.array_equal(dev[:, 5], dev[:, 2]) and np.array_equal(dev[:, 7], np.arange(steps, dtype=np.float32))
    assert _same_stream(eng, rs)
    assert eng.ctl()["t_sac"] == steps
    eng.close()


def _actor_bytes(eng):
    out = []
    for name, seg in eng.segments.items():
        if name.startswith("actor") and seg["role"] == 1:
            off, n = seg["offset"] // 4, seg["rows"] * seg["cols"]
            out += [eng.v[blk][0][off: off + n].cpu().numpy().copy() for blk in ("params", "adam_m", "adam_v")]
    return out


@pytest.mark.parametrize("case", ["base", "hc", "layer_norm"])
def test_bc_replay_identity(gpu_available, monkeypatch, case):
    """Graph replay == eager, and step(5) == five step(1): the actor range (weights and moments) and
    the statistics rows byte for byte."""
    n = 5
    outs = []
    for mode in ("eager", "graph", "ones"):
        eng, ocfg, st, nrm, mn, expert = _pair(monkeypatch, case, seed=21)
        eng.rng_set_state(np.random.RandomState(5).get_state())
        prs = np.random.RandomState(8)
        eng.push_perms(np.stack([prs.permutation(eng.cfg.expert_batch) for _ in range(n)]))
        if mode == "ones":
            for i in range(n):
                eng.step(1, num_timesteps=i)
        else:
            eng.step(n, eager=mode == "eager")
        eng.sync()
        outs.append((eng.stats(n).copy(), _actor_bytes(eng), eng.rng_get_state()))
        eng.close()
    for other in outs[1:]:
        assert np.array_equal(outs[0][0], other[0])
        for x, y in zip(outs[0][1], other[1]):
            assert np.array_equal(x, y)
        assert L._same_stream(outs[0][2], other[2])
    assert np.all(outs[0][0][:, 5] > 0)


def test_bc_plan_structure(gpu_available, monkeypatch):
    """At the HalfCheetah shapes (S 17, A 6, actor 256 x 2, models 512 x 2, 20 expert rows): no launch
    named for a critic, target or alpha; strictly fewer chain launches than the SAC-EO plan at the same
    shapes, and at most 9; the forced generic plan keeps every head on its row kernel."""
    bc, *_ = _pair(monkeypatch, "hc")
    eo, *_ = make_pair(hidden=(256, 256), model_hidden=(512, 512), ne=20, B=256, use_expert=True,
                       normalizers="random")
    gen, *_ = _pair(monkeypatch, "hc_generic")
    chain, chain_eo, chain_gen = _chain(bc), _chain(eo), _chain(gen)
    names = [l["name"] for l in chain]
    print("bc:", names, "\neo:", [l["name"] for l in chain_eo], "\ngeneric:", [l["name"] for l in chain_gen])
    for plan in (chain, chain_gen):
        for l in plan:
            parts = l["name"].replace("+", ".").split(".")
            assert not {"q", "q0", "q1", "t0", "t1", "critic", "pi", "alpha", "target"} & set(parts), l["name"]
            assert l["kernel"] not in ("k_qhead", "k_alpha_final"), l
    assert len(chain) < len(chain_eo), (len(chain), len(chain_eo))
    assert len(chain) <= 9, names
    assert [l["name"] for l in bc.plan_info()][:2] == ["rng", "gather"]
    # generic: one launch per layer and direction, the three heads on row kernels
    kern = [l["kernel"] for l in chain_gen]
    assert kern.count("k_actor_head") == 1 and kern.count("k_actor_bwd") == 1 and kern.count("k_bc_final") == 1
    assert all("+" not in l["name"] for l in chain_gen)
    assert len(chain_gen) > len(chain)
    for e in (bc, eo, gen):
        e.close()


# ------------------------------------------------------------------------------ the training loop
def _run_bc(flags):
    alg_obj, d, ak, total, oenvs, rs_state = L._build("bc", flags)
    S, A = alg_obj.s_dim, alg_obj.a_dim
    mk, msk = d["model_kwargs"], d["model_setup_kwargs"]
    ocfg = O.Config(S=S, A=A, hidden=tuple(d["actor_kwargs"]["actor_layers"]), act="relu", B=L.SMALL["B"],
                    gamma=ak["gamma"], tau=ak["soft_tau"], lr_q=ak["q_crit_lr"], lr_pi=ak["mbpo_actor_lr"],
                    lr_alpha=ak["mbpo_alpha_lr"], init_temperature=ak["init_temperature"], epsilon=ak["epsilon"],
                    model_hidden=tuple(mk["model_layers"]), num_models=int(mk["num_models"]), model_act="relu",
                    lr_model=ak["model_lr"], reward_loss_coef=msk["reward_loss_coef"],
                    critic_hidden=tuple(d["critic_kwargs"]["critic_layers"]))
    st = L._oracle_state(alg_obj, ocfg)
    ex = alg_obj.expert.get_weights()
    expert = ([np.asarray(w, np.float64) for w in ex[:-1]], np.asarray(ex[-1], np.float64))
    dev_rng = []
    hook = alg_obj._episode_normalizer_update

    def rec(episode):
        dev_rng.append(alg_obj.engine.rng_get_state())
        return hook(episode)
    alg_obj._episode_normalizer_update = rec
    name = alg_obj.train(total, d)
    dev_rng.append(alg_obj.engine.rng_get_state())
    n_upd = alg_obj.engine.ctl()["step_seq"]
    dev = alg_obj.engine.stats(n_upd)
    orc = BCLoopOracle(ocfg, st, oenvs[0], oenvs[2], expert, dict(ak, num_models=mk["num_models"]), rs_state,
                       ak["alg_seed"], max_episode_steps=1000).train(total)
    return alg_obj, ak, name, dev, dev_rng, orc


@pytest.mark.parametrize("flags", [
    [],
    ["--update_normalizers", "--only_model_normalizer"],
    ["--num_models", "1"],
    ["--num_models", "3"],
    ["--expert_batch_size", "12"],
])
def test_bc_train_loop_matches_oracle(gpu_available, flags):
    """BC.train on the device against BCLoopOracle: every update's BC_MSE_loss, the global stream bit
    for bit at every episode boundary (a stray speculative draw would move it), the per-episode expert
    diagnostics and the last model-fit loss."""
    from sac_eo.algs import BC
    from sac_eo.common.logger import load_log
    alg_obj, ak, name, dev, dev_rng, orc = _run_bc(flags)
    assert type(alg_obj) is BC
    ref = np.array([u["mse_loss"] for u in orc.update_stats])
    assert dev.shape[0] == ref.shape[0] == L.SMALL["episodes"] * L.SMALL["ep_len"]
    err = L._series_err(dev[:, 5], ref)
    assert len(dev_rng) == len(orc.episode_rng)
    for i, (a, b) in enumerate(zip(dev_rng, orc.episode_rng)):
        assert L._same_stream(a, b), f"global stream differs at episode boundary {i}"
    log = load_log(os.path.join(ak["save_path"], name))
    os.remove(os.path.join(ak["save_path"], name))
    tr = log["train"]
    assert np.array_equal(np.asarray(tr["BC_MSE_loss"], np.float32), dev[:, 5])
    for k in ("alpha_loss", "p_loss", "epsilon"):
        assert k not in tr
    od = np.array(orc.diag)
    dd = np.stack([np.asarray(tr["model_MSE_on_expert_data"], np.float64),
                   np.asarray(tr["model_MSE_on_expert_counterfactual_action"], np.float64)], 1)
    ml = np.asarray(tr["model_loss_last"], np.float64)
    print(f"bc {flags}: {dev.shape[0]} updates, MSE series error {err:.2e}, diagnostics "
          f"{L._rel_drift(dd, od[:, :2]):.2e}, fit loss {L._rel_drift(ml, np.array(orc.fit_last)):.2e}")
    assert err < L.LOSS_TOL, err
    np.testing.assert_allclose(dd, od[:, :2], rtol=L.LOSS_TOL)
    np.testing.assert_allclose(ml, np.array(orc.fit_last), rtol=L.LOSS_TOL)
    if "--update_normalizers" in flags:
        for kk in ("s_rms", "delta_rms"):
            a, b = getattr(alg_obj.model_normalizer, kk), getattr(orc.model_normalizer, kk)
            assert a.t_last == b.t_last
            np.testing.assert_allclose(np.asarray(a.mean, np.float64), np.asarray(b.mean, np.float64), rtol=1e-5,
                                       atol=1e-6)
    alg_obj.engine.close()
