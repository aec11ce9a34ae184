#!/usr/bin/env python3
"""Bit-identity of two libsacx builds: plans, arenas and returned values, case by case.

A host-side change of sacx.cpp (the plan builders, the graph capture, the inference paths) must leave every
launch table and every computed bit as the parent commit's library has them.  For each named case this runs,
in a fresh child process against the library SACX_LIBPATH names (default: the in-tree build), a fixed-seed
learner with a fixed NumPy stream state and pushed permutations, and prints one line:

  case <name> plan=<sha256 of the plan_info listing: name, kernel, grid, block, flops, bytes>:<launches>
       arena=<sha256 of the whole arena after the steps> out=<sha256 of the returned values>

The cases (CASES) by family: fused.* / generic.* / bc.* the SAC-family update plans; act.*, evaluate, rollout.*,
expert_diag* and critic_forward, srn.* the inference paths (srn.*: on a handle with reward nets); dp.* the
data-parallel split; fit.* the world-model fit (plan = model_plan_info); ppo.*, vc.*, trpo.* the on-policy plans of a
trainable GaussianActor / SoftMaxActor handle (plan = ppo_plan_info / vcritic_plan_info / trpo_plan_info).

  SACX_LIBPATH=tools/libvar/libsacx_parent.so python tools/plan_identity.py run > parent.txt
  python tools/plan_identity.py run > new.txt
  python tools/plan_identity.py compare parent.txt new.txt       # EQUAL / DIFF per case; exit 1 on a DIFF
  python tools/plan_identity.py list

Each child runs under its own time limit (--timeout, seconds) and the parent stops at the first child that
fails.  Run a library twice before comparing: a case whose arena differs between two runs of the same library
is not run-to-run deterministic and shows nothing.  tools/build_variant.sh builds the parent's library.
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("sac-expert_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

OFF = {"SACX_HEAD_PART": "0", "SACX_FOLD_HBW": "0"}
EO = dict(use_expert=True, ne=12, model_hidden=(128, 96))      # Hm0 % 64 == 0: the hbw fold takes the expert rows too
PACK = {"SACX_T32": "2"}          # what the packed test sets where the handle's own choice depends on the device
GAUSS = dict(gaussian_model=True, scale_model_loss=True)
SRN = dict(separate_reward_nn=True, reward_hidden=(64, 48), reward_act="elu")
CASES = {
    # ---- the fused plan, plain SAC: B = 64, hidden (64, 64) -- head fold, head partials and hbw fold on
    "fused.base": dict(kind="sac"),
    "fused.nofusehead": dict(kind="sac", env={"SACX_FUSE_HEAD": "0"}),
    "fused.nofolds": dict(kind="sac", env=OFF),
    "fused.nofwd2": dict(kind="sac", env={"SACX_FWD2": "0"}),
    "fused.h96x80": dict(kind="sac", kw=dict(hidden=(96, 80))),                      # H1 % 64 != 0
    "fused.critic128x64": dict(kind="sac", kw=dict(wm=dict(critic_hidden=(128, 64)))),   # Hc != H
    "fused.pss": dict(kind="sac", kw=dict(per_state_std=True)),                      # Aout = 12 > 8
    "fused.ln": dict(kind="sac", kw=dict(layer_norm=True)),
    "fused.seeds4": dict(kind="sac", kw=dict(seeds=4)),
    "fused.seeds8": dict(kind="sac", kw=dict(seeds=8)),
    "fused.seeds8.t32": dict(kind="sac", kw=dict(seeds=8), env=PACK),
    "fused.bf16.xbf2": dict(kind="sac", kw=dict(B=128, gemm_bf16=True), env={"SACX_T32": "1", "SACX_WBF": "1", "SACX_XBF": "2"}),
    "fused.bf16.xbf1": dict(kind="sac", kw=dict(B=128, gemm_bf16=True), env={"SACX_T32": "1", "SACX_WBF": "1", "SACX_XBF": "1"}),
    # ---- the fused plan, SAC-EO
    "fused.eo.nm1": dict(kind="sac", kw=dict(EO, num_models=1)),
    "fused.eo.nm2": dict(kind="sac", kw=dict(EO, num_models=2)),
    "fused.eo.nm3": dict(kind="sac", kw=dict(EO, num_models=3)),
    "fused.eo.nofusehead": dict(kind="sac", kw=EO, env={"SACX_FUSE_HEAD": "0"}),
    "fused.eo.nofoldhbw": dict(kind="sac", kw=EO, env={"SACX_FOLD_HBW": "0"}),
    "fused.eo.m96x64": dict(kind="sac", kw=dict(EO, model_hidden=(96, 64))),             # the fold off by shape
    "fused.eo.ln": dict(kind="sac", kw=dict(EO, layer_norm=True)),
    "fused.eo.dclip": dict(kind="sac", kw=dict(EO, delta_clip_pred=0.25)),
    # ---- the generic plan: tests/test_gpu_depth.py's cases
    "generic.actor1": dict(kind="sac", kw=dict(hidden=(112,))),
    "generic.actor3": dict(kind="sac", kw=dict(hidden=(96, 64, 80))),
    "generic.critic1": dict(kind="sac", kw=dict(wm=dict(critic_hidden=(96,)))),
    "generic.all4": dict(kind="sac", kw=dict(hidden=(64, 48, 48, 32), wm=dict(critic_hidden=(64, 64, 32, 48)), act="tanh")),
    "generic.ln3": dict(kind="sac", kw=dict(hidden=(64, 80, 48), layer_norm=True)),
    "generic.pss3": dict(kind="sac", kw=dict(hidden=(64, 64, 64), per_state_std=True, act="elu")),
    "generic.generic2": dict(kind="sac", kw=dict(hidden=(96, 64)), env={"SACX_GENERIC": "1"}),
    "generic.eo_models1": dict(kind="sac", kw=dict(hidden=(64, 64, 64), use_expert=True, ne=12, model_hidden=(128,))),
    "generic.eo_models3": dict(kind="sac", kw=dict(use_expert=True, ne=12, model_hidden=(96, 64, 80))),
    "generic.eo_generic2": dict(kind="sac", kw=dict(use_expert=True, ne=12, model_hidden=(96, 128)), env={"SACX_GENERIC": "1"}),
    "generic.eo_nm4_deep": dict(kind="sac", kw=dict(hidden=(48, 64, 48), use_expert=True, model_hidden=(64, 96, 64), num_models=4,
                                                    ne=16, wm=dict(critic_hidden=(64, 32, 64)))),
    # ---- BC
    "bc.folded2": dict(kind="sac", kw=dict(EO, bc=True, epsilon=1.0)),
    "bc.generic3": dict(kind="sac", kw=dict(EO, bc=True, epsilon=1.0, hidden=(48, 64, 48), model_hidden=(64, 96, 64))),
    "bc.ln2": dict(kind="sac", kw=dict(EO, bc=True, epsilon=1.0, layer_norm=True)),
    "bc.generic2.one_model": dict(kind="sac", kw=dict(EO, bc=True, epsilon=1.0, num_models=1, ne=11), env={"SACX_GENERIC": "1"}),
    # ---- the inference paths on the HeadArgs builder (40 rows: past the one-workgroup-per-row kernel)
    "act.squashed.stochastic": dict(kind="act", det=False),
    "act.squashed.deterministic": dict(kind="act", det=True),
    "act.gaussian.stochastic": dict(kind="act", det=False, gaussian=True),
    "act.gaussian.deterministic": dict(kind="act", det=True, gaussian=True),
    "evaluate": dict(kind="evaluate"),
    "rollout.h3.n8": dict(kind="rollout"),
    "expert_diag": dict(kind="diag"),
    # ---- the data-parallel split (dp_split_adam): two in-process ranks on one device
    "dp.fused": dict(kind="dp"),
    "dp.generic": dict(kind="dp", kw=dict(hidden=(96, 64, 80))),
    # ---- the world-model fit (build_model_plan): 2 eager steps, then 3 graph-replayed ones, 40 rows per model;
    #      plan = model_plan_info
    "fit.mse.nm2": dict(kind="fit"),
    "fit.gauss": dict(kind="fit", kw=dict(wm=GAUSS)),
    "fit.srn.nm2": dict(kind="fit", kw=dict(wm=SRN)),
    "fit.srn.nm5": dict(kind="fit", kw=dict(wm=SRN, num_models=5)),                       # 10 problems: the split levels
    "fit.srn.m3r1": dict(kind="fit", kw=dict(model_hidden=(64, 48, 64), wm=dict(SRN, reward_hidden=(64,)))),   # Lf != Dr
    "fit.srn.m1r3": dict(kind="fit", kw=dict(model_hidden=(64,), wm=dict(SRN, reward_hidden=(64, 48, 64)))),   # Lf != Dm
    "fit.clip.mse": dict(kind="fit", kw=dict(model_max_grad_norm=0.05)),
    "fit.clip.gauss": dict(kind="fit", kw=dict(model_max_grad_norm=0.05, wm=GAUSS)),
    "fit.nopre": dict(kind="fit", env={"SACX_MPRE": "0"}),                                # the gather folded: model.gather+fwd01
    "fit.nofuse": dict(kind="fit", env={"SACX_MFUSE": "0"}),
    "fit.mtile0": dict(kind="fit", env={"SACX_MTILE": "0"}),
    "fit.mtile2": dict(kind="fit", env={"SACX_MTILE": "2"}),
    "fit.mt32all": dict(kind="fit", env={"SACX_MT32": "15"}),
    "fit.seeds2": dict(kind="fit", kw=dict(seeds=2)),
    # ---- the on-policy plans on a trainable GaussianActor handle (S = 17, A = 6, 64 x 64, tanh): 2 eager steps
    #      of 33 rows, then 3 graph-replayed ones; neglogp and dist on 40 rows
    "ppo.plain": dict(kind="ppo"),
    "ppo.ln": dict(kind="ppo", cfg=dict(layer_norm=True)),
    "ppo.pss": dict(kind="ppo", cfg=dict(per_state_std=True)),
    "ppo.softmax": dict(kind="ppo", softmax=True),
    "ppo.learners2": dict(kind="ppo", learners=2),
    "vc.nc1": dict(kind="vc", nc=1),
    "vc.nc2": dict(kind="vc", nc=2),
    "vc.nc1.h3": dict(kind="vc", nc=1, hidden=(64, 48, 64)),
    # TRPO on a table of one chunk + 5 rows (`first` / `last` of a chunk differ): gradient, one Fisher product, a step
    "trpo.plain": dict(kind="trpo"),
    "trpo.ln": dict(kind="trpo", cfg=dict(layer_norm=True)),
    "trpo.softmax": dict(kind="trpo", softmax=True),
    # ---- the eager net passes: sacx_critic_forward, model_gemms with reward nets / with 3 models
    "critic_forward": dict(kind="critic"),
    "srn.model_forward": dict(kind="model_forward", kw=dict(wm=SRN)),
    "srn.rollout.h3.n8": dict(kind="rollout", kw=dict(wm=SRN)),
    "srn.expert_diag": dict(kind="diag", kw=dict(wm=SRN)),
    "expert_diag.nm3": dict(kind="diag", kw=dict(num_models=3)),
}


def sha(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def plan_sha(plan):
    txt = "\n".join(f"{l['name']} {l['kernel']} {l['grid']} {l['block']} {l['flops']!r} {l['bytes']!r}" for l in plan)
    return f"{hashlib.sha256(txt.encode()).hexdigest()[:16]}:{len(plan)}"


def child(name):
    import numpy as np
    from helpers import load_learner, make_learner, make_pair
    c = CASES[name]
    kind = c["kind"]
    kw = dict(B=64, hidden=(64, 64), act="relu", seed=3, normalizers="random", N=2000, done_p=0.02)
    kw.update(c.get("kw", {}))
    outs, plan = [], None
    if kind == "sac":
        n0, n1 = 3, 20
        eng, ocfg, st, buf, nrm, expert = make_pair(**kw)
        K = int(kw.get("seeds", 1))
        for k in range(K):
            eng.select_seed(k)
            if k > 0:               # the other packed seeds: their own learners
                lk = {a: kw[a] for a in ("hidden", "B", "act", "N", "normalizers", "done_p") if a in kw}
                _, stk, bufk, nrmk, exk = make_learner(seed=kw["seed"] + 7 * k, **lk)
                load_learner(eng, stk, bufk, nrmk, exk, 0.1)
            eng.rng_set_state(np.random.RandomState(17 + k).get_state())
            if expert is not None and eng.cfg.num_models > 1:
                rs = np.random.RandomState(900 + k)
                eng.push_perms(np.stack([rs.permutation(eng.cfg.expert_batch) for _ in range(n0 + n1)]))
        eng.select_seed(0)
        eng.step(n0, eager=True)    # eager, then graphs with the alpha branch merged into the next update
        eng.step(n1)
        eng.sync()
        for k in range(K):
            eng.select_seed(k)
            outs.append(eng.stats(n0 + n1))
        engs = [eng]
    elif kind == "dp":
        import torch
        from sac_eo.engine import Engine, EngineConfig
        B = kw["B"]
        ocfg, st, buf, nrm, _ = make_learner(hidden=kw["hidden"], B=B, act=kw["act"], N=kw["N"], seed=kw["seed"],
                                             normalizers=kw["normalizers"], done_p=kw["done_p"])
        stream = torch.cuda.current_stream()
        engs = []
        for r in range(2):
            e = Engine(EngineConfig(s_dim=17, a_dim=6, hidden=kw["hidden"], activation=kw["act"], batch=B // 2,
                                    buffer_capacity=kw["N"], graph_steps=8), stream=stream, dp_local=(2, r))
            load_learner(e, st, buf, nrm, None, 0.1)
            e.rng_set_state(np.random.RandomState(900 + r).get_state())
            engs.append(e)
        Engine.dp_local_step(engs, 23, num_timesteps=0, ts_increment=1)
        for e in engs:
            e.sync()
            outs.append(e.stats(23))
        eng = engs[0]
    elif kind == "fit":
        nm, mb, K = int(kw.get("num_models", 2)), 40, int(kw.get("seeds", 1))
        kw = dict(dict(use_expert=True, ne=12, model_hidden=(64, 64), model_batch=mb), **kw)
        eng, ocfg, st, buf, nrm, expert = make_pair(**kw)
        idx = np.random.RandomState(13).randint(kw["N"], size=(K, 5, nm, mb))
        for k in range(K):
            eng.select_seed(k)
            if k > 0:
                _, stk, bufk, nrmk, exk = make_learner(**dict({a: v for a, v in kw.items() if a not in ("seeds", "model_batch",
                                                       "model_max_grad_norm")}, seed=kw["seed"] + 7 * k))
                load_learner(eng, stk, bufk, nrmk, exk, 0.1)
            eng.model_fit(idx[k, :2], eager=True)
            eng.model_fit(idx[k, 2:])
            eng.sync()
            outs.append(eng.model_stats(5))
        plan = eng.model_plan_info()
        engs = [eng]
    elif kind in ("ppo", "vc", "trpo"):
        plan, engs = onpolicy(c, outs)
    else:
        from sac_eo.engine import Engine, EngineConfig
        import sac_oracle as O
        if c.get("gaussian"):       # the plain GaussianActor: inference only, std_mult and output norm set
            S, A = 11, 3
            ocfg = O.Config(S=S, A=A, hidden=(64, 64), act="tanh", per_state_std=True)
            st = O.init_state(ocfg, seed=8, bias_scale=0.2, actor_gain=2.0)
            eng = Engine(EngineConfig(s_dim=S, a_dim=A, hidden=(64, 64), activation="tanh", batch=1, buffer_capacity=1,
                                      per_state_std=True, graph_steps=1, actor_gaussian=True, actor_std_mult=0.6,
                                      actor_output_norm=True))
            eng.set_net("actor", st.actor)
            eng.set_logstd(np.full((1, A), -0.7, np.float32))
        else:
            eng, ocfg, st, buf, nrm, expert = make_pair(**dict(kw, **EO))
        S, A = ocfg.S, ocfg.A
        r = np.random.RandomState(9)
        eng.rng_set_state(np.random.RandomState(29).get_state())
        if kind == "act":
            obs = (r.normal(size=(40, S)) * 2).astype(np.float32)
            outs.append(eng.act(obs, deterministic=c["det"]).cpu().numpy())
        elif kind == "evaluate":
            outs += [t.cpu().numpy() for t in eng.evaluate((r.normal(size=(40, S)) * 2).astype(np.float32))]
        elif kind == "critic":
            obs, act = (r.normal(size=(40, S)) * 2).astype(np.float32), r.uniform(-1, 1, (40, A)).astype(np.float32)
            for i, net in enumerate(("q0", "q1", "t0", "t1")):
                outs.append(eng.critic_forward(net, obs, act, value=bool(i & 1)).cpu().numpy())
        elif kind == "model_forward":
            obs, act = (r.normal(size=(40, S)) * 2).astype(np.float32), r.uniform(-1, 1, (40, A)).astype(np.float32)
            for k in range(2):
                outs += [t.cpu().numpy() for t in eng.model_forward(k, obs, act, 0.05, 0.3)]
        elif kind == "rollout":
            outs += [t.cpu().numpy() for t in eng.rollout(1, (r.normal(size=(8, S)) * 1.5).astype(np.float32), 3, False)]
        else:
            s_e = (r.normal(size=(40, S)) * 2).astype(np.float32)
            a_e = r.uniform(-1, 1, (40, A)).astype(np.float32)
            sp_e = (s_e + r.normal(size=(40, S)) * 0.1).astype(np.float32)
            for disc in (False, True):
                d = eng.expert_diag(s_e, a_e, sp_e, disc=disc)
                outs += [np.asarray(d[k], np.float64) for k in sorted(d)]
        eng.sync()
        outs.append(eng.rng_get_state()[1])
        engs = [eng]
    arena = sha(*[e.arena_all.cpu().numpy() for e in engs])
    print(f"case {name} plan={plan_sha(plan if plan is not None else engs[0].plan_info())} arena={arena} out={sha(*outs)}", flush=True)
    for e in engs:
        e.close()


def onpolicy(c, outs):
    """The PPO step, the VCritic step and the TRPO update of a trainable GaussianActor / SoftMaxActor handle: fills
    `outs`, returns (the family's plan_info listing, [engine])."""
    import numpy as np
    import ppo_ref as R
    import sac_oracle as O
    import vcritic_ref as V
    from helpers import nontrivial_normalizers
    from sac_eo.engine import Engine, EngineConfig
    kind, S, A, mb = c["kind"], 17, 6, 33
    soft, K, nc = bool(c.get("softmax")), int(c.get("learners", 0)), int(c.get("nc", 0))
    chid = tuple(c.get("hidden", (64, 64)))
    n = 50                                               # table rows (TRPO: set below, from the engine's chunk)
    cfg = O.Config(S=S, A=A, hidden=(64, 64), actor_acts=("tanh", "tanh"), **c.get("cfg", {}))
    eng = Engine(EngineConfig(s_dim=S, a_dim=A, hidden=(64, 64), activation="tanh", critic_hidden=chid, batch=mb,
                              buffer_capacity=8208 if kind == "trpo" else n, per_state_std=cfg.per_state_std, actor_layer_norm=cfg.layer_norm,
                              actor_gaussian="train", graph_steps=1, vcritics=nc, softmax=soft, learners=K, trpo=kind == "trpo"))
    if kind == "trpo":                                    # one chunk of a whole-table pass and 5 rows: two chunks,
        n = int(eng.segments["trpo.X"]["rows"]) + 5       # whose `first` / `last` differ (over the capacity: an error)
    rows = []
    for k in range(max(K, 1)):                            # each learner's own state, table and indices
        if K:
            eng.select_seed(k)
        rng = np.random.RandomState(100 + 7 * k)
        st = R.init_state(cfg, seed=20 + k, logstd=0.2 * rng.normal(size=A) - 0.3, gain=0.5, dt=np.float32)
        nrm = nontrivial_normalizers(rng, S, A)
        s = (rng.normal(size=(n, S)) * rng.uniform(0.3, 2.0, S)).astype(np.float32)
        a = rng.randint(0, A, n).astype(np.float32) if soft else rng.normal(size=(n, A)).astype(np.float32)
        adv = (rng.normal(size=n) * 1.5 + 0.4).astype(np.float32)
        rtg = (rng.normal(size=n) * 4 + 1).astype(np.float32)
        eng.set_normalizers(nrm.s_mean, nrm.s_den, nrm.a_mean, nrm.a_den, ret_den=2.7)
        for i, w in enumerate(V.init_state(S, chid, max(nc, 1), seed=40 + k, dt=np.float32).critics[:nc]):
            eng.set_net(f"v{i}", w)

        def give(move):                                   # the policy, `move` updates after the rollout
            mv = np.random.RandomState(300 + k)
            eng.set_net("actor", [w + (move * mv.normal(size=w.shape)).astype(np.float32) for w in st.actor])
            if not soft:
                eng.set_logstd(st.logstd)
        give(0.0)
        if kind == "ppo":
            eng.ppo_begin(s, a, adv)
            give(0.05)
        elif kind == "vc":
            for i in range(nc):
                eng.vcritic_begin(i, s[: n - 2 * i], rtg[: n - 2 * i])
        rows.append((s, a, rtg))
    if kind != "trpo":                                    # 5 steps' table rows per learner
        idx = np.stack([[np.random.RandomState(500 + 10 * k + j).permutation(n - 2 * max(nc - 1, 0))[:mb] for j in range(5)]
                        for k in range(max(K, 1))]).astype(np.int32)
    if kind == "ppo":
        par = dict(eps_ppo=0.2, actor_lr=3e-4, max_grad_norm=0.5)
        for sl, eager in ((slice(0, 2), True), (slice(2, 5), False)):
            if K:
                eng.ppo_steps_packed(idx[:, sl], eager=eager, **par)
            else:
                eng.ppo_steps(idx[0, sl], eager=eager, **par)
        eng.sync()
        for k in range(max(K, 1)):
            if K:
                eng.select_seed(k)
            end = eng.ppo_end(0.2)
            outs += [eng.ppo_stats(5), np.array([float(end[q]) for q in sorted(end)]),
                     eng.neglogp(rows[k][0][:40], rows[k][1][:40]).cpu().numpy()]
            outs += [t.cpu().numpy() for t in eng.dist(rows[k][0][:40]) if t is not None]
        plan = eng.ppo_plan_info(mb)
    elif kind == "vc":
        for sl, eager in ((slice(0, 2), True), (slice(2, 5), False)):
            eng.vcritic_steps(idx[0, sl], critic_lr=1e-3, eager=eager)
        eng.sync()
        end = eng.vcritic_end()
        outs += [eng.vcritic_stats(5), np.array(end["critic_loss"] + [end["n_steps"]], np.float64)]
        for i in range(nc):
            outs += [eng.vcritic_value(i, rows[0][0][:40]).cpu().numpy(),
                     eng.vcritic_loss(i, rows[0][0][:40], rows[0][2][:40]).cpu().numpy()]
        plan = eng.vcritic_plan_info(mb)
    else:
        par = dict(delta=0.01, cg_it=5, trust_sub=1, trust_damp=0.5, kl_maxfactor=1.5)
        s, a, _ = rows[0]
        eng.trpo_begin(s, a, adv, **par)
        g = eng.trpo_grad(flat=True)
        f = eng.trpo_fvp(g, flat=True)
        step = eng.trpo_step(**par)
        outs += [g.cpu().numpy(), f.cpu().numpy(), np.array([float(step[q]) for q in sorted(step)])] + eng.get_net("actor")
        plan = eng.trpo_plan_info(n)
    eng.sync()
    return plan, [eng]


def run(names, timeout):
    for name in names:
        env = dict(os.environ, **CASES[name].get("env", {}))
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", name], env=env, timeout=timeout,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result after {timeout} s; stopped")
        lines = [l for l in p.stdout.splitlines() if l.startswith("case ")]
        if p.returncode != 0 or len(lines) != 1:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"case {name}: child exited with {p.returncode}; stopped")
        print(lines[0], flush=True)


def compare(fa, fb):
    def load(f):
        with open(f) as fh:
            return {l.split()[1]: l.strip() for l in fh if l.startswith("case ")}
    a, b = load(fa), load(fb)
    diff = 0
    for name in a:
        same = a[name] == b.get(name)
        diff += not same
        print(f"{'EQUAL' if same else 'DIFF '}   {a[name]}" + ("" if same else f"\n        {b.get(name, 'case ' + name + ' missing')}"))
    missing = [n for n in b if n not in a]
    for n in missing:
        print(f"DIFF    case {n} missing from {fa}")
    print(f"{len(a) - diff} equal, {diff + len(missing)} differ")
    return 1 if diff or missing else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--cases", default="", help="comma-separated names or prefixes (default: all)")
    r.add_argument("--timeout", type=float, default=120.0, help="seconds per case")
    sub.add_parser("child").add_argument("name")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    sub.add_parser("list")
    a = ap.parse_args()
    if a.cmd == "list":
        print("\n".join(CASES))
    elif a.cmd == "child":
        child(a.name)
    elif a.cmd == "compare":
        sys.exit(compare(a.a, a.b))
    else:
        sel = [s for s in a.cases.split(",") if s]
        run([n for n in CASES if not sel or any(n == s or n.startswith(s + ".") for s in sel)], a.timeout)


if __name__ == "__main__":
    main()
