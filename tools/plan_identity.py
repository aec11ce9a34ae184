#!/usr/bin/env python3
"""Bit-identity of two libsacx builds: plans, arenas and returned values, case by case.

A host-side change of sacx.cpp (the plan builders, the graph capture, the inference paths) must leave every
launch table and every computed bit as the parent commit's library has them.  For each named case this runs,
in a fresh child process against the library SACX_LIBPATH names (default: the in-tree build), a fixed-seed
learner with a fixed NumPy stream state and pushed permutations, and prints one line:

  case <name> plan=<sha256 of the plan_info listing: name, kernel, grid, block, flops, bytes>:<launches>
       arena=<sha256 of the whole arena after the steps> out=<sha256 of the returned values>

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
    outs = []
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
    print(f"case {name} plan={plan_sha(eng.plan_info())} arena={arena} out={sha(*outs)}", flush=True)
    for e in engs:
        e.close()


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
