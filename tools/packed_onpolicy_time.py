"""Time of the packed on-policy steps (Engine.ppo_steps_packed / vcritic_steps_packed on an
EngineConfig(learners=K) engine) against K times the one-learner step, and of one ``mbrl`` policy-update
iteration of 4 runs, packed against serial.

Steps: the Pendulum and HalfCheetah shapes of tools/ppo_time.py (S 3 A 1 / S 17 A 6, 64 x 2 tanh, one critic,
minibatches of 312 from 10,000-row tables, 320 steps per call).  K = 1 is the one-learner call
(ppo_steps / vcritic_steps); K = 2, 4, 8 the packed call.  With ``--parent-lib`` (a libsacx.so built from the
parent commit) the one-learner step is also measured on that library, in fresh processes ALTERNATING with this
tree's (``--rounds`` of each): the packed figures stand beside K x the parent's step, and the parent's own
min - max spread over its repeats is the noise floor the one-learner medians are held to.

Iteration: HalfCheetah at the defaults of tools/mbrl_time.py (10,000 simulated rows per update over 2 models
512 x 2, 320 critic steps and 320 actor steps of 312 rows), 4 runs: serial = four one-learner engines, one run's
iteration after another; packed = one engine of 4 learners, the sim data, ``*_begin`` and ``*_end`` per learner
and ONE packed steps call for the critics and one for the actors.

Every figure: untimed passes first (graphs captured; two for the steps, one for the iteration), then ``--repeats``
timed passes, the device synchronised, a host clock around the work and a final synchronise.  The steps' index
arrays are all drawn before the first call, so that the timed calls follow one another.  Each library runs in a process of its own (a process
loads one libsacx); no more than one process holds the GPU at a time.

Usage: packed_onpolicy_time.py [--parent-lib PATH] [--repeats 5] [--rounds 2] [--out profiles/packed_onpolicy_time_v1.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sac-expert_amd")]

import numpy as np   # noqa: E402

SHAPES = {"pendulum": dict(S=3, A=1), "halfcheetah": dict(S=17, A=6)}
N_ROWS, MB, STEPS = 10_000, 312, 320
NEW = ("sacx_learners_init", "sacx_ppo_steps_packed", "sacx_vcritic_steps_packed")
PPO_KW = dict(eps_ppo=0.2, max_grad_norm=0.5, ent_reg=True, alpha_lr=1e-3, ent_targ=0.0)


def _parent_library_shim():
    """The parent's library lacks the three packed entry points, which sac_eo._native binds at load: they
    become stubs that fail (this tool calls none of them on that library)."""
    real = ctypes.CDLL

    class Parent(real):
        def __getattr__(self, name):
            if name in NEW:
                stub = ctypes.CFUNCTYPE(ctypes.c_int)(lambda *a: -1)
                setattr(self, name, stub)
                return stub
            return super().__getattr__(name)
    ctypes.CDLL = Parent


def clocked(fn, eng):
    import torch
    eng.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.sync()
    return time.perf_counter() - t0


def build(shape, K):
    from sac_eo.engine import Engine, EngineConfig
    from sac_eo.nets import create_nn_weights
    S, A = SHAPES[shape]["S"], SHAPES[shape]["A"]
    eng = Engine(EngineConfig(s_dim=S, a_dim=A, hidden=(64, 64), activation="tanh", batch=MB, buffer_capacity=N_ROWS,
                              actor_gaussian="train", graph_steps=1, vcritics=1, **({"learners": K} if K > 1 else {})))
    for k in range(K):
        eng.select_seed(k)
        rng = np.random.default_rng(1 + k)
        eng.set_net("actor", create_nn_weights(rng, S, A, (64, 64), 0.01))
        eng.set_net("v0", create_nn_weights(rng, S, 1, (64, 64), 1.0))
        rs = np.random.RandomState(2 + k)
        s = rs.normal(size=(N_ROWS, S)).astype(np.float32)
        mean, ls, _ = eng.dist(s)
        a = mean.cpu().numpy() + np.exp(ls.cpu().numpy()) * rs.normal(size=(N_ROWS, A)).astype(np.float32)
        eng.ppo_begin(s, a, rs.normal(size=N_ROWS).astype(np.float32))
        eng.vcritic_begin(0, s, rs.normal(size=N_ROWS).astype(np.float32))
    eng.sync()
    return eng


def child_steps(Ks, repeats):
    """us per (packed) step of K learners, both kinds, both shapes -> {"<kind> <shape> K": [repeats]}."""
    out = {}
    for shape in SHAPES:
        for K in Ks:
            eng = build(shape, K)
            rs = np.random.RandomState(3)
            draw = lambda: np.stack([[rs.permutation(N_ROWS)[:MB] for _ in range(STEPS)] for _ in range(K)]).astype(np.int32)
            if K == 1:
                runs = {"ppo": lambda i: eng.ppo_steps(i[0], actor_lr=3e-4, **PPO_KW),
                        "critic": lambda i: eng.vcritic_steps(i[0], critic_lr=3e-4)}
            else:
                runs = {"ppo": lambda i: eng.ppo_steps_packed(i, actor_lr=[3e-4] * K, **PPO_KW),
                        "critic": lambda i: eng.vcritic_steps_packed(i, critic_lr=[3e-4] * K)}
            # every call's indices are drawn before the first one: the timed calls follow one another without
            # the host's draw (K x 320 permutations, 30 ms per learner) idling the device between them
            idxs = [draw() for _ in range(repeats + 2)]
            for kind, run in runs.items():
                run(idxs[0])                                  # untimed: every graph captured and replayed once,
                run(idxs[1])                                  # and once more
                out[f"{kind} {shape} {K}"] = [clocked(lambda: run(i), eng) * 1e6 / STEPS for i in idxs[2:]]
            eng.close()
    return out


def child_iteration(repeats, runs=4):
    """ms per policy-update iteration of `runs` runs: serial engines against one packed engine."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("mbrl_time", os.path.join(ROOT, "tools", "mbrl_time.py"))
    mt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mt)
    from sac_eo.engine import Engine
    import dataclasses
    rs = np.random.RandomState(3)
    par = dict(eps_ppo=0.2, max_grad_norm=0.5, ent_reg=False, alpha_lr=3e-4, ent_targ=-float(mt.A))

    def shuffles():
        out = []
        for _ in range(mt.ITS):
            idx = np.arange(mt.SIM)
            rs.shuffle(idx)
            out.append(idx[:mt.NMB * mt.MB].reshape(mt.NMB, mt.MB))
        return np.concatenate(out).astype(np.int32)

    def fill(eng, k):
        from sac_eo.nets import create_nn_weights
        rng = np.random.default_rng(1 + k)
        eng.set_net("actor", create_nn_weights(rng, mt.S, mt.A, (64, 64), 0.01))
        eng.set_net("v0", create_nn_weights(rng, mt.S, 1, (64, 64), 1.0))
        for m in range(mt.NM):
            eng.set_net(f"m{m}", create_nn_weights(rng, mt.S + mt.A, mt.S + 1, (512, 512), 0.01))
        r2 = np.random.RandomState(2 + k)
        eng.append(r2.normal(size=(mt.HELD, mt.S)).astype(np.float32), r2.uniform(-1, 1, (mt.HELD, mt.A)).astype(np.float32),
                   r2.normal(size=mt.HELD).astype(np.float32), r2.normal(size=(mt.HELD, mt.S)).astype(np.float32),
                   np.zeros(mt.HELD, np.float32))
        eng.rng_seed(5 + k)

    first, _ = mt.build(torch.device("cuda"))
    cfg = first.cfg
    first.close()
    serial = [Engine(cfg) for _ in range(runs)]
    for k, e in enumerate(serial):
        fill(e, k)
    packed = Engine(dataclasses.replace(cfg, learners=runs))
    for k in range(runs):
        packed.select_seed(k)
        fill(packed, k)
    parts = {}

    def note(key, t):
        parts.setdefault(key, []).append(t * 1e3)

    def serial_iteration(rec):
        for e in serial:
            t0 = time.perf_counter()
            tabs = mt.device_tables(e)
            e.sync()
            t1 = time.perf_counter()
            e.vcritic_begin(0, tabs[0], tabs[3])
            e.vcritic_steps(shuffles(), critic_lr=3e-4)
            e.vcritic_end()
            t2 = time.perf_counter()
            e.ppo_begin(tabs[0], tabs[1], tabs[2])
            e.ppo_steps(shuffles(), actor_lr=3e-4, **par)
            e.ppo_end(0.2)
            t3 = time.perf_counter()
            if rec:
                note("serial sim data", t1 - t0), note("serial critic", t2 - t1), note("serial actor", t3 - t2)

    def packed_iteration(rec):
        t0 = time.perf_counter()
        tabs = []
        for k in range(runs):
            packed.select_seed(k)
            tabs.append(mt.device_tables(packed))
        packed.sync()
        t1 = time.perf_counter()
        for k in range(runs):
            packed.select_seed(k)
            packed.vcritic_begin(0, tabs[k][0], tabs[k][3])
        tb = time.perf_counter()
        packed.vcritic_steps_packed(np.stack([shuffles() for _ in range(runs)]), critic_lr=3e-4)
        packed.sync()
        ts = time.perf_counter()
        for k in range(runs):
            packed.select_seed(k)
            packed.vcritic_end()
        t2 = time.perf_counter()
        for k in range(runs):
            packed.select_seed(k)
            packed.ppo_begin(tabs[k][0], tabs[k][1], tabs[k][2])
        ub = time.perf_counter()
        packed.ppo_steps_packed(np.stack([shuffles() for _ in range(runs)]), actor_lr=3e-4, **par)
        packed.sync()
        us = time.perf_counter()
        for k in range(runs):
            packed.select_seed(k)
            packed.ppo_end(0.2)
        t3 = time.perf_counter()
        if rec:
            note("packed sim data", t1 - t0), note("packed critic", t2 - t1), note("packed actor", t3 - t2)
            note("packed critic, the shuffles + the one packed steps call", ts - tb)
            note("packed actor, the shuffles + the one packed steps call", us - ub)
            note("packed per-learner passes (sim data, begin, end)", (t3 - t0) - (ts - tb) - (us - ub))

    serial_iteration(False)
    packed_iteration(False)                                   # untimed: graphs captured
    tot = {"serial iteration": [], "packed iteration": []}
    for _ in range(repeats):                                  # alternating
        tot["serial iteration"].append(clocked(lambda: serial_iteration(True), serial[-1]) * 1e3)
        tot["packed iteration"].append(clocked(lambda: packed_iteration(True), packed) * 1e3)
    # the serial parts are per run: summed over the runs of a repeat
    for k in list(parts):
        if k.startswith("serial"):
            v = np.asarray(parts[k]).reshape(repeats, runs).sum(1)
            parts[k] = v.tolist()
    for e in serial:
        e.close()
    packed.close()
    return {**tot, **parts}


def run_child(lib, args, child, parent=False):
    env = dict(os.environ)
    if lib:
        env["SACX_LIBPATH"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--child", child] + \
        (["--parent-shim"] if parent else [])
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=900)
    if res.returncode != 0:
        raise SystemExit(f"child failed ({res.returncode}): {' '.join(cmd)}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_onpolicy_time_v1.txt"))
    ap.add_argument("--child", default=None, help="(internal) steps:<K,K,...> or iteration")
    ap.add_argument("--parent-shim", action="store_true", help="(internal) the library is the parent commit's")
    args = ap.parse_args()
    if args.child:
        if args.parent_shim:
            _parent_library_shim()
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("packed_onpolicy_time.py needs the GPU (no CPU fallback)")
        if args.child.startswith("steps:"):
            out = child_steps([int(x) for x in args.child[6:].split(",")], args.repeats)
        else:
            out = child_iteration(args.repeats)
        print(json.dumps(out), flush=True)
        return
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)

    fmt = lambda v: f"median {np.median(v):.3f}, min {np.min(v):.3f}, max {np.max(v):.3f}"
    say(f"packed_onpolicy_time: {STEPS} steps of {MB} rows per call, {args.repeats} repeats after the untimed passes; "
        f"parent library {'given' if args.parent_lib else 'not given'}, {args.rounds} alternating rounds")
    one = {"parent": {}, "tree": {}}
    for r in range(args.rounds):                              # alternating: parent, this tree, parent, ...
        for who, lib in (("parent", args.parent_lib), ("tree", None)):
            if who == "parent" and not lib:
                continue
            for key, us in run_child(lib, args, "steps:1", parent=who == "parent").items():
                one[who].setdefault(key, []).extend(us)
                say(f"one learner, {who} library, round {r}, {key[:-2]}: " + " ".join(f"{x:.3f}" for x in us) + " us/step")
    packed = run_child(None, args, "steps:2,4,8")
    for kind in ("ppo", "critic"):
        for shape in SHAPES:
            key = f"{kind} {shape} 1"
            tree = one["tree"][key]
            say(f"{kind} step {shape} K=1 (the one-learner call), this tree: {fmt(tree)} us/step")
            base = float(np.median(tree))
            if one["parent"]:
                par = one["parent"][key]
                base = float(np.median(par))
                spread = (np.max(par) - np.min(par)) / base
                diff = (np.median(tree) - base) / base
                say(f"{kind} step {shape} K=1, parent library: {fmt(par)} us/step; its min-max spread {100 * spread:.2f} % "
                    f"(the noise floor); this tree's median differs by {100 * diff:+.2f} %: "
                    f"{'inside' if abs(diff) <= spread else 'OUTSIDE'} the floor")
            for K in (2, 4, 8):
                us = packed[f"{kind} {shape} {K}"]
                say(f"{kind} step {shape} K={K} packed, each repeat: " + " ".join(f"{x:.3f}" for x in us) + " us per packed step")
                say(f"{kind} step {shape} K={K} packed: {fmt(us)} us per packed step = {np.median(us) / K:.3f} us per learner-step; "
                    f"K x the {'parent' if one['parent'] else 'one-learner'} step = {K * base:.3f} us: "
                    f"{K * base / np.median(us):.2f}x")
    it = run_child(None, args, "iteration")
    say("one mbrl policy-update iteration, HalfCheetah defaults (tools/mbrl_time.py), 4 runs, ms:")
    for key, v in it.items():
        say(f"  {key}: {fmt(v)} ms")
    s, p = np.median(it["serial iteration"]), np.median(it["packed iteration"])
    rest = np.median(it["packed per-learner passes (sim data, begin, end)"])
    say(f"  serial / packed: {s / p:.2f}x; the per-learner passes are {100 * rest / p:.0f} % of the packed iteration")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
