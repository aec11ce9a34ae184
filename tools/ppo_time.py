"""Time of one PPO minibatch step through Engine.ppo_steps (a trainable GaussianActor handle), and the
generic BC plan's per-launch time measured in the same session as the yardstick.

Shapes: the Pendulum shape of the reference's golden log (S 3, A 1, 64 x 2 tanh, minibatches of 312:
10,000 rollout rows in 32 minibatches) and a HalfCheetah shape (S 17, A 6, 64 x 2 tanh, 312).  Per shape:
one ``ppo_begin`` on a 10,000-row rollout, one untimed call of 320 steps (the graphs of 64 steps are
captured there), then ``--repeats`` timed calls of 320 steps each: the device is synchronised, then a host
clock around ppo_steps(320 x 312 indices) + synchronise.  Reported: the step's launches, us per step
(each repeat, median, min), us per launch.  Then the BC update on its generic plan (tools/bc_time.py
--generic: HalfCheetah shapes, 2,000 updates per call): us per update and per launch (chain launches +
the sampler's and the gather's share counted as the plan lists them).

The expectation to confirm or refute: a step costs its launches x the per-launch cost of the generic plan
(~6.5 us per launch).

Usage: ppo_time.py [--steps 320] [--repeats 5] [--out profiles/ppo_time_v1.txt]"""
import argparse
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sac-expert_amd")]

import numpy as np   # noqa: E402

SHAPES = {"pendulum": dict(S=3, A=1), "halfcheetah": dict(S=17, A=6)}
N_ROWS, MB = 10_000, 312


def build(shape, device):
    from sac_eo.engine import Engine, EngineConfig
    from sac_eo.nets import create_nn_weights
    S, A = SHAPES[shape]["S"], SHAPES[shape]["A"]
    eng = Engine(EngineConfig(s_dim=S, a_dim=A, hidden=(64, 64), activation="tanh", batch=MB, buffer_capacity=N_ROWS,
                              actor_gaussian="train", graph_steps=1), device=device)
    rng = np.random.default_rng(1)
    eng.set_net("actor", create_nn_weights(rng, S, A, (64, 64), 0.01))
    rs = np.random.RandomState(2)
    s = rs.normal(size=(N_ROWS, S)).astype(np.float32)
    mean, ls, _ = eng.dist(s)
    a = mean.cpu().numpy() + np.exp(ls.cpu().numpy()) * rs.normal(size=(N_ROWS, A)).astype(np.float32)
    eng.ppo_begin(s, a, rs.normal(size=N_ROWS).astype(np.float32))
    eng.sync()
    return eng


def time_ppo(shape, steps, repeats, say):
    import torch
    eng = build(shape, torch.device("cuda"))
    plan = [l["name"] for l in eng.ppo_plan_info(MB)]
    rs = np.random.RandomState(3)
    kw = dict(eps_ppo=0.2, actor_lr=3e-4, max_grad_norm=0.5, ent_reg=True, alpha_lr=1e-3, ent_targ=0.0)
    draw = lambda: np.stack([rs.permutation(N_ROWS)[:MB] for _ in range(steps)]).astype(np.int32)
    eng.ppo_steps(draw(), **kw)                          # untimed: every graph captured and replayed once
    eng.sync()
    us = []
    for r in range(repeats):
        idx = draw()
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.ppo_steps(idx, **kw)
        eng.sync()
        us.append((time.perf_counter() - t0) * 1e6 / steps)
        say(f"ppo {shape} repeat {r}: {us[-1]:.3f} us/step")
    log = eng.ppo_end(0.2)
    med = float(np.median(us))
    say(f"ppo {shape}: {len(plan)} launches per minibatch step: {' | '.join(plan)}")
    say(f"ppo {shape}: {steps} steps x {repeats}: median {med:.3f} us/step, min {np.min(us):.3f}, max {np.max(us):.3f}; "
        f"{med / len(plan):.3f} us per launch; after {log['n_steps']} steps tv {log['tv']:.4g} kl {log['kl']:.4g}")
    eng.close()
    return med, len(plan)


def time_bc_generic(repeats, say, updates=2000):
    import torch
    spec = importlib.util.spec_from_file_location("bc_time", os.path.join(ROOT, "tools", "bc_time.py"))
    bc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bc)
    os.environ["SACX_GENERIC"] = "1"
    try:
        eng = bc.build("bc", torch.device("cuda"))
    finally:
        del os.environ["SACX_GENERIC"]
    plan = [l["name"] for l in eng.plan_info()]
    chain = [n for n in plan if n not in ("rng", "gather")]
    gen = np.random.default_rng(5)
    eng.push_perms(np.stack([gen.permutation(20) for _ in range(eng.cfg.perm_capacity)]))
    eng.prepare(updates)
    eng.step(updates, num_timesteps=0, ts_increment=1)
    eng.sync()
    us = []
    for r in range(repeats):
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.step(updates, num_timesteps=0, ts_increment=1)
        eng.sync()
        us.append((time.perf_counter() - t0) * 1e6 / updates)
        say(f"bc generic repeat {r}: {us[-1]:.3f} us/update")
    med = float(np.median(us))
    say(f"bc generic: {len(chain)} chain launches (+ sampler, gather on the side stream): {' | '.join(chain)}")
    say(f"bc generic: {updates} updates x {repeats}: median {med:.3f} us/update, min {np.min(us):.3f}; "
        f"{med / len(chain):.3f} us per chain launch")
    eng.close()
    return med / len(chain)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=320)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_time_v1.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ppo_time.py needs the GPU (no CPU fallback)")
    from sac_eo import _native
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)

    say(f"ppo_time: library {os.path.relpath(_native.LIB_PATH, ROOT)}; device {torch.cuda.get_device_name(0)}")
    res = {shape: time_ppo(shape, args.steps, args.repeats, say) for shape in SHAPES}
    per_launch = time_bc_generic(args.repeats, say)
    for shape, (med, n) in res.items():
        say(f"summary {shape}: {n} launches x {per_launch:.3f} us (generic BC per launch) = {n * per_launch:.1f} us expected, "
            f"{med:.1f} us measured ({med / (n * per_launch):.2f}x)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
