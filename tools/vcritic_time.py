"""Time of one critic minibatch step through Engine.vcritic_steps and of Engine.gae, with the PPO actor
step (tools/ppo_time.py) timed in the same session as the yardstick.

Shapes: the Pendulum and HalfCheetah critic shapes (S 3 / 17, 64 x 2 tanh), minibatches of 312 from
10,000-row tables, 1, 2 and 3 critics (3: the dW problems take a second launch).  Per case: ``vcritic_begin`` per critic, one untimed call of 320 steps
(the graphs of 64 steps are captured there), then ``--repeats`` timed calls of 320 steps each: the device
is synchronised, then a host clock around vcritic_steps(320 x 312 indices) + synchronise.  ``gae`` (both
value passes and the scan, one critic): 10,000 rows as one trajectory and as 2,000 five-row ones; a timed
window is ``--gae-calls`` (200) calls back to back and one synchronise (a single call is 0.06 - 0.5 ms: too
short for a host clock), one untimed window, then ``--repeats`` timed ones; ``gae_values`` (the scan alone)
likewise.  Reported: the step's launches, us per step (each repeat, median, min - max), us per launch.

The expectation to confirm or refute: a critic step costs its launches x the PPO step's per-launch cost.

Usage: vcritic_time.py [--steps 320] [--repeats 5] [--gae-calls 200] [--out profiles/vcritic_time_v1.txt]"""
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


def build(shape, nc, device):
    from sac_eo.engine import Engine, EngineConfig
    from sac_eo.nets import create_nn_weights
    S, A = SHAPES[shape]["S"], SHAPES[shape]["A"]
    eng = Engine(EngineConfig(s_dim=S, a_dim=A, hidden=(64, 64), activation="tanh", batch=MB, buffer_capacity=N_ROWS,
                              actor_gaussian="train", graph_steps=1, vcritics=nc), device=device)
    rng = np.random.default_rng(1)
    for k in range(nc):
        eng.set_net(f"v{k}", create_nn_weights(rng, S, 1, (64, 64), 1.0))
    return eng


def timed(fn, sync, repeats, per):
    import torch
    us = []
    for _ in range(repeats):
        sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        sync()
        us.append((time.perf_counter() - t0) * 1e6 / per)
    return us


def time_steps(shape, nc, steps, repeats, say):
    import torch
    eng = build(shape, nc, torch.device("cuda"))
    S = SHAPES[shape]["S"]
    rs = np.random.RandomState(2)
    for k in range(nc):
        eng.vcritic_begin(k, rs.normal(size=(N_ROWS, S)).astype(np.float32), rs.normal(size=N_ROWS).astype(np.float32))
    plan = [l["name"] for l in eng.vcritic_plan_info(MB)]
    draw = lambda: np.stack([rs.permutation(N_ROWS)[:MB] for _ in range(steps)]).astype(np.int32)
    eng.vcritic_steps(draw(), critic_lr=3e-4)            # untimed: every graph captured and replayed once
    eng.sync()
    idx = [draw() for _ in range(repeats)]
    it = iter(idx)
    us = timed(lambda: eng.vcritic_steps(next(it), critic_lr=3e-4), eng.sync, repeats, steps)
    for r, x in enumerate(us):
        say(f"vcritic {shape} x{nc} repeat {r}: {x:.3f} us/step")
    out = eng.vcritic_end()
    med = float(np.median(us))
    say(f"vcritic {shape} x{nc}: {len(plan)} launches per minibatch step: {' | '.join(plan)}")
    say(f"vcritic {shape} x{nc}: {steps} steps x {repeats}: median {med:.3f} us/step, min {np.min(us):.3f}, max {np.max(us):.3f}; "
        f"{med / len(plan):.3f} us per launch; after {out['n_steps']} steps critic_loss "
        f"{' '.join(f'{float(x):.4g}' for x in out['critic_loss'])}")
    eng.close()
    return med, len(plan)


def time_gae(shape, repeats, calls, say):
    import torch
    eng = build(shape, 1, torch.device("cuda"))
    S = SHAPES[shape]["S"]
    rs = np.random.RandomState(4)
    dev = lambda x: torch.as_tensor(x, device="cuda")
    s, sp = [dev(rs.normal(size=(N_ROWS, S)).astype(np.float32)) for _ in range(2)]
    r, d = dev(rs.normal(size=N_ROWS).astype(np.float32)), dev(np.zeros(N_ROWS, np.float32))
    v_s, v_sp = eng.vcritic_value(0, s), eng.vcritic_value(0, sp)
    for what, traj in (("one 10,000-row trajectory", np.zeros(N_ROWS)), ("2,000 five-row trajectories", np.arange(N_ROWS) // 5)):
        for name, one in (("gae", lambda: eng.gae(0, s, r, sp, d, traj, 0.99, 0.95)),
                          ("gae_values", lambda: eng.gae_values(v_s, v_sp, r, d, traj, 0.99, 0.95))):
            def window():
                for _ in range(calls):
                    one()
            window()                                     # untimed
            us = timed(window, eng.sync, repeats, calls)
            say(f"{name} {shape}, {what}: {calls} calls x {repeats}: median {np.median(us):.1f} us per call, min {np.min(us):.1f}, "
                f"max {np.max(us):.1f} (each call uploads its segment ids: 40 KB host to device)")
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=320)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--gae-calls", type=int, default=200, help="gae calls inside one timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcritic_time_v1.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vcritic_time.py needs the GPU (no CPU fallback)")
    from sac_eo import _native
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)

    say(f"vcritic_time: library {os.path.relpath(_native.LIB_PATH, ROOT)}; device {torch.cuda.get_device_name(0)}")
    res = {(shape, nc): time_steps(shape, nc, args.steps, args.repeats, say) for shape in SHAPES for nc in (1, 2, 3)}
    for shape in SHAPES:
        time_gae(shape, args.repeats, args.gae_calls, say)
    spec = importlib.util.spec_from_file_location("ppo_time", os.path.join(ROOT, "tools", "ppo_time.py"))
    pt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pt)
    ppo = {shape: pt.time_ppo(shape, args.steps, args.repeats, say) for shape in SHAPES}      # the yardstick, same session
    for (shape, nc), (med, n) in res.items():
        per = ppo[shape][0] / ppo[shape][1]
        say(f"summary {shape} x{nc}: {n} launches x {per:.3f} us (the PPO step's per launch) = {n * per:.1f} us expected, "
            f"{med:.1f} us measured ({med / (n * per):.2f}x)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
