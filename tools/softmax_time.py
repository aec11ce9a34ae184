"""Time of one PPO minibatch step on a softmax handle (SoftMaxActor, EngineConfig(softmax=True)) against the
Gaussian step of the same shape, in the same session.

Shape: HalfCheetah-like S 17, A 6 (six actions on the softmax handle), 64 x 2 tanh; a 10,000-row table,
minibatches of 312.  Per handle: one ``ppo_begin``, one untimed call of 320 steps (the graphs of 64 steps
are captured there), then ``--repeats`` timed calls of 320 steps each: the device is synchronised, then a
host clock around ppo_steps(320 x 312 indices) + synchronise.  The two handles' repeats alternate.
Reported: each step's launches, us per step (each repeat, median, min), us per launch, and the ratio of the
medians.

The expectation to confirm or refute: the softmax step's median is at most 1.05 x the Gaussian step's (the
step is bound by its launch count, DESIGN 6.10, and the softmax step has no more launches).

Usage: softmax_time.py [--steps 320] [--repeats 5] [--out profiles/softmax_time_v1.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sac-expert_amd")]

import numpy as np   # noqa: E402

S, A = 17, 6
N_ROWS, MB = 10_000, 312


def build(softmax, device):
    from sac_eo.engine import Engine, EngineConfig
    from sac_eo.nets import create_nn_weights
    eng = Engine(EngineConfig(s_dim=S, a_dim=A, hidden=(64, 64), activation="tanh", batch=MB, buffer_capacity=N_ROWS,
                              actor_gaussian="train", graph_steps=1, softmax=softmax), device=device)
    eng.set_net("actor", create_nn_weights(np.random.default_rng(1), S, A, (64, 64), 0.01))
    rs = np.random.RandomState(2)
    s = rs.normal(size=(N_ROWS, S)).astype(np.float32)
    mean, ls, _ = eng.dist(s)
    if softmax:                                          # a ~ the policy: the Gumbel argmax on its logits
        a = np.argmax(mean.cpu().numpy() - np.log(-np.log(rs.random_sample(size=(N_ROWS, A)))), -1).astype(np.float32)
    else:
        a = mean.cpu().numpy() + np.exp(ls.cpu().numpy()) * rs.normal(size=(N_ROWS, A)).astype(np.float32)
    eng.ppo_begin(s, a, rs.normal(size=N_ROWS).astype(np.float32))
    eng.sync()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=320)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_time_v1.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("softmax_time.py needs the GPU (no CPU fallback)")
    from sac_eo import _native
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)

    say(f"softmax_time: library {os.path.relpath(_native.LIB_PATH, ROOT)}; device {torch.cuda.get_device_name(0)}")
    kinds = ("gaussian", "softmax")
    engs = {k: build(k == "softmax", torch.device("cuda")) for k in kinds}
    plans = {k: [(l["name"], l["kernel"]) for l in engs[k].ppo_plan_info(MB)] for k in kinds}
    rs = np.random.RandomState(3)
    kw = dict(eps_ppo=0.2, actor_lr=3e-4, max_grad_norm=0.5, ent_reg=True, alpha_lr=1e-3, ent_targ=0.0)
    draw = lambda: np.stack([rs.permutation(N_ROWS)[:MB] for _ in range(args.steps)]).astype(np.int32)
    for k in kinds:                                      # untimed: every graph captured and replayed once
        engs[k].ppo_steps(draw(), **kw)
        engs[k].sync()
    us = {k: [] for k in kinds}
    for r in range(args.repeats):
        for k in kinds:
            idx = draw()
            engs[k].sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            engs[k].ppo_steps(idx, **kw)
            engs[k].sync()
            us[k].append((time.perf_counter() - t0) * 1e6 / args.steps)
            say(f"{k} repeat {r}: {us[k][-1]:.3f} us/step")
    med = {}
    for k in kinds:
        log = engs[k].ppo_end(0.2)
        med[k] = float(np.median(us[k]))
        say(f"{k}: {len(plans[k])} launches per minibatch step: {' | '.join(n for n, _ in plans[k])}")
        say(f"{k}: {args.steps} steps x {args.repeats}: median {med[k]:.3f} us/step, min {np.min(us[k]):.3f}, "
            f"max {np.max(us[k]):.3f}; {med[k] / len(plans[k]):.3f} us per launch; after {log['n_steps']} steps "
            f"tv {log['tv']:.4g} kl {log['kl']:.4g}")
        engs[k].close()
    ratio = med["softmax"] / med["gaussian"]
    say(f"summary: softmax {med['softmax']:.3f} us/step / gaussian {med['gaussian']:.3f} us/step = {ratio:.4f} "
        f"(expected <= 1.05: {'met' if ratio <= 1.05 else 'MISSED'})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
