"""Time of one TRPO update through Engine.trpo_begin + trpo_step (a trainable GaussianActor handle with
``trpo=True``), and the PPO update of the same shape measured in the same session beside it.

Shapes: the ``mbrl`` defaults -- 10,000 rollout rows, actor 64 x 2 tanh, ``cg_it`` 20, ``trust_sub`` 1,
``trust_damp`` 0.01, ``delta_trpo`` 0.02, ``kl_maxfactor`` 1.5 -- at Pendulum (S 3, A 1) and HalfCheetah
(S 17, A 6) dimensions.  Per shape: one untimed update (the graph of the solve is captured there), the
weights restored, then ``--repeats`` timed updates from the same weights: the device is synchronised, then a
host clock around trpo_begin + trpo_step (which ends synchronised).  Also timed alone: one Fisher-vector
product (200 ``trpo_fvp`` calls on a device vector per window, one synchronise at the end) and the solve's
share.  Reported: the launches of one Fisher product, ms per update (each repeat, median, min, max), the CG
iterations run and the line-search trials implied by ``adj``, us per Fisher product and per launch; then one
PPO update (``ppo_begin`` + 320 steps of 312 rows + ``ppo_end``) the same way.

Nothing is promised in advance: what is measured is written down.

Usage: trpo_time.py [--repeats 5] [--out profiles/trpo_time_v1.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sac-expert_amd")]

import numpy as np   # noqa: E402

SHAPES = {"pendulum": dict(S=3, A=1), "halfcheetah": dict(S=17, A=6)}
N_ROWS, MB = 10_000, 312
PAR = dict(delta=0.02, cg_it=20, trust_sub=1, trust_damp=0.01, kl_maxfactor=1.5, ent_reg=False, ent_targ=0.0,
           alpha_lr=0.0, adv_center=True, adv_scale=True)


def build(shape, device):
    from sac_eo.engine import Engine, EngineConfig
    from sac_eo.nets import create_nn_weights
    S, A = SHAPES[shape]["S"], SHAPES[shape]["A"]
    eng = Engine(EngineConfig(s_dim=S, a_dim=A, hidden=(64, 64), activation="tanh", batch=MB, buffer_capacity=N_ROWS,
                              actor_gaussian="train", graph_steps=1, trpo=True), device=device)
    rng = np.random.default_rng(1)
    w = create_nn_weights(rng, S, A, (64, 64), 0.01)
    eng.set_net("actor", w)
    rs = np.random.RandomState(2)
    s = rs.normal(size=(N_ROWS, S)).astype(np.float32)
    mean, ls, _ = eng.dist(s)
    a = mean.cpu().numpy() + np.exp(ls.cpu().numpy()) * rs.normal(size=(N_ROWS, A)).astype(np.float32)
    adv = rs.normal(size=N_ROWS).astype(np.float32)
    eng.sync()
    return eng, w, (s, a, adv)


def time_shape(shape, repeats, say):
    import torch
    eng, w, (s, a, adv) = build(shape, torch.device("cuda"))
    dev = [torch.as_tensor(x).to(eng.device) for x in (s, a, adv)]
    plan = [l["name"] for l in eng.trpo_plan_info(N_ROWS)]
    chunks = plan.count("trpo.acc")
    say(f"trpo {shape}: one Fisher product over {N_ROWS} rows = {len(plan)} launches in {chunks} chunks of <= 4096 rows "
        f"({len(plan) // chunks} per chunk): {' | '.join(plan[:len(plan) // chunks])}")

    def reset():
        eng.set_net("actor", w)
        eng.set_logstd(np.zeros((1, SHAPES[shape]["A"]), np.float32))

    reset()
    eng.trpo_begin(*dev, **PAR)
    log = eng.trpo_step(**PAR)                            # untimed: the solve's graph is captured here
    info = eng.trpo_solve_info()
    ms = []
    for r in range(repeats):
        reset()
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.trpo_begin(*dev, **PAR)
        log = eng.trpo_step(**PAR)
        ms.append((time.perf_counter() - t0) * 1e3)
        say(f"trpo {shape} repeat {r}: {ms[-1]:.3f} ms/update")
    info = eng.trpo_solve_info()
    trials = 1 if log["adj"] == 1.0 else (11 if log["adj"] == 0.0 else 1 + int(round(-2 * np.log2(log["adj"]))))
    med = float(np.median(ms))
    say(f"trpo {shape}: {repeats} updates: median {med:.3f} ms/update, min {np.min(ms):.3f}, max {np.max(ms):.3f}; "
        f"cg iterations run {info['cg_iters']} of {PAR['cg_it']}, line-search evaluations {1 + trials} "
        f"(adj {log['adj']:.4g}, kl {float(log['kl']):.4g}, improve {float(log['improve']):.4g})")
    # one Fisher product alone, and the gradient pass
    reset()
    eng.trpo_begin(*dev, **PAR)
    x = eng.trpo_grad(flat=True)
    eng.trpo_fvp(x)
    eng.sync()
    us = []
    for r in range(repeats):
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(200):
            eng.trpo_fvp(x)
        eng.sync()
        us.append((time.perf_counter() - t0) * 1e6 / 200)
    fm = float(np.median(us))
    say(f"trpo {shape}: one Fisher product (graph replay + the two vector copies of trpo_fvp): median {fm:.1f} us "
        f"(min {np.min(us):.1f}, max {np.max(us):.1f}); {fm / len(plan):.2f} us per launch; "
        f"{PAR['cg_it'] + 1} of them = {(PAR['cg_it'] + 1) * fm / 1e3:.3f} ms of the update")
    # the PPO update of the same rollout, the same session
    reset()
    rs = np.random.RandomState(3)
    kw = dict(eps_ppo=0.2, actor_lr=3e-4, max_grad_norm=0.5, ent_reg=False, alpha_lr=0.0, ent_targ=0.0)
    draw = lambda: np.stack([rs.permutation(N_ROWS)[:MB] for _ in range(320)]).astype(np.int32)
    eng.ppo_begin(*dev)
    eng.ppo_steps(draw(), **kw)
    eng.ppo_end(0.2)
    pm = []
    for r in range(repeats):
        idx = draw()
        eng.sync()
        t0 = time.perf_counter()
        eng.ppo_begin(*dev)
        eng.ppo_steps(idx, **kw)
        eng.ppo_end(0.2)
        pm.append((time.perf_counter() - t0) * 1e3)
    pmed = float(np.median(pm))
    say(f"ppo {shape}: ppo_begin + 320 steps of {MB} rows + ppo_end: median {pmed:.3f} ms/update, min {np.min(pm):.3f}, "
        f"max {np.max(pm):.3f} ({len(eng.ppo_plan_info(MB))} launches per step)")
    say(f"summary {shape}: TRPO {med:.3f} ms | PPO {pmed:.3f} ms per update ({med / pmed:.2f}x)")
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trpo_time_v1.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trpo_time.py needs the GPU (no CPU fallback)")
    from sac_eo import _native
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)

    say(f"trpo_time: library {os.path.relpath(_native.LIB_PATH, ROOT)}; device {torch.cuda.get_device_name(0)}")
    for shape in SHAPES:
        time_shape(shape, args.repeats, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
