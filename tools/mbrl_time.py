"""Time of the sim data of one policy update of alg_type mbrl, on the device (Engine.sim_collect +
Engine.gae, rows never leaving the GPU) against the host path the tree offers for the same work
(Engine.rollout -> host TrajectoryBuffer.add_batch -> get_update_info -> NumPy rows), and of one whole
``_update_actor_critic`` iteration split into sim data / critic / actor.

Shapes: HalfCheetah (S 17, A 6) with the parser's defaults: sim_batch_size 10,000 and sim_horizon 5 over 2
models (1,000 trajectories of 5 steps per model), models 512 x 2 relu, actor and one critic 64 x 2 tanh,
32 minibatches x 10 iterations (320 steps of 312 rows), an env ring holding 20,000 rows.

Per path one untimed pass (graphs captured, staging allocated), then ``--repeats`` timed passes, the two
paths ALTERNATING; a timed pass is: device synchronised, a host clock around the work and a final
synchronise.  "Ready" means: the tables ``vcritic_begin`` / ``ppo_begin`` take exist -- CUDA tensors on the
device path, NumPy arrays on the host path (whose upload the updates then still pay).  Reported: each
repeat, median, min - max; the launches of one ``sim_collect`` and of a ``rollout`` of the same shape
(the captured graphs' kernel nodes); ``sim_collect`` alone against launches x the PPO step's us per launch
measured in the same session (tools/ppo_time.py).

Usage: mbrl_time.py [--repeats 7] [--out profiles/mbrl_time_v1.txt]"""
import argparse
import contextlib
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sac-expert_amd")]

import numpy as np   # noqa: E402

S, A, NM, SIM, H, NMB, ITS, HELD = 17, 6, 2, 10_000, 5, 32, 10, 20_000
GAMMA, LAM = 0.995, 0.97
PER = SIM // NM
NTRAJ = PER // H
MB = SIM // NMB


def build(device):
    from sac_eo.engine import Engine, EngineConfig
    from sac_eo.nets import create_nn_weights
    eng = Engine(EngineConfig(s_dim=S, a_dim=A, hidden=(64, 64), activation="tanh", batch=MB, buffer_capacity=HELD,
                              actor_gaussian="train", world_models=True, vcritics=1, model_hidden=(512, 512),
                              model_activation="relu", num_models=NM, model_batch=200, graph_steps=1, gamma=GAMMA),
                 device=device)
    rng = np.random.default_rng(1)
    eng.set_net("actor", create_nn_weights(rng, S, A, (64, 64), 0.01))
    eng.set_net("v0", create_nn_weights(rng, S, 1, (64, 64), 1.0))
    for k in range(NM):
        eng.set_net(f"m{k}", create_nn_weights(rng, S + A, S + 1, (512, 512), 0.01))
    rs = np.random.RandomState(2)
    rows = [rs.normal(size=(HELD, S)).astype(np.float32), rs.uniform(-1, 1, (HELD, A)).astype(np.float32),
            rs.normal(size=HELD).astype(np.float32), rs.normal(size=(HELD, S)).astype(np.float32), np.zeros(HELD, np.float32)]
    eng.append(*rows)
    eng.rng_seed(5)
    eng.sync()
    return eng, rows[0]


class _BoundCritic:
    """What gae_batch needs of a critic bound to a device engine."""

    def __init__(self, eng):
        self._engine, self._index, self._net = eng, 0, "v0"


@contextlib.contextmanager
def host_rng(eng):
    np.random.set_state(eng.rng_get_state())
    try:
        yield
    finally:
        eng.rng_set_state(np.random.get_state())


def device_tables(eng):
    import torch
    per = []
    for k in range(NM):
        s, a, r, sp, d, traj = eng.sim_collect(k, NTRAJ, H)
        adv, rtg, rtg_sp = eng.gae(0, s, r, sp, d, traj, GAMMA, LAM)
        per.append((s, a, adv, rtg))
    return tuple(torch.cat(x, 0) for x in zip(*per))


def host_tables(eng, held_s, critic):
    from sac_eo.common.buffer_utils import aggregate_data
    from sac_eo.common.buffers import TrajectoryBuffer
    per = []
    for k in range(NM):
        with host_rng(eng):                              # TrajectoryBuffer.get_states(batch_size)
            idx = np.random.randint(HELD, size=NTRAJ)
        out = [t.cpu().numpy() for t in eng.rollout(k, held_s[idx], H)]
        buf = TrajectoryBuffer(S, A, GAMMA, LAM, None)
        buf.add_batch(*out)
        s, a, adv, rtg, _, _ = buf.get_update_info(critic)
        per.append((s, a, adv, rtg))
    return tuple(aggregate_data(x) for x in zip(*per))


def clocked(fn, eng):
    import torch
    eng.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3, out


def stats(x):
    return f"median {np.median(x):.3f} ms, min {np.min(x):.3f}, max {np.max(x):.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mbrl_time_v1.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mbrl_time.py needs the GPU (no CPU fallback)")
    from sac_eo import _native
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)

    say(f"mbrl_time: library {os.path.relpath(_native.LIB_PATH, ROOT)}; device {torch.cuda.get_device_name(0)}")
    say(f"shapes: S {S} A {A}, {NM} models 512x2, {NTRAJ} trajectories x {H} steps per model ({SIM} rows per update), "
        f"{ITS} x {NMB} minibatches of {MB}, ring of {HELD} rows")
    eng, held_s = build(torch.device("cuda"))
    critic = _BoundCritic(eng)
    # untimed passes: graphs captured, staging allocated
    device_tables(eng)
    n_collect = eng.rollout_launches()
    host_tables(eng, held_s, critic)
    n_roll = eng.rollout_launches()
    say(f"launches: one sim_collect({NTRAJ} x {H}) = {n_collect} kernel launches; a rollout of the same shape = {n_roll}")
    dev, host = [], []
    for r in range(args.repeats):                        # alternating
        dev.append(clocked(lambda: device_tables(eng), eng)[0])
        host.append(clocked(lambda: host_tables(eng, held_s, critic), eng)[0])
        say(f"sim data repeat {r}: device {dev[-1]:.3f} ms, host path {host[-1]:.3f} ms")
    say(f"sim data per policy update, device (sim_collect + gae, CUDA tables): {stats(dev)}")
    say(f"sim data per policy update, host path (rollout -> TrajectoryBuffer -> get_update_info, NumPy tables): {stats(host)}")
    say(f"ratio of medians host / device: {np.median(host) / np.median(dev):.1f}x")
    # sim_collect alone (both models), and the whole iteration's three parts
    only = [clocked(lambda: [eng.sim_collect(k, NTRAJ, H) for k in range(NM)], eng)[0] for _ in range(args.repeats)]
    say(f"sim_collect alone, {NM} calls: {stats(only)}")
    rs = np.random.RandomState(3)
    par = dict(eps_ppo=0.2, actor_lr=3e-4, max_grad_norm=0.5, ent_reg=False, alpha_lr=3e-4, ent_targ=-float(A))

    def shuffles(n):
        out = []
        for _ in range(ITS):
            idx = np.arange(n)
            rs.shuffle(idx)
            out.append(idx[:NMB * MB].reshape(NMB, MB))
        return np.concatenate(out).astype(np.int32)

    def critic_update(t):
        eng.vcritic_begin(0, t[0], t[3])
        eng.vcritic_steps(shuffles(SIM), critic_lr=3e-4)
        return eng.vcritic_end()

    def actor_update(t):
        eng.ppo_begin(t[0], t[1], t[2])
        eng.ppo_steps(shuffles(SIM), **par)
        return eng.ppo_end(0.2)

    tabs = device_tables(eng)
    critic_update(tabs)
    actor_update(tabs)                                   # untimed: the step graphs captured
    parts = {"sim data": [], "critic": [], "actor": []}
    for r in range(args.repeats):
        t_sim, tabs = clocked(lambda: device_tables(eng), eng)
        t_c, _ = clocked(lambda: critic_update(tabs), eng)
        t_a, _ = clocked(lambda: actor_update(tabs), eng)
        for k, v in zip(parts, (t_sim, t_c, t_a)):
            parts[k].append(v)
        say(f"iteration repeat {r}: sim data {t_sim:.3f} ms, critic {t_c:.3f} ms, actor {t_a:.3f} ms")
    for k, v in parts.items():
        say(f"one _update_actor_critic iteration, {k}: {stats(v)}")
    tot = sum(np.median(v) for v in parts.values())
    say("shares of the iteration (medians): " + ", ".join(f"{k} {100 * np.median(v) / tot:.0f} %" for k, v in parts.items()))
    eng.close()
    spec = importlib.util.spec_from_file_location("ppo_time", os.path.join(ROOT, "tools", "ppo_time.py"))
    pt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pt)
    med, n = pt.time_ppo("halfcheetah", 320, 5, say)         # the yardstick, same session
    per = med / n
    want = NM * n_collect * per / 1e3
    say(f"summary: {NM} x {n_collect} launches x {per:.3f} us (the PPO step's per launch) = {want:.3f} ms expected for "
        f"sim_collect alone, {np.median(only):.3f} ms measured ({np.median(only) / want:.2f}x)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
