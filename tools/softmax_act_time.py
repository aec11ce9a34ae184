"""Per-call time of ``SoftMaxActor.sample`` with ``device_sample`` False (logits to the host, the stream's
624-word state to the host, the draw, the state back) and True (``sacx_softmax_act_host``: draw and pick on the
device), and the phases of one ``--alg_type mfrl`` iteration.

Shapes: S = 8, A = 4 (LunarLander's), actor 64 x 2 tanh, n = 1 and 16 rows.  Per n: 200 warm-up calls per
path, then 2,000 timed calls per path, the two paths alternated call by call (each from the stream where the
other left it), three repeats; a host clock around the call, which is synchronous on either path.  Reported per
repeat and path: median, mean, p10, p90 in us; then the ratio of the medians.  Then ``time_env_data`` /
``time_critic`` / ``time_actor`` of every iteration of a discrete ``mfrl`` run (LunarLander-v2, ppo, batches of
400 steps), from its log.

Nothing is promised in advance: what is measured is written down.

Usage: softmax_act_time.py [--out profiles/softmax_act_time_v1.txt]"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sac-expert_amd")]

import numpy as np   # noqa: E402

S, A, HIDDEN = 8, 4, (64, 64)
WARM, CALLS, REPEATS = 200, 2000, 3


class _Space:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Env:
    observation_space, action_space = _Space(shape=(S,)), _Space(n=A, shape=())


def build():
    from sac_eo.actors.discrete_actors import SoftMaxActor
    from sac_eo.engine import Engine, EngineConfig
    eng = Engine(EngineConfig(s_dim=S, a_dim=A, hidden=HIDDEN, activation="tanh", batch=16, buffer_capacity=64,
                              actor_gaussian="train", graph_steps=1, softmax=True))
    actor = SoftMaxActor(_Env(), list(HIDDEN), ["tanh"], 1.0, rng=np.random.default_rng(1))
    actor._bind(eng)
    eng.rng_set_state(np.random.RandomState(3).get_state())
    return eng, actor


def time_rows(actor, eng, n, say):
    s = np.random.RandomState(5).normal(size=(n, S)).astype(np.float32)
    medians = {False: [], True: []}
    for rep in range(REPEATS):
        for dev in (False, True):
            actor.device_sample = dev
            for _ in range(WARM):
                actor.sample(s)
        t = {False: np.empty(CALLS), True: np.empty(CALLS)}
        for i in range(CALLS):
            for dev in (False, True):
                actor.device_sample = dev
                t0 = time.perf_counter()
                actor.sample(s)
                t[dev][i] = time.perf_counter() - t0
        for dev in (False, True):
            us = t[dev] * 1e6
            medians[dev].append(float(np.median(us)))
            say(f"n={n:2d} repeat {rep} device_sample={str(dev):5s}: median {np.median(us):8.1f} us  mean {us.mean():8.1f}  "
                f"p10 {np.percentile(us, 10):8.1f}  p90 {np.percentile(us, 90):8.1f}  ({CALLS} calls)")
    h, d = float(np.median(medians[False])), float(np.median(medians[True]))
    say(f"n={n:2d}: host path {h:.1f} us, device path {d:.1f} us per call (median of the repeats' medians): "
        f"host / device = {h / d:.2f}x")
    return h, d


def mfrl_iteration(say):
    import sac_eo.train as T
    from sac_eo.common.logger import load_log
    with tempfile.TemporaryDirectory() as tmp:
        path = T.main(["--alg_type", "mfrl", "--mf_algo", "ppo", "--env_name", "LunarLander-v2", "--actor_layers", "64", "64",
                       "--critic_layers", "64", "64", "--total_timesteps", "1600", "--env_batch_size_init", "400",
                       "--env_batch_size", "400", "--env_horizon", "200", "--seed", "1", "--save_path", tmp])
        tr = load_log(path)[0]["train"]
    for i in range(len(tr["steps"])):
        say(f"mfrl LunarLander-v2 ppo iteration {i}: {int(tr['steps'][i])} env steps  time_env_data {tr['time_env_data'][i] * 1e3:8.1f} ms "
            f"({tr['time_env_data'][i] / tr['steps'][i] * 1e6:6.1f} us per env step, the env and the host loop included)  "
            f"time_critic {tr['time_critic'][i] * 1e3:7.1f} ms  time_actor {tr['time_actor'][i] * 1e3:7.1f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_act_time_v1.txt"))
    args = ap.parse_args()
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)
    import torch
    say(f"softmax_act_time: S={S} A={A} hidden={HIDDEN} warm-up {WARM} timed {CALLS} repeats {REPEATS}; "
        f"{torch.cuda.get_device_name(0)}")
    eng, actor = build()
    for n in (1, 16):
        time_rows(actor, eng, n, say)
    eng.close()
    mfrl_iteration(say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
