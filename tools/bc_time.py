"""Time of one update through Engine.step at the HalfCheetah shapes (S 17, A 6, actor / critics
256 x 2, world models 512 x 2, batch 256, 20 expert rows): the BC update (--leg bc) or the SAC-EO
update (--leg eo, the comparison point: BC's dependent chain is a strict subset of it).

The permutation ring is filled once; the graphs are captured (prepare) and one untimed call of the
same size runs first.  Per repeat: the device is synchronised, then a host clock around
step(--updates) + synchronise.  Prints each repeat, the median and the minimum in
us / update, and the plan's launch count (chain launches: without the sampler and the gather).
SACX_LIBPATH selects the library, so `--leg eo` can run on another build of libsacx.

Usage: bc_time.py --leg bc|eo [--updates 2000] [--repeats 7] [--generic]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sac-expert_amd")]

import numpy as np   # noqa: E402


def build(leg, device, buffer_rows=1_000_000):
    import torch
    from sac_eo.engine import Engine, EngineConfig
    from sac_eo.nets import create_nn_weights
    S, A, hidden = 17, 6, (256, 256)
    kw = dict(bc=True) if leg == "bc" else {}
    ecfg = EngineConfig(s_dim=S, a_dim=A, hidden=hidden, activation="relu", batch=256, buffer_capacity=buffer_rows,
                        use_expert=True, expert_batch=20, expert_capacity=20, graph_steps=256, **kw)
    eng = Engine(ecfg, device=device)
    rng = np.random.default_rng(1)
    eng.set_net("actor", create_nn_weights(rng, S, A, hidden, 0.01))
    for j in range(2):
        w = create_nn_weights(rng, S + A, 1, hidden, 1.0)
        eng.set_net(f"q{j}", w)
        eng.set_net(f"t{j}", w)
        eng.set_net(f"m{j}", create_nn_weights(rng, S + A, S + 1, (512, 512), 0.01))
    g = torch.Generator(device=device)
    g.manual_seed(2)
    N = buffer_rows
    sig = torch.rand(S, device=device, generator=g) * 4.9 + 0.1
    eng.append(torch.randn(N, S, device=device, generator=g) * sig, torch.rand(N, A, device=device, generator=g) * 2 - 1,
               torch.randn(N, device=device, generator=g), torch.randn(N, S, device=device, generator=g) * sig,
               torch.zeros(N, device=device))
    ers = np.random.RandomState(3)
    eng.set_expert(ers.normal(size=(20, S)), ers.normal(size=(20, S)), 1e-3)
    eng.rng_seed(4)
    eng.sync()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("bc", "eo"), required=True)
    ap.add_argument("--updates", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--generic", action="store_true", help="the generic plan (SACX_GENERIC=1)")
    args = ap.parse_args()
    if args.generic:
        os.environ["SACX_GENERIC"] = "1"
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bc_time.py needs the GPU (no CPU fallback)")
    from sac_eo import _native
    eng = build(args.leg, torch.device("cuda"))
    plan = eng.plan_info()
    chain = [l["name"] for l in plan if l["name"] not in ("rng", "gather")]
    n = args.updates
    gen = np.random.default_rng(5)                        # the whole permutation ring, once (as bench.py)
    eng.push_perms(np.stack([gen.permutation(20) for _ in range(eng.cfg.perm_capacity)]))
    eng.prepare(n)
    eng.step(n, num_timesteps=0, ts_increment=1)          # untimed: every graph replayed once
    eng.sync()
    us = []
    for r in range(args.repeats):
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.step(n, num_timesteps=0, ts_increment=1)
        eng.sync()
        us.append((time.perf_counter() - t0) * 1e6 / n)
        print(f"leg {args.leg} repeat {r}: {us[-1]:.3f} us/update", flush=True)
    row = eng.stats(1)[0]
    print(f"leg {args.leg}{' (generic plan)' if args.generic else ''}: library {_native.LIB_PATH}")
    print(f"leg {args.leg}: {len(chain)} chain launches (+ sampler, gather): {' | '.join(chain)}")
    print(f"leg {args.leg}: {n} updates x {args.repeats}: median {np.median(us):.3f} us/update, min {np.min(us):.3f}, "
          f"max {np.max(us):.3f}  ({1e6 / np.median(us):.0f} updates/s); last stats row p_loss {row[2]:.6g} mse {row[5]:.6g}")
    eng.close()


if __name__ == "__main__":
    main()
