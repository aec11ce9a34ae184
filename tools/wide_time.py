"""Wide hidden layers (513 .. 1,024) at the HalfCheetah SAC-EO shapes (S 17, A 6, B 256, 20 expert rows,
model minibatch 200): the launches of one update (plan_info) and one fit step (model_plan_info), us per
update of graph replays (sacx_time_graph) and us per graph-replayed fit step (as tools/model_fit_time.py).
usage: python tools/wide_time.py [model widths] [actor widths] [critic widths]   (comma separated;
defaults 1024,1024 / 256,256 / the actor's).  512,512 gives the fused plan's figures to compare with."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sac-expert_amd")]

import numpy as np   # noqa: E402


def widths(i, default):
    return tuple(int(x) for x in sys.argv[i].split(",")) if len(sys.argv) > i and sys.argv[i] else default


def main():
    import torch
    from sac_eo.engine import Engine, EngineConfig
    from sac_eo.nets import create_nn_weights
    mh, ah = widths(1, (1024, 1024)), widths(2, (256, 256))
    ch = widths(3, ah)
    S, A, B, N, ne = 17, 6, 256, 200_000, 20
    dev = torch.device("cuda", 0)
    eng = Engine(EngineConfig(s_dim=S, a_dim=A, hidden=ah, critic_hidden=None if ch == ah else ch, activation="relu", batch=B,
                              buffer_capacity=N, use_expert=True, expert_batch=ne, expert_capacity=ne,
                              model_hidden=mh, graph_steps=int(os.environ.get("SACX_GRAPH_STEPS", "256"))), device=dev)
    rng = np.random.default_rng(0)
    eng.set_net("actor", create_nn_weights(rng, S, A, ah, 0.01))
    for j in range(2):
        w = create_nn_weights(rng, S + A, 1, ch, 1.0)
        eng.set_net(f"q{j}", w)
        eng.set_net(f"t{j}", w)
        eng.set_net(f"m{j}", create_nn_weights(rng, S + A, S + 1, mh, 0.01))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    sig = torch.rand(S, device=dev, generator=g) * 4.9 + 0.1
    eng.append(torch.randn(N, S, device=dev, generator=g) * sig, torch.rand(N, A, device=dev, generator=g) * 2 - 1,
               torch.randn(N, device=dev, generator=g), torch.randn(N, S, device=dev, generator=g) * sig,
               torch.zeros(N, device=dev))
    ers = np.random.RandomState(2)
    eng.set_expert(ers.normal(size=(ne, S)), ers.normal(size=(ne, S)), 1e-3)
    gen = np.random.default_rng(3)
    eng.push_perms(np.stack([gen.permutation(ne) for _ in range(4096)]))
    eng.sync()
    tag = f"actor {ah} critics {ch} models {mh}"
    plan = [p for p in eng.plan_info()]
    print(f"{tag}: {len(plan)} launches per update:", " ".join(p["name"] for p in plan), flush=True)
    eng.step(eng.cfg.graph_steps)
    eng.sync()
    for rep in range(3):
        print(f"{tag}: update {eng.time_graph(4) * 1e3:.2f} us (graph replay, sacx_time_graph)", flush=True)
    mb, n = eng.cfg.model_batch, 512
    idx = np.random.RandomState(3).randint(N, size=(n + 64, 2, mb)).astype(np.int32)
    eng.model_fit(idx[:64])
    eng.sync()
    fit = eng.model_plan_info()
    print(f"{tag}: {len(fit)} launches per fit step:", " ".join(p["name"] for p in fit), flush=True)
    for rep in range(3):
        t0 = time.perf_counter()
        eng.model_fit(idx[64:])
        eng.sync()
        print(f"{tag}: fit step {(time.perf_counter() - t0) / n * 1e6:.2f} us (graph replay, {n} steps); "
              f"last loss {eng.model_stats(1)[0]}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
