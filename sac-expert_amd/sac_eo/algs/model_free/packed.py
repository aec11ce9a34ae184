"""K learners' on-policy updates in one launch chain (the reference's ``--runs K``, ``train.py:148-152``, over
``ppo.py:55-83`` and ``base_onpolicy_alg.py:219-283``).

``update_packed(updaters, rollouts)`` takes K ``PPO`` objects, or K ``VCriticUpdate`` objects, bound to the K
learners of ONE ``EngineConfig(learners=K)`` engine (each through its ``SeedView``), in learner order, and
each learner's rollout: for ``PPO`` the reference's 6-tuple, for ``VCriticUpdate`` ``(rollout_data_all, B)``.
It runs every learner's prepare (``*_begin`` and the shuffles, drawn from that learner's own stream), then
ONE packed steps call (``Engine.ppo_steps_packed`` / ``vcritic_steps_packed``: every learner's minibatch steps
in the launches of one learner's), then every finish (``*_end``, the log, adaptlr).  It returns the K logs
that ``update`` on K one-learner engines returns: each learner's steps are bit-identical to its own run's.

The learners must ask for the same number of steps of the same minibatch size; otherwise ``RuntimeError``."""
import numpy as np

from .critic_update import VCriticUpdate
from .ppo import PPO


def _shared_engine(updaters):
    views = [u.engine for u in updaters]
    eng = getattr(views[0], "_eng", None)
    if eng is None or any(getattr(v, "_eng", None) is not eng for v in views):
        raise ValueError("update_packed: the updaters must be bound to the learners of one packed engine "
                         "(EngineConfig(learners=K), one SeedView each)")
    if [int(v.seed_index) for v in views] != list(range(int(eng.seeds))):
        raise ValueError(f"update_packed: one updater per learner of the engine, in learner order (it holds {eng.seeds})")
    return eng


def update_packed(updaters, rollouts):
    updaters, rollouts = list(updaters), list(rollouts)
    if not updaters or len(updaters) != len(rollouts):
        raise ValueError("update_packed: one rollout per updater")
    ppo = isinstance(updaters[0], PPO)
    if not all(isinstance(u, PPO if ppo else VCriticUpdate) for u in updaters):
        raise ValueError("update_packed: a list of PPO objects, or a list of VCriticUpdate objects")
    ctxs = [u.update_prepare(r) if ppo else u.update_prepare(*r) for u, r in zip(updaters, rollouts)]
    eng = _shared_engine(updaters)
    shapes = {None if c["idx"] is None else tuple(c["idx"].shape) for c in ctxs}
    if len(shapes) != 1:
        raise RuntimeError("packed runs diverged: the learners' updates differ in (n_steps, minibatch rows) "
                           f"({sorted(map(str, shapes))}); use --serial_runs or drop --pack_runs")
    if ctxs[0]["idx"] is not None:
        idx = np.stack([c["idx"] for c in ctxs])
        lrs = [c["lr"] for c in ctxs]
        if ppo:
            par = updaters[0].step_params()
            if any(u.step_params() != par for u in updaters):
                raise ValueError("update_packed: the learners' PPO parameters differ (only actor_lr is per learner)")
            eng.ppo_steps_packed(idx, actor_lr=lrs, **par)
        else:
            eng.vcritic_steps_packed(idx, critic_lr=lrs)
    return [u.update_finish(c) for u, c in zip(updaters, ctxs)]
