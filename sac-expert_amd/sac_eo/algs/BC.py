"""BC — imitation only, through the world models (reference ``sac_eo/algs/BC.py``).

The reference's ``BC.py`` differs from its ``SAC_expert.py`` in the update alone: ``_update``
(``:303-306``) runs ``_update_actor`` (``:309-363``) -- ``actor.sample(s_e)`` through world models
0 / 1 (or model 0 alone), ``MSE_loss = mean(0.5 sum (sp_e - sp_pred)^2)``, Adam on the actor -- and
nothing else: no replay batch, no targets, no critics, no alpha, no Polyak step.  The env loop, the
per-episode model fit, the expert collection and batch draw, the MSE diagnostics and the adaptive
epsilon preprocessing are SAC_exp's, inherited here; the engine is built with ``bc=True``
(``sacx_config.use_expert = SACX_EXPERT_BC``), so ``Engine.step`` runs the critic-free update chain and
draws only the reference's randoms (the expert normals; the ``self.rng.shuffle`` permutation comes
from ``_pre_update`` as in SAC-EO).  The critics, targets and alpha are constructed, bound and dumped
as in the reference, and never trained.
"""
import numpy as np

from .SAC_expert import SAC_exp


class BC(SAC_exp):
    def __init__(self, idx, env, env_eval, env_expert, actor, expert, init_expert_rms_stats, v_critic, q_targets,
                 q_critics, models, alg_kwargs, mf_update_kwargs):
        super().__init__(idx, env, env_eval, env_expert, actor, expert, init_expert_rms_stats, v_critic, q_targets,
                         q_critics, models, alg_kwargs, mf_update_kwargs)

    def _engine_config(self, k):
        cfg = super()._engine_config(k)
        cfg.bc = True
        return cfg

    def _flush_update_logs(self):
        """The per-update log of _update_actor (BC.py:360-363): BC_MSE_loss alone, read back from the
        device statistics ring."""
        n = len(self._eps_log)
        if n == 0:
            return
        st = self.engine.stats(n)
        for i in range(n):
            self.logger.log_train({"BC_MSE_loss": np.float32(st[i, 5])})
        self._eps_log = []
