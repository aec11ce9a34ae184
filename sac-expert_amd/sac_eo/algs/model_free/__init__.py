"""On-policy updates (reference ``sac_eo/algs/model_free/`` and ``BaseOnPolicyAlg._update_critics``).
``PPO`` trains a plain ``GaussianActor`` on the device and ``VCriticUpdate`` its ``VCritic``s.  ``TRPO`` lives
in ``sac_eo.algs.model_free.trpo`` and is importable by that path only: it is not re-exported here while
``init_alg`` refuses ``mf_algo='trpo'``."""
from .critic_update import VCriticUpdate
from .ppo import PPO, minibatches

__all__ = ["PPO", "VCriticUpdate", "minibatches"]
