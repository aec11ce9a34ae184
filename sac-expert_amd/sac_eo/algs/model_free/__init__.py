"""On-policy updates (reference ``sac_eo/algs/model_free/`` and ``BaseOnPolicyAlg._update_critics``).
``PPO`` trains a plain ``GaussianActor`` on the device and ``VCriticUpdate`` its ``VCritic``s; ``TRPO``
is not built."""
from .critic_update import VCriticUpdate
from .ppo import PPO, minibatches

__all__ = ["PPO", "VCriticUpdate", "minibatches"]
