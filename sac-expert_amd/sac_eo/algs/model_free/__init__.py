"""On-policy actor updates (reference ``sac_eo/algs/model_free/``).  ``PPO`` trains a plain
``GaussianActor`` on the device; ``TRPO`` and the critic update are not built."""
from .ppo import PPO, minibatches

__all__ = ["PPO", "minibatches"]
