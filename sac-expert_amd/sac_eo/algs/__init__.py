from .init_alg import init_alg
from .BC import BC
from .SAC import SAC
from .SAC_expert import SAC_exp

__all__ = ["init_alg", "BC", "SAC", "SAC_exp"]
