"""init_alg (reference ``sac_eo/algs/init_alg.py:9-34``)."""
from .BC import BC
from .SAC import SAC
from .SAC_expert import SAC_exp


def init_alg(idx, env, env_eval, env_expert, actor, critics, q_targets, q_critics, models, alg_kwargs,
             mf_update_kwargs, expert, init_expert_rms_stats):
    alg_type = alg_kwargs["alg_type"]
    if alg_type == "sac":
        return SAC(idx, env, env_eval, actor, critics, q_targets, q_critics, models, alg_kwargs, mf_update_kwargs)
    if alg_type == "sac_imit":
        return SAC_exp(idx, env, env_eval, env_expert, actor, expert, init_expert_rms_stats, critics, q_targets,
                       q_critics, models, alg_kwargs, mf_update_kwargs)
    if alg_type == "bc":
        return BC(idx, env, env_eval, env_expert, actor, expert, init_expert_rms_stats, critics, q_targets,
                  q_critics, models, alg_kwargs, mf_update_kwargs)
    if alg_type == "mbrl":
        # the parser's default is 'trpo'; the reference's TRPO reads grad_final / epsilon, which exist only
        # with expert_reg (trpo.py): there is nothing sound to port, so only PPO runs
        mf_algo = alg_kwargs.get("mf_algo", "trpo")
        if mf_algo != "ppo":
            raise NotImplementedError(f"alg_type 'mbrl' with mf_algo {mf_algo!r}: TRPO is not built; pass --mf_algo ppo")
        from .mbrl_onpolicy_alg import MBRLOnPolicyAlg
        return MBRLOnPolicyAlg(idx, env, env_eval, actor, critics, models, alg_kwargs, mf_update_kwargs)
    if alg_type == "mfrl":
        # the model-free on-policy loop (base_onpolicy_alg.py): PPO or TRPO on the true environment
        mf_algo = alg_kwargs.get("mf_algo", "trpo")
        if mf_algo not in ("ppo", "trpo"):
            raise ValueError(f"alg_type 'mfrl': invalid mf_algo {mf_algo!r} (ppo or trpo)")
        from .mfrl_onpolicy_alg import MFRLOnPolicyAlg
        return MFRLOnPolicyAlg(idx, env, env_eval, actor, critics, alg_kwargs, mf_update_kwargs)
    raise ValueError("invalid alg_type")
