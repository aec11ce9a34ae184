"""init_actor (reference ``sac_eo/actors/init_actor.py:8-30``)."""
from .continuous_actors import GaussianActor, SquashedGaussianActor
from .discrete_actors import SoftMaxActor


def init_actor(env, actor_layers, actor_activations, actor_gain, actor_std_mult, actor_init_type, actor_layer_norm,
               actor_weights, actor_per_state_std=False, actor_squash=False, actor_output_norm=False, **unused):
    """Builds the actor: the squashed Gaussian with ``actor_squash`` (the SAC learner), else the
    plain Gaussian (an imported expert, or the on-policy learner).  A Discrete space (``.n`` and no
    ``.low``) gives the SoftMaxActor of the on-policy path, which ignores ``actor_squash``,
    ``actor_per_state_std``, ``actor_output_norm`` and ``actor_std_mult`` as the reference does
    (``init_actor.py:8-30``)."""
    if hasattr(env.action_space, "n") and not hasattr(env.action_space, "low"):
        actor = SoftMaxActor(env, actor_layers, actor_activations, actor_gain, actor_init_type, actor_layer_norm)
        if actor_weights is not None:
            actor.set_weights(actor_weights)
        return actor
    if not hasattr(env.action_space, "low"):
        raise TypeError("Only Box and Discrete action spaces are supported")
    cls = SquashedGaussianActor if actor_squash else GaussianActor
    actor = cls(env, actor_layers, actor_activations, actor_gain, actor_init_type, actor_layer_norm, actor_std_mult,
                actor_per_state_std, actor_output_norm)
    if actor_weights is not None:
        actor.set_weights(actor_weights)
    return actor
