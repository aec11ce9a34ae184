"""SoftMaxActor (reference ``sac_eo/actors/discrete_actors.py:8-117``): the softmax policy of a
Discrete action space, for the on-policy updates (``PPO``, ``TRPO``).

The reference's class does not construct as written (it hands ``BaseActor.__init__`` four of six
arguments and reads a ``_nn`` nobody builds); this is the one reading that makes it run:
``_nn = create_nn(s_dim, a_dim, layers, activations, gain)`` with ``a_dim = flatdim(Discrete(n)) = n``,
``init_type`` 'orthogonal' and no layer norm unless passed, and ``trainable`` the net's variables only
(there is no ``logstd``).  Everything else is as written.

Until an algorithm binds it the actor holds its weights in the Keras ``get_weights()`` order; once
bound they live in the arena of a trainable engine built with ``softmax=True``, and ``neglogp`` /
``entropy`` / ``kl`` / ``get_kl_info`` run on the GPU (``sacx_ppo_*`` in their categorical meaning).
``sample`` takes the logits from the engine and draws on the host; with ``device_sample = True`` (the
model-free loop sets it: there ``sample`` runs once per env step) the draw and the pick run on the device
too (``Engine.softmax_act`` / ``softmax_act_host``), from the same stream.
"""
import numpy as np

from ..nets import create_nn_weights
from .continuous_actors import _as_out


def gumbel_argmax(logits, u):
    """``discrete_actors.py:32-40`` on f32 logits [n, A] and the uniforms u [n, A] (f64, or None for the
    deterministic form): the Gumbel noise g = float32(-log(-log u)) formed in f64 and rounded once, then the
    first-index argmax of the f32 ``(logits - max) + g`` -- the reference's
    ``argmax(a_logits - np.log(-np.log(u)))``."""
    x = np.asarray(logits, np.float32)
    x = x - x.max(axis=-1, keepdims=True)
    if u is not None:
        with np.errstate(divide="ignore"):
            g = (-np.log(-np.log(np.asarray(u, np.float64)))).astype(np.float32)
        x = x + g
    return np.argmax(x, axis=-1)


class SoftMaxActor:
    """Softmax policy for discrete action spaces."""

    squash = False
    per_state_std = False
    output_norm = False
    std_mult = 1.0
    softmax = True
    device_sample = False       # True: sample() draws and picks on the device (Engine.softmax_act*)

    def __init__(self, env, layers, activations, gain, init_type='orthogonal', layer_norm=False, rng=None):
        space = env.action_space
        if not hasattr(space, "n") or hasattr(space, "low"):
            raise TypeError("Only Discrete action space supported")
        self.s_dim = int(np.prod(env.observation_space.shape))
        self.a_dim = int(space.n)                         # flatdim(Discrete(n))
        if not 1 <= self.a_dim <= 32:
            raise NotImplementedError(f"SoftMaxActor: the device runs 1 to 32 actions (got {self.a_dim})")
        self.layers = list(layers)
        self.activations = list(activations)
        self.activation = self.activations[0]
        self.layer_norm = bool(layer_norm)
        self.gain, self.init_type = gain, init_type
        rng = rng if rng is not None else np.random.default_rng(np.random.randint(2 ** 31))
        self._w = create_nn_weights(rng, self.s_dim, self.a_dim, self.layers, gain, self.layer_norm)
        self.d = int(sum(int(np.prod(x.shape)) for x in self._w))     # :19-20
        self._engine = None
        self._net = None

    # ------------------------------------------------------------------ binding
    def _bind(self, engine, net="actor", with_logstd=False):
        """Moves the weights into ``engine`` (a softmax engine) and serves them from there."""
        if not getattr(engine.cfg, "softmax", False):
            raise RuntimeError("SoftMaxActor binds to a softmax engine (EngineConfig(actor_gaussian='train', softmax=True))")
        engine.set_net(net, self._w)
        self._engine, self._net = engine, net

    @property
    def trainable(self):
        return self.get_weights()

    def get_weights(self, flat=False):
        """``discrete_actors.py:102-107``."""
        w = self._engine.get_net(self._net) if self._engine is not None else [x.copy() for x in self._w]
        if flat:
            return np.concatenate([np.asarray(x).reshape(-1) for x in w], -1)
        return w

    def set_weights(self, weights, from_flat=False, increment=False):
        """``discrete_actors.py:109-117``: ``from_flat`` (``flat_to_list`` over the trainables),
        ``increment`` (added to the current weights); nothing is floored."""
        if from_flat:
            flat = np.asarray(weights).reshape(-1)
            if flat.size != self.d:
                raise ValueError(f"a flat weight vector holds {self.d} values, got {flat.size}")
            weights, o = [], 0
            for x in self._w:
                weights.append(flat[o:o + x.size].reshape(x.shape))
                o += x.size
        if increment:
            weights = [np.asarray(x) + y for x, y in zip(weights, self.get_weights())]
        weights = [np.asarray(x, np.float32) for x in weights]
        if len(weights) != len(self._w) or any(x.shape != y.shape for x, y in zip(weights, self._w)):
            raise ValueError("SoftMaxActor.set_weights: the list does not match the net's variables")
        self._w = weights
        if self._engine is not None:
            self._engine.set_net(self._net, self._w)

    def set_rms(self, normalizer):
        self.s_rms = normalizer.get_rms()[0]

    # ------------------------------------------------------------------ the distribution calls
    def _softmax_engine(self):
        if self._engine is None:
            raise RuntimeError("actor is not bound to a device engine (build the algorithm first)")
        return self._engine

    def _rows(self, s):
        return np.asarray(s, np.float32).reshape(-1, self.s_dim)

    def sample(self, s, deterministic=False):
        """``discrete_actors.py:22-42``: the logits from the engine; unless deterministic,
        ``u = np.random.random(size=(n, A))`` drawn under the engine's copy of the global stream, then
        the Gumbel argmax.  The deterministic form draws nothing.  ``tf.squeeze`` on the result."""
        eng = self._softmax_engine()
        if self.device_sample:
            rows = self._rows(s)
            if rows.shape[0] <= 16:                      # the env loop's few rows: one pinned copy each way
                a = eng.softmax_act_host(rows, deterministic)
            else:
                a = eng.softmax_act(rows, deterministic).cpu().numpy()
            return _as_out(np.squeeze(a.astype(np.int64)))
        logits = eng.dist(self._rows(s))[0].cpu().numpy()
        u = None
        if not deterministic:
            np.random.set_state(eng.rng_get_state())
            try:
                u = np.random.random(size=logits.shape)
            finally:
                eng.rng_set_state(np.random.get_state())
        return _as_out(np.squeeze(gumbel_argmax(logits, u)))

    def clip(self, a):
        return a

    def neglogp(self, s, a):
        """softmax_cross_entropy_with_logits(one_hot(a), logits) per row (:47-54), squeezed."""
        out = self._softmax_engine().neglogp(self._rows(s), np.asarray(a).reshape(-1)).cpu().numpy()
        return _as_out(np.squeeze(out))

    def entropy(self, s):
        """-sum_j p_j log p_j per row (:56-66)."""
        return _as_out(self._softmax_engine().dist(self._rows(s))[2].cpu().numpy())

    def get_kl_info(self, s):
        """The raw logits [n, A] (:98-100)."""
        return self._softmax_engine().dist(self._rows(s))[0].cpu().numpy()

    def kl(self, s, kl_info_ref):
        """sum_j p_cur ((l_cur - lse_cur) - (l_ref - lse_ref)) per row (:68-96)."""
        ref = np.ascontiguousarray(np.asarray(kl_info_ref, np.float32).reshape(-1, self.a_dim))
        return _as_out(self._softmax_engine().kl(self._rows(s), ref, None).cpu().numpy())
