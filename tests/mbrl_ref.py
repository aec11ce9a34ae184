"""The model-based on-policy loop (``_collect_sim_data_all``, ``_update_models``, ``_update_actor_critic``:
``UpdateRef`` at the end, composed from the oracle's model-fit step, ``vcritic_ref`` and ``ppo_ref``) and its
data path (reference ``sac_eo/algs/mbrl_onpolicy_alg.py:76-100`` over
``sac_eo/common/buffers.py`` get_states, ``sac_eo/common/samplers.py:73-122`` and
``sac_eo/actors/continuous_actors.py:103-127``) restated in NumPy on the oracle's primitives.  Test
infrastructure only.

The compute dtype is the state's (``O.SACState.astype``): fp64 for the parity bars, fp32 for envelopes.
The state is the oracle's ``SACState`` (its actor / logstd read as a plain GaussianActor, its world
models); ``std_mult`` is the actor's ``--actor_std_mult``.
"""
import numpy as np

import sac_oracle as O


def ring_rows(rows, capacity):
    """What a FIFO ring of ``capacity`` rows holds after ``rows`` were appended, oldest first
    (TrajectoryBuffer's truncation, buffers.py:41-71): logical row 0 = the oldest row held."""
    rows = np.asarray(rows)
    return rows[max(0, rows.shape[0] - capacity):]


def draw_indices(rs, rows_held, n_traj):
    """TrajectoryBuffer.get_states(batch_size): np.random.randint(rows_held, size=n_traj)."""
    return rs.randint(rows_held, size=n_traj)


def sim_rollout(st, cfg, nrm, s_init, horizon, k, rs, deterministic=False, delta_clip=0.0, reward_clip=0.0,
                std_mult=1.0, clip_action=True):
    """batch_simtrajectory_sampler (samplers.py:73-122) with GaussianActor.sample
    (continuous_actors.py:103-123) and world model ``k`` as the env: per step a = mean + exp(logstd) u,
    u = rs.normal(size=(n, A)) cast to f32 (none when deterministic); the model steps on
    actor.clip(a) (:125-127; ``clip_action=False`` leaves it out: the tests' counter-example); a
    GaussianModel then draws rs.normal(size=(n, S)).  -> (s, a, r, sp, d) of shapes [n,H,S], [n,H,A],
    [n,H], [n,H,S], [n,H]; ``a`` is the raw action."""
    dt = st.alpha.dtype.type
    F = lambda x: O._F(dt, x)
    nrmc = nrm.cast(dt)
    s = np.asarray(s_init, dt).reshape(-1, cfg.S)
    n = s.shape[0]
    lim = F(cfg.act_limit)
    out = dict(s=[], a=[], r=[], sp=[], d=[])
    for _ in range(horizon):
        u = np.zeros((n, cfg.A), dt) if deterministic else O.f32_noise(rs.normal(size=(n, cfg.A))).astype(dt)
        a = O.gaussian_actor_sample(st.actor, st.logstd, cfg, nrm, s, u, std_mult=std_mult)
        ac = np.clip(a, -lim, lim) if clip_action else a
        xm = np.concatenate([O._norm(s, nrmc.s_mean, nrmc.s_den), O._norm(ac, nrmc.a_mean, nrmc.a_den)], 1)
        dn, rn, _ = O.model_predict(st, cfg, k, xm)
        if delta_clip:
            dn = np.clip(dn, -F(delta_clip), F(delta_clip))
        if reward_clip:
            rn = np.clip(rn, -F(reward_clip), F(reward_clip))
        if cfg.gaussian_model:
            dn = O._model_noise(st, cfg, k, dn, O.f32_noise(rs.normal(size=dn.shape)))
        sp = s + (dn * nrmc.d_den + nrmc.d_mean)
        r = rn * nrmc.r_den + nrmc.r_mean
        for key, v in (("s", s), ("a", a), ("r", r), ("sp", sp), ("d", np.zeros(n, bool))):
            out[key].append(v)
        s = sp
    return tuple(np.stack(out[key], axis=1) for key in ("s", "a", "r", "sp", "d"))


def sim_collect(st, cfg, nrm, ring_s, n_traj, horizon, k, rs, **kw):
    """One pass of _collect_sim_data (mbrl_onpolicy_alg.py:89-93): the index draw, s_all[idx], the
    rollout.  ``ring_s``: the states held, oldest first.  -> (idx, (s, a, r, sp, d)) with the rows
    flattened trajectory-major ([n H, .]: add_batch's order) and traj = the running trajectory id."""
    idx = draw_indices(rs, ring_s.shape[0], n_traj)
    s, a, r, sp, d = sim_rollout(st, cfg, nrm, ring_s[idx], horizon, k, rs, **kw)
    n, H = s.shape[0], s.shape[1]
    traj = np.repeat(np.arange(n, dtype=np.int32), H)
    return idx, (s.reshape(n * H, -1), a.reshape(n * H, -1), r.reshape(-1), sp.reshape(n * H, -1), d.reshape(-1), traj)


def losses_eval(st, cfg, nrm, k, s, sp, a, r):
    """get_losses_eval (continuous_models.py:304-319, :133-148): (mse_loss, r_loss), no clip, the plain
    squared error of the predicted mean for either model class."""
    dt = st.alpha.dtype.type
    nrmc = nrm.cast(dt)
    s, sp, a, r = [np.asarray(x, dt) for x in (s, sp, a, r)]
    pred, _, _ = O.model_forward(st, cfg, nrm, k, s, a)
    dn = ((sp - s) - nrmc.d_mean) / nrmc.d_den
    rn = (r - nrmc.r_mean) / nrmc.r_den
    half = O._F(dt, 0.5)
    return (float(np.mean(half * ((dn - pred[:, :cfg.S]) ** 2).sum(-1))),
            float(np.mean(half * (rn - pred[:, cfg.S]) ** 2)))


# ---------------------------------------------------------------------------------------------------
# The global stream through one MBRLOnPolicyAlg iteration: the draws of _collect_env_data (one
# normal(size=(1, A)) per env step), _update_models and _update_actor_critic in the reference's order,
# and nothing else.  Values are not computed: these functions only move ``rs``.
def model_fit_draws(rs, n_all, B, epochs, model_batch, shuffle=True, holdout_ratio=0.0, holdout_epochs=5,
                    max_updates=1e5, holdout_loss=lambda ep: 0.0):
    """_update_models (mbrl_onpolicy_alg.py:188-261).  -> (epochs run, steps per fit call)."""
    n_train = n_all
    if holdout_ratio > 0.0:
        n_train = int(n_all * (1 - holdout_ratio))
        rs.shuffle(np.arange(n_all))
    best, since, updates, calls, pending = np.inf, 0, 0, [], 0
    ep = -1
    for ep in range(epochs):
        for _ in range(B if shuffle else 1):
            rs.shuffle(np.arange(n_train))
        per_epoch = n_train // model_batch
        take = int(min(per_epoch, max_updates - updates))
        updates += take
        pending += take
        stop = updates >= max_updates
        if holdout_ratio > 0.0 or stop:
            calls.append(pending)
            pending = 0
        if stop:
            break
        if holdout_ratio > 0.0:
            loss = holdout_loss(ep)
            if loss < best:
                best, since = loss, 0
            else:
                since += 1
            if since >= holdout_epochs:
                break
    if pending:
        calls.append(pending)
    return ep + 1, calls


def sim_passes(per_model, horizon, batch_type="steps"):
    """The (num_traj, horizon) passes of _collect_sim_data (mbrl_onpolicy_alg.py:76-100)."""
    out, cur = [], 0
    while cur < per_model:
        remaining = per_model - cur
        if batch_type == "steps":
            n, h = int(remaining / horizon), horizon
            if n == 0:
                n, h = 1, remaining
        else:
            n, h = remaining, horizon
        out.append((n, h))
        cur += n * h if batch_type == "steps" else n
    return out


def actor_critic_draws(rs, rows_held, B, S, A, sim_batch_size, horizon, num_mf_updates, num_critics, critic_it,
                       critic_nmb, actor_it, actor_nmb, gaussian_model=False, batch_type="steps", sim_buffer_size=None):
    """_update_actor_critic (mbrl_onpolicy_alg.py:124-174): per update and model the passes' index draws and
    step normals, then the critic update's shuffles (base_onpolicy_alg.py:231-242) and the PPO update's
    (ppo.py:48-62).  -> rows per update."""
    per_model = int(sim_batch_size / B)
    rows_upd = []
    for _ in range(num_mf_updates):
        tables = []
        for _k in range(B):
            rows = 0
            for n, h in sim_passes(per_model, horizon, batch_type):
                rs.randint(rows_held, size=n)
                for _t in range(h):
                    rs.normal(size=(n, A))
                    if gaussian_model:
                        rs.normal(size=(n, S))
                rows += n * h
            tables.append(min(rows, sim_buffer_size) if sim_buffer_size else rows)
        n_crit = min(tables) if num_critics == B else sum(tables)
        for _i in range(critic_it):
            rs.shuffle(np.arange(n_crit))
        for _i in range(actor_it):
            rs.shuffle(np.arange(sum(tables)))
        rows_upd.append(sum(tables))
    return rows_upd


# ---------------------------------------------------------------------------------------------------
# The VALUES of one MBRLOnPolicyAlg._update(): _update_models and _update_actor_critic over
# _collect_sim_data_all, composed from the oracle's model-fit step, vcritic_ref and ppo_ref.  The compute
# dtype is the states' (fp64 for the bars; fp32 under sac_oracle.MATMUL_ORDERS for the envelope).
class UpdateRef:
    """``sac``: the oracle's SACState (its world models and their optimiser; its actor / logstd are
    re-pointed at ``ppo``'s before every rollout), ``ppo``: ppo_ref.PPOState, ``vst``: vcritic_ref.VState;
    ``rows``: the env data held, oldest first (s, a, sp, r); ``kw``: the algorithm's keys; ``rs``: the
    global stream."""

    def __init__(self, sac, ppo, vst, cfg, vacts, nrm, rows, kw, ppo_kw, rs):
        import ppo_ref as R
        import vcritic_ref as V
        self.R, self.V = R, V
        self.sac, self.ppo, self.vst, self.cfg, self.vacts, self.nrm = sac, ppo, vst, cfg, list(vacts), nrm
        self.rows, self.kw, self.rs = rows, dict(kw), rs
        self.B = len(sac.models)
        self.dt = ppo.alpha.dtype.type
        self.ppo_ref = R.PPORef(ppo, cfg, nrm, ppo_kw, rs)
        self.vc_ref = V.VCriticUpdateRef(vst, self.vacts, nrm, dict(critic_lr=kw["critic_lr"],
                                                                    critic_update_it=kw["critic_update_it"],
                                                                    critic_nminibatch=kw["critic_nminibatch"]), rs)

    # ------------------------------------------------------------------ mbrl_onpolicy_alg.py:176-298
    def update_models(self):
        kw, rs, sac, cfg, nrm, B = self.kw, self.rs, self.sac, self.cfg, self.nrm, self.B
        s_all, a_all, sp_all, r_all = self.rows
        n_all = len(r_all)
        take = lambda idx: (s_all[idx], a_all[idx], sp_all[idx], r_all[idx])
        loss = lambda k, d: O.model_loss(sac, cfg, nrm, k, d[0], d[2], d[1], d[3], kw.get("delta_clip_loss") or 0.0,
                                         kw.get("reward_clip_loss") or 0.0)
        ratio = kw["model_holdout_ratio"]
        train, hold, n_train = take(np.arange(n_all)), None, n_all
        if ratio > 0.0:
            n_train = int(n_all * (1 - ratio))
            idx = np.arange(n_all)
            rs.shuffle(idx)
            train, hold = take(idx[:n_train]), take(idx[n_train:])
        best, since, updates, mb = np.inf, 0, 0, kw["model_batch_size"]
        ep = -1
        for ep in range(kw["model_num_epochs"]):
            idx = np.tile(np.arange(n_train), (B, 1))
            for row in idx:
                rs.shuffle(row)
            parts = np.array_split(idx, np.arange(0, n_train, mb)[1:], axis=1)
            if n_train % mb != 0:
                parts = parts[:-1]
            for p in parts:
                O.model_fit_step(sac, cfg, nrm, [(train[0][p[k]], train[1][p[k]], train[2][p[k]], train[3][p[k]])
                                                 for k in range(B)], max_grad_norm=kw.get("model_max_grad_norm"))
                updates += 1
                if updates >= kw["model_max_updates"]:
                    break
            if updates >= kw["model_max_updates"]:
                break
            if ratio > 0.0:
                tot = sum(loss(k, hold) for k in range(B))
                if tot < best:
                    best, since = tot, 0
                else:
                    since += 1
                if since >= kw["model_holdout_epochs"]:
                    break
        logs = []
        for k in range(B):
            mse, rl = losses_eval(sac, cfg, nrm, k, s_all, sp_all, a_all, r_all)
            logs.append(dict(model_loss=loss(k, take(np.arange(n_all))), model_loss_train=loss(k, train),
                             model_loss_holdout=loss(k, hold) if ratio > 0.0 else np.inf, model_loss_mse=mse,
                             model_loss_reward=rl))
        return dict(model_loss_epochs=ep + 1, updates=updates), logs

    # ------------------------------------------------------------------ mbrl_onpolicy_alg.py:72-122
    def collect_sim_data_all(self):
        """-> per model (s, a, adv, rtg) of the dtype, the GAE with critic idx (num_critics == B) or 0."""
        R, V, kw, dt = self.R, self.V, self.kw, self.dt
        self.sac.actor, self.sac.logstd = self.ppo.actor, self.ppo.logstd
        per_model = int(kw["sim_batch_size"] / self.B)
        out = []
        for k in range(self.B):
            parts, t0 = [], 0
            for n, h in sim_passes(per_model, kw["sim_horizon"], kw.get("sim_batch_type", "steps")):
                _, rows = sim_collect(self.sac, self.cfg, self.nrm, self.rows[0], n, h, k, self.rs,
                                      std_mult=self.ppo.std_mult)
                parts.append(rows[:5] + (rows[5] + t0,))
                t0 += n
            s, a, r, sp, d, traj = [np.concatenate(x, 0) for x in zip(*parts)]
            w = self.vst.critics[k if len(self.vst.critics) == self.B else 0]
            v_s, v_sp = V.value(w, self.vacts, self.nrm, s, dt), V.value(w, self.vacts, self.nrm, sp, dt)
            adv, rtg, _, _ = V.gae_batch_loop(v_s, v_sp, r, d.astype(np.float64), traj, kw["gamma"], kw["lam"])
            out.append((s, a, np.asarray(adv, dt), np.asarray(rtg, dt)))
        return out

    # ------------------------------------------------------------------ mbrl_onpolicy_alg.py:124-174
    def update_actor_critic(self):
        R, kw, dt = self.R, self.kw, self.dt
        env_s = self.rows[0]
        d0 = R.forward(self.ppo, self.cfg, self.nrm, env_s)
        ent = float(np.mean(R.entropy_of(d0)))
        mean_ref, ls_ref = d0.mean.copy(), d0.ls.copy()
        upd = []
        for _ in range(kw["num_mf_updates"]):
            per = self.collect_sim_data_all()
            log_c, _ = self.vc_ref.update([p[0] for p in per], [p[3] for p in per], self.B)
            s, a, adv = [np.concatenate([p[i] for p in per], 0) for i in range(3)]
            log_a = self.ppo_ref.update(s, a, adv)
            upd.append(dict(steps_update=len(adv), critic_loss=[c["critic_loss"] for c in log_c], **log_a))
        klv = float(np.mean(R.kl(self.ppo, self.cfg, self.nrm, env_s, mean_ref, ls_ref)))
        return upd, dict(ent_agg=ent, kl_agg=klv, alpha_agg=float(self.ppo.alpha))

    def update(self):
        fit, model_logs = self.update_models()
        upd, agg = self.update_actor_critic()
        return dict(fit=fit, models=model_logs, updates=upd, agg=agg)
