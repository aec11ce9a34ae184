/*
 * sacx.h -- C ABI of libsacx, the MI355X-native SAC / SAC-EO update engine.
 *
 * The reference (noc-lab/sac-expert, TensorFlow-eager Python) has no FFI: its
 * hot path sits behind duck-typed Python objects.  This ABI is the boundary a
 * binding (ctypes here) calls in place of the reference
 * functions named next to each entry.  Everything is plain C: opaque handle,
 * plain pointers and sizes, int status codes (0 = OK, < 0 = error, message in
 * sacx_last_error).  No torch types cross the boundary.
 *
 * Memory model: the caller allocates ONE device arena (any allocator, e.g. a
 * torch uint8 CUDA tensor), binds it with sacx_bind(), and addresses named
 * tensors inside it through the segment table (sacx_layout).  Weights use the
 * Keras (in, out) row-major layout with the bias stored as one extra row
 * (W_ext = [W ; b]), so reference get_weights()/set_weights() lists map onto
 * views (sac_eo/common/nn_utils.py:59-76).  Every call is asynchronous on the
 * bound HIP stream unless stated otherwise.  A handle is not re-entrant; use
 * one handle per learner (per GPU / per seed), or one handle of packed seeds.
 *
 * Packed seeds (cfg.seeds = K > 1): the handle holds K independent learners --
 * the reference's --runs (sac_eo/train.py:118-152), each with its own weights,
 * optimiser state, replay ring and RNG stream -- in K equal arena blocks
 * sacx_seed_stride() bytes apart, each laid out as sacx_layout() describes.
 * sacx_sac_step advances all K in the same kernel launches (grid z = seed).
 * The data-path and RNG calls (append, expert rows, permutations, RNG state,
 * actor_act, rollout, expert_diag, model_fit, resync) address the seed chosen with
 * sacx_seed_select (default 0); the *_seeds forms address every seed at once.
 * The data-parallel mode needs K = 1.
 */
#ifndef SACX_H
#define SACX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SACX_ABI_VERSION 8
#define SACX_MAX_DEPTH 4    /* hidden layers per net (create_nn's layers list, nn_utils.py:100-138) */
#define SACX_MAX_WIDTH 1024 /* widest hidden layer of any net; above 512 the handle runs the generic plan */
#define SACX_MAX_MODELS 8   /* --num_models */

typedef struct sacx_handle sacx_handle;

enum sacx_activation { SACX_ACT_RELU = 0, SACX_ACT_TANH = 1, SACX_ACT_ELU = 2 };
enum sacx_dtype { SACX_F32 = 0, SACX_I32 = 1, SACX_I64 = 2, SACX_U32 = 3, SACX_F64 = 4 };
enum sacx_role { SACX_ROLE_WORK = 0, SACX_ROLE_PARAM = 1, SACX_ROLE_TARGET = 2, SACX_ROLE_STATE = 3 };

/* sacx_config.use_expert.  Any non-zero value means "world models exist": the arena layout, the
   models' normaliser set, sacx_model_fit, sacx_rollout, sacx_expert_diag, sacx_expert_set and
   sacx_perm_push are the same for EO and BC (the reference's BC constructs critics, targets and
   alpha too; they stay allocated, settable and gettable).
   SACX_EXPERT_BC (BC.py:303-363, BC._update_actor): sacx_sac_step runs the actor-only imitation
   update -- actor.sample(s_e) through world models 0 / 1, loss = mean(0.5 sum (sp_e - sp_pred)^2),
   Adam on the actor.  The sampler draws only the expert normals (no randint, no target / policy /
   alpha noise); critics, targets and alpha keep weights, moments and step counts; the statistics row
   holds the MSE in SACX_STAT_MSE_LOSS and SACX_STAT_P_LOSS, alpha in SACX_STAT_ALPHA, zeros in the
   critic / alpha / nlp columns.  sacx_config.epsilon and sacx_expert_set's epsilon are not part of
   the BC loss.  Not with gemm_bf16, seeds > 1 or the data-parallel modes. */
#define SACX_EXPERT_OFF 0
#define SACX_EXPERT_EO 1
#define SACX_EXPERT_BC 2
/* SACX_EXPERT_MODELS (MBRLOnPolicyAlg, mbrl_onpolicy_alg.py + base_onpolicy_alg.py): the world models and
   everything that serves them -- the nets m<k>, mnorm.*, sacx_model_fit, sacx_model_forward / _sample /
   _loss / _losses_eval, sacx_rollout, sacx_sim_collect -- beside a PPO-trained GaussianActor and its
   VCritics, with no expert term and no SAC / BC plan.  Only with actor_gaussian ==
   SACX_ACTOR_GAUSSIAN_TRAIN; expert_batch / expert_capacity are not used (pass 0); sacx_expert_set,
   sacx_perm_push and sacx_expert_diag fail on it.  The replay ring holds the env data
   (sacx_buffer_append); the rollout's actor step is GaussianActor.sample (see sacx_rollout). */
#define SACX_EXPERT_MODELS 3

/* sacx_config.actor_gaussian.
   SACX_ACTOR_GAUSSIAN_TRAIN: a plain (unsquashed) GaussianActor that is trained on-policy by the PPO
   actor update (sac_eo/algs/model_free/ppo.py through GaussianActor.neglogp / entropy / kl /
   get_kl_info, continuous_actors.py:132-192): the sacx_ppo_* entry points below.  Its arena holds the
   "ppo.*" segments beside the layout of a SACX_ACTOR_GAUSSIAN handle: the rollout table (s, a, adv and
   the per-row nlp_old, mean_ref, ls_ref; cfg.buffer_capacity rows at most), the minibatch row buffers
   (cfg.batch rows at most), alpha with its Adam moments ("ppo.alpha"), the step statistics ring
   ("ppo.stats": loss, mean entropy, grad_norm_pre, grad_norm_post, alpha, the surrogate mean, the
   minibatch advantage std + 1e-8, the step number).  It acts as a SACX_ACTOR_GAUSSIAN handle does.
   Refused at sacx_create: actor_output_norm (no backward is built for it), gemm_bf16, seeds > 1,
   use_expert SACX_EXPERT_EO / _BC (SACX_EXPERT_MODELS adds the world models); sacx_dp_init / sacx_dp_init_local fail on it.  sacx_sac_step and
   sacx_actor_evaluate fail on it as on a SACX_ACTOR_GAUSSIAN handle.
   sacx_softmax_init (below) turns such a handle into SoftMaxActor's (discrete_actors.py:8-117): the same
   layout, the net's outputs read as logits, the action rows one index each; sacx_config is unchanged. */
#define SACX_ACTOR_SQUASHED 0
#define SACX_ACTOR_GAUSSIAN 1
#define SACX_ACTOR_GAUSSIAN_TRAIN 2

/* Flags for sacx_sac_step. */
#define SACX_STEP_EXTERNAL_RANDOMS 1  /* skip the device sampler: caller filled slot0.idx / slot0.noise */
#define SACX_STEP_EAGER 2             /* launch kernels directly instead of replaying a hipGraph */
/* floats in the pinned staging buffer of each half (append / act) of the *_host entry points:
   one append_host_seeds call takes seeds*n*(2S+A+2) <= this, act_host_seeds seeds*n*(S+A) */
#define SACX_STAGE_FLOATS 65536

/* Hyper-parameters; names follow sac_eo/common/train_parser.py. */
typedef struct sacx_config {
    int32_t abi_version;        /* = SACX_ABI_VERSION */
    int32_t s_dim;              /* observation dim (HalfCheetah 17, Humanoid 376) */
    int32_t a_dim;              /* action dim (6, 17) */
    int32_t hidden[2];          /* --actor_layers / --critic_layers (same for both) */
    int32_t activation;         /* --actor_activations / --critic_activations */
    int32_t batch;              /* --sac_batch_size */
    int64_t buffer_capacity;    /* --env_buffer_size (ring capacity, rows) */
    int32_t per_state_std;      /* --actor_per_state_std */
    int32_t use_expert;         /* SACX_EXPERT_OFF / _EO (alg_type sac_imit) / _BC (alg_type bc) / _MODELS (mbrl) */
    int32_t expert_capacity;    /* --expert_buffer_size */
    int32_t expert_batch;       /* rows of expert data per update (even) */
    int32_t model_hidden[2];    /* --model_layers */
    int32_t model_activation;   /* --model_activations */
    int32_t model_batch;        /* --model_batch_size */
    int32_t target_update_int;  /* --target_update_int */
    int32_t graph_steps;        /* updates per captured hipGraph (0 -> 128, max 256) */
    int32_t stats_capacity;     /* rows of the per-update statistics ring (0 -> 4096) */
    int32_t perm_capacity;      /* per-update expert permutations held on device (0 -> 4096) */
    float gamma;                /* --gamma */
    float tau;                  /* --soft_tau */
    float lr_q;                 /* --q_crit_lr */
    float lr_pi;                /* --mbpo_actor_lr */
    float lr_alpha;             /* --mbpo_alpha_lr */
    float lr_model;             /* --model_lr */
    float init_temperature;     /* --init_temperature (alpha var = log of it) */
    float target_entropy;       /* -len(action) (SAC_expert.py:46) */
    float act_limit;            /* action_space.high (continuous_actors.py:252) */
    float epsilon;              /* --epsilon (expert weight) */
    float reward_loss_coef;     /* --reward_loss_coef */
    int32_t gemm_bf16;          /* 1: the MLP GEMMs take bf16 operands (rounded on load) with fp32
                                   accumulation, fp32 master weights / Adam (config C5); 0: fp32 */
    int32_t seeds;              /* independent learners packed in this handle (0/1 = one; <= 64) */
    /* --- ABI 4 --- */
    int32_t actor_gaussian;     /* 0: SquashedGaussianActor (SAC, continuous_actors.py:237-379); 1: GaussianActor
                                   (:9-123), inference only (sacx_actor_act) -- an expert imported from a log
                                   (sac_eo/train.py:65-86 builds it without actor_squash) */
    float actor_std_mult;       /* --actor_std_mult (GaussianActor.logstd_init; 0 -> 1) */
    int32_t actor_output_norm;  /* --actor_output_norm (GaussianActor mean normalisation) */
    int32_t actor_layer_norm;   /* --actor_layer_norm: Dense -> LayerNormalization -> tanh on layer 0
                                   (nn_utils.py:110-119) */
    int32_t num_models;         /* --num_models for SAC-EO: 1 .. SACX_MAX_MODELS world models (0 -> 2); all are
                                   fitted in one model-Adam step, the expert term uses the first two sections of
                                   array_split(perm, num_models) (SAC_expert.py:297-336) */
    float model_max_grad_norm;  /* --model_max_grad_norm: clip_by_global_norm(grads, max_norm * num_models)
                                   of the model fit (mbrl_onpolicy_alg.py:315-317); <= 0: None */
    float delta_clip_loss;      /* --delta_clip_loss of MSEModel.get_loss in the model fit; <= 0: None */
    float reward_clip_loss;     /* --reward_clip_loss of MSEModel.get_loss in the model fit; <= 0: None */
    int32_t act_per_layer;      /* 1: act_layers below give each hidden layer's activation; 0: `activation`
                                   (actor, critics) and `model_activation` for every hidden layer */
    int32_t act_layers[3][2];   /* [actor | critics | world models][hidden layer 0, 1]: a sacx_activation
                                   value; the --actor_activations / --critic_activations / --model_activations
                                   lists of nn_utils.py:5-22 */
    /* --- ABI 5 --- */
    float delta_clip_pred;      /* --delta_clip_pred: MSEModel.sample clips the normalised delta prediction
                                   (base_world_model.py:80-82) in the SAC-EO expert term; <= 0: None */
    /* --- ABI 6 --- */
    int32_t single_seed_plan;   /* packed seeds: 1 = every seed sums as a one-seed handle does (the
                                   one-seed plan's head folds and fused heads; 32x32 workgroup tiles, which
                                   accumulate exactly as 16x16 ones, still by the packed row count), so
                                   each is bit-identical to its one-seed run (sac_eo.train --runs in
                                   lock-step); 0 = the packed plan (separate heads from 4 seeds: faster) */
    /* --- ABI 7 --- */
    int32_t gaussian_model;     /* --gaussian_model: GaussianModel world models (init_world_models.py:13-16):
                                   a trainable logstd [1, S] per model after its net (segment m<k>.logstd,
                                   continuous_models.py:24-27), the Gaussian NLL fit loss (:101-131), and
                                   exp(logstd) * u noise in sample(deterministic=False) / step (:36-70) */
    int32_t scale_model_loss;   /* --scale_model_loss: GaussianModel's loss times the stop-gradient
                                   mean(exp(logstd)^2) (:122-127) */
    int32_t separate_reward_nn; /* --separate_reward_nn (base_world_model.py:32-37): the model net has S
                                   outputs and a reward net r<k> ([S+A] -> reward_hidden -> 1) predicts
                                   the reward (:72-74), fitted in the same step */
    int32_t reward_hidden[2];   /* --reward_layers (2 hidden layers; 0 -> 512) */
    int32_t reward_act_layers[2]; /* --reward_activations per hidden layer (sacx_activation) */
    int32_t critic_hidden[2];   /* --critic_layers when they differ from --actor_layers (0: = hidden) */
    /* --- ABI 8 --- */
    int32_t net_depth[4];       /* hidden layers of [actor | critics | world models | reward nets]: 0 -> the two of
                                   hidden / critic_hidden / model_hidden / reward_hidden (and their activations);
                                   1..SACX_MAX_DEPTH -> net_hidden / net_acts below give every layer (the
                                   --actor_layers / --critic_layers / --model_layers / --reward_layers lists,
                                   train_parser.py:56-57, :107-108, of any length).  Any net not of 2 layers runs
                                   the generic launch plan (unfused, every layer its own GEMM problem) */
    int32_t net_hidden[4][SACX_MAX_DEPTH];   /* widths, [1, SACX_MAX_WIDTH]; a used net with a
                                                layer above 512 puts the handle on the generic plan */
    int32_t net_acts[4][SACX_MAX_DEPTH];     /* per-layer sacx_activation */
} sacx_config;

typedef struct sacx_segment {
    char name[48];
    uint64_t offset;            /* bytes from arena base */
    int64_t rows;
    int64_t cols;
    int32_t dtype;              /* enum sacx_dtype */
    int32_t role;               /* enum sacx_role */
} sacx_segment;

typedef struct sacx_launch_info {
    char name[32];              /* stage name, e.g. "critic.dW+adam" */
    char kernel[32];            /* kernel symbol family, e.g. "k_gemm" */
    int32_t grid;               /* workgroups */
    int32_t block;              /* threads per workgroup */
    double flops;               /* algorithmic FLOPs of the launch (unpadded shapes) */
    double bytes;               /* algorithmic HBM/L2 bytes of the launch */
} sacx_launch_info;

/* Statistics row written per update into the stats ring (float32 x 8). */
enum sacx_stat { SACX_STAT_Q1_LOSS = 0, SACX_STAT_Q2_LOSS, SACX_STAT_P_LOSS, SACX_STAT_ALPHA_LOSS,
                 SACX_STAT_ALPHA, SACX_STAT_MSE_LOSS, SACX_STAT_NLP_MEAN, SACX_STAT_STEP };

/* --- lifecycle ------------------------------------------------------------ */
/* Replaces the construction done by init_actor / init_critics / init_alg
 * (sac_eo/actors/init_actor.py:8-30, sac_eo/critics/init_critic.py:5-38,
 * sac_eo/algs/init_alg.py:9-34): validates the config, computes the layout. */
int sacx_create(const sacx_config* cfg, sacx_handle** out);
void sacx_destroy(sacx_handle* h);
const char* sacx_last_error(const sacx_handle* h);   /* NULL handle: error of the last failed create */
int64_t sacx_arena_bytes(const sacx_handle* h);   /* all seeds */
/* Bytes between consecutive seeds' arena blocks (packed seeds; = the arena size for one). */
int64_t sacx_seed_stride(const sacx_handle* h);
/* Packed seeds: the seed (0 <= seed < cfg.seeds) that the per-seed calls address. */
int sacx_seed_select(sacx_handle* h, int32_t seed);
int sacx_layout(const sacx_handle* h, sacx_segment* segs, int32_t cap, int32_t* n_out);
/* Binds the caller-owned arena (>= sacx_arena_bytes, 256-B aligned) and the HIP
 * stream (hipStream_t as void*, NULL = default stream); builds the launch plan.
 * The caller zero-fills the arena and writes weights / normalisers / RNG state
 * through the segment views before the first step. */
int sacx_bind(sacx_handle* h, void* arena, uint64_t bytes, void* stream);

/* --- data path ------------------------------------------------------------ */
/* TrajectoryBuffer.add (sac_eo/common/buffers.py:41-71): appends n rows at the
 * ring head with FIFO truncation to buffer_capacity.  Device pointers, rows of
 * s[n,S], a[n,A], r[n], sp[n,S], d[n] (0/1 as float). */
int sacx_buffer_append(sacx_handle* h, const float* s, const float* a, const float* r,
                       const float* sp, const float* d, int64_t n);
/* expert_reg of _expert_preprocess (sac_eo/algs/SAC_expert.py:375-424): the
 * expert rows (device pointers s_e[n,S], sp_e[n,S]) used by every following
 * update, and the regulariser weight epsilon. */
int sacx_expert_set(sacx_handle* h, const float* s_e, const float* sp_e, int32_t n, float epsilon);
/* Host array perms[n_steps, expert_batch]: the self.rng.shuffle permutations
 * (sac_eo/algs/SAC_expert.py:301-303) for the next n_steps updates. */
int sacx_perm_push(sacx_handle* h, const int32_t* perms, int64_t n_steps);

/* --- RNG (the reference's global NumPy legacy MT19937 stream) ------------- */
/* np.random.seed / RandomState.set_state / get_state (sac_eo/common/seeding.py:12).
 * set/get are synchronous with respect to the bound stream. */
int sacx_rng_seed(sacx_handle* h, uint32_t seed);
int sacx_rng_set_state(sacx_handle* h, const uint32_t key[624], int32_t pos, int32_t has_gauss, double gauss);
int sacx_rng_get_state(sacx_handle* h, uint32_t key[624], int32_t* pos, int32_t* has_gauss, double* gauss);

/* --- the hot path ---------------------------------------------------------- */
/* n_steps x SAC_exp._update / SAC._update (sac_eo/algs/SAC_expert.py:463-477,
 * sac_eo/algs/SAC.py:236-250): sample + gather, twin-Q target, Q1/Q2 Adam,
 * actor (+ expert term) Adam, alpha Adam + clamp, Polyak.  ts_increment is
 * added to num_timesteps after every update (1 = SAC_exp.train, 0 = repeated
 * updates at one env step as in SAC.train). */
int sacx_sac_step(sacx_handle* h, int64_t n_steps, int64_t num_timesteps, int32_t ts_increment,
                  int32_t flags);
/* Captures, instantiates and uploads every hipGraph that sacx_sac_step(h, n_steps, ..., flags)
 * will replay (n_steps / graph_steps full graphs + one graph of the remainder), without
 * running an update, so a following sacx_sac_step(n_steps) launches only cached graphs.
 * (No reference counterpart: TF-eager has no capture step.)  Synchronous. */
int sacx_prepare(sacx_handle* h, int64_t n_steps, int32_t flags);
/* n_steps x _apply_model_grads (sac_eo/algs/mbrl_onpolicy_alg.py:301-319) as
 * called by SAC_exp._update_models (sac_eo/algs/SAC_expert.py:519-550): each
 * step fits both world models on their own minibatch and applies one Keras
 * Adam over all model variables.  idx: host array [n_steps, 2, model_batch]
 * of replay-logical row indices (the caller's np.random.shuffle minibatches
 * of model_data, mapped into the replay ring).  Per-step summed loss goes to
 * the "mstats" ring.  Requires use_expert. */
int sacx_model_fit(sacx_handle* h, const int32_t* idx, int64_t n_steps, int32_t flags);
/* SquashedGaussianActor.sample (sac_eo/actors/continuous_actors.py:270-306) on n device
 * rows obs[n,S] -> act_out[n,A] (device): normalise, MLP, a = act_limit*tanh(mu + std*u).
 * deterministic != 0: u = 0 and the RNG is untouched (the reference draws nothing);
 * otherwise u = np.random.normal(size=(n,A)) from the device copy of the global stream,
 * in the order the reference would draw it.  Behaviour-policy inference for the env loop. */
int sacx_actor_act(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, float* act_out);

/* --- host-pointer forms for the env loop (SAC_exp.train, sac_eo/algs/SAC_expert.py:585-605:
 * one host observation -> actor.sample -> env.step -> buffer.add per timestep) -------------- */
/* sacx_buffer_append with HOST rows: packed into a library-owned pinned, device-mapped buffer
 * that k_append reads in place (no DMA copy; chunked above 64 Ki floats).  Asynchronous: returns
 * once the rows are packed, so the caller's arrays may be reused immediately. */
int sacx_buffer_append_host(sacx_handle* h, const float* s, const float* a, const float* r,
                            const float* sp, const float* d, int64_t n);
/* sacx_actor_act with HOST obs[n,S] in and HOST act_out[n,A] out, through the same mapped
 * buffer (the normaliser reads obs and the head writes actions in place).  Synchronous: waits
 * for the action kernel (and so for any update queued before it) before returning the actions.
 * Drop-in cadence (SAC_expert.py:779-797: sample, _update, env.step, add): after a one-update
 * sacx_sac_step it also queues the next update's sampler draw behind the action kernel (for the
 * ring as it is now), which the next sacx_sac_step(h, 1, ...) uses when the ring still has that
 * size; that step then also runs the previous update's alpha branch, folded into its launches. */
int sacx_actor_act_host(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, float* act_out);
/* Both for EVERY seed of a packed handle in one launch chain: K runs of the reference's
 * --runs (sac_eo/train.py:118-152) stepping their env loops in lock-step hand over n rows each.
 * Arrays are [seeds, n, ...] in seed order; each seed appends to its own ring / acts with its
 * own actor, normaliser and RNG stream (as sacx_seed_select + the calls above would, seed by
 * seed).  act: n <= 16 rows per seed, no --actor_layer_norm. */
int sacx_buffer_append_host_seeds(sacx_handle* h, const float* s, const float* a, const float* r,
                                  const float* sp, const float* d, int64_t n);
int sacx_actor_act_host_seeds(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, float* act_out);

/* --- the reference objects' standalone network calls (device rows in, device rows out) -- */
/* SquashedGaussianActor.evaluate (sac_eo/actors/continuous_actors.py:327-379) on s[n,S]:
 * u = np.random.normal(size=(n, A)) from the device copy of the global stream, x = mu + std*u,
 * pi_out[n,A] = act_limit*tanh(x), nlp_out[n] = neglogp_adjusted. */
int sacx_actor_evaluate(sacx_handle* h, const float* s, int64_t n, float* pi_out, float* nlp_out);
/* QCritic._forward / value (sac_eo/critics/critics.py:84-103) of net 0 / 1 (q_critics) or
 * 2 / 3 (q_targets) on s[n,S], a[n,A]: out[n] = the [n,1] net output (value = 0), or that
 * times max(ret_rms.std, 1e-8) (value = 1). */
int sacx_critic_forward(sacx_handle* h, int32_t net, const float* s, const float* a, int64_t n, int32_t value,
                        float* out);
/* BaseWorldModel._forward + MSEModel.sample / step (sac_eo/models/base_world_model.py:65-87,
 * sac_eo/models/continuous_models.py:225-254) of world model `model` on s[n,S], a[n,A].
 * delta_clip / reward_clip > 0: --delta_clip_pred / --reward_clip_pred.  Outputs (each
 * nullable): pred_out[n,S+1] = [delta_n | r_n] after the clips, sp_out[n,S] = s +
 * delta_rms.denormalize(delta_n) (sample), r_out[n] = r_rms.denormalize(r_n) (step).
 * Requires use_expert. */
int sacx_model_forward(sacx_handle* h, int32_t model, const float* s, const float* a, int64_t n, float delta_clip,
                       float reward_clip, float* pred_out, float* sp_out, float* r_out);
/* sacx_model_forward with GaussianModel's noise (continuous_models.py:36-70, ABI 7): stochastic != 0
 * on a gaussian_model handle draws u = np.random.normal(size=(n, S)) from the device stream and
 * adds exp(logstd) * u to the clipped delta_n before sp_out (GaussianModel.sample(deterministic=False)
 * and .step); pred_out stays the mean.  stochastic = 0, or an MSEModel handle: sacx_model_forward. */
int sacx_model_sample(sacx_handle* h, int32_t model, const float* s, const float* a, int64_t n,
                      int32_t stochastic, float delta_clip, float reward_clip, float* pred_out, float* sp_out,
                      float* r_out);
/* MSEModel.get_loss (continuous_models.py:280-302) of world model `model` on s, sp [n,S],
 * a [n,A], r [n]: loss_out[0] = mean_i 0.5||clip(norm(sp-s)) - delta_pred||^2 +
 * reward_loss_coef * 0.5 (clip(norm(r)) - r_pred)^2, the clips > 0 being --delta_clip_loss /
 * --reward_clip_loss; on a gaussian_model handle GaussianModel.get_loss (:101-131), the delta
 * term 0.5 sum_j (((norm(sp-s) - delta_pred) / e^l)^2 + 2 l + log 2 pi) (x mean(e^{2l}) with
 * scale_model_loss).  loss_out is device memory.  Requires use_expert. */
int sacx_model_loss(sacx_handle* h, int32_t model, const float* s, const float* sp, const float* a, const float* r,
                    int64_t n, float delta_clip_loss, float reward_clip_loss, float* loss_out);
/* batch_simtrajectory_sampler (sac_eo/common/samplers.py:73-122) with world model `model`
 * as the environment (MSEModel.reset / step, sac_eo/models/continuous_models.py:225-258)
 * and the actor's sample() (continuous_actors.py:270-306), all on the device.
 * s_init[n,S] (device) -> s_out[n,H,S], a_out[n,H,A], r_out[n,H], sp_out[n,H,S], d_out[n,H]
 * (uint8; always 0: MSEModel.step never terminates).  Per step t: a = sample(s_t) drawing
 * np.random.normal(size=(n, A)) from the device stream (nothing when deterministic);
 * (delta_n, r_n) = model([norm s_t, norm clip(a)]), clipped to +-delta_clip / +-reward_clip
 * when > 0 (--delta_clip_pred / --reward_clip_pred); a GaussianModel (ABI 7) then draws
 * normal(size=(n, S)) and adds exp(logstd) * u (GaussianModel.step, :36-54; n <= 4096);
 * s_{t+1} = s_t + delta_n*den + mean.  Requires use_expert (the models exist only then).
 * On a SACX_EXPERT_MODELS handle the actor step is GaussianActor.sample (continuous_actors.py:103-123,
 * as sacx_actor_act has it: logstd_init, the log 1e-3 floor, per_state_std, layer norm): a_out gets
 * the raw mean + exp(logstd) * u, and the model steps on actor.clip(a) = clip(a, -act_limit,
 * act_limit) (samplers.py:93-95). */
int sacx_rollout(sacx_handle* h, int32_t model, const float* s_init, int64_t n, int32_t horizon,
                 int32_t deterministic, float delta_clip, float reward_clip, float* s_out, float* a_out,
                 float* r_out, float* sp_out, uint8_t* d_out);
/* One pass of MBRLOnPolicyAlg._collect_sim_data (mbrl_onpolicy_alg.py:89-93) on the device:
 * idx = np.random.randint(rows_held, size=n_traj) from the device copy of the global stream
 * (TrajectoryBuffer.get_states, buffers.py; the replay minibatch's integer draw with the bound = the
 * rows now in the ring), s_init = the raw states of those ring rows in logical order (0 = the oldest
 * row held, as s_all[idx] after the FIFO truncation), then sacx_rollout from them.  Outputs as
 * sacx_rollout's ([n_traj, H, .], trajectory-major: the row order add_batch produces).  No host round
 * trip: the draw rides in the first sampler launch ahead of step 0's normals and step 0's prep
 * reads the indices, so the call adds at most one launch (the deterministic case's draw) to a
 * sacx_rollout of the same shape.  Replays a captured graph per (model, shape, clips, pointers);
 * SACX_ROLL_GRAPH=0 runs it eagerly.  Errors: an empty ring, n_traj / horizon < 0, n_traj > 65536,
 * a GaussianModel with n_traj > 4096.  Requires use_expert. */
int sacx_sim_collect(sacx_handle* h, int32_t model, int64_t n_traj, int32_t horizon, int32_t deterministic,
                     float delta_clip, float reward_clip, float* s_out, float* a_out, float* r_out, float* sp_out,
                     uint8_t* d_out);
/* get_losses_eval (continuous_models.py:304-319, :133-148) of world model `model` on s, sp [n,S],
 * a [n,A], r [n], from one forward (clip=False): out[0] = mean_i 0.5||norm(sp-s) - delta_pred||^2
 * (a GaussianModel's predicted mean: the same plain squared error), out[1] = mean_i 0.5 (norm(r) -
 * r_pred)^2.  out: DEVICE float[2].  Requires use_expert. */
int sacx_model_losses_eval(sacx_handle* h, int32_t model, const float* s, const float* sp, const float* a,
                           const float* r, int64_t n, float* out);
/* Expert diagnostics on the device, n <= 2048 expert rows (device).
 * flags = 0: model_MSE_on_expert_data and _counterfactual_action (SAC_expert.py:579-608):
 *   out[0] = mean over the nm models of mean_i 0.5||model.sample(s_e, a_e) - sp_e||^2,
 *   out[1] = the same with a = actor.sample(s_e, deterministic=False) (draws n*A normals
 *   from the device stream), out[2 .. 2+nm) / out[2+nm .. 2+2nm) = per model (nm = 1: model 0
 *   twice).  n * max(nm, 2) <= 4096.
 * flags & SACX_DIAG_DISC: _calc_disc (:427-460): s_disc_i = ||sp_pred0 - sp_pred1||_2 on
 *   (s_e, counterfactual a); out[0] = sum, out[1] = max, out[2] = median, out[3 + i] = ratio.
 *   The models sample with deterministic=False: GaussianModels draw normal(size=(n, S)) each,
 *   every model in order (only models 0 and 1 enter the distance), after the counterfactual
 *   action's draw (:437, :446).
 * flags & SACX_DIAG_EXPERT_ACTIONS (use_expert_actions): a_e replaces the counterfactual
 *   action (no draw; out[1] = out[0]).  delta_clip > 0: --delta_clip_pred.  out: device, >= 2 + 2
 *   max(nm, 2) floats (3 + n with DISC).  The adaptive epsilon of :383-418 is scalar host arithmetic. */
enum { SACX_DIAG_DISC = 1, SACX_DIAG_EXPERT_ACTIONS = 2 };
int sacx_expert_diag(sacx_handle* h, const float* s_e, const float* a_e, const float* sp_e, int32_t n,
                     int32_t flags, float delta_clip, float* out);
/* --- the PPO actor update of a trainable GaussianActor (SACX_ACTOR_GAUSSIAN_TRAIN handles) ------
 * Every call below fails with a message on any other handle.  Device rows in, device rows out,
 * asynchronous on the bound stream unless stated; rows go through the actor in chunks of 1024. */
/* GaussianActor.neglogp (continuous_actors.py:132-138) on s[n,S], a[n,A]: nlp_out[n] =
 * 0.5 sum_j (((a - mean) / e^ls)^2 + 2 ls + log 2 pi), (mean, ls) = _forward(s) (:74-100: the state
 * normalised, ls = logstd + log(std_mult), or log(softplus(raw)) + log(std_mult) - log(log 2) with
 * per_state_std, floored at log 1e-3). */
int sacx_ppo_neglogp(sacx_handle* h, const float* s, const float* a, int64_t n, float* nlp_out);
/* GaussianActor._forward / get_kl_info / entropy (:74-100, :186-192, :140-143) on s[n,S]:
 * mean_out[n,A], logstd_out[n,A], ent_out[n] = 0.5 sum_j (2 ls + log 2 pi + 1); each nullable. */
int sacx_ppo_dist(sacx_handle* h, const float* s, int64_t n, float* mean_out, float* logstd_out, float* ent_out);
/* GaussianActor.kl(direction='forward') (:159-184) on s[n,S] against mean_ref[n,A], logstd_ref[n,A]:
 * kl_out[n] = 0.5 sum_j (((mean - mean_ref)^2 + e^{2 ls_ref}) / e^{2 ls} + 2 ls - 2 ls_ref - 1). */
int sacx_ppo_kl(sacx_handle* h, const float* s, const float* mean_ref, const float* logstd_ref, int64_t n,
                float* kl_out);
/* The head of PPO.update (ppo.py:43-46): stores the rollout s[n,S], a[n,A], adv[n] (device pointers,
 * 1 <= n <= cfg.buffer_capacity) as the table the steps gather from, computes with the weights as
 * they stand neglogp_old, the reference distribution (kl_info_ref) and the mean entropy over all
 * rows, and resets the per-update accumulators (the two grad-norm sums, the step count). */
int sacx_ppo_begin(sacx_handle* h, const float* s, const float* a, const float* adv, int64_t n);
/* Run-time inputs of the minibatch steps (PPO._setup's update_kwargs, ppo.py:13-39).  actor_lr is
 * the CURRENT rate of the actor's Adam: the adaptlr rule (:109-117) changes it between update()
 * calls while the iteration count and the moments persist, so it is read from device memory by the
 * step's launches and is no constant of a captured graph. */
typedef struct sacx_ppo_params {
    float eps_ppo;          /* clip range: r in [1 - eps, 1 + eps] */
    float max_grad_norm;    /* clip_by_global_norm bound; <= 0: None (both norms the same) */
    float ent_targ;
    float alpha_lr;
    float actor_lr;
    int32_t ent_reg;        /* != 0: Keras Adam on alpha (gradient mean(ent) - ent_targ), then max(alpha, 0) */
    int32_t adv_center;     /* adv - mean(adv) over the minibatch (:71-75) */
    int32_t adv_scale;      /* / (std(adv) + 1e-8), the std of the uncentred minibatch (:72, :76-77) */
} sacx_ppo_params;
/* n_steps x PPO._apply_actor_grad (ppo.py:122-147, :225-239, the expert_reg is None branch) on
 * the minibatches idx[n_steps, mb] (HOST array of table rows, each in [0, n); 1 <= mb <= cfg.batch):
 * gather + advantage statistics, the actor forward, the clipped surrogate - alpha (mean(ent) -
 * ent_targ) with TF's gradient rules, alpha's step (with the alpha from before it in the actor
 * gradient), clip_by_global_norm, Keras Adam on the actor's trainables (logstd included unless
 * per_state_std) at params->actor_lr.  No host synchronisation between the steps; replayed as
 * captured graphs of 64 / 8 / 1 steps, or launched directly with SACX_STEP_EAGER (bit-identical).
 * Requires a sacx_ppo_begin.  Each step appends a row to the "ppo.stats" ring. */
int sacx_ppo_steps(sacx_handle* h, const int32_t* idx, int64_t n_steps, int32_t mb, const sacx_ppo_params* params,
                   int32_t flags);
/* The tail of PPO.update (ppo.py:86-106) over the table's rows with the weights as they stand now:
 * out[0] = ent (from sacx_ppo_begin), out[1] = tv = 0.5 mean |r - 1|, out[2] = mean kl against the
 * reference distribution, out[3] = outside_clip = mean(|r - 1| > eps_ppo), out[4] / out[5] =
 * grad_norm_pre / grad_norm_post averaged over the steps since sacx_ppo_begin (0 without a step),
 * out[6] = alpha, out[7] = the step count.  out: HOST double[8] (the f32 device values widened;
 * outside_clip is the row count over n in f64, as np.mean of booleans).  Synchronous. */
int sacx_ppo_end(sacx_handle* h, float eps_ppo, double* out);
/* The launches of one minibatch step of mb rows, as sacx_plan_info. */
int sacx_ppo_plan_info(sacx_handle* h, int32_t mb, struct sacx_launch_info* out, int32_t cap, int32_t* n_out);

/* --- VCritics beside the trainable GaussianActor: value, GAE and the critic update ----------------
 * The critic side of MBRLOnPolicyAlg._update_actor_critic (buffer.get_update_info -> _update_critics;
 * _update_actor is the sacx_ppo_* calls above).  SACX_ACTOR_GAUSSIAN_TRAIN handles only; every call
 * fails with a message elsewhere, and (but for sacx_vcritic_init) on a handle without critics.
 * Device rows in, device rows out, asynchronous on the bound stream unless stated; whole-table
 * passes go through a critic in chunks of 1024 rows. */
/* Gives the handle n_critics VCritics (1 .. SACX_MAX_MODELS: num_models under --critic_ensemble, else
 * 1, init_critic.py:10): nets [S] -> the critic layers -> 1 with the handle's critic description
 * (critic_hidden / net_depth[1] / net_hidden[1] / net_acts[1]).  After sacx_create and before
 * sacx_arena_bytes / sacx_layout / sacx_bind are used, as sacx_dp_init.  Appends, behind the "ppo.*"
 * segments (every other segment keeps its offset): "v<k>.l<i>" (W_ext, one contiguous parameter
 * range over all critics), "vc.adam_m" / "vc.adam_v" / "vc.grad" (that range's Adam moments and
 * gradients, each one range length behind the last), "vc.ctl" (int64 x 16: steps run, Adam
 * iterations, each critic's table rows), "vc.par", the tables "vc.s" [n_critics x buffer_capacity, S]
 * and "vc.rtg" [n_critics, buffer_capacity], the rings "vc.stats" (a row per step: the summed loss,
 * SACX_MAX_MODELS per-critic losses, the step number) and "vc.idx", and the work rows of a step
 * (n_critics x batch rows), of the whole-table passes and of the GAE scan.  Errors: a second call, a
 * bound handle, another handle kind, n_critics out of range. */
int sacx_vcritic_init(sacx_handle* h, int32_t n_critics);
/* VCritic._forward / value (critics.py:30-40) of critic `critic` on s[n,S], the state normalised
 * with norm.s_*: out[n] = the net's output (value = 0), or that times norm.ret_den (value = 1). */
int sacx_vcritic_value(sacx_handle* h, int32_t critic, const float* s, int64_t n, int32_t value, float* out);
/* gae (buffer_utils.py:11-42) on given values over a batch of trajectories, in f64 as NumPy computes
 * it: delta = r + gamma (1 - d) v_sp - v_s; adv_t = delta_t + gamma lam adv_{t+1}, restarted
 * wherever traj[t+1] != traj[t] (gae_batch's sections, :63-65); rtg = adv + v_s; rtg_sp =
 * (rtg - r) / gamma; each rounded to f32 once, at the store.  v_s, v_sp, r, d: float[n]; traj:
 * int32[n]; 1 <= n <= cfg.buffer_capacity; gamma > 0.  A parallel segmented scan (two launches). */
int sacx_gae_values(sacx_handle* h, const float* v_s, const float* v_sp, const float* r, const float* d,
                    const int32_t* traj, int64_t n, double gamma, double lam, float* adv_out, float* rtg_out,
                    float* rtg_sp_out);
/* gae_batch (buffer_utils.py:44-83) with critic `critic`: value(s) and value(sp) (s, sp: [n,S]), then
 * the arithmetic above, with no host round trip. */
int sacx_gae(sacx_handle* h, int32_t critic, const float* s, const float* r, const float* sp, const float* d,
             const int32_t* traj, int64_t n, double gamma, double lam, float* adv_out, float* rtg_out, float* rtg_sp_out);
/* VCritic.get_loss (critics.py:42-49) of critic `critic` on s[n,S], rtg[n]: loss_out[0] (DEVICE float)
 * = 0.5 mean((rtg / ret_den - v)^2), v the net's output (the reference's value / ret_den: the same up
 * to an f32 ulp).  1 <= n <= cfg.buffer_capacity. */
int sacx_vcritic_loss(sacx_handle* h, int32_t critic, const float* s, const float* rtg, int64_t n, float* loss_out);
/* Stores s[n,S], rtg[n] (1 <= n <= cfg.buffer_capacity) as critic `critic`'s table, the rows the
 * steps gather from (base_onpolicy_alg.py:226-229).  Tables may differ in length. */
int sacx_vcritic_begin(sacx_handle* h, int32_t critic, const float* s, const float* rtg, int64_t n);
/* n_steps x _apply_critic_grads (base_onpolicy_alg.py:244-251, :269-283) on the minibatches
 * idx[n_steps, mb] (HOST array; 1 <= mb <= cfg.batch): the SAME row indices for every critic, each
 * on its own table, so every index must be below the shortest table (n_samples = min, :231) and
 * every critic needs a table.  Loss = the sum over the critics of get_loss; no clipping; one Keras
 * Adam over all critics' variables (one iteration count, kept across calls; moments per variable) at
 * critic_lr, which is written to "vc.par" in stream order and read by the launches (no constant of a
 * captured graph).  No host synchronisation between the steps; replayed as captured graphs of
 * 64 / 8 / 1 steps, or launched directly with SACX_STEP_EAGER (bit-identical).  A refused call
 * touches nothing.  Each step appends a row to the "vc.stats" ring. */
int sacx_vcritic_steps(sacx_handle* h, const int32_t* idx, int64_t n_steps, int32_t mb, float critic_lr, int32_t flags);
/* The tail of _update_critics (base_onpolicy_alg.py:253-264): out[k] = critic k's get_loss over its
 * whole table with the weights as they stand (0 for k >= n_critics), out[SACX_MAX_MODELS] = the
 * critics' Adam iteration count (every step run on the handle so far).  out: HOST
 * double[SACX_MAX_MODELS + 1].  Synchronous. */
int sacx_vcritic_end(sacx_handle* h, double* out);
/* The launches of one critic step of mb rows per critic, as sacx_plan_info. */
int sacx_vcritic_plan_info(sacx_handle* h, int32_t mb, struct sacx_launch_info* out, int32_t cap, int32_t* n_out);

/* --- the TRPO actor update of the trainable GaussianActor ---------------------------------------
 * TRPO.update (sac_eo/algs/model_free/trpo.py:34-317, the expert_reg is None branch, with the one
 * reading that makes it run: grad_final := neg_pg), update_utils.cg, GaussianActor.set_weights.
 * SACX_ACTOR_GAUSSIAN_TRAIN handles only; every call but sacx_trpo_init fails with a message on a
 * handle without it.  "Flat" vectors are the floats of the actor's contiguous trainable range of the
 * arena, actor.l0 .. actor.logstd (each layer as [W; b], then the layer norm's gamma ; beta, then
 * logstd, with the padding between segments, which holds 0): sacx_layout gives the offsets.
 *
 * sacx_trpo_init: after sacx_create and before sacx_arena_bytes / sacx_layout / sacx_bind, in either
 * order with sacx_vcritic_init.  Appends the "trpo.*" segments behind what the handle holds: the flat
 * vectors ("trpo.vec": pg_vec, x, r, p, z, the saved weights, the step), the device scalars of
 * conjugate gradient and the line search, and the rows of a chunk of a whole-table pass
 * (min(buffer_capacity, 4096) rows).  A handle without the call keeps its layout byte for byte.
 * Fails on another handle kind, on a bound handle and on a second call. */
int sacx_trpo_init(sacx_handle* h);
typedef struct sacx_trpo_params {
    float delta;            /* delta_trpo: the trust region's KL bound */
    float trust_damp;       /* F(x) = H x + trust_damp x */
    float kl_maxfactor;     /* the line search accepts kl <= kl_maxfactor * delta */
    float ent_targ;
    float alpha_lr;
    int32_t cg_it;          /* 1 .. 255 */
    int32_t trust_sub;      /* the Fisher product runs on s_all[::trust_sub] */
    int32_t ent_reg, adv_center, adv_scale;
} sacx_trpo_params;
/* trpo.py:36-63, :170-176: stores the rollout as sacx_ppo_begin does (neglogp_old, the reference
 * distribution, the mean entropy), normalises the advantages over the whole table, and leaves
 * pg_vec = -(d loss / d theta) of loss = mean(-r adv) - alpha (mean(ent) - ent_targ) in "trpo.vec"
 * row 0; with ent_reg alpha then takes its Keras Adam step and max(alpha, 0).  No synchronisation. */
int sacx_trpo_begin(sacx_handle* h, const float* s, const float* a, const float* adv, int64_t n,
                    const sacx_trpo_params* params);
/* pg_vec as sacx_trpo_begin left it -> out_dev (a flat device vector). */
int sacx_trpo_grad(sacx_handle* h, float* out_dev);
/* One Fisher-vector product (trpo.py:200-227) on flat device vectors: out = H x + trust_damp x with
 * H = (1 / n_sub) sum_i J_i^T M_i J_i over the rows s_all[::trust_sub] of the table, at the weights
 * as they stand (trust_sub, trust_damp: sacx_trpo_begin's).  flags: SACX_STEP_EAGER launches
 * directly instead of replaying the captured graph (bit-identical).  No synchronisation. */
int sacx_trpo_fvp(sacx_handle* h, const float* x_dev, float* out_dev, int32_t flags);
/* trpo.py:178-198, :229-317: conjugate gradient (cg_it iterations from x = 0, the r.r < 1e-10 break
 * as a device flag), vFv, eta, the backtracking line search (one synchronisation per trial).
 * out[8] = ent, tv_pre, kl_pre, tv, kl, adj, improve, alpha.  A zero gradient (every |g| <= 1e-8)
 * or delta == 0 gives the zero step.  vFv <= 0 (or not finite) fails with a message and leaves the
 * weights untouched (the reference carries NaNs on).  flags: SACX_STEP_EAGER as above. */
int sacx_trpo_step(sacx_handle* h, const sacx_trpo_params* params, int32_t flags, double* out);
/* The launches of one Fisher product over `rows` rows, as sacx_plan_info. */
int sacx_trpo_plan_info(sacx_handle* h, int64_t rows, struct sacx_launch_info* out, int32_t cap, int32_t* n_out);

/* --- SoftMaxActor on the trainable handle: discrete actions for PPO and TRPO --------------------
 * SoftMaxActor (sac_eo/actors/discrete_actors.py:8-117) with the one reading that makes the class
 * construct: _nn = create_nn(s_dim, a_dim, layers, activations, gain), a_dim = n of Discrete(n), the
 * trainables the net's variables only.  After sacx_create and before sacx_arena_bytes / sacx_layout /
 * sacx_bind, in any order with sacx_vcritic_init and sacx_trpo_init.  The layout does not change
 * ("actor.logstd" keeps its words and is no trainable: no gradient, no Adam, in neither norm); a
 * handle without the call keeps its layout and results byte for byte.  Fails on a handle that is
 * not SACX_ACTOR_GAUSSIAN_TRAIN, with per_state_std, with SACX_EXPERT_MODELS (the world models take
 * continuous actions and the reference defines no encoding) or any other use_expert, on a bound
 * handle and on a second call.
 * After the call the actor net's a_dim outputs are logits and the entry points above carry the
 * categorical meaning, every value on the row's max-shifted logits (:33, :49, :58, :82):
 *   sacx_ppo_neglogp, sacx_ppo_begin, sacx_trpo_begin: a is a[n], one action index per row stored
 *     as float; neglogp = softmax_cross_entropy_with_logits(one_hot(a), logits) (:47-54) = -log p_a.
 *     An index outside [0, a_dim) is tf.one_hot's all-zero row: neglogp 0, no gradient through r.
 *   sacx_ppo_dist: mean_out[n,A] = the raw logits (get_kl_info, :98-100), logstd_out must be NULL,
 *     ent_out[n] = -sum_j p_j log p_j (:56-66).
 *   sacx_ppo_kl: mean_ref[n,A] = the reference logits, logstd_ref must be NULL; kl_out[n] =
 *     sum_j p_j ((l_j - lse) - (l_ref_j - lse_ref)) (:68-96).
 *   sacx_ppo_steps, sacx_ppo_end: ppo.py:122-239, :91-106 with that neglogp and entropy; the same
 *     statistics, alpha step and global-norm clip; Adam over the net's variables.
 *   sacx_trpo_grad, sacx_trpo_fvp, sacx_trpo_step: flat vectors span actor.l0 up to where
 *     actor.logstd begins; the Fisher product is (1 / n_sub) sum_i J_i^T (diag(p_i) - p_i p_i^T) J_i,
 *     the Hessian of the mean kl at cur = ref; the line search uses the categorical kl; set_weights
 *     (:109-117) floors nothing.
 *   sacx_actor_act, its _host forms, sacx_rollout and sacx_sim_collect fail: a softmax handle samples
 *     on the host from sacx_ppo_dist's logits (:22-42), or on the device with sacx_softmax_act /
 *     sacx_softmax_act_host (below). */
int sacx_softmax_init(sacx_handle* h);

/* SoftMaxActor.sample (discrete_actors.py:22-42) on the device, for a bound softmax handle.
 * obs [n,S] -> act_out [n] int32 action indices.  The logits are the actor net's (normaliser, MLP).
 * deterministic == 0: u = np.random.random(size=(n, A)) from the device copy of the global MT19937
 *   stream, row-major, two words per double (((w0>>5) * 2^26 + (w1>>6)) / 2^53, no rejection; the
 *   gauss cache -- has_gauss, gauss -- is left as it is); g = float32(-log(-log u)) formed in f64
 *   and rounded once (u = 0: g = -inf); the action is the first-index argmax of the f32
 *   (logits - rowmax) + g.  u_out (device [n,A] doubles, or NULL) receives u itself.
 * deterministic != 0: draws nothing, the stream is untouched; the argmax of the logits.
 * n <= 16 rows of a two-layer net without layer norm take one workgroup per row (as
 * sacx_actor_act's few-rows path); everything else the generic chain in chunks of 1,024 rows.
 * Device pointers, stream-ordered.  On a packed-learners handle the call acts for the learner chosen
 * with sacx_seed_select.  Fails on an unbound handle, on a handle without sacx_softmax_init, for
 * n < 0 and for null obs / act_out. */
int sacx_softmax_act(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, int32_t* act_out,
                     double* u_out);
/* sacx_softmax_act with HOST obs[n,S] in and HOST act_out[n] out, through the act half of the mapped
 * pinned staging buffer; synchronous, as sacx_actor_act_host. */
int sacx_softmax_act_host(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, int32_t* act_out);

/* --- packed on-policy learners: K PPO and VCritic steps in one launch chain --------------------
 * The reference's only parallelism is --runs K (sac_eo/train.py:148-152): K independent learners.
 * For the on-policy loop a minibatch step (ppo.py:55-83; base_onpolicy_alg.py:219-283) is paced by
 * its launch count and not by its arithmetic, so K learners' steps run in the same launches.
 *
 * sacx_learners_init: K in [2, SACX_MAX_LEARNERS] on a SACX_ACTOR_GAUSSIAN_TRAIN handle, with or without
 * SACX_EXPERT_MODELS, sacx_vcritic_init and sacx_softmax_init, AFTER those init calls and before
 * sacx_arena_bytes / sacx_layout / sacx_bind.  The handle then holds K learners as a packed SAC handle
 * holds K seeds: sacx_seed_stride = the one-learner arena rounded up to 64 KiB, sacx_arena_bytes = K
 * strides, the layout inside a learner's block byte for byte the one-learner handle's; sacx_config is
 * not involved (cfg.seeds stays 1).  Fails with a message on another handle kind, on a bound handle,
 * on a second call, on K out of range and on a handle that had sacx_trpo_init; sacx_trpo_init and
 * sacx_vcritic_init fail after it.  TRPO's conjugate gradient and line search stay one learner per handle.
 * After it every per-learner entry point (sacx_ppo_begin / _end / _neglogp / _dist / _kl,
 * sacx_vcritic_begin / _end / _value / _loss, sacx_gae*, sacx_sim_collect, sacx_rollout, sacx_model_fit,
 * sacx_model_losses_eval, sacx_actor_act*, the RNG state, sacx_resync) works on the learner chosen with
 * sacx_seed_select, and sacx_ppo_steps / sacx_vcritic_steps fail with a message naming the calls below. */
#define SACX_MAX_LEARNERS 64
int sacx_learners_init(sacx_handle* h, int32_t K);
/* train.py:148-152 over ppo.py:55-83 (the actor half of base_onpolicy_alg.py:219-283's update): n_steps
 * minibatch steps of EVERY learner in the launches of one learner's step (sacx_ppo_steps' plan at grid z = K).  idx[K][n_steps][mb] (HOST): learner k's rows
 * of ITS rollout table (each learner needs a sacx_ppo_begin; the tables may differ in length);
 * params[K]: learner k's run-time inputs (its own actor_lr, as the adaptlr rule makes them differ).
 * n_steps and mb are common.  Each learner reads its own index ring, "ppo.par", "ppo.alpha", control
 * block and statistics rows, and ends bit for bit where sacx_ppo_steps on a one-learner handle holding
 * its state ends.  Graphs of 64 / 8 / 1 steps in a cache of their own; SACX_STEP_EAGER launches directly. */
int sacx_ppo_steps_packed(sacx_handle* h, const int32_t* idx, int64_t n_steps, int32_t mb, const sacx_ppo_params* params,
                          int32_t flags);
/* train.py:148-152 over base_onpolicy_alg.py:219-283 (the critic half, beside ppo.py:55-83's actor
 * steps): the same for sacx_vcritic_steps, at any critic count: idx[K][n_steps][mb] (HOST; learner k's indices below ITS shortest critic table), critic_lr[K]. */
int sacx_vcritic_steps_packed(sacx_handle* h, const int32_t* idx, int64_t n_steps, int32_t mb, const float* critic_lr,
                              int32_t flags);

int sacx_sync(sacx_handle* h);
/* Brings the arena to the state the calls so far define, without waiting: runs an alpha branch
 * the drop-in loop's one-update steps deferred (its alpha Adam, stats row and counters; see
 * sacx_actor_act_host) and undoes a speculative sampler draw.  Every entry point but act, append
 * and the speculative step does this itself; a caller that reads or writes the arena directly
 * (segment views) calls it first.  sacx_sync = sacx_settle + a wait for the bound stream. */
int sacx_settle(sacx_handle* h);

/* After the caller restored the arena's PARAM / TARGET / STATE segments (a resume
 * snapshot, sac_eo Engine.load_state): re-reads the host mirrors of the device counters
 * (update and model-fit sequence numbers that place host-pushed permutations / indices). */
int sacx_resync(sacx_handle* h);

/* --- data-parallel mode (config C4: one learner over k GPUs) --------------------
 * Not in the reference (its --runs are independent learners, sac_eo/train.py:118-152):
 * each rank samples its local batch from its own buffer and stream; the critic, actor
 * (+logstd) and alpha gradients are summed over the ranks by RCCL inside the update
 * graph (three all-reduces per update: 2*P_q, P_a + A, 1 floats) and every rank applies
 * the same Keras Adam with gradient/k, so weights stay identical when they start so.
 * With batch = B/k this is the B-row update of SAC.py:236-250 (the losses are means).
 * sacx_dp_unique_id: on one rank, fills id_out (cap >= 128 bytes), returns its size.
 * sacx_dp_init: on every rank after sacx_create, before sacx_bind, on the rank's device.
 * Plain SAC only (use_expert = 0). */
int sacx_dp_unique_id(void* id_out, int32_t cap);
int sacx_dp_init(sacx_handle* h, const void* id, int32_t nranks, int32_t rank);
/* The same protocol with the ranks as handles of ONE process (<= 8, no RCCL): sacx_dp_init_local
 * on each (before sacx_bind; all bound to one stream), then sacx_dp_local_step(handles in rank
 * order, ...) runs n_steps updates of every rank eagerly, interleaved at the all-reduce points,
 * where one kernel sums the ranks' gradient ranges in rank order and writes the sum back to each
 * (ncclAllReduce(sum)'s result; with two ranks bit for bit).  The reduce is the only difference
 * from the RCCL mode: the plans, local-gradient stores and Adam apply launches are the same. */
int sacx_dp_init_local(sacx_handle* h, int32_t nranks, int32_t rank);
int sacx_dp_local_step(sacx_handle* const* handles, int32_t nranks, int64_t n_steps, int64_t num_timesteps,
                       int32_t ts_increment);

/* --- measurement ----------------------------------------------------------- */
/* One-update sacx_sac_step calls that replayed the sampler-less graph on randoms drawn
 * speculatively by the preceding sacx_actor_act_host (the drop-in loop's cadence act -> step ->
 * append of SAC_expert.py:779-797); the other steps drew their own.  -1 for a NULL handle. */
int64_t sacx_spec_hits(const sacx_handle* h);
/* Kernel launches of the sacx_rollout / sacx_sim_collect graph this handle captured last (0 before the
 * first capture; a replayed call captures nothing).  -1 for a NULL handle. */
int64_t sacx_rollout_launches(const sacx_handle* h);
int sacx_plan_info(const sacx_handle* h, sacx_launch_info* out, int32_t cap, int32_t* n_out);
/* The launches of one world-model fitting step (sacx_model_fit) of the selected seed, as
 * sacx_plan_info (use_expert handles; *n_out = 0 before the first sacx_model_fit builds them). */
int sacx_model_plan_info(const sacx_handle* h, sacx_launch_info* out, int32_t cap, int32_t* n_out);
/* Runs n_steps updates eagerly with a HIP event around every launch on the
 * bound stream and returns the summed device milliseconds per launch index
 * (array of length n_launches from sacx_plan_info).  Each step is queued
 * behind a ~3 ms device-side wait so the deltas are back-to-back device time,
 * not host launch latency.  Synchronous. */
int sacx_profile(sacx_handle* h, int64_t n_steps, double* ms_per_launch, int32_t cap);

/* Replays the captured update graph (graph_steps updates, device sampler) n_replays
 * times between two HIP events on the bound stream and returns the elapsed ms.
 * skip_kernel names a kernel family (sacx_launch_info.kernel, e.g. "k_gemm") whose
 * launches are left out of the graph: the difference of the two timings is that
 * family's in-pipeline time.  With a family skipped the updates are meaningless and
 * the state must be discarded (measurement only).  Synchronous. */
int sacx_time_graph(sacx_handle* h, int64_t n_replays, const char* skip_kernel, double* ms_out);
/* Replays a copy of the update graph in which every launch of `kernel` (only "k_gemm")
 * records per-workgroup start/end device ticks (s_memrealtime, 100 MHz) into its own
 * slots; returns the mean launch span (first workgroup start .. last workgroup end) in
 * us, the summed span per update and the launches per graph replay.  The replays are
 * real updates.  Synchronous. */
int sacx_time_kernels(sacx_handle* h, const char* kernel, int32_t n_replays, double* avg_us, double* us_per_update,
                      int64_t* n_launches);

#ifdef __cplusplus
}
#endif
#endif /* SACX_H */
