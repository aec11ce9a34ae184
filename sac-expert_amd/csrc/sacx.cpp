// libsacx host side: arena layout, launch plan of one SAC / SAC-EO update,
// hipGraph capture and the C ABI declared in include/sacx.h.
//
// One update (SAC_expert.py:463-477) is planned as this launch sequence
// (reference function each stage restates in brackets):
//   rng            sampler: randint + all normals of the update   [buffers.py:136, continuous_actors.py:351]
//   gather         replay rows -> normalised staging               [buffers.py:137-141, normalizer.py:36-41]
//   actor.fwd0/1   actor MLP on [sp ; s ; s_expert]               [continuous_actors.py:327-331]
//   actor.head     evaluate(sp), evaluate(s), sample(s_expert)     [continuous_actors.py:270-379]
//   q.fwd0/1       target nets on (sp,a'), critics on (s,a), models on (s_e, c_a)
//   q.head         min target, TD target, critic loss grads, expert MSE  [SAC_expert.py:211-250, 321-334]
//   critic.bwd1    dX through critic layer 2 (+ model layer 2)
//   critic.adam    dW of q0/q1 + Keras Adam + Polyak into t0/t1  [SAC_expert.py:243,250,362-373]
//   pi.q.fwd0/1    updated critics on (s, pi(s))                  [SAC_expert.py:314-317]
//   pi.q.head      min + policy loss grads                        [SAC_expert.py:317-319]
//   pi.q.bwd1      dX through critic layer 2
//   actor.head.bwd action grads -> tanh-Gaussian backward -> actor layer 3 dX
//   actor.bwd1     dX through actor layer 2
//   actor.adam     dW of the actor (+ logstd) + Keras Adam        [SAC_expert.py:336-338]
//   alpha.fwd0/1   updated actor on s                              [SAC_expert.py:341-343]
//   alpha.head     evaluate + alpha loss + Adam + clamp + stats   [SAC_expert.py:345-356]
#include "sacx.h"
#include "sacx_internal.h"
#include "vcritic.h"
#include "trpo.h"
#include "mt_jump.h"
#include "sampler_sched.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <chrono>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

using namespace sacx;

namespace {

std::string g_create_error;

inline int64_t r4(int64_t x) { return (x + 3) & ~int64_t(3); }

struct RollKey {             // sacx_rollout graph cache key (memcmp'd: no padding holes)
    int32_t model;
    int32_t seed;             // packed seeds: the selected seed (its arena block)
    int64_t n;
    int32_t horizon, deterministic;
    float delta_clip, reward_clip;
    const void* ptrs[6];
};
static_assert(sizeof(RollKey) == 4 + 4 + 8 + 4 + 4 + 4 + 4 + 6 * 8, "RollKey is packed");

struct SegInfo {
    std::string name;
    uint64_t off;
    int64_t rows, cols;
    int dtype, role;
};

struct Launch {
    enum Kind { RNG, GATHER, GEMM, AHEAD, QHEAD, ABWD, FINAL, MGATHER, MLOSS, MFINAL, ALLREDUCE, APPLY, AAPPLY,
                GNORM, LNORM, PPOGATHER, PPOHEAD, GNPART, PPOFINAL, VCGATHER, VCHEAD, VCFINAL, VCADAM,
                TRIN, TRTAN, TRHEAD, TRACC, TRCG } kind;
    std::string name;
    RngArgs rng;
    GatherArgs gather;
    GemmArgs gemm;
    HeadArgs head;
    FinalArgs fin;
    QHeadArgs qh;
    ActorBwdArgs ab;
    MGatherArgs mg;
    MLossArgs ml;
    MFinalArgs mf;
    AdamApplyArgs ap;          // APPLY
    GNormArgs gn;              // GNORM
    LNArgs ln;                 // LNORM
    PpoGatherArgs pg;          // PPOGATHER
    PpoHeadArgs ph;            // PPOHEAD
    PpoFinalArgs pf;           // PPOFINAL (GNPART: gn)
    VcGatherArgs vg;           // VCGATHER
    VcHeadArgs vh;             // VCHEAD
    VcFinalArgs vf;            // VCFINAL
    VcAdamArgs va;             // VCADAM
    TrInArgs ti;               // TRIN
    TrTanArgs tt;              // TRTAN
    TrHeadArgs th;             // TRHEAD
    TrAccArgs ta;              // TRACC
    TrCgArgs tc;               // TRCG
    float* ar_buf = nullptr;   // ALLREDUCE: in-place sum over the data-parallel ranks
    int64_t ar_count = 0;
    int grid = 0, block = 256;
    int pre_steps = 0;         // MGATHER: > 0 the pre-gather of that many fit steps (launch_mgather)
    double flops = 0, bytes = 0;
    bool after_final = false;  // graph: waits for the previous update's alpha branch
    bool alpha_branch = false; // graph: runs on the side stream beside the next update's first launches
    bool frees_slot = false;   // graph: the launch that carries the folded alpha rows (last reader of a slot)
    // graph: the critics' forward on the buffer rows (s, a) runs on its own stream, between
};

const char* kernel_family(Launch::Kind k) {
    switch (k) {
        case Launch::RNG: return "k_rng";
        case Launch::GATHER: return "k_gather";
        case Launch::GEMM: return "k_gemm";
        case Launch::AHEAD: return "k_actor_head";
        case Launch::QHEAD: return "k_qhead";
        case Launch::ABWD: return "k_actor_bwd";
        case Launch::FINAL: return "k_alpha_final";
        case Launch::MGATHER: return "k_mgather";
        case Launch::MLOSS: return "k_mloss";
        case Launch::MFINAL: return "k_mfinal";
        case Launch::ALLREDUCE: return "rccl_allreduce";
        case Launch::APPLY: return "k_adam_apply";
        case Launch::AAPPLY: return "k_alpha_apply";
        case Launch::GNORM: return "k_gnorm";
        case Launch::LNORM: return "k_ln";
        case Launch::PPOGATHER: return "k_ppo_gather";
        case Launch::PPOHEAD: return "k_ppo_head";
        case Launch::GNPART: return "k_gnorm";
        case Launch::PPOFINAL: return "k_ppo_final";
        case Launch::VCGATHER: return "k_vc_gather";
        case Launch::VCHEAD: return "k_vc_head";
        case Launch::VCFINAL: return "k_vc_final";
        case Launch::VCADAM: return "k_vc_adam";
        case Launch::TRIN: return "k_trpo_in";
        case Launch::TRTAN: return "k_trpo_tan";
        case Launch::TRHEAD: return "k_trpo_head";
        case Launch::TRACC: return "k_trpo_acc";
        case Launch::TRCG: return "k_trpo_cg";
    }
    return "?";
}

}  // namespace

// One net's hidden layers: create_nn's layers list and its activations (nn_utils.py:100-138)
struct NetDims {
    std::vector<int> h, act;
    int D() const { return (int)h.size(); }
};

struct sacx_handle {
    sacx_config cfg{};
    std::string err;
    // dims
    int S = 0, A = 0, H0 = 0, H1 = 0, B = 0, Aout = 0, ne = 0, Hm0 = 0, Hm1 = 0, ecap = 0;
    int Hc0 = 0, Hc1 = 0;     // the critics' hidden sizes (--critic_layers; H0 / H1 are the actor's)
    int ldS = 0, ldQ = 0, stride = 0, Ra = 0, Rb = 0, n_norm = 0;
    // hidden-layer activations per net and layer (nn_utils.py:5-22 create_activations): actor,
    // critics, world models
    int aact[2] = {0, 0}, cact[2] = {0, 0}, macts[2] = {0, 0};
    int64_t cap = 0;
    int graph_steps = 128, stats_cap = 4096, perm_cap = 4096, mb = 0, mfit_cap = 1024;
    int nm = 0;               // SAC-EO world models (--num_models: 1 .. SACX_MAX_MODELS)
    int ne_perm = 0;          // expert rows per update permutation (expert_batch); ne = the rows the update
                              // uses: all of them (1 or 2 models), else the first two array_split sections
    // hidden layers of [actor, critics, world models, reward nets]; H0 / H1 (Hc*, Hm*, Hr*) and the act
    // pairs above are the first and the last hidden layer of each
    NetDims nd[4];
    bool deep = false;        // a net of other than 2 hidden layers: the generic plans (build_plan_generic)
    bool wide = false;        // a used net has a hidden layer above 512 (sets deep): no fold, no k_fwd2, no ROWK
                              // variant takes such a row -- the per-layer GEMMs and the wide row kernels do
    int64_t roll_nodes = 0;   // launches of the rollout / sim_collect graph captured last
    bool models_only = false; // use_expert == SACX_EXPERT_MODELS: world models beside the PPO-trained actor, no expert rows
    bool bc = false;          // use_expert == SACX_EXPERT_BC: the actor-only imitation update (build_plan_bc)
    // world-model variants (ABI 7): GaussianModel (a logstd per model, the NLL fit loss, noise in
    // sample / step) and --separate_reward_nn (a reward net r<k> beside each model net m<k>)
    bool gm = false, srn = false, lscale = false;
    int Om = 0;               // model-net outputs: S + 1 (the reward as the last column), or S (srn)
    int Hr0 = 0, Hr1 = 0;     // the reward nets' hidden sizes (srn)
    int racts[2] = {0, 0};    // their hidden-layer activations
    bool ln = false;          // --actor_layer_norm: Dense -> LayerNorm -> tanh on the actor's layer 0
    // actor_gaussian == SACX_ACTOR_GAUSSIAN_TRAIN: the PPO actor step (sacx_ppo_*, build_ppo_plan)
    bool ppo = false;
    // host mirrors of a learner's on-policy counters: one entry per learner (sacx_learners_init), the
    // per-learner entry points use the selected learner's (op())
    struct OnPolicyHost {
        int64_t ppo_rows = 0; // rows of the rollout table (sacx_ppo_begin; 0: none yet)
        int64_t ppo_seq = 0;  // minibatch steps issued (mirrors PpoCtl::seq: the index ring position)
        int64_t vc_rows[MAX_MODELS] = {0, 0, 0, 0, 0, 0, 0, 0};   // rows of each critic's table (mirrors VcCtl::n_rows)
        int64_t vc_seq = 0;   // critic steps issued (mirrors VcCtl::seq: the index ring position)
    };
    std::vector<OnPolicyHost> onp = std::vector<OnPolicyHost>(1);
    OnPolicyHost& op() { return onp[(size_t)sel]; }
    // sacx_learners_init: K > 1 learners of the on-policy loop in K arena blocks (seeds = K); 0: none.
    // sacx_ppo_steps_packed / sacx_vcritic_steps_packed run learner 0's plan at grid z = K: plans and
    // graphs of their own (the one-learner plans hold the selected learner's pointers)
    int learners = 0;
    std::map<int, std::vector<Launch>> ppo_pk_plans, vc_pk_plans;
    std::map<std::pair<int, int>, hipGraphExec_t> ppo_pk_graphs, vc_pk_graphs;
    std::map<int, std::vector<Launch>> ppo_plans;                  // minibatch rows -> one step's launches
    std::map<std::pair<int, int>, hipGraphExec_t> ppo_graphs;      // (minibatch rows, steps) -> graph
    // sacx_vcritic_init: the VCritics beside the trainable actor (sacx_vcritic_*, sacx_gae*, build_vc_plan)
    int vc = 0;               // critics (0: none; the layout is then the handle's own)
    int64_t vc_pstride = 0;   // floats between the critics' parameters, Adam moments and gradients
    std::map<int, std::vector<Launch>> vc_plans;
    std::map<std::pair<int, int>, hipGraphExec_t> vc_graphs;
    // sacx_trpo_init: the TRPO actor update (sacx_trpo_*)
    bool trpo = false;
    int trpo_chunk = 0;       // rows per launch chain of a whole-table pass
    int64_t trpo_nv = 0;      // floats of the actor's contiguous trainable range (actor.l0 .. actor.logstd)
    int64_t trpo_rows = 0;    // rows of the table sacx_trpo_begin took (0: none yet)
    int32_t trpo_sub = 1;     // its trust_sub
    hipGraphExec_t trpo_graph = nullptr;               // the captured CG solve ...
    std::tuple<int64_t, int32_t, int32_t> trpo_gkey{0, 0, 0};   // ... of (rows, trust_sub, cg_it)
    hipGraphExec_t trpo_fgraph = nullptr;              // one Fisher product p -> z ...
    std::pair<int64_t, int32_t> trpo_fkey{0, 0};       // ... of (rows, trust_sub)
    // sacx_softmax_init: the actor net's outputs are SoftMaxActor's logits (discrete_actors.py:8-117); the
    // trainables end before actor.logstd, which stays in the layout untouched
    bool softmax = false;
    // layout
    std::vector<SegInfo> segs;
    std::map<std::string, size_t> seg_index;
    uint64_t arena_bytes = 0;
    uint64_t param_off = 0;
    int64_t p_stride = 0;  // floats
    // packed seeds: K learners in K arena blocks seed_bytes apart; `arena` is the block of the
    // selected seed (the per-seed calls), arena0 seed 0's (the plans: grid z covers the rest)
    int seeds = 1, sel = 0;
    int plan_seeds = 1;       // the seed count the plan's shape decisions see (1 with single_seed_plan)
    uint64_t seed_bytes = 0;
    char* arena0 = nullptr;
    // binding
    char* arena = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t cap_stream = nullptr, rng_stream = nullptr;
    bool bound = false;
    std::vector<Launch> plan[NSLOT];
    int64_t slot_bytes = 0;   // distance between consecutive update-input slots
    int nbatch = 4;           // sampler batch (updates per k_rng launch)
    int nslot = 8;            // update-input slots the ring rotates over (a multiple of nbatch, >= 2 nbatch)
    int grow = 0;             // largest batch of the grown schedule of long graphs (sampler_sched.h; 0: nbatch throughout)
    // bf16 weight shadows (SACX_WBF, default on): the matrices (segment "wbf.<name>") and whether
    // add_gemm wires them into the problems it builds (the update plans only)
    struct WbfMat { std::string name; int K, N; };
    std::vector<WbfMat> wbf_mats;
    int wbf_enabled = 3;      // SACX_WBF: 0 off, 1 weights + layer-0 activations, 2 weights only, 3 activations only
    int xbf = 0;              // transposed bf16 images of critic.adam's X operands (SACX_XBF; C5, B % 128 == 0):
                              // 0 off, 1 the critic rows (k_gather) and layer-0 outputs (q.fwd0), 2 the rows only
    bool wbf_attach = false;
    bool wbf_live = false;    // the update plans read / maintain the shadows (refreshed per step call)
    hipEvent_t seg_start = nullptr;   // run_segments: the call's start on the bound stream (before set_ctl)
    // run_segments' cross-stream edges as stream memory operations on signal memory instead of
    // event markers (SACX_SEG_SIG: 1 the side stream's batch-ready edges, 2 (default) also batch
    // 0's, whose marker on the bound stream held segment 0 back: the driver's command 16.00-16.03k
    // -> 16.20-16.23k, r06_ab_seg_sig_v1.txt); 0 where the device lacks stream wait-value
    int seg_sig = 2;
    uint64_t* sig_mem[2] = {nullptr, nullptr};   // batches drawn (side stream), batch 0 drawn (bound stream)
    uint64_t sig_seq[2] = {0, 0};
    std::vector<std::string> abf_segs;          // activation segments with a bf16 shadow ("abf.<name>")
    std::vector<std::pair<const float*, const float*>> abf_written;   // plan build: ranges a wired producer stores
    bool rng_split = false;   // k_rng + k_polar (rng.pairs): the polar transform spread over the GPU
    int pcap = 0;             // polar pairs per update (rng.pairs rows per update)
    // the drop-in loop's draw beside the act (k_act_rng, plain SAC, no split sampler) stores its
    // accepted pairs' words in rng.spairs and the gather queued behind it computes the normals on
    // spare workgroups: the fp64 log / sqrt leave the draw's one workgroup (SACX_SPEC_POLAR)
    bool spec_polar = false;
    bool spec_polar_live = false;   // the queued speculative draw stored pairs
    int spcap = 0;
    bool rng_jump = false;    // segmented sampler (k_mtj_*): the update sampler's launches
    int jL = 0;               // its segment length (words)
    int jsmax = 0;            // segments its work area holds
    int mtj_ramp = 3;         // a graph's first mtj_ramp sampler batches take it (SACX_MTJ_RAMP), the rest k_rng
    int mtj_under = 0;        // tests: cap its segment count (SACX_MTJ_UNDER: forces the redraw fallback)
    int tile32 = 0;           // plan GEMMs on 32x32 workgroup tiles: 1 all, 2 FWD / DX only (SACX_T32)
    int tile32_plan = 0;      // the tile32 a plan of plan_seeds seeds would take: the folds follow it
    int dwl = 0;              // dW + Adam launches on k_dwl: 0 never, 1 when K >= 512, 2 always (SACX_DWL)
    int dwl_nh = 1;           // k_dwl tile width in 16-column halves (SACX_DWL_NH: 1 -> 32x16, 2 -> 32x32)
    int mfuse = 2;            // model fit folds (SACX_MFUSE): 1 the loss into model.fwd2's epilogue and k_mfinal
                              // into model.bwd2, 2 also k_mgather into model.fwd0's operand loads (default);
                              // 3 also model.bwd2 into model.bwd1 (generated operand, heads of <= 32
                              // outputs; bit-identical, measured slower: HC 49.7 vs 46.9 us per step)
    int unaligned_b = 1;      // dX launches: float4 loads of W_ext rows at any 4-B offset (SACX_UNALIGNED)
    int fwd2 = 1;             // two-layer forward pairs as one k_fwd2 launch where they qualify (SACX_FWD2)
    int mtile = 1;            // model fit tiles: 0 16x16, 1 16x16 + wide dW on 32x32, 2 the handle's (SACX_MTILE)
    int mt32 = 5;             // fit launches on 32x32 tiles under mtile 1 (SACX_MT32): 1 model.bwd1, 2 model.fwd1, 4 model.bwd2, 8 model.fwd2
    int dw_round_tiles = 1280;  // 16x16 dW tiles resident at once (SACX_DW_ROUND)
                              // (32x32 tiles accumulate as 16x16 ones: only the folds change sums)
    int xcd_map = 1;          // GEMM tiles XCD-contiguous (xcd_tile)
    int afin = 1;             // k_fwd2's folded alpha finalisation split over q.head's rows (SACX_AFIN; 0: ticket)
    int mfwd2 = 1;            // the fit's gather + model.fwd0 + model.fwd1 as one k_fwd2 launch (SACX_MFWD2)
    int mpre = 1;             // the fit's minibatch rows pre-gathered for a block of steps (SACX_MPRE): the
                              // steps read the staging slots mfit.Xs / mfit.Ts instead of gathering on load
    // data-parallel mode (sacx_dp_init): each rank's local-batch gradients are summed over
    // dp_ranks by RCCL inside the update graph, then every rank applies the same Adam
    int dp_ranks = 0, dp_rank = 0;
    bool dp_local = false;    // sacx_dp_init_local: the ranks are handles of this process (no RCCL)
    ncclComm_t comm = nullptr;
    bool nccl_failed = false;
    // world-model fitting, per seed (packed seeds fit one seed at a time: its arena block's plan)
    std::vector<std::vector<Launch>> mplans;
    std::vector<Launch> mpres;   // per seed: the pre-gather launch of its fit plan (kind RNG: none)
    std::vector<std::map<int, hipGraphExec_t>> mgraphs;   // per seed: fit steps per graph -> graph
    std::vector<int64_t> mfit_hosts;   // model steps issued per seed (mirror ctl->mfit_seq)
    std::map<std::tuple<int, int, int>, hipGraphExec_t> graphs;   // (G, with_rng, skipped kind)
    std::vector<std::pair<RollKey, hipGraphExec_t>> roll_graphs;     // sacx_rollout replays
    std::vector<hipEvent_t> events;
    uint32_t* done_host = nullptr;   // pinned completion counter of act_host's rows (ActRowArgs::done)
    uint32_t* done_dev = nullptr;
    uint32_t done_seq = 0;           // its value once every row launched so far has finished
    bool act_poll = true;            // act_host waits on the counter, not on the stream (SACX_ACT_POLL=0: event)
    float* pin = nullptr;            // pinned host staging (2 x STAGE_CAP floats), the _host entry points:
    float* pin_dev = nullptr;        // [0, STAGE_CAP) appends, [STAGE_CAP, 2 STAGE_CAP) acts; pin_dev is its
                                     // device-side address (kernels read / write it in place)
    hipEvent_t pin_ev = nullptr;     // the last kernel that reads it
    bool pin_pending = false;
    int64_t seq_host = 0;  // updates issued (mirrors ctl->step_seq)
    // Speculative sampler of the drop-in loop (the reference's cadence act -> _update -> env.step ->
    // add, SAC_expert.py:779-797): when the caller steps one update at a time, sacx_actor_act_host
    // queues the next update's randint + normals right behind the action kernel and returns once
    // the action is back, so the draw runs while the host has the action; the next
    // sacx_sac_step(1) then replays a graph without the sampler if the ring still holds the size
    // the draw assumed.  Every other consumer of the RNG stream first undoes the draw (spec_cancel).
    bool spec_enabled = true;  // SACX_SPEC=0: off
    bool spec_live = false;    // a speculative draw is queued
    bool last_step_one = false;  // the last sacx_sac_step was a plain one-update step
    // k_act_rng's held append signals its reads of the staging rows through done_host[1] instead of
    // an event recorded behind it (SACX_APP_CTR); app_seq = the count the host expects
    bool app_ctr = true;         // (and the acts record act_ev only when the host does not poll)
    bool app_ctr_pending = false;
    uint32_t app_seq = 0;
    bool act_ev_live = true;     // act_ev marks the last act (false: nothing recorded, poll only)
    int64_t spec_size = 0;     // the ring size it assumed
    int64_t spec_hits = 0;     // one-update steps that used a speculative draw (sacx_spec_hits)
    int spec_slot = 1;         // the slot the queued draw fills (1 or 2: never the pending alpha's)
    // The alpha branch (alpha.fwd, alpha.head, alpha.final) of the last speculative one-update
    // step is deferred into the next one (merged_body, as inside a captured multi-update graph):
    // the next act needs the updated actor, not alpha.  alpha_pending = that update's slot, or -1;
    // every entry point that could observe or disturb it runs it first (settle).
    int alpha_pending = -1;
    // k_set_ctl skipped when the control block already holds the values: a speculative step(1)
    // right after another with num_timesteps advanced by ts_increment (the folded alpha.final's
    // add) -- the drop-in loop's cadence.  settle() and resync forget it.
    // Deferred append (SACX_APP_DEFER): a 1-row append_host right after a one-update step is held
    // (its row in the pinned staging) and runs as one more workgroup of the next act's k_act_rng
    // launch -- the drop-in cadence's act -> step(1) -> append; every other entry point queues it
    // first (flush_append, from settle and the ring's other users)
    bool app_defer = true;
    bool app_pending = false;
    AppendArgs app_args{};
    bool ctl_skip = true;     // SACX_CTL_SKIP=0: always launch it
    // a fork / join graph's first sampler batch (one update) on the chain's own stream, as the segment
    // graphs do: the chain's first update then does not wait on a cross-queue edge (SACX_G_INLINE0)
    bool g_inline0 = true;
    bool ctl_known = false;
    int64_t ctl_nts = 0;
    int32_t ctl_inc = 0;
    int64_t cur_size_host = 0; // mirrors ctl->cur_size (appends, resync)
    int64_t n_appends = 0;     // sacx_buffer_append calls (a full ring changes content, not size)
    int64_t spec_appends = 0;  // n_appends when the speculative draw was queued
    bool act_rng = true;       // deterministic act + speculative draw in one launch (k_act_rng; SACX_ACT_RNG=0: two)
    hipEvent_t act_ev = nullptr;   // end of the last act_host kernel chain (its actions are on the host)

    uint64_t add(const std::string& name, int64_t rows, int64_t cols, int dtype, int role) {
        const int esz = (dtype == SACX_I64 || dtype == SACX_F64) ? 8 : 4;
        const uint64_t off = (arena_bytes + 255) & ~uint64_t(255);
        segs.push_back({name, off, rows, cols, dtype, role});
        seg_index[name] = segs.size() - 1;
        arena_bytes = off + (uint64_t)(rows * cols * esz);
        return off;
    }
    void alias(const std::string& name, uint64_t off, int64_t rows, int64_t cols, int dtype, int role) {
        segs.push_back({name, off, rows, cols, dtype, role});
        seg_index[name] = segs.size() - 1;
    }
    const SegInfo& seg(const std::string& n) const { return segs.at(seg_index.at(n)); }
    uint64_t off_of(const std::string& n) const { return seg(n).off; }
    template <class T>
    T* ptr(const std::string& n) const { return reinterpret_cast<T*>(arena + seg(n).off); }
    float* f(const std::string& n) const { return ptr<float>(n); }
    // seed 0's segment (the packed launches relocate it by blockIdx.z * seed_bytes)
    float* f0(const std::string& n) const { return reinterpret_cast<float*>(arena0 + seg(n).off); }
    Ctl* ctl() const { return ptr<Ctl>("ctl"); }
    Ctl* ctl0() const { return reinterpret_cast<Ctl*>(arena0 + seg("ctl").off); }
    uint64_t total_bytes() const { return seeds > 1 ? (uint64_t)seeds * seed_bytes : arena_bytes; }
};

namespace {

// a segment of the normaliser set the world models use: mnorm.* (SAC-EO) -- or norm.* on a handle
// without models, where only the update's own normaliser exists
std::string mnorm(const sacx_handle* h, const char* x) {
    return std::string(h->cfg.use_expert ? "mnorm." : "norm.") + x;
}

// the actor's output head (the Dense layer after its last hidden one)
std::string actor_head_name(const sacx_handle* h) { return "actor.l" + std::to_string(h->nd[0].D()); }

int fail(sacx_handle* h, const std::string& msg) {
    if (h) h->err = msg;
    return -1;
}

// Undoes a queued speculative draw (drawn on the bound stream, so stream order alone puts the
// restore after it): restores the RNG state it started from.  keep_state: nothing to restore
// (the caller overwrites the state anyway).
int spec_cancel(sacx_handle* h, bool keep_state = false) {
    if (!h->spec_live) return 0;
    h->spec_live = false;
    // every seed's state (packed seeds: one block per seed, seed_bytes apart)
    const size_t pitch = h->seeds > 1 ? (size_t)h->seed_bytes : sizeof(RngState);
    if (!keep_state &&
        hipMemcpy2DAsync(h->arena0 + h->off_of("rng"), pitch, h->arena0 + h->off_of("rng.spec"), pitch,
                         sizeof(RngState), (size_t)h->seeds, hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
        return fail(h, "spec restore");
    return 0;
}

// the handles the speculative draw applies to: one learner, its own RNG stream
// (never for BC: its update draws no randint, and the speculative draw's fixed-bound randint would
// consume words of the stream the reference's BC never draws)
bool spec_mode(const sacx_handle* h) {
    return h->spec_enabled && h->dp_ranks == 0 && !h->dp_local && h->nslot >= 3 && !h->bc;
}

#define HIPCHK(h, x)                                                                    \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) return fail((h), std::string(#x " -> ") + hipGetErrorString(e_)); \
    } while (0)

constexpr int ACT_CAP = 1024;   // rows per sacx_actor_act launch chain
constexpr int MFIT_GRAPH = 64;      // model-fit steps per captured graph (then 8, then 1)
static_assert(MFIT_GRAPH <= MFIT_PRE, "a fit graph's steps fit one pre-gather block");
constexpr int STAGE_CAP = SACX_STAGE_FLOATS;   // floats in the pinned host staging buffer of the _host entry points
constexpr int ROLL_CAP = 4096;  // trajectories per sacx_rollout launch chain
constexpr int SIM_IDX_CAP = 65536;  // trajectories per sacx_sim_collect call (the index draw's buffer)

void build_layout(sacx_handle* h) {
    const int S = h->S, A = h->A, H0 = h->H0, H1 = h->H1, B = h->B;
    const int F = SACX_F32;
    // ---------------- parameters (Keras W_ext = [W ; b] per Dense layer)
    h->arena_bytes = 0;
    // Keras Dense layers l0 .. l<D> (the last one the output head) of a net with hidden widths w
    auto net = [&](const std::string& n, int in, int out, int role, const std::vector<int>& w) {
        int k = in;
        for (size_t l = 0; l < w.size(); ++l) {
            h->add(n + ".l" + std::to_string(l), k + 1, w[l], F, role);
            k = w[l];
        }
        h->add(n + ".l" + std::to_string(w.size()), k + 1, out, F, role);
    };
    net("actor", S, h->Aout, SACX_ROLE_PARAM, h->nd[0].h);
    if (h->ln) h->add("actor.ln", 2, H0, F, SACX_ROLE_PARAM);     // LayerNormalization gamma ; beta
    h->add("actor.logstd", 1, A, F, SACX_ROLE_PARAM);
    const int Hc0 = h->Hc0, Hc1 = h->Hc1;      // the critics' (--critic_layers)
    net("q0", S + A, 1, SACX_ROLE_PARAM, h->nd[1].h);
    net("q1", S + A, 1, SACX_ROLE_PARAM, h->nd[1].h);
    net("t0", S + A, 1, SACX_ROLE_TARGET, h->nd[1].h);
    net("t1", S + A, 1, SACX_ROLE_TARGET, h->nd[1].h);
    h->add("alpha", 1, 1, F, SACX_ROLE_PARAM);
    if (h->cfg.use_expert) {
        // per model, in model.trainable order (continuous_models.py:27-32, :216-221): the model net,
        // GaussianModel's logstd, the separate reward net -- one contiguous range (the global-norm clip)
        for (int k = 0; k < h->nm; ++k) {
            const std::string m = "m" + std::to_string(k);
            net(m, S + A, h->Om, SACX_ROLE_PARAM, h->nd[2].h);
            if (h->gm) h->add(m + ".logstd", 1, S, F, SACX_ROLE_PARAM);
            if (h->srn) net("r" + std::to_string(k), S + A, 1, SACX_ROLE_PARAM, h->nd[3].h);
        }
    }
    const uint64_t pbytes = (h->arena_bytes + 255) & ~uint64_t(255);
    h->param_off = 0;
    h->p_stride = (int64_t)(pbytes / 4);
    h->alias("params", 0, 1, h->p_stride, F, SACX_ROLE_PARAM);
    h->arena_bytes = pbytes;
    h->add("adam_m", 1, h->p_stride, F, SACX_ROLE_STATE);
    h->add("adam_v", 1, h->p_stride, F, SACX_ROLE_STATE);
    h->add("grad", 1, h->p_stride, F, SACX_ROLE_WORK);   // data-parallel gradients (+3 p_stride)
    // ---------------- normalisers (normalizer.py: (x - mean) / max(std, 1e-8))
    h->add("norm.s_mean", 1, S, F, SACX_ROLE_STATE);
    h->add("norm.s_den", 1, S, F, SACX_ROLE_STATE);
    h->add("norm.a_mean", 1, A, F, SACX_ROLE_STATE);
    h->add("norm.a_den", 1, A, F, SACX_ROLE_STATE);
    h->add("norm.d_mean", 1, S, F, SACX_ROLE_STATE);
    h->add("norm.d_den", 1, S, F, SACX_ROLE_STATE);
    h->add("norm.r", 1, 2, F, SACX_ROLE_STATE);  // r_mean, r_den
    h->add("norm.ret_den", 1, 1, F, SACX_ROLE_STATE);
    // bf16 shadows of the SAC nets' hidden-layer weights (config C5, 32x32 forward tiles): the
    // forward launches read B from them (wbf_pos layout), the Adam epilogues keep them current
    h->wbf_mats.clear();
    if (h->cfg.gemm_bf16 && !h->deep && (h->wbf_enabled == 1 || h->wbf_enabled == 2)) {
        const char* nets[] = {"actor", "q0", "q1", "t0", "t1"};
        for (const char* n : nets) {
            const bool act = std::string(n) == "actor";
            const int in = act ? S : S + A, h0 = act ? H0 : Hc0, h1 = act ? H1 : Hc1;
            for (int l = 0; l < 2; ++l) {
                const int K = l == 0 ? in : h0, N = l == 0 ? h0 : h1;
                const std::string w = std::string(n) + ".l" + std::to_string(l);
                h->add("wbf." + w, N, wbf_ld_of(K) / 2, SACX_U32, SACX_ROLE_WORK);
                h->wbf_mats.push_back({w, K, N});
            }
        }
    }
    // the world models' own normaliser set (SAC_expert.py:53-54, :139-144): a copy of norm.*
    // unless --only_model_normalizer gives the models a RunningNormalizers of their own
    if (h->cfg.use_expert) {
        h->add("mnorm.s_mean", 1, S, F, SACX_ROLE_STATE);
        h->add("mnorm.s_den", 1, S, F, SACX_ROLE_STATE);
        h->add("mnorm.a_mean", 1, A, F, SACX_ROLE_STATE);
        h->add("mnorm.a_den", 1, A, F, SACX_ROLE_STATE);
        h->add("mnorm.d_mean", 1, S, F, SACX_ROLE_STATE);
        h->add("mnorm.d_den", 1, S, F, SACX_ROLE_STATE);
        h->add("mnorm.r", 1, 2, F, SACX_ROLE_STATE);
    }
    // ---------------- control + RNG
    h->add("ctl", 1, CTL_WORDS, SACX_I64, SACX_ROLE_STATE);
    const uint64_t roff = h->add("rng", 1, sizeof(RngState) / 4, SACX_U32, SACX_ROLE_STATE);
    h->alias("rng.key", roff, 1, 624, SACX_U32, SACX_ROLE_STATE);
    h->alias("rng.pos", roff + offsetof(RngState, pos), 1, 2, SACX_I32, SACX_ROLE_STATE);
    h->alias("rng.gauss", roff + offsetof(RngState, gauss), 1, 1, SACX_F64, SACX_ROLE_STATE);
    h->add("rng.spec", 1, sizeof(RngState) / 4, SACX_U32, SACX_ROLE_WORK);   // state before a speculative draw
    // Split sampler (many normals per update, Humanoid): k_rng ranks the accepted polar pairs and
    // stores their four words; k_polar turns them into normals over the whole GPU
    h->rng_split = h->n_norm > 16384;
    if (const char* e = std::getenv("SACX_RNG_SPLIT")) h->rng_split = std::atoi(e) != 0;
    if (h->rng_split) {
        h->pcap = (h->n_norm + 1) / 2;
        h->add("rng.pairs", (int64_t)NBATCH_MAX * h->pcap, 4, SACX_U32, SACX_ROLE_WORK);
        h->add("rng.pairs_oi", 1, NBATCH_MAX, SACX_I32, SACX_ROLE_WORK);
    }
    h->spec_polar = !h->rng_split && !h->cfg.use_expert && h->n_norm > 0;
    if (const char* e = std::getenv("SACX_SPEC_POLAR")) h->spec_polar = h->spec_polar && std::atoi(e) != 0;
    if (h->spec_polar) {
        h->spcap = (h->n_norm + 1) / 2;
        h->add("rng.spairs", h->spcap, 4, SACX_U32, SACX_ROLE_WORK);
        h->add("rng.spairs_oi", 1, 1, SACX_I32, SACX_ROLE_WORK);
    }
    // Segmented sampler (k_mtj_*): a sampler batch of many words (Humanoid: ~135k per update)
    // is twisted as ~16 segments of L words from jumped-ahead windows and ranked over the GPU
    // instead of on one workgroup.  L: a 4-update batch in ~16 segments, >= the 20,561 words
    // every jump reads; the work area holds a batch of NBATCH_MAX updates
    {
        const double per = 2.0 * h->B + (double)((h->n_norm + 1) >> 1) * (4.0 / 0.78539816339744831);
        h->rng_jump = per >= 40000.0;
        if (const char* e = std::getenv("SACX_RNG_JUMP")) h->rng_jump = std::atoi(e) != 0;
        if (h->rng_jump) {
            int64_t L = ((int64_t)std::ceil(per * 1.02 / 4.0) + 63) / 64 * 64;
            if (const char* e = std::getenv("SACX_MTJ_L")) L = std::atoll(e);
            L = std::max<int64_t>(L, MTJ_HEAD);
            const double words = NBATCH_MAX * per;
            const double est = 624.0 + 1.02 * words + 8.0 * std::sqrt(words) + 64.0 * NBATCH_MAX + 1024.0 + MTJ_HEAD;
            int smax = (int)std::ceil((est - 1.0) / (double)L) + 1;
            smax = (int)std::max<int64_t>(2, std::min<int64_t>(smax, ((int64_t)MTJ_MAXCHK * MTJ_CHK - 9) / L));
            h->jL = (int)L;
            h->jsmax = smax;
            h->add("rng.jw", 1, mtj_layout(L, smax).total, SACX_U32, SACX_ROLE_WORK);
            // x^(kL) mod phi as per-chunk set-bit lists (mt_jump_lists), uploaded at bind
            h->add("rng.jc", 1, mt_jump_lists_words(smax - 1, MTJ_CH), SACX_I32, SACX_ROLE_STATE);
        }
    }
    // per-slot update inputs: the sampler + gather run ahead of the updates on a side stream,
    // so everything they write rotates over a ring of slots.  A cheap sampler (HC: 1,536 normals
    // per update) gets 128 slots: a graph of up to 128 updates draws every input at its start,
    // with no sampler launch waiting on the update chain (a 20-update graph otherwise waits
    // ~0.1 ms at update 8 for a sampler batch the runtime releases only when the chain reaches
    // it), and a longer one draws 64 updates per batch (sampler_sched.h); four or more packed
    // seeds multiply the ring and keep 32; an expensive sampler (Humanoid: 10 MB of slot rows
    // per update) keeps 8, the footprint the caches hold
    h->nslot = h->n_norm <= 16384 ? (h->seeds >= 4 ? 32 : NSLOT) : 8;
    if (const char* e = std::getenv("SACX_NSLOT")) h->nslot = std::max(2, std::min(NSLOT, std::atoi(e)));
    const int ne1 = std::max(1, h->ne);
    // config C5: critic.adam's bf16 32x32 tiles read X^T (the critic rows, the critics' layer-0
    // outputs) from transposed images their producers write (k_gather, q.fwd0's epilogue) instead
    // of converting strided fp32 columns; B % 128 == 0, so the images have no pad positions
    h->xbf = 0;
    if (const char* e = std::getenv("SACX_CTL_SKIP")) h->ctl_skip = std::atoi(e) != 0;
    if (const char* e = std::getenv("SACX_APP_CTR")) h->app_ctr = std::atoi(e) != 0;
    if (const char* e = std::getenv("SACX_SEG_SIG")) h->seg_sig = std::atoi(e);
    if (const char* e = std::getenv("SACX_G_INLINE0")) h->g_inline0 = std::atoi(e) != 0;
    if (const char* e = std::getenv("SACX_APP_DEFER")) h->app_defer = std::atoi(e) != 0;
    if (const char* e = std::getenv("SACX_XBF"))
        if (h->cfg.gemm_bf16 && !h->deep && B % 128 == 0) h->xbf = std::max(0, std::min(2, std::atoi(e)));
    for (int s = 0; s < h->nslot; ++s) {
        const std::string sl = "slot" + std::to_string(s);
        h->add(sl + ".idx", 1, B, SACX_I32, SACX_ROLE_WORK);
        h->add(sl + ".noise", 1, h->n_norm, F, SACX_ROLE_WORK);
        h->add(sl + ".Xa", h->Ra, h->ldS, F, 0);   // actor rows [sp ; s ; s_e] (normalised)
        h->add(sl + ".Xq", B, h->ldQ, F, 0);       // critic rows [s | a]
        h->add(sl + ".Xt", B, h->ldQ, F, 0);       // target rows [sp | pi(sp)]
        h->add(sl + ".Xp", B, h->ldQ, F, 0);       // policy rows [s | pi(s)]
        h->add(sl + ".Xm", ne1, h->ldQ, F, 0);     // expert rows [s_e | pi(s_e)]
        h->add(sl + ".r", 1, B, F, 0);
        h->add(sl + ".d", 1, B, F, 0);
        h->add(sl + ".se_raw", ne1, S, F, 0);
        h->add(sl + ".spe_raw", ne1, S, F, 0);
        if (h->xbf) h->add(sl + ".xbfq", S + A, wbf_ld_of(B) / 2, SACX_U32, SACX_ROLE_WORK);
    }
    h->slot_bytes = (int64_t)(h->off_of("slot1.idx") - h->off_of("slot0.idx"));
    for (int k = 1; k < h->nslot; ++k)   // the batched sampler / gather address slot k as slot 0 + k * slot_bytes
        for (const char* nm : {".idx", ".noise", ".Xa", ".Xq", ".Xt", ".Xp", ".Xm", ".r", ".d", ".se_raw", ".spe_raw", ".xbfq"})
            if ((std::string(nm) != ".xbfq" || h->xbf) &&
                (h->off_of("slot" + std::to_string(k) + nm) != h->off_of(std::string("slot0") + nm) + k * (uint64_t)h->slot_bytes)) {
                fprintf(stderr, "sacx: slot layout is not uniform\n");
                abort();
            }
    // ---------------- data
    h->add("replay", h->cap, h->stride, F, SACX_ROLE_STATE);
    const int ecap = std::max(1, h->ecap);
    h->add("expert.s", ecap, S, F, SACX_ROLE_STATE);
    h->add("expert.sp", ecap, S, F, SACX_ROLE_STATE);
    h->add("perm", h->perm_cap, std::max(1, h->ne_perm), SACX_I32, SACX_ROLE_STATE);
    h->add("stats", h->stats_cap, 8, F, SACX_ROLE_STATE);
    h->add("red", 1, std::max(1024, (B + 3) / 4), F, SACX_ROLE_WORK);
    h->add("ws.afin", 1, sizeof(AfinPre) / 4, F, SACX_ROLE_WORK);   // the split alpha finalisation's snapshot
    // ---------------- workspace
    const int Ra = h->Ra, Rb = h->Rb, Hm0 = std::max(1, h->Hm0), Hm1 = std::max(1, h->Hm1);
    // actor activations; rows [Ra4, Ra4 + B) hold the alpha evaluate() of an update
    // (aliased ws.Hl1 / ws.Hl2) so one grouped head launch can serve both
    const int Ra4 = (Ra + 3) & ~3;
    // a chain's per-layer buffers: <p>1 = hidden layer 0, <p>2 = the last hidden layer -- one segment
    // each at two layers (the fused plans' layout), with one layer <p>2 aliases <p>1; the middle layers
    // <p>m<i> of deeper nets (the generic plans) are added at the end of the workspace (mids)
    auto last = [&](const std::string& n2, const std::string& n1, int64_t rows, int w2, int D) -> uint64_t {
        if (D >= 2) return h->add(n2, rows, w2, F, 0);
        const SegInfo& s1 = h->seg(n1);
        h->alias(n2, s1.off, s1.rows, s1.cols, F, 0);
        return s1.off;
    };
    struct Mid { std::string p; int64_t rows; int net; };
    std::vector<Mid> mids;
    const int Da = h->nd[0].D(), Dc = h->nd[1].D(), Dm = h->nd[2].D(), Dr = h->nd[3].D();
    const uint64_t oHa1 = h->add("ws.Ha1", Ra4 + B, H0, F, 0);
    const uint64_t oHa2 = last("ws.Ha2", "ws.Ha1", Ra4 + B, H1, Da);
    mids.push_back({"ws.Ham", Ra4 + B, 0});
    // Ha2 . W3 per 16-column tile of actor.fwd1 (rows as ws.Ha2), summed by the head rows
    h->add("ws.hpart", Ra4 + B, (int64_t)h->Aout * ((H1 + 15) / 16), F, 0);
    h->add("ws.c_t", Rb, A, F, 0);
    h->add("ws.c_std", Rb, A, F, 0);
    h->add("ws.c_u", Rb, A, F, 0);
    h->add("ws.c_mask", Rb, A, F, 0);
    h->add("ws.nlp_t", 1, B, F, 0);
    h->add("ws.nlp_p", 1, B, F, 0);
    h->add("ws.nlp3", 1, B, F, 0);
    h->add("ws.Hq1", 4 * B, Hc0, F, 0);
    last("ws.Hq2", "ws.Hq1", 4 * B, Hc1, Dc);
    if (Dc >= 2) h->add("ws.Dq2", 2 * B, Hc1, F, 0);
    h->add("ws.Dq1", 2 * B, Hc0, F, 0);
    if (Dc < 2) last("ws.Dq2", "ws.Dq1", 2 * B, Hc1, Dc);
    mids.push_back({"ws.Hqm", 4 * B, 1});
    mids.push_back({"ws.Dqm", 2 * B, 1});
    h->add("ws.gq", 2, B, F, 0);
    h->add("ws.lq", 2, B, F, 0);
    h->add("ws.Hp1", 2 * B, Hc0, F, 0);
    last("ws.Hp2", "ws.Hp1", 2 * B, Hc1, Dc);
    h->add("ws.Dp1", 2 * B, Hc0, F, 0);
    if (h->deep) {                    // the generic plan's policy-row deltas (the fused one keeps partials)
        last("ws.Dp2", "ws.Dp1", 2 * B, Hc1, Dc);
        mids.push_back({"ws.Hpm", 2 * B, 1});
        mids.push_back({"ws.Dpm", 2 * B, 1});
    }
    h->add("ws.lp", 1, B, F, 0);
    h->add("ws.gp", 2, B, F, 0);                 // policy-row output gradients of q0, q1
    h->add("ws.apart", 2 * B, ((Hc0 + 15) / 16) * A, F, 0);  // their action-gradient partials (folded head bwd)
    h->add("ws.mpart", ne1, ((Hm0 + 15) / 16) * A, F, 0);       // the expert rows' ones (SAC-EO, model.bwd1)
    h->add("ws.ones", 1, std::max(std::max(Rb, B), std::max(1, h->mb)) + 4, F, SACX_ROLE_STATE);
    h->add("ws.Hm1", ne1, Hm0, F, 0);
    last("ws.Hm2", "ws.Hm1", ne1, Hm1, Dm);
    if (Dm >= 2) h->add("ws.Dm2", ne1, Hm1, F, 0);
    h->add("ws.Dm1", ne1, Hm0, F, 0);
    if (Dm < 2) last("ws.Dm2", "ws.Dm1", ne1, Hm1, Dm);
    if (h->cfg.use_expert) {
        mids.push_back({"ws.Hmm", ne1, 2});
        mids.push_back({"ws.Dmm", ne1, 2});
    }
    h->add("ws.mse", ne1, (S + 15) / 16, F, 0);       // per-column-tile partials of the expert MSE
    h->add("ws.dout", ne1, S, F, 0);                  // d loss / d model output (expert rows)
    h->add("ws.Da3", Rb, h->Aout, F, 0);
    if (Da >= 2) h->add("ws.Da2", Rb, H1, F, 0);
    h->add("ws.Da1", Rb, H0, F, 0);
    if (Da < 2) last("ws.Da2", "ws.Da1", Rb, H1, Da);
    mids.push_back({"ws.Dam", Rb, 0});
    h->add("ws.E", Rb, A, F, 0);
    h->alias("ws.Hl1", oHa1 + (uint64_t)Ra4 * H0 * 4, B, H0, F, 0);
    h->alias("ws.Hl2", oHa2 + (uint64_t)Ra4 * H1 * 4, B, H1, F, 0);
    // bf16 shadows of the layer-0 outputs the 32x32 bf16 forward tiles of layer 1 read as A
    // (H0 a multiple of 128: every shadow position holds a k < H0; not under the layer norm,
    // which rewrites the actor's layer-0 output after the GEMM)
    h->abf_segs.clear();
    if (h->cfg.gemm_bf16 && !h->deep && (h->wbf_enabled == 1 || h->wbf_enabled == 3))
        for (const char* n : {"ws.Ha1", "ws.Hq1", "ws.Hp1"}) {
            const bool act = std::string(n) == "ws.Ha1";
            const int w = act ? H0 : Hc0;
            if (w % 128 != 0 || (act && h->ln)) continue;
            const auto& sg = h->seg(n);
            h->add(std::string("abf.") + n, sg.rows, w / 2, SACX_U32, SACX_ROLE_WORK);
            h->abf_segs.push_back(n);
        }
    // (config C5) the critics' layer-0 outputs transposed: one image per q.fwd0 problem (t0 t1 q0 q1)
    if (h->xbf == 1) h->add("xbf.ws.Hq1", 4 * (int64_t)Hc0, wbf_ld_of(B) / 2, SACX_U32, SACX_ROLE_WORK);
    // behaviour-policy inference (sacx_actor_act), up to ACT_CAP rows per launch chain
    h->add("act.X", ACT_CAP, h->ldS, F, 0);
    // (sacx_critic_forward's too; the generic plans' nets alternate between the two: any layer's width)
    auto wmax = [&](int n) { return *std::max_element(h->nd[n].h.begin(), h->nd[n].h.end()); };
    h->add("act.H1", ACT_CAP, h->deep ? std::max(wmax(0), wmax(1)) : std::max(H0, Hc0), F, 0);
    h->add("act.H2", ACT_CAP, h->deep ? std::max(wmax(0), wmax(1)) : std::max(H1, Hc1), F, 0);
    h->add("act.noise", 1, (int64_t)ACT_CAP * A, F, 0);
    if (h->ln) {                      // layer-norm caches of the update's actor rows
        h->add("ws.ln_xhat", h->Ra, H0, F, 0);
        h->add("ws.ln_rstd", 1, h->Ra, F, 0);
        h->add("ws.ln_gy", h->Rb, H0, F, 0);
        h->add("ws.ln_gb", h->Rb, H0, F, 0);
    }
    h->add("act.Xq", ACT_CAP, h->ldQ, F, 0);          // sacx_critic_forward input [norm s | norm a]
    h->add("act.Q", ACT_CAP, 1, F, 0);                // sacx_critic_forward output
    if (h->cfg.use_expert) {          // world-model fitting (A16)
        const int R2 = h->nm * h->mb, O = S + 1;
        // the models' output rows: a rollout chunk, or every model on the diagnostics' <= 2048 rows
        const int64_t RR = std::max<int64_t>(ROLL_CAP, (int64_t)h->nm * 2048);
        h->add("mfit.idx", h->mfit_cap, R2, SACX_I32, SACX_ROLE_WORK);
        h->add("ws.gnorm", 1, GNORM_PARTS + 1, F, 0);   // clip_by_global_norm partials + scale
        h->add("mstats", h->stats_cap, 2, F, SACX_ROLE_STATE);
        h->add("ws.Xf", R2, h->ldQ, F, 0);
        h->add("ws.Tf", R2, O, F, 0);
        h->add("mfit.Xs", MFIT_PRE, (int64_t)R2 * h->ldQ, F, 0);   // pre-gathered rows / targets of a block of steps
        h->add("mfit.Ts", MFIT_PRE, (int64_t)R2 * O, F, 0);
        h->add("ws.Hf1", R2, Hm0, F, 0);
        last("ws.Hf2", "ws.Hf1", R2, Hm1, Dm);
        h->add("ws.Of", R2, O, F, 0);
        h->add("ws.Df3", R2, r4(O), F, 0);    // float4 rows: model.bwd2's A operand
        if (Dm >= 2) h->add("ws.Df2", R2, Hm1, F, 0);
        h->add("ws.Df1", R2, Hm0, F, 0);
        if (Dm < 2) last("ws.Df2", "ws.Df1", R2, Hm1, Dm);
        mids.push_back({"ws.Hfm", R2, 2});
        mids.push_back({"ws.Dfm", R2, 2});
        // fit-loss partials (per row: k_mloss); --separate_reward_nn: then one per row of the reward heads
        h->add("ws.lf", 1, (int64_t)R2 * ((O + 15) / 16) + (h->srn ? R2 : 0), F, 0);
        if (h->srn) {                 // the reward nets' fit activations / deltas
            const int Hr0 = h->Hr0, Hr1 = h->Hr1;
            h->add("ws.Hrf1", R2, Hr0, F, 0);
            last("ws.Hrf2", "ws.Hrf1", R2, Hr1, Dr);
            h->add("ws.Drf3", R2, 4, F, 0);         // d loss / d reward (float4 rows)
            if (Dr >= 2) h->add("ws.Drf2", R2, Hr1, F, 0);
            h->add("ws.Drf1", R2, Hr0, F, 0);
            if (Dr < 2) last("ws.Drf2", "ws.Drf1", R2, Hr1, Dr);
            mids.push_back({"ws.Hrfm", R2, 3});
            mids.push_back({"ws.Drfm", R2, 3});
            h->add("roll.R1", RR, h->deep ? wmax(3) : Hr0, F, 0);
            h->add("roll.R2", RR, h->deep ? wmax(3) : Hr1, F, 0);
        }
        if (h->gm) {                  // logstd-gradient partials per model, 16-row tile and column
            h->add("ws.lgp", h->nm * ((h->mb + 15) / 16), S, F, 0);
            h->add("roll.mnoise", 1, RR * S, F, 0);   // exp(logstd) * u noise (sample / step, every model's)
        }
        // model rollout (sacx_rollout), up to ROLL_CAP trajectories per launch chain
        h->add("roll.X", ROLL_CAP, h->ldS, F, 0);
        h->add("roll.H1", ROLL_CAP, h->deep ? wmax(0) : H0, F, 0);
        h->add("roll.H2", ROLL_CAP, h->deep ? wmax(0) : H1, F, 0);
        h->add("roll.noise", 1, (int64_t)ROLL_CAP * A, F, 0);
        h->add("roll.A", ROLL_CAP, A, F, 0);
        h->add("roll.Xm", ROLL_CAP, h->ldQ, F, 0);
        h->add("roll.M1", RR, h->deep ? wmax(2) : Hm0, F, 0);
        h->add("roll.M2", RR, h->deep ? wmax(2) : Hm1, F, 0);
        h->add("roll.O", RR, O, F, 0);
        // sacx_sim_collect's drawn ring rows (only the new handle kind: the others keep their layout)
        if (h->models_only) h->add("roll.idx", 1, SIM_IDX_CAP, SACX_I32, 0);
    }
    // the middle hidden layers (1 .. D-2) of nets deeper than two layers: <p>m<i>
    for (const Mid& m : mids)
        for (int i = 1; i + 1 < h->nd[m.net].D(); ++i)
            h->add(m.p + std::to_string(i), m.rows, h->nd[m.net].h[i], F, 0);
    // the PPO actor step of a trainable GaussianActor handle: after everything else, so the segments
    // of every other handle kind keep their offsets
    if (h->ppo) {
        const int64_t cap = h->cap;
        static_assert(sizeof(PpoCtl) == 64 && sizeof(PpoPar) == 64, "ppo.ctl is 8 int64, ppo.par 16 words");
        h->add("ppo.ctl", 1, 8, SACX_I64, SACX_ROLE_STATE);
        h->add("ppo.par", 1, 16, F, SACX_ROLE_WORK);
        h->add("ppo.alpha", 1, 3, F, SACX_ROLE_STATE);       // alpha (starts at 0, ppo.py:36), Adam m, v
        h->add("ppo.acc", 1, 8, F, SACX_ROLE_STATE);
        h->add("ppo.log", 1, 8, F, SACX_ROLE_STATE);
        h->add("ppo.stats", h->stats_cap, 8, F, SACX_ROLE_STATE);
        h->add("ppo.idx", PPO_IDX_CAP, B, SACX_I32, SACX_ROLE_WORK);
        // the rollout table and what sacx_ppo_begin computes per row
        h->add("ppo.s", cap, S, F, SACX_ROLE_STATE);
        h->add("ppo.a", cap, A, F, SACX_ROLE_STATE);
        h->add("ppo.adv", 1, cap, F, SACX_ROLE_STATE);
        h->add("ppo.nlp_old", 1, cap, F, SACX_ROLE_STATE);
        h->add("ppo.mean_ref", cap, A, F, SACX_ROLE_STATE);
        h->add("ppo.ls_ref", cap, A, F, SACX_ROLE_STATE);
        h->add("ppo.tmp", 2, cap, F, 0);                     // per-row entropy / |r - 1|, kl of the whole-rollout passes
        // the minibatch rows of a step (the hidden layers and deltas are the update's ws.Ha* / ws.Da*)
        h->add("ppo.X", B, h->ldS, F, 0);
        h->add("ppo.A", B, A, F, 0);
        h->add("ppo.advn", 1, B, F, 0);
        h->add("ppo.nlpo", 1, B, F, 0);
        h->add("ppo.rl", 2, B, F, 0);                        // per-row loss, entropy
        h->add("ppo.O", std::max(B, ACT_CAP), h->Aout, F, 0);   // the actor's output rows (a step's, or a chunk's)
        h->add("ppo.gnorm", 1, GNORM_PARTS, F, 0);
    }
    h->arena_bytes = (h->arena_bytes + 255) & ~uint64_t(255);
}

// ---------------------------------------------------------------- GEMM problem helpers
GemmProb prob_fwd(const float* X, int ldx, int M, int K, const float* Wext, int N, float* C, int act) {
    GemmProb p{};
    p.A = X; p.lda = ldx; p.a_kc = 1; p.ones_row = -1;
    p.B = Wext; p.ldb = N; p.b_kc = 0;
    p.M = M; p.N = N; p.K = K;
    p.bias = Wext + (size_t)K * N;
    p.C = C; p.ldc = N;
    p.epi = EPI_FWD; p.act = act;
    return p;
}

// C = (D * W^T) (.) act'(Hprev), W_ext is [(K_in+1) x N_out]; C is [M x K_in]
GemmProb prob_dx(const float* D, int M, int Nout, const float* Wext, int Kin, const float* Hprev, float* C, int act) {
    GemmProb p{};
    p.A = D; p.lda = Nout; p.a_kc = 1; p.ones_row = -1;
    p.B = Wext; p.ldb = Nout; p.b_kc = 1;   // B[k][n] = W[n][k]
    p.M = M; p.N = Kin; p.K = Nout;
    p.H = Hprev; p.ldh = Kin;
    p.C = C; p.ldc = Kin;
    p.epi = EPI_DACT; p.act = act;
    return p;
}

// dW_ext = [X | 1]^T * D over R rows, then Adam (+ Polyak into T)
GemmProb prob_dw(const float* X, int ldx, int Kin, int R, const float* D, int Nout, float* P, float* T, int group) {
    GemmProb p{};
    p.A = X; p.lda = ldx; p.a_kc = 0; p.ones_row = Kin;
    p.B = D; p.ldb = Nout; p.b_kc = 0;
    p.M = Kin + 1; p.N = Nout; p.K = R;
    p.P = P; p.T = T; p.ldp = Nout;
    p.epi = EPI_ADAM; p.group = group; p.grad_scale = 1.f;
    return p;
}

// algorithmic counts (the fused layer 0 counted once, not per column tile)
double gemm_flops(const GemmProb& p) { return 2.0 * p.M * p.N * p.K; }
double gemm_bytes(const GemmProb& p) {
    double b = 4.0 * ((double)p.M * p.K + (double)p.K * p.N + (double)p.M * p.N);
    if (p.epi == EPI_ADAM) b += 4.0 * p.M * p.N * (p.T ? 8 : 6) - 4.0 * p.M * p.N;
    if (p.epi == EPI_DACT) b += 4.0 * p.M * p.N;
    return b;
}

// The bf16 weight shadows of a problem (SACX_WBF): a forward problem on 32x32 tiles reads the
// shadow of its B; a dW + Adam problem stores the shadows of the P and T it updates
void wbf_wire(sacx_handle* h, GemmProb& p, int mode, bool t32) {
    auto find = [&](const float* w) -> const sacx_handle::WbfMat* {
        for (const auto& m : h->wbf_mats)
            if (w != nullptr && w == h->f(m.name)) return &m;
        return nullptr;
    };
    if (mode == GM_FWD && t32) {
        const auto* m = find(p.B);
        if (m && m->K == p.K && m->N == p.N && p.ldb == p.N) {
            p.wbf = h->ptr<uint16_t>("wbf." + m->name);
            p.wbf_ld = wbf_ld_of(m->K);
            p.wbf_per = wbf_per_of(m->K);
        }
        // activations: a plain forward problem whose output lies in a shadowed segment stores its
        // shadow; a layer-1 problem reads A from the shadow when a wired producer of this plan
        // stores every row it reads (ranges recorded in build order: producers come first)
        for (const auto& n : h->abf_segs) {
            const auto& sg = h->seg(n);
            const float* base = h->f(n);
            const float* end = base + (size_t)sg.rows * sg.cols;
            if (p.C && p.C >= base && p.C < end && p.ldc == sg.cols && p.N == sg.cols && p.mse == 0 &&
                p.C + (size_t)p.M * p.ldc <= end) {
                p.obf = h->ptr<uint16_t>("abf." + n) + (p.C - base);
                h->abf_written.push_back({p.C, p.C + (size_t)p.M * p.ldc});
            }
            if (p.A >= base && p.A < end && p.lda == sg.cols && p.K == sg.cols && p.headp == 0) {
                const float* a1 = p.A + (size_t)p.M * p.lda;
                bool covered = false;
                for (const auto& w : h->abf_written) covered = covered || (p.A >= w.first && a1 <= w.second);
                if (covered) p.abf = h->ptr<uint16_t>("abf." + n) + (p.A - base);
            }
        }
    } else if (mode == GM_DW && p.epi == EPI_ADAM) {
        const auto* m = find(p.P);
        if (!m || m->K != p.M - 1 || m->N != p.N || p.ldp != p.N) return;
        p.wbf = h->ptr<uint16_t>("wbf." + m->name);
        p.wbf_ld = wbf_ld_of(m->K);
        p.wbf_per = wbf_per_of(m->K);
        p.wbf_k = m->K;
        if (const auto* t = find(p.T)) p.obf = h->ptr<uint16_t>("wbf." + t->name);
    }
}

AdamConsts adam_consts(const sacx_handle* h) {
    AdamConsts c{};
    c.lr[GRP_Q] = h->cfg.lr_q;
    c.lr[GRP_PI] = h->cfg.lr_pi;
    c.lr[GRP_ALPHA] = h->cfg.lr_alpha;
    c.lr[GRP_MODEL] = h->cfg.lr_model;
    c.tau_keep = (float)(1.0 - (double)h->cfg.tau);
    c.tau_take = h->cfg.tau;
    c.target_update_int = h->cfg.target_update_int;
    return c;
}

// The tile shapes a GEMM launch may take, in the values of sacx_handle::tile32 / dwl; -1: the handle's.  A plan
// whose tiles are its own (the world-model fit, a TRPO chunk) passes them; every other launch takes the default
struct GemmTiles { int tile32 = -1, dwl = -1; };

void add_gemm(sacx_handle* h, std::vector<Launch>& plan, const std::string& name, std::vector<GemmProb> ps, GemmTiles tl = {}) {
    if (tl.tile32 < 0) tl.tile32 = h->tile32;
    if (tl.dwl < 0) tl.dwl = h->dwl;
    Launch L{};
    L.kind = Launch::GEMM;
    L.name = name;
    // 32x32 workgroup tiles for plain FWD / DX / DW launches when the handle asks for them
    // (packed seeds: many tiles per launch); head-prologue and fused two-layer launches stay 16x16
    // (tile32 = 2: forward / dX launches only -- the dW + Adam epilogue's registers cost occupancy)
    bool t32 = tl.tile32 > 0;
    // tile32 = 2 keeps dW + Adam on 16x16 tiles (their registers cost occupancy), except a launch
    // whose 16x16 tiles exceed what is resident at once (5 workgroups on each of 256 CUs): there
    // the last tiles start a whole workgroup time late (Humanoid critic.adam: 1,378 tiles, 11 us
    // of skew in a 23 us launch), and 32x32 tiles -- bit-identical sums -- run in one round
    // (tools/dw_bench.hip: Humanoid critic.adam 23.7 -> 21.0 us fp32, 21.1 -> 14.3 us bf16)
    int tiles16 = 0;
    for (auto& p : ps) tiles16 += ((p.M + 15) / 16) * ((p.N + 15) / 16);
    const bool dw_wide = tiles16 > h->dw_round_tiles;
    for (auto& p : ps)
        t32 = t32 && p.headp == 0 && !(tl.tile32 == 2 && p.epi == EPI_ADAM && !dw_wide) && p.hbw == 0;
    // dW + Adam launches with long reductions take k_dwl (32x32 tiles, LDS-DMA staged rows)
    bool dwl = tl.dwl > 0;
    int kmax = 0;
    for (auto& p : ps) {
        dwl = dwl && p.epi == EPI_ADAM;
        kmax = std::max(kmax, (int)p.K);
    }
    dwl = dwl && (tl.dwl == 2 || kmax >= 512);
    if (dwl) t32 = false;
    const int ts = (t32 || dwl) ? 32 : 16;
    const int tsn = dwl ? 16 * h->dwl_nh : ts;    // k_dwl: 32 x 16 NH tiles
    int tiles = 0;
    for (auto& p : ps) {
        p.tiles_n = (p.N + tsn - 1) / tsn;
        p.tile_begin = tiles;
        tiles += ((p.M + ts - 1) / ts) * p.tiles_n;
        L.flops += gemm_flops(p);
        L.bytes += gemm_bytes(p);
    }
    L.gemm.t32 = t32 ? 1 : 0;
    if (ps.size() > GEMM_MAXP) { fprintf(stderr, "sacx: too many GEMM problems in %s\n", name.c_str()); abort(); }
    // every problem of a launch must share the operand/epilogue mode (k_gemm template)
    auto mode_of = [](const GemmProb& p) {
        return p.epi == EPI_ADAM ? GM_DW : (p.epi == EPI_DACT ? GM_DX : GM_FWD);
    };
    const int mode = mode_of(ps[0]);
    bool vec = false;   // any problem with float4 loads (each problem carries its own flag)
    for (auto& p : ps) {
        // 32-bit buffer offsets: every operand the GEMM reads must stay below 2 GiB
        const double ext = 4.0 * ((double)p.M * p.lda + (double)p.K * p.ldb + p.N);
        if (ext >= 2147483648.0) { fprintf(stderr, "sacx: operand too large in %s\n", name.c_str()); abort(); }
    }
    for (auto& p : ps) {
        if (mode_of(p) != mode) { fprintf(stderr, "sacx: mixed GEMM modes in %s\n", name.c_str()); abort(); }
        const bool akc = p.a_kc != 0, bkc = p.b_kc != 0;
        if (akc != (mode != GM_DW) || bkc != (mode == GM_DX)) { fprintf(stderr, "sacx: bad operand layout in %s\n", name.c_str()); abort(); }
        if (mode == GM_DW && p.bscale == nullptr) p.bscale = h->f("ws.ones");
        // float4 loads along k: a K that is not a multiple of 4 (S+A = 23, 393; S = 17) still
        // qualifies when the row stride holds round4(K) (the zero pad columns of the staging
        // slabs): the over-read elements meet B values that load_b zeroes past K
        const int64_t k4 = r4(p.K);
        const bool v_a = (p.lda % 4 == 0) && (k4 <= p.lda) && ((((uintptr_t)p.A) & 15) == 0) &&
                         ((((uintptr_t)p.wgen) & 15) == 0);
        // dX: B = W_ext rows (n < N = K_in, so a row's float4 over-read past K stays inside W_ext: the
        // bias row follows the last); rows at any 4-B offset with h->unaligned_b (dword-aligned 16-B
        // buffer loads), whose elements past K meet A's zero pad (A rows are 16-B aligned)
        const bool b_al = (p.ldb % 4 == 0) && (k4 <= p.ldb) && ((((uintptr_t)p.B) & 15) == 0);
        const bool v_b = mode == GM_DX ? (b_al || (h->unaligned_b && (((uintptr_t)p.B) & 3) == 0)) : true;
        p.vec = (mode != GM_DW && v_a && v_b && p.K >= 4) ? 1 : 0;
        vec = vec || p.vec;
    }
    if (h->wbf_attach && h->cfg.gemm_bf16)
        for (auto& p : ps) wbf_wire(h, p, mode, t32);
    if (dwl) {
        // 16-B row pieces need 16-B aligned rows in every seed's arena block
        const bool sa = h->seeds <= 1 || h->seed_bytes % 16 == 0;
        for (auto& p : ps) {
            const bool a4 = sa && p.lda >= 4 && p.lda % 4 == 0 && (((uintptr_t)p.A) & 15) == 0;
            const bool b4 = sa && p.ldb >= 4 && p.ldb % 4 == 0 && (((uintptr_t)p.B) & 15) == 0;
            p.vec = (a4 ? 1 : 0) | (b4 ? 2 : 0);
        }
    }
    // forward launches with world-model head rows (mse epilogues) take their own variant,
    // so the others do not hold the mse operands in registers
    for (auto& p : ps)
        if (mode == GM_FWD && p.mse) L.gemm.rowk = GR_MSE_HEAD;
    L.gemm.dwl = dwl ? (h->dwl_nh == 1 ? 2 : 1) : 0;    // 2: 32x16 tiles, 1: 32x32
    L.gemm.mode = mode;
    L.gemm.vec = vec ? 1 : 0;
    for (size_t i = 0; i < ps.size(); ++i) L.gemm.probs[i] = ps[i];
    L.gemm.nprob = (int)ps.size();
    L.gemm.total_tiles = tiles;
    L.gemm.xcd_map = h->xcd_map;
    L.gemm.bf16 = h->cfg.gemm_bf16 != 0;
    L.gemm.p_stride = h->p_stride;
    L.gemm.ctl = h->ctl();
    L.gemm.adam = adam_consts(h);
    L.grid = tiles;
    plan.push_back(L);
}

// Gives the GEMM launch `L` of a plan its variant.  A mode or tile shape that has no kernel for it is a
// bug of the builder (seeds are packed later, by pack_seeds: launch_gemm checks the whole combination)
void set_rows(Launch& L, GemmRows rows) {
    if (L.kind != Launch::GEMM || !gemm_variant_ok(L.gemm.mode, rows, L.gemm.t32 != 0, false, L.gemm.dwl)) {
        fprintf(stderr, "sacx: no GEMM kernel for %s with rows %d (mode %d, t32 %d, dwl %d)\n", L.name.c_str(), (int)rows,
                L.gemm.mode, L.gemm.t32, L.gemm.dwl);
        abort();
    }
    L.gemm.rowk = rows;
}

// Replaces the plan's last two launches -- the layers 0 and 1 of the same nets, as add_gemm built
// them -- by one k_fwd2 launch (GM_FWD2) when the pair qualifies: fp32, one seed, 16x16 tiles, plain
// forward problems (layer 1 optionally with the actor head's partial dots, GR_HEAD_PART), at most 4 nets,
// K0 <= 32, H0 a multiple of 64 up to 256, layer 1 reading exactly layer 0's output.  wide0: a plain
// layer 0 is the world-model fit's, on pre-gathered rows (GR_PREGATHERED: up to 512 wide).  Returns
// whether it fused.
bool fuse_fwd2(sacx_handle* h, std::vector<Launch>& plan, const std::string& name, bool wide0 = false) {
    if (plan.size() < 2 || h->wide) return false;     // (k_fwd2 holds layer 0's rows in LDS: <= 512 wide)
    Launch& L0 = plan[plan.size() - 2];
    Launch& L1 = plan[plan.size() - 1];
    const GemmArgs &a0 = L0.gemm, &a1 = L1.gemm;
    if (L0.kind != Launch::GEMM || L1.kind != Launch::GEMM || a0.mode != GM_FWD || a1.mode != GM_FWD) return false;
    if (a0.t32 || a1.t32 || a0.dwl || a1.dwl || a0.bf16 || a0.nseeds > 1 || (h->seeds > 1 && h->learners == 0)) return false;
    // layer 0 may carry the actor head (target tile prologues from the head's partial dots,
    // which keep the prologue free of barriers, and head rows as extra workgroups)
    const bool head = a0.rowk == GR_ACTOR_HEAD;
    // or layer 0 gathers its rows from the replay ring (the world-model fit's model.fwd0), or
    // reads them pre-gathered: the fit's layer 0, up to 512 wide
    const bool gather = a0.rowk == GR_GATHER || (wide0 && a0.rowk == GR_NONE);
    if ((a0.rowk != GR_NONE && !head && !gather) || (a1.rowk != GR_NONE && a1.rowk != GR_HEAD_PART) ||
        ((head || gather) && a1.rowk != GR_NONE) ||
        a0.has_final || a1.has_final || a0.nprob != a1.nprob || a0.nprob > 4)
        return false;
    if (head && (a0.head.part == nullptr || a0.head.H1 > 256 || a0.head.A > 16)) return false;
    bool vec = true;
    for (int i = 0; i < a0.nprob; ++i) {
        const GemmProb &p0 = a0.probs[i], &p1 = a1.probs[i];
        if (p0.mse || p1.mse || (p0.headp && !head) || p1.headp || p0.K > 32 || p0.N % 64 != 0 ||
            p0.N > (gather ? 512 : 256) ||
            p1.K != p0.N || p1.A != p0.C || p1.lda != p0.ldc || p1.M != p0.M || p1.N % 16 != 0)
            return false;
        vec = vec && p0.vec;
    }
    Launch F = L1;
    F.name = name;
    GemmArgs& g = F.gemm;
    const int n = a0.nprob;
    int tiles = 0;
    for (int i = 0; i < n; ++i) {
        g.probs[i] = a0.probs[i];
        GemmProb q = a1.probs[i];
        q.tiles_n = (q.N + 63) / 64;
        q.tile_begin = tiles;
        tiles += ((q.M + 15) / 16) * q.tiles_n;
        g.probs[n + i] = q;
    }
    g.nprob = 2 * n;
    g.mode = GM_FWD2;
    g.vec = vec ? 1 : 0;
    g.total_tiles = tiles;
    g.rowk = head ? GR_PAIR_HEAD : a0.rowk == GR_GATHER ? GR_GATHER : gather ? GR_PREGATHERED : a1.rowk;
    if (!gemm_variant_ok(GM_FWD2, g.rowk, false, false, 0)) {
        fprintf(stderr, "sacx: no k_fwd2 kernel for %s with rows %d\n", name.c_str(), g.rowk);
        abort();
    }
    if (a0.rowk == GR_GATHER) g.mg = a0.mg;
    if (head) {
        g.head = a0.head;
        g.hfin = a0.hfin;
        g.head_block0 = a0.head_block0;
    }
    if (head && a0.row_blocks != 0) return false;   // plain SAC: the head rows come with merged_body only
    g.row_blocks = 0;
    F.grid = tiles;
    F.frees_slot = L0.frees_slot || L1.frees_slot;
    F.block = head ? SACX_FWD2_HEAD_NW * 64 : 1024;     // k_fwd2 waves (16; the fit's gather variant too)
    F.flops = L0.flops + L1.flops;
    F.bytes = L0.bytes + L1.bytes;
    plan.pop_back();
    plan.pop_back();
    plan.push_back(F);
    return true;
}

// Appends the problems of GEMM launch `b` to launch `a` (same mode; tile ranges follow a's).
bool merge_gemm(GemmArgs& a, const GemmArgs& b) {
    if (a.mode == GM_FWD2 || b.mode == GM_FWD2) {
        // two k_fwd2 launches: layer-0 problems, then layer-1 problems, each launch's in order
        const int na = a.nprob / 2, nb = b.nprob / 2;
        if (a.mode != b.mode || na + nb > 4 || a.vec != b.vec) return false;
        GemmProb l0[4], l1[4];
        for (int i = 0; i < na; ++i) { l0[i] = a.probs[i]; l1[i] = a.probs[na + i]; }
        for (int i = 0; i < nb; ++i) {
            l0[na + i] = b.probs[i];
            l1[na + i] = b.probs[nb + i];
            l1[na + i].tile_begin += a.total_tiles;
        }
        for (int i = 0; i < na + nb; ++i) { a.probs[i] = l0[i]; a.probs[na + nb + i] = l1[i]; }
        a.nprob = 2 * (na + nb);
        a.total_tiles += b.total_tiles;
        if (b.rowk == GR_HEAD_PART) a.rowk = GR_HEAD_PART;   // head partials: per problem (ppart null or not)
        return true;
    }
    if (a.mode != b.mode || a.t32 != b.t32 || a.dwl != b.dwl || a.nprob + b.nprob > GEMM_MAXP) return false;
    for (int i = 0; i < b.nprob; ++i) {
        GemmProb p = b.probs[i];
        p.tile_begin += a.total_tiles;
        a.probs[a.nprob + i] = p;
    }
    a.nprob += b.nprob;
    a.total_tiles += b.total_tiles;
    a.vec = a.vec || b.vec;
    if (b.rowk == GR_MSE_HEAD) {   // world-model head rows: the forward variant with mse operands
        if (a.rowk != GR_NONE && a.rowk != GR_MSE_HEAD) return false;
        a.rowk = GR_MSE_HEAD;
    }
    return true;
}

// Packed seeds: every launch of an update plan runs all seeds (grid z), relocating its
// seed-0 arena pointers by blockIdx.z * seed_bytes.
void pack_seeds(Launch& L, int64_t stride, int n) {
    L.rng.sstride = L.gather.sstride = L.gemm.sstride = L.head.sstride = L.fin.sstride = L.qh.sstride =
        L.ab.sstride = stride;
    L.rng.nseeds = L.gather.nseeds = L.gemm.nseeds = L.head.nseeds = L.fin.nseeds = L.qh.nseeds = L.ab.nseeds = n;
    L.ln.sstride = stride;
    L.ln.nseeds = n;
    // the on-policy steps (sacx_ppo_steps_packed / sacx_vcritic_steps_packed)
    L.pg.sstride = L.ph.sstride = L.pf.sstride = L.gn.sstride = L.ap.sstride = stride;
    L.pg.nseeds = L.ph.nseeds = L.pf.nseeds = L.gn.nseeds = L.ap.nseeds = n;
    L.vg.sstride = L.vh.sstride = L.vf.sstride = L.va.sstride = stride;
    L.vg.nseeds = L.vh.nseeds = L.vf.nseeds = L.va.nseeds = n;
}

// Data-parallel mode: the dW launch `L` stores its local gradients (+3 p_stride) instead of
// running Adam; RCCL sums the contiguous gradient range [first, last] over the ranks and
// k_adam_apply runs the Adam (and Polyak into the same range at `targ`) with scale 1/ranks.
void dp_split_adam(sacx_handle* h, std::vector<Launch>& plan, const std::string& first, const std::string& last,
                   const std::string& targ, int group, int nlaunch = 1) {
    std::string base;
    for (int j = 0; j < nlaunch; ++j) {        // the last nlaunch dW launches (add_gemm_split's)
        Launch& G = plan[plan.size() - 1 - j];
        for (int i = 0; i < G.gemm.nprob; ++i) G.gemm.probs[i].epi = EPI_STORE;
        base = G.name.substr(0, G.name.find(".adam"));
        G.name = base + ".grad" + G.name.substr(G.name.find(".adam") + 5);
    }
    const AdamConsts gadam = adam_consts(h);
    const uint64_t o0 = h->off_of(first);
    const SegInfo& sl = h->seg(last);
    const int64_t n = (int64_t)((sl.off + (uint64_t)(sl.rows * sl.cols) * 4 - o0) / 4);
    float* P = h->f(first);
    Launch R{};
    R.kind = Launch::ALLREDUCE;
    R.name = base + ".allreduce";
    R.ar_buf = P + 3 * h->p_stride;
    R.ar_count = n;
    R.grid = 0;
    R.bytes = 8.0 * n;
    plan.push_back(R);
    Launch U{};
    U.kind = Launch::APPLY;
    U.name = base + ".adam";
    AdamApplyArgs& a = U.ap;
    a.P = P; a.n = n; a.p_stride = h->p_stride; a.group = group;
    a.t_off = targ.empty() ? 0 : (int64_t)(h->off_of(targ) - o0) / 4;
    a.grad_scale = (float)(1.0 / (double)h->dp_ranks);
    a.ctl = h->ctl();
    a.adam = gadam;
    U.grid = (int)((n + 255) / 256);
    U.bytes = 4.0 * n * (targ.empty() ? 7 : 9);
    plan.push_back(U);
}

// The update's inputs in slot `slot`: the sampler (randint + every normal of the update,
// buffers.py:136, continuous_actors.py:351) and the gather of the replay / expert rows into the
// normalised staging slabs (buffers.py:137-141, normalizer.py:36-41).  Every plan starts with them.
// BC (SACX_EXPERT_BC, BC.py:309-336): no replay batch, so the sampler draws no integers and only the
// expert normals (ne * A: len(sec0) * A then len(sec1) * A, one contiguous stretch of the stream), and
// the gather takes the expert rows alone (B = 0: they are rows [0, ne) of Xa / Xm)
void plan_inputs(sacx_handle* h, std::vector<Launch>& plan, int slot) {
    const int S = h->S, A = h->A, B = h->bc ? 0 : h->B, ne = h->ne;
    const int n_norm = h->bc ? ne * A : h->n_norm;
    const int ldS = h->ldS, ldQ = h->ldQ;
    const std::string sl = "slot" + std::to_string(slot);
    auto W = [&](const std::string& n) { return h->f(n); };
    int32_t* idx = h->ptr<int32_t>(sl + ".idx");
    float* noise = h->f(sl + ".noise");
    float *Xa = W(sl + ".Xa"), *Xq = W(sl + ".Xq"), *Xt = W(sl + ".Xt"), *Xp = W(sl + ".Xp"), *Xm = W(sl + ".Xm");
    float *r_in = W(sl + ".r"), *d_in = W(sl + ".d"), *se_raw = W(sl + ".se_raw"), *spe_raw = W(sl + ".spe_raw");
    // ---- sampler
    {
        Launch L{};
        L.kind = Launch::RNG;
        L.name = "rng";
        L.rng.st = h->ptr<RngState>("rng");
        L.rng.ctl = h->ctl();
        L.rng.n_int = B;
        L.rng.n_norm = n_norm;
        L.rng.out_idx = idx;
        L.rng.out_norm = noise;
        L.rng.slot = slot;
        L.rng.reset_seq = 1;   // cleared for the chained launches of a captured graph
        L.rng.nupd = 1;
        L.rng.slot_bytes = h->slot_bytes;
        if (h->rng_split) {
            L.rng.pairs = h->ptr<uint32_t>("rng.pairs");
            L.rng.pairs_oi = h->ptr<int32_t>("rng.pairs_oi");
            L.rng.pcap = h->pcap;
        }
        if (h->rng_jump) {
            L.rng.jw = h->ptr<uint32_t>("rng.jw");
            L.rng.jc = h->ptr<uint32_t>("rng.jc");
            L.rng.jL = h->jL;
            L.rng.jsmax = h->jsmax;
            L.rng.junder = h->mtj_under;
        }
        L.grid = 1;
        L.block = 1024;
        L.bytes = 4.0 * (B + n_norm) + 2.0 * sizeof(RngState);
        plan.push_back(L);
    }
    // ---- gather
    {
        Launch L{};
        L.kind = Launch::GATHER;
        L.name = "gather";
        GatherArgs& g = L.gather;
        g.replay = W("replay"); g.cap = h->cap; g.stride = h->stride;
        g.S = S; g.A = A; g.B = B; g.ne = ne; g.idx = idx; g.ctl = h->ctl();
        g.s_mean = W("norm.s_mean"); g.s_den = W("norm.s_den");
        g.a_mean = W("norm.a_mean"); g.a_den = W("norm.a_den");
        g.ms_mean = W(mnorm(h, "s_mean")); g.ms_den = W(mnorm(h, "s_den"));
        g.Xa = Xa; g.ldS = ldS; g.Xq = Xq; g.Xt = Xt; g.Xp = Xp; g.Xm = Xm; g.ldQ = ldQ;
        g.r = r_in; g.d = d_in; g.slot = slot; g.nupd = 1; g.slot_bytes = h->slot_bytes;
        g.exp_s = W("expert.s"); g.exp_sp = W("expert.sp");
        g.perm_ring = h->nm == 1 ? nullptr : h->ptr<int32_t>("perm"); g.perm_cap = h->perm_cap;
        g.perm_ld = h->ne_perm;
        g.se_raw = se_raw; g.spe_raw = spe_raw;
        L.grid = (B + ne + 3) / 4;
        L.bytes = 4.0 * (B * (2.0 * S + A + 2) + ne * 2.0 * S) + 4.0 * (B * (2.0 * ldS + 3.0 * ldQ + 2));
        plan.push_back(L);
    }
}

// alpha.final (k_alpha_final: the alpha loss / Adam / clamp, SAC_expert.py:340-356, and the update's
// statistics row) behind the alpha.head launch that ends `plan`; in the data-parallel mode the local
// alpha gradient, its all-reduce and k_alpha_apply
void plan_alpha_final(sacx_handle* h, std::vector<Launch>& plan, int nm) {
    const int B = h->B, ne = h->ne, S = h->S;
    const bool eo = h->cfg.use_expert != 0;
    auto W = [&](const std::string& n) { return h->f(n); };
    {
        const Launch& AH = plan.back();
        Launch L{};
        L.kind = Launch::FINAL;
        L.name = "alpha.final";
        FinalArgs& f = L.fin;
        f.nred = AH.grid;
        f.alpha = W("alpha"); f.alpha_m = f.alpha + h->p_stride; f.alpha_v = f.alpha + 2 * h->p_stride;
        f.ctl = h->ctl();
        f.adam = adam_consts(h);
        f.target_entropy = h->cfg.target_entropy;
        f.B = B; f.ne = ne; f.use_expert = eo; f.nm = nm;
        f.lq = W("ws.lq"); f.lp = W("ws.lp"); f.mse_rows = W("ws.mse"); f.red = W("red");
        f.mse_tiles = (S + 15) / 16;
        f.stats = W("stats"); f.stats_cap = h->stats_cap;
        L.grid = 1;
        L.block = 64;
        L.bytes = 4.0 * (f.nred + 3.0 * B + ne);
        if (h->dp_ranks > 0) {              // alpha gradient: local -> all-reduce -> Adam + counters
            f.alpha_g = W("alpha") + 3 * h->p_stride;
            f.grad_scale = (float)(1.0 / (double)h->dp_ranks);
            L.name = "alpha.grad";
            plan.push_back(L);
            Launch R{};
            R.kind = Launch::ALLREDUCE;
            R.name = "alpha.allreduce";
            R.ar_buf = f.alpha_g;
            R.ar_count = 1;
            plan.push_back(R);
            Launch U{};
            U.kind = Launch::AAPPLY;
            U.name = "alpha.adam";
            U.fin = f;
            U.grid = 1;
            U.block = 64;
            plan.push_back(U);
        } else {
            plan.push_back(L);
        }
    }
}

// Config C5: the bf16 32x32 dW + Adam problems whose X is the slot's critic rows (Xq) or a critic's
// layer-0 output (ws.Hq1, written by a bf16 32x32 forward problem earlier in the plan) read X^T
// from a transposed image instead (GemmProb::abf); its producer -- k_gather (xbfq) or that
// forward problem's epilogue (tbf) -- is told to write it.  Bit-identical: the image holds the
// bf16 values the converting loads make, in the order they pack them.
void xbf_wire(sacx_handle* h, std::vector<Launch>& plan, int slot) {
    if (!h->xbf || !h->wbf_attach) return;
    const int S = h->S, A = h->A, B = h->B, Hc0 = h->Hc0, ld = wbf_ld_of(B);
    const std::string sl = "slot" + std::to_string(slot);
    const float* Xq = h->f(sl + ".Xq");
    const float* Hq1 = h->f("ws.Hq1");
    Launch* gather = nullptr;
    for (Launch& L : plan)
        if (L.kind == Launch::GATHER) gather = &L;
    for (size_t i = 0; i < plan.size(); ++i) {
        Launch& L = plan[i];
        if (L.kind != Launch::GEMM || L.gemm.mode != GM_DW || !L.gemm.t32 || L.gemm.dwl || !L.gemm.bf16) continue;
        for (int j = 0; j < L.gemm.nprob; ++j) {
            GemmProb& p = L.gemm.probs[j];
            if (p.K != B || p.a_kc != 0) continue;
            if (p.A == Xq && p.ones_row == S + A && gather != nullptr) {
                p.abf = h->ptr<uint16_t>(sl + ".xbfq");
                gather->gather.xbfq = h->ptr<uint16_t>(sl + ".xbfq");
                continue;
            }
            const int64_t d = p.A - Hq1;
            if (h->xbf != 1 || d < 0 || d % ((int64_t)B * Hc0) != 0 || d / ((int64_t)B * Hc0) >= 4 || p.lda != Hc0 || p.ones_row != Hc0)
                continue;
            uint16_t* img = h->ptr<uint16_t>("xbf.ws.Hq1") + (size_t)(d / ((int64_t)B * Hc0)) * Hc0 * ld;
            for (size_t q = 0; q < i && p.abf == nullptr; ++q) {
                Launch& F = plan[q];
                if (F.kind != Launch::GEMM || F.gemm.mode != GM_FWD || !F.gemm.t32 || !F.gemm.bf16 || F.gemm.rowk != GR_NONE) continue;
                for (int c = 0; c < F.gemm.nprob; ++c) {
                    GemmProb& f = F.gemm.probs[c];
                    if (f.C == p.A && f.M == B && f.N == Hc0 && f.ldc == Hc0 && f.mse == 0 && f.ppart == nullptr) {
                        f.tbf = img;
                        p.abf = img;
                    }
                }
            }
        }
    }
}

// Appends one GEMM launch per GEMM_MAXP problems (a launch's problems travel by value): `name`,
// then name.1, name.2, ...  Returns the launches added.
int add_gemm_split(sacx_handle* h, std::vector<Launch>& plan, const std::string& name, const std::vector<GemmProb>& ps,
                   GemmTiles tl = {}) {
    int n = 0;
    for (size_t i = 0; i < ps.size(); i += GEMM_MAXP, ++n) {
        std::vector<GemmProb> part(ps.begin() + i, ps.begin() + std::min(ps.size(), i + GEMM_MAXP));
        add_gemm(h, plan, n == 0 ? name : name + "." + std::to_string(n), part, tl);
    }
    return n;
}

// The plan's last n launches (a dW family) store their gradients at +3 p_stride instead of applying them: a
// clip or a sum over chunks comes first
void store_grads(std::vector<Launch>& plan, int n) {
    for (int j = 0; j < n; ++j) {
        Launch& G = plan[plan.size() - 1 - j];
        for (int i = 0; i < G.gemm.nprob; ++i) G.gemm.probs[i].epi = EPI_STORE;
    }
}

// Keras Adam over the n parameters from P on their stored gradients times the device scalar `scale_dev`
Launch adam_apply_launch(sacx_handle* h, const std::string& name, float* P, int64_t n, int group, const float* scale_dev,
                         int t_adv) {
    Launch U{};
    U.kind = Launch::APPLY;
    U.name = name;
    AdamApplyArgs& a = U.ap;
    a.P = P; a.n = n; a.p_stride = h->p_stride; a.group = group; a.t_off = 0;
    a.grad_scale = 1.f; a.scale_dev = scale_dev;
    a.ctl = h->ctl(); a.adam = adam_consts(h); a.t_adv = t_adv;
    U.grid = (int)((n + 255) / 256);
    U.bytes = 4.0 * n * 7;
    return U;
}

// ---------------------------------------------------------------- shared plan builders
// What the update plans (fused and generic SAC / SAC-EO, BC, the PPO step, a TRPO chunk) have in common: the
// actor's forward, dX and dW chains over a caller's buffers, the critics' and the world models' problems by
// net and layer, and the arguments of the head row kernels (k_actor_head, k_qhead, k_actor_bwd and the
// head backward folded into actor.bwd1).  What is specific to a caller (EPI_STORE, bscale, wgen, headp,
// t_adv, the data-parallel split, folds, a launch's flops / bytes once rows ride on it) it applies to what
// these return.

// hidden-layer buffer i of a chain of D layers: <p>1 (layer 0), <p>2 (the last), <p>m<i>
std::string chain_name(const std::string& p, int i, int D) {
    return p + (i == 0 ? "1" : i == D - 1 ? "2" : "m" + std::to_string(i));
}
float* chain_buf(sacx_handle* h, const std::string& p, int i, int D) { return h->f(chain_name(p, i, D)); }

std::string layer_name(const std::string& net, int i) { return net + ".l" + std::to_string(i); }

// One pass through one MLP on one slab of M rows.  Layer i of `net` is the segment <net>.l<i>, nd its widths and
// activations.  Layer 0 reads K0 columns of X; hidden layer i writes H[i] and takes its delta in D[i] (empty: a
// forward-only pass), both already at the slab's first row; the head (layer nd->D()) writes N columns of `out`
// and takes its delta from `dout`.  What a caller's launch adds to a problem (loss epilogues, bscale, generated
// operands, partials) it applies to what the three builders return.
struct NetPass {
    std::string net;
    const NetDims* nd; int group;            // GRP_*: whose Adam constants the dW problems take
    const float* X; int ldx, K0;
    int M;
    std::vector<float*> H, D;
    int N; float* out; int ldo;              // the head: width, forward output and its row stride
    const float* dout; int lddo;             //           its delta and that row stride
};

// layer i's input: X, or the hidden layer below
struct NetIn { const float* p; int ld, K; };
NetIn net_in(const NetPass& c, int i) {
    if (i == 0) return {c.X, c.ldx, c.K0};
    return {c.H[i - 1], c.nd->h[i - 1], c.nd->h[i - 1]};
}

// forward, layers 0 .. D (D: the head, no activation)
GemmProb net_fwd_prob(sacx_handle* h, const NetPass& c, int i) {
    const NetIn in = net_in(c, i);
    if (i < c.nd->D()) return prob_fwd(in.p, in.ld, c.M, in.K, h->f(layer_name(c.net, i)), c.nd->h[i], c.H[i], c.nd->act[i]);
    GemmProb p = prob_fwd(in.p, in.ld, c.M, in.K, h->f(layer_name(c.net, i)), c.N, c.out, ACT_NONE);
    p.ldc = c.ldo;
    return p;
}

// dX, layers D .. 1: the delta at layer i's output to layer i - 1's
GemmProb net_dx_prob(sacx_handle* h, const NetPass& c, int i) {
    const bool head = i == c.nd->D();
    GemmProb p = prob_dx(head ? c.dout : c.D[i], c.M, head ? c.N : c.nd->h[i], h->f(layer_name(c.net, i)), c.nd->h[i - 1],
                         c.H[i - 1], c.D[i - 1], c.nd->act[i - 1]);
    if (head) p.lda = c.lddo;
    return p;
}

// dW + Adam (+ Polyak into T), layers 0 .. D
GemmProb net_dw_prob(sacx_handle* h, const NetPass& c, int i, float* T = nullptr) {
    const bool head = i == c.nd->D();
    const NetIn in = net_in(c, i);
    GemmProb p = prob_dw(in.p, in.ld, in.K, c.M, head ? c.dout : c.D[i], head ? c.N : c.nd->h[i], h->f(layer_name(c.net, i)), T,
                         c.group);
    if (head) p.ldb = c.lddo;
    return p;
}

// A pass of net `net` (widths h->nd[ndi]) over the chains Hn from row hrow0 and Dn from row drow0 (chain_buf;
// Dn empty: forward only; a layer the layout holds no delta buffer for stays null).  The head is the caller's
NetPass chain_pass(sacx_handle* h, const std::string& net, int ndi, int group, const float* X, int ldx, int K0, int M,
                   const std::string& Hn, size_t hrow0, const std::string& Dn = "", size_t drow0 = 0) {
    NetPass c{};
    c.net = net; c.nd = &h->nd[ndi]; c.group = group; c.X = X; c.ldx = ldx; c.K0 = K0; c.M = M;
    const int D = c.nd->D();
    auto have = [&](int i) { return h->seg_index.count(chain_name(Dn, i, D)) != 0; };
    for (int i = 0; i < D; ++i) {
        c.H.push_back(chain_buf(h, Hn, i, D) + hrow0 * c.nd->h[i]);
        if (!Dn.empty()) c.D.push_back(have(i) ? chain_buf(h, Dn, i, D) + drow0 * c.nd->h[i] : nullptr);
    }
    return c;
}

// --actor_layer_norm puts Dense -> LayerNorm -> tanh on layer 0 (nn_utils.py:110-119).  Forward: k_ln on
// rows [r0, r1) of the pre-norm output Z, caching xhat / rstd for the rows below cache_rows
Launch ln_fwd_launch(sacx_handle* h, const std::string& name, float* Z, int r0, int r1, float* xhat, float* rstd,
                     int cache_rows) {
    const int M = r1 - r0, H0 = h->H0;
    Launch L{};
    L.kind = Launch::LNORM;
    L.name = name;
    LNArgs& a = L.ln;
    a.mode = 0; a.H = H0; a.Z = Z; a.nrange = 1; a.r[0] = r0; a.r[1] = r1;
    a.gamma = h->f("actor.ln"); a.xhat = xhat; a.rstd = rstd; a.cache_rows = cache_rows;
    L.grid = (M + 3) / 4;
    L.flops = 8.0 * M * H0;
    L.bytes = 4.0 * M * H0 * 3;
    return L;
}

// Backward: dY -> dZ through the norm on rows [0, M) of dY (cache rows from xrow0); dY*xhat, dY for gamma / beta
Launch ln_bwd_launch(sacx_handle* h, float* dY, int M, float* xhat, float* rstd, int xrow0, float* gy, float* gb) {
    const int H0 = h->H0;
    Launch N{};
    N.kind = Launch::LNORM;
    N.name = "actor.ln.bwd";
    LNArgs& a = N.ln;
    a.mode = 1; a.H = H0; a.Z = dY; a.r[1] = M; a.gamma = h->f("actor.ln");
    a.xhat = xhat; a.rstd = rstd; a.xrow0 = xrow0;
    a.gy = gy; a.gb = gb;
    N.grid = (M + 3) / 4;
    N.flops = 8.0 * M * H0;
    N.bytes = 4.0 * M * H0 * 5;
    return N;
}

// Where one pass through the actor lives.  The forward reads M rows of X and writes rows
// [hrow0, hrow0 + M) of the hidden buffers H[i]; the dX and dW problems read those rows beside rows
// [0, M) of the delta buffers D[i], of D3 (the delta at the output layer) and of E (the logstd rows).
struct ActorPass {
    const float* X; int ldx;                // the input rows and their leading dimension
    int M;                                  // rows
    int hrow0;                              // first row of the pass in H[i] (and in the layer-norm cache: xrow0)
    std::vector<float*> H, D;               // per hidden layer: output, delta
    float* O = nullptr;                     // the output layer as a plain GEMM (the PPO step, a TRPO chunk), else null
    float *D3, *E;
    float *xhat, *rstd; int cache_rows;     // layer norm: the forward's cache
    float *gy, *gb;                         //             the backward's rows for the gamma / beta sums
};

// the update plans' workspace: ws.Ha / ws.Da, ws.Da3, ws.E, ws.ln_*
ActorPass actor_pass_ws(sacx_handle* h, const float* X, int M, int hrow0, int cache_rows) {
    const int Da = h->nd[0].D();
    ActorPass c{};
    c.X = X; c.ldx = h->ldS; c.M = M; c.hrow0 = hrow0; c.cache_rows = cache_rows;
    for (int i = 0; i < Da; ++i) {
        c.H.push_back(chain_buf(h, "ws.Ha", i, Da));
        c.D.push_back(chain_buf(h, "ws.Da", i, Da));
    }
    c.D3 = h->f("ws.Da3"); c.E = h->f("ws.E");
    if (h->ln) {
        c.xhat = h->f("ws.ln_xhat"); c.rstd = h->f("ws.ln_rstd"); c.gy = h->f("ws.ln_gy"); c.gb = h->f("ws.ln_gb");
    }
    return c;
}

// the pass as a NetPass: the hidden rows from hrow0, the head on O / D3
NetPass actor_net_pass(sacx_handle* h, const ActorPass& c) {
    NetPass p{};
    p.net = "actor"; p.nd = &h->nd[0]; p.group = GRP_PI; p.X = c.X; p.ldx = c.ldx; p.K0 = h->S; p.M = c.M;
    for (int i = 0; i < p.nd->D(); ++i) p.H.push_back(c.H[i] + (size_t)c.hrow0 * p.nd->h[i]);
    p.D = c.D;
    p.N = p.ldo = p.lddo = h->Aout; p.out = c.O; p.dout = c.D3;
    return p;
}

// <name><i> for every hidden layer, k_ln (`ln_name`) behind layer 0's (layer 0 without its activation then),
// and for the output layer where the pass has an O
void actor_fwd_chain(sacx_handle* h, std::vector<Launch>& plan, const ActorPass& c, const std::string& name,
                     const std::string& ln_name, GemmTiles tl = {}) {
    const NetPass p = actor_net_pass(h, c);
    for (int i = 0; i < p.nd->D() + (c.O ? 1 : 0); ++i) {
        GemmProb q = net_fwd_prob(h, p, i);
        if (i == 0 && h->ln) q.act = ACT_NONE;
        add_gemm(h, plan, name + std::to_string(i), {q}, tl);
        if (i == 0 && h->ln)
            plan.push_back(ln_fwd_launch(h, ln_name, c.H[0], c.hrow0, c.hrow0 + c.M, c.xhat, c.rstd, c.cache_rows));
    }
}

// actor.bwd<i> from layer `from` down to 1: the delta at layer i's output (D3 at the output layer) to
// layer i - 1's, with tanh' at the norm's output under layer norm; then actor.ln.bwd
void actor_bwd_chain(sacx_handle* h, std::vector<Launch>& plan, const ActorPass& c, int from, GemmTiles tl = {}) {
    const NetPass p = actor_net_pass(h, c);
    for (int i = from; i >= 1; --i) {
        GemmProb q = net_dx_prob(h, p, i);
        if (i == 1 && h->ln) q.act = ACT_TANH;
        add_gemm(h, plan, "actor.bwd" + std::to_string(i), {q}, tl);
    }
    if (h->ln) plan.push_back(ln_bwd_launch(h, c.D[0], c.M, c.xhat, c.rstd, c.hrow0, c.gy, c.gb));
}

// the actor's dW problems in parameter order: layers 0 .. Da-1, the output layer, logstd unless
// per_state_std, gamma and beta under layer norm
std::vector<GemmProb> actor_dw_probs(sacx_handle* h, const ActorPass& c) {
    const NetPass np = actor_net_pass(h, c);
    const int H0 = h->H0;
    std::vector<GemmProb> pw;
    for (int i = 0; i <= np.nd->D(); ++i) pw.push_back(net_dw_prob(h, np, i));
    if (!h->cfg.per_state_std && !h->softmax) {
        GemmProb p = prob_dw(c.E, 1, 0, c.M, c.E, h->A, h->f("actor.logstd"), nullptr, GRP_PI);
        p.ones_row = 0;   // single all-ones row: column sums of E
        pw.push_back(p);
    }
    if (h->ln) {          // gamma, beta: column sums of dY*xhat and dY
        for (int k = 0; k < 2; ++k) {
            float* gsrc = k ? c.gb : c.gy;
            GemmProb p = prob_dw(gsrc, 1, 0, c.M, gsrc, H0, h->f("actor.ln") + (size_t)k * H0, nullptr, GRP_PI);
            p.ones_row = 0;
            pw.push_back(p);
        }
    }
    return pw;
}

// The actor's trainables are one contiguous parameter range, actor.l0 .. actor.logstd (with per_state_std
// the logstd variable is no trainable: its gradient stays 0 and Adam leaves it): its base (null before
// sacx_bind) and float count.  A softmax handle's range ends where actor.logstd begins (the net only).
struct ParamRange { float* P; int64_t n; };
ParamRange actor_range(const sacx_handle* h) {
    const SegInfo& sl = h->seg("actor.logstd");
    const uint64_t end = h->softmax ? sl.off : sl.off + (uint64_t)(sl.rows * sl.cols) * 4;
    return {h->arena ? h->f("actor.l0") : nullptr, (int64_t)((end - h->off_of("actor.l0")) / 4)};
}

// GaussianActor.logstd_init (continuous_actors.py:39-44), f32: log(std_mult), - log(log 2) with per_state_std
float logstd_init(const sacx_handle* h) {
    const double sm = h->cfg.actor_std_mult > 0.f ? h->cfg.actor_std_mult : 1.0;
    return (float)(std::log(sm) - (h->cfg.per_state_std ? std::log(std::log(2.0)) : 0.0));
}

// the trainable GaussianActor's distribution over the output rows O [m, Aout]
PpoDist ppo_dist(sacx_handle* h, const float* O) {
    PpoDist d{};
    d.O = O; d.A = h->A; d.Aout = h->Aout; d.per_state_std = h->cfg.per_state_std;
    d.logstd = h->f("actor.logstd");
    d.logstd_init = logstd_init(h);
    d.softmax = h->softmax ? 1 : 0;
    return d;
}

// The expert term's world models (at most two) and their sections of the ne expert rows: model k takes
// rows [k * half, k * half + mrows) of Xm and of the ws.Hm / ws.Dm chain
struct ExpertSplit { int nm, mrows, half; };
ExpertSplit expert_split(const sacx_handle* h) {
    const int nm = std::min(h->nm, 2);
    return {nm, nm == 1 ? h->ne : h->ne / 2, h->ne / 2};
}

// model k's pass on its rows of Xm = [s_e | pi(s_e)] (null: no layer 0) and of the ws.Hm / ws.Dm chain; the
// delta at the head is its delta-s columns in ws.dout (the head's forward: model_head_probs)
NetPass expert_pass(sacx_handle* h, const float* Xm, int k) {
    const ExpertSplit e = expert_split(h);
    const size_t r0 = (size_t)k * e.half;
    NetPass c = chain_pass(h, "m" + std::to_string(k), 2, GRP_MODEL, Xm ? Xm + r0 * h->ldQ : nullptr, h->ldQ, h->S + h->A, e.mrows,
                           "ws.Hm", r0, "ws.Dm", r0);
    c.N = c.lddo = h->S; c.dout = h->f("ws.dout") + r0 * h->S;
    return c;
}

// model k's hidden layer i
GemmProb model_fwd_prob(sacx_handle* h, const float* Xm, int k, int i) { return net_fwd_prob(h, expert_pass(h, Xm, k), i); }

// the models' head on the expert rows + the MSE against sp_e (SAC_expert.py:319-332, BC.py:340-352), `mse`
// its epilogue's flags
std::vector<GemmProb> model_head_probs(sacx_handle* h, int mse, const float* se_raw, const float* spe_raw) {
    const ExpertSplit e = expert_split(h);
    const int S = h->S, Hm1 = h->Hm1, Dm = h->nd[2].D(), mtn = (S + 15) / 16;
    std::vector<GemmProb> pm;
    for (int k = 0; k < e.nm; ++k) {
        float* Wh = h->f(layer_name("m" + std::to_string(k), Dm));
        GemmProb p{};
        p.A = h->f("ws.Hm2") + (size_t)k * e.half * Hm1; p.lda = Hm1; p.a_kc = 1; p.ones_row = -1;
        p.B = Wh; p.ldb = h->Om; p.b_kc = 0;                 // W_ext [(Hm1+1) x Om], Om = S (+1)
        p.M = e.mrows; p.N = S; p.K = Hm1;                   // delta-s columns only
        p.bias = Wh + (size_t)Hm1 * h->Om;
        p.C = h->f("ws.dout") + (size_t)k * e.half * S; p.ldc = S;
        p.epi = EPI_FWD; p.act = ACT_NONE;
        p.mse = mse; p.grad_scale = 1.f / (float)e.mrows;    // the mean over the section's rows
        p.dclip = h->cfg.delta_clip_pred > 0.f ? h->cfg.delta_clip_pred : 0.f;
        p.se_raw = se_raw + (size_t)k * e.half * S; p.spe_raw = spe_raw + (size_t)k * e.half * S;
        p.dmean = h->f("mnorm.d_mean"); p.dden = h->f("mnorm.d_den");
        p.part = h->f("ws.mse") + (size_t)k * e.half * mtn;
        pm.push_back(p);
    }
    return pm;
}

// the models' dX problems at level i (Dm: from the head's delta-s columns) down to their layer-0 output,
// the expert rows' action gradient
std::vector<GemmProb> model_bwd_probs(sacx_handle* h, int i) {
    const int Dm = h->nd[2].D();
    std::vector<GemmProb> pb;
    for (int k = 0; k < expert_split(h).nm; ++k) {
        GemmProb p = net_dx_prob(h, expert_pass(h, nullptr, k), i);
        if (i == Dm) p.ldb = h->Om;          // the head's delta-s columns: B[n][k] = W_ext[n][k], stride Om
        pb.push_back(p);
    }
    return pb;
}

// The critics' problems by net and layer, as model_fwd_prob.  A chain (ws.Hq / ws.Dq: the target and critic
// rows, ws.Hp / ws.Dp: the policy rows) holds one slab of B rows per net: t0 t1 q0 q1 in ws.Hq, q0 q1 in the
// others.  Forward: `net`'s hidden layer i into slab `slab` of chain Hn, layer 0 reading X = [s | a]
NetPass critic_pass(sacx_handle* h, const std::string& net, const float* X, const std::string& Hn, int hslab,
                    const std::string& Dn = "", int dslab = 0) {
    return chain_pass(h, net, 1, GRP_Q, X, h->ldQ, h->S + h->A, h->B, Hn, (size_t)hslab * h->B, Dn, (size_t)dslab * h->B);
}
GemmProb critic_fwd_prob(sacx_handle* h, const std::string& net, const float* X, const std::string& Hn, int slab, int i) {
    return net_fwd_prob(h, critic_pass(h, net, X, Hn, slab), i);
}

// dX: the delta at `net`'s hidden layer i to layer i - 1, slab `dslab` of chain Dn, with act' at slab `hslab`
// of chain Hn.  gen: the A operand is slab `hslab` of Hn at layer i instead, for a caller that generates the
// delta from it on load (wgen, gen_act)
GemmProb critic_dx_prob(sacx_handle* h, const std::string& net, const std::string& Hn, int hslab, const std::string& Dn,
                        int dslab, int i, bool gen = false) {
    const NetPass c = critic_pass(h, net, nullptr, Hn, hslab, Dn, dslab);
    GemmProb p = net_dx_prob(h, c, i);
    if (gen) p.A = c.H[i];
    return p;
}

// dW + Keras Adam + Polyak into t<k> of q<k>'s layer i on the critic rows Xq (i = Dc: the output layer, from
// the loss gradient ws.gq)
GemmProb critic_dw_prob(sacx_handle* h, int k, const float* Xq, int i) {
    NetPass c = critic_pass(h, "q" + std::to_string(k), Xq, "ws.Hq", 2 + k, "ws.Dq", k);
    c.N = c.lddo = 1; c.dout = h->f("ws.gq") + (size_t)k * h->B;
    return net_dw_prob(h, c, i, h->f(layer_name("t" + std::to_string(k), i)));
}

// k_qhead's arguments on the last hidden rows H2, D2 the delta it writes there (nullable).  mode 0 (q.head):
// twin-Q target, TD target from the rewards r and terminals d, the critic losses; mode 1 (pi.q.head): min,
// tie split, the policy loss rows and the output gradients of q0 / q1
QHeadArgs q_head_args(sacx_handle* h, int mode, const float* H2, float* D2, const float* r, const float* d) {
    const NetDims& nc = h->nd[1];
    const int Dc = nc.D();
    const char* nets[4] = {"t0", "t1", "q0", "q1"};
    QHeadArgs q{};
    q.mode = mode; q.B = h->B; q.H1 = h->Hc1; q.H2 = H2;
    for (int k = 0; k < (mode ? 2 : 4); ++k) q.W3[k] = h->f(layer_name(nets[mode ? 2 + k : k], Dc));
    q.act = nc.act[Dc - 1]; q.D2 = D2; q.g = h->f(mode ? "ws.gp" : "ws.gq"); q.loss_rows = h->f(mode ? "ws.lp" : "ws.lq");
    q.alpha = h->f("alpha"); q.nlp = h->f(mode ? "ws.nlp_p" : "ws.nlp_t"); q.r = r; q.d = d;
    if (mode == 0) q.gamma = h->cfg.gamma;
    q.ret_den = h->f("norm.ret_den");
    q.w_sac = (mode && h->cfg.use_expert) ? (float)(1.0 - (double)h->cfg.epsilon) : 1.f;
    // (the SAC-EO world-model head on the expert rows runs as GEMM problems with the mse epilogue, not as rows here)
    q.ne = 0; q.ctl = h->ctl();
    return q;
}

// k_actor_head's arguments on the rows H2 of the actor's last hidden layer, `part` their head partials
// (GR_HEAD_PART) or null; the caller adds the segments, the row counts, the cache rows and alpha_mode.
// update: an update's actor.head -- its sample segments write the world models' inputs (their normaliser for
// the action columns) and its cached rows feed the backward (ws.c_*).  alpha.head and the inference paths
// have neither.
HeadArgs head_args(sacx_handle* h, const float* H2, const float* part, bool update) {
    HeadArgs a{};
    a.H2 = H2; a.ldh = h->H1; a.W3 = h->f(actor_head_name(h)); a.logstd = h->f("actor.logstd");
    a.part = part; a.tq = (h->H1 + 15) / 16;
    a.H1 = h->H1; a.A = h->A; a.Aout = h->Aout; a.S = h->S; a.ldQ = h->ldQ; a.per_state_std = h->cfg.per_state_std;
    a.lim = h->cfg.act_limit; a.a_mean = h->f("norm.a_mean"); a.a_den = h->f("norm.a_den");
    if (update) {
        a.ma_mean = h->f(mnorm(h, "a_mean")); a.ma_den = h->f(mnorm(h, "a_den"));
        a.c_t = h->f("ws.c_t"); a.c_std = h->f("ws.c_std"); a.c_u = h->f("ws.c_u"); a.c_mask = h->f("ws.c_mask");
    }
    return a;
}

// actor.head as a launch of its own over rows [0, rows) of ws.Ha2, rows [cache0, rows) cached for the
// backward; the segments are the caller's
Launch actor_head_rows(sacx_handle* h, const float* part, int rows, int cache0) {
    Launch L{};
    L.kind = Launch::AHEAD;
    L.name = "actor.head";
    L.head = head_args(h, h->f("ws.Ha2"), part, true);
    L.head.total_rows = rows;
    L.head.cache_row0 = cache0;
    L.head.cache_row1 = rows;
    L.grid = (rows + 3) / 4;
    L.flops = 2.0 * rows * h->H1 * h->Aout;
    L.bytes = 4.0 * rows * (h->H1 + 6.0 * h->A);
    return L;
}

// the SAC / SAC-EO update's: evaluate(sp) -> the target rows, evaluate(s) -> the policy rows, sample(s_e) ->
// the world models' rows
Launch actor_head_launch(sacx_handle* h, int slot, const float* part) {
    const int B = h->B, A = h->A;
    const std::string sl = "slot" + std::to_string(slot);
    float* noise = h->f(sl + ".noise");
    Launch L = actor_head_rows(h, part, h->Ra, B);
    L.frees_slot = true;
    HeadArgs& a = L.head;
    a.nseg = h->cfg.use_expert ? 3 : 2;
    a.seg[0] = {0, B, 0, 0, noise, h->f(sl + ".Xt"), h->f("ws.nlp_t")};
    a.seg[1] = {B, 2 * B, 0, 0, noise + (size_t)B * A, h->f(sl + ".Xp"), h->f("ws.nlp_p")};
    a.seg[2] = {2 * B, 2 * B + h->ne, 1, 0, noise + (size_t)2 * B * A, h->f(sl + ".Xm"), nullptr};
    return L;
}

// alpha.head: evaluate(s) of the updated actor on the alpha rows (ws.Hl2), the per-workgroup partials of
// sum(-nlp + H) for alpha.final
Launch alpha_head_launch(sacx_handle* h, int slot, const float* part) {
    const int B = h->B;
    Launch L{};
    L.kind = Launch::AHEAD;
    L.name = "alpha.head";
    HeadArgs& a = L.head;
    a = head_args(h, h->f("ws.Hl2"), part, false);
    a.nseg = 1;
    a.seg[0] = {0, B, 0, 0, h->f("slot" + std::to_string(slot) + ".noise") + (size_t)(2 * B + h->ne) * h->A, nullptr, h->f("ws.nlp3")};
    a.total_rows = B;
    a.cache_row0 = 1 << 30;
    a.alpha_mode = 1;
    L.fin.red = h->f("red");
    L.fin.target_entropy = h->cfg.target_entropy;
    L.grid = (B + 3) / 4;
    L.flops = 2.0 * B * h->H1 * h->Aout;
    L.bytes = 4.0 * B * h->H1;
    return L;
}

// The shapes the two partial folds have kernels for (the head's partial dots out of the actor's last layer;
// the head backward as actor.bwd1's prologue, from partial action gradients).  A caller adds its own gating.
bool head_part_shape(const sacx_handle* h) { return h->Aout <= 8 && h->H1 <= 256 && h->H1 % 64 == 0; }
bool fold_hbw_shape(const sacx_handle* h) {
    const bool critics = !h->bc, models = h->cfg.use_expert != 0;   // whose layer 0 writes the partials
    return h->Aout <= 8 && h->H1 <= 256 && h->H1 % 16 == 0 && (!critics || (h->Hc0 <= 256 && h->Hc0 % 64 == 0)) &&
           (!models || (h->Hm0 <= 512 && h->Hm0 % 64 == 0));
}

// A forward problem of the actor's last hidden layer also writes the head's dots with W3 as per-column-tile
// partials (GR_HEAD_PART), from `ppart` on
void head_part_dots(sacx_handle* h, GemmProb& p, float* ppart) {
    p.pw = h->f(actor_head_name(h)); p.pw_ld = 1; p.pw_cs = h->Aout; p.pw_n = h->Aout;   // W3[n][o] at n * Aout + o
    p.ppart = ppart;
}

// A dX problem down to the layer-0 output of a net on [s | a] writes per-tile partial action gradients
// instead of C (read by no one else): its tiles' products with the action rows of that layer's W_ext [. x H0]
void part_action_grad(sacx_handle* h, GemmProb& p, const float* W0, int H0, float* ppart) {
    p.pw = W0 + (size_t)h->S * H0;
    p.pw_ld = H0; p.pw_cs = 1; p.pw_n = h->A;
    p.ppart = ppart;
    p.C = nullptr;
}

// actor.head.bwd on the row kernel (k_actor_bwd): the action gradients of the B policy rows through layer 0
// of q0 / q1 and of the expert rows through the world models', the tanh-Gaussian backward, the delta at the
// actor's last hidden layer.  gpol: the policy rows' output gradients where ws.Dp1 is the unscaled delta
// (the fused plan's linearity), null where it is the loss-scaled one.  B = 0: BC, the expert rows alone
Launch actor_head_bwd_launch(sacx_handle* h, int B, bool expert, const float* gpol) {
    const NetDims& na = h->nd[0];
    const int ne = h->ne, rows = B + ne, A = h->A, H1 = h->H1, Hm0 = h->Hm0, Hc0 = B ? h->Hc0 : 0, Da = na.D();
    const int nm = expert_split(h).nm;
    Launch L{};
    L.kind = Launch::ABWD;
    L.name = "actor.head.bwd";
    ActorBwdArgs& b = L.ab;
    b.B = B; b.ne = ne; b.S = h->S; b.A = A; b.Aout = h->Aout; b.H0 = Hc0; b.H1 = H1; b.Hm0 = Hm0;   // Dp1 / Wq1: critic
    b.per_state_std = h->cfg.per_state_std; b.lim = h->cfg.act_limit;
    if (B) { b.Dp1 = h->f("ws.Dp1"); b.Wq1[0] = h->f("q0.l0"); b.Wq1[1] = h->f("q1.l0"); }
    b.Dm1 = h->f("ws.Dm1");
    if (expert) { b.Wm1[0] = h->f("m0.l0"); b.Wm1[1] = h->f(nm > 1 ? "m1.l0" : "m0.l0"); }
    b.a_den = h->f("norm.a_den"); b.ma_den = h->f(mnorm(h, "a_den")); b.alpha = h->f("alpha"); b.ctl = h->ctl();
    b.use_expert = expert;
    b.c_t = h->f("ws.c_t"); b.c_std = h->f("ws.c_std"); b.c_u = h->f("ws.c_u"); b.c_mask = h->f("ws.c_mask");
    b.W3a = h->f(actor_head_name(h)); b.Ha2 = h->f("ws.Ha2") + (size_t)B * H1;
    b.act = (Da == 1 && h->ln) ? ACT_TANH : na.act[Da - 1];   // layer norm: tanh' at the norm's output
    b.Da3 = h->f("ws.Da3"); b.Da2 = h->f("ws.Da2"); b.E = h->f("ws.E");
    b.gpol = gpol;
    L.grid = (rows + 3) / 4;
    L.flops = 2.0 * B * 2 * Hc0 * A + 2.0 * ne * Hm0 * A + 2.0 * rows * H1 * h->Aout;
    L.bytes = 4.0 * (2.0 * B * Hc0 + ne * Hm0 + 2.0 * rows * H1);
    return L;
}

// actor.head.bwd as the tile prologue of actor.bwd1 (two-layer actors): Da3 from the per-tile partial action
// gradients (part_action_grad: pi.q.bwd1's for the B policy rows, model.bwd1's for the expert rows), Da2
// generated on load (an MFMA from Da3 and W3a) and stored by column tile 0.  Appends the launch and returns
// it: the flops / bytes of the prologue are the caller's
Launch& head_bwd_fold(sacx_handle* h, std::vector<Launch>& plan, int B, bool expert) {
    const int ne = h->ne, rows = B + ne, H0 = h->H0, H1 = h->H1;
    GemmProb p = prob_dx(h->f("ws.Ha2") + (size_t)B * H1, rows, H1, h->f("actor.l1"), H0, h->f("ws.Ha1") + (size_t)B * H0,
                         h->f("ws.Da1"), h->ln ? ACT_TANH : h->aact[0]);
    p.wgen = h->f("actor.l2");               // W3a [(H1+1) x Aout]
    p.gen_act = h->aact[1];                  // act'(Ha2)
    p.hbw = 1;
    add_gemm(h, plan, "actor.head.bwd+actor.bwd1", {p});
    Launch& L = plan.back();
    set_rows(L, GR_HEAD_BWD);
    HeadBwdArgs& b = L.gemm.hbw;
    b.B = B; b.A = h->A; b.Aout = h->Aout; b.per_state_std = h->cfg.per_state_std; b.tq = B ? (h->Hc0 + 15) / 16 : 0;
    b.lim = h->cfg.act_limit; b.part = B ? h->f("ws.apart") : nullptr; b.gpol = B ? h->f("ws.gp") : nullptr;
    b.a_den = h->f("norm.a_den"); b.ma_den = h->f(mnorm(h, "a_den")); b.alpha = h->f("alpha");
    b.c_t = h->f("ws.c_t"); b.c_std = h->f("ws.c_std"); b.c_u = h->f("ws.c_u"); b.c_mask = h->f("ws.c_mask");
    b.Da3 = h->f("ws.Da3"); b.E = h->f("ws.E"); b.Da2 = h->f("ws.Da2");
    b.ne = ne; b.tqm = (h->Hm0 + 15) / 16; b.mpart = expert ? h->f("ws.mpart") : nullptr; b.ctl = expert ? h->ctl() : nullptr;
    return L;
}

// ---------------------------------------------------------------- the fused update plan
// Two hidden layers per net (any other depth: build_plan_generic).  The shared builders give the problems
// and the row kernels' arguments; what makes this the fused plan stays here: the head folded into q.fwd0,
// the policy rows on critic.adam, model.head merged into pi.q.fwd*, the linearity fusion of the critic and
// policy backward, fuse_fwd2 and xbf_wire.
void build_plan(sacx_handle* h, int slot) {
    std::vector<Launch>& plan = h->plan[slot];
    plan.clear();
    const int S = h->S, A = h->A, H1 = h->H1, B = h->B, Aout = h->Aout, Rb = h->Rb;
    const int Hm0 = h->Hm0, Hc0 = h->Hc0, Hc1 = h->Hc1;   // the critics' hidden sizes (--critic_layers; H0 / H1: the actor's)
    // expert rows of world model k: [k * half, (k + 1) * half) with 2 or more models (the expert term
    // takes models 0 and 1, SAC_expert.py:325-326), all with one
    const ExpertSplit es = expert_split(h);
    const int nm = es.nm, half = es.half;
    const int ldS = h->ldS;
    const int c1 = h->cact[1];
    const bool eo = h->cfg.use_expert != 0;
    const std::string sl = "slot" + std::to_string(slot);
    float* noise = h->f(sl + ".noise");
    float* noise_t = noise;
    float* noise_pi = noise + (size_t)B * A;
    float* noise_e = noise + (size_t)2 * B * A;
    auto W = [&](const std::string& n) { return h->f(n); };
    float *Xa = W(sl + ".Xa"), *Xq = W(sl + ".Xq"), *Xt = W(sl + ".Xt"), *Xp = W(sl + ".Xp"), *Xm = W(sl + ".Xm");
    float *r_in = W(sl + ".r"), *d_in = W(sl + ".d"), *se_raw = W(sl + ".se_raw"), *spe_raw = W(sl + ".spe_raw");
    float *Ha2 = W("ws.Ha2"), *Hq2 = W("ws.Hq2"), *Hp2 = W("ws.Hp2");
    const char* qn[4] = {"t0", "t1", "q0", "q1"};
    auto qk = [](int k) { return "q" + std::to_string(k); };

    plan_inputs(h, plan, slot);
    // the two forward layers of a net as two launches (a fused two-layer tile recomputing
    // layer 0 per column tile measured slower once the alpha branch and the heads share
    // launches: 12.06k vs 12.33k updates/s)
    auto fwd_pair = [&](const std::string& name, const std::vector<GemmProb>& p0, const std::vector<GemmProb>& p1) {
        add_gemm(h, plan, name + "0", p0);
        add_gemm(h, plan, name + "1", p1);
    };
    // the same pair as ONE k_fwd2 launch where it qualifies (fuse_fwd2), else the two launches
    auto fwd_pair2 = [&](const std::string& name, const std::vector<GemmProb>& p0, const std::vector<GemmProb>& p1) {
        fwd_pair(name, p0, p1);
        if (h->fwd2) fuse_fwd2(h, plan, name + "01");
    };
    // ---- actor forward on [sp ; s ; s_e]
    const int Ra4 = (h->Ra + 3) & ~3;       // first row of the alpha rows (ws.Hl1 / ws.Hl2 alias Ha1 / Ha2)
    // actor.fwd1 writes the head's Ha2 . W3 as per-column-tile partials (GR_HEAD_PART), so the head
    // rows and the target-tile prologues sum 16 values per output instead of re-reading Ha2
    // rows.  SACX_HEAD_PART=0 keeps the row dots (A/B measurement).
    const char* hpe = std::getenv("SACX_HEAD_PART");
    const int tqh = (H1 + 15) / 16;
    const bool head_part = head_part_shape(h) && (hpe ? std::atoi(hpe) != 0 : h->tile32_plan == 0);
    // the partials of the head rows from row r0 of Ha2 on
    auto hpart = [&](int r0) { return head_part ? W("ws.hpart") + (size_t)r0 * Aout * tqh : nullptr; };
    // the actor's two layers on a pass's rows (--actor_layer_norm: k_ln behind layer 0), layer 1 with the
    // head partials, the pair as one k_fwd2 launch where it qualifies
    auto actor_fwd = [&](const ActorPass& c, const std::string& name, const std::string& ln_name) {
        actor_fwd_chain(h, plan, c, name, ln_name);
        if (head_part) {
            head_part_dots(h, plan.back().gemm.probs[0], hpart(c.hrow0));
            set_rows(plan.back(), GR_HEAD_PART);
        }
        if (!h->ln && h->fwd2) fuse_fwd2(h, plan, name + "01");
    };
    actor_fwd(actor_pass_ws(h, Xa, h->Ra, 0, h->Ra), "actor.fwd", "actor.ln");
    // actor.head folded into q.fwd0 (plain SAC): the target tiles compute their rows' actions
    // in a prologue, the policy rows (and the previous update's alpha rows) run as extra
    // workgroups of the same launch.  SACX_FUSE_HEAD=0 keeps the separate launch.
    const char* fh = std::getenv("SACX_FUSE_HEAD");
    // Packed seeds (>= 4) keep the separate launch: the prologue recomputes each tile's 16 rows
    // once per column tile, which a full GPU of seeds pays for (measured 34.3k vs 31.6k updates/s
    // at 8 seeds); one seed gains the launch it saves.
    // SAC-EO as well: the expert rows (sample -> the world models' inputs Xm) ride as row
    // workgroups of q.fwd0, and the models' forward shifts one launch later (layer 0 in q.fwd1,
    // layer 1 in pi.q.fwd0, the MSE head in pi.q.fwd1)
    const bool fuse_head = Aout <= 16 && S + A <= 64 && H1 % 16 == 0 && H1 <= 512 &&
                           (fh ? std::atoi(fh) != 0 : h->plan_seeds < 4);
    // actor.head.bwd folded into actor.bwd1 (plain SAC; the expert rows' model gradients keep
    // the row kernel): pi.q.bwd1 writes per-tile partial action gradients, actor.bwd1's tiles
    // finish them.  SACX_FOLD_HBW=0 keeps the separate launch (A/B measurement).
    const char* fhb = std::getenv("SACX_FOLD_HBW");
    const int tq = (Hc0 + 15) / 16;        // action-gradient partials per row (the critics' layer-0 tiles)
    // The folded launch itself keeps 16x16 tiles (its prologue and generated A operand); the
    // partial-writing launches may take 32x32 tiles.  On 32x32 (packed) plans both folds are off
    // by default: there the launches are bound by workgroup residency, not by their number, and
    // the folds' extra work loses (HC 8 seeds, A/B x2: both on 42.3k, hbw fold only 43.4k, head
    // partials only 43.1k, both off 43.9k updates/s; tools/pk_ab.sh).
    const bool fold_hbw = fold_hbw_shape(h) && (fhb ? std::atoi(fhb) != 0 : h->tile32_plan == 0);
    // ---- actor head
    HeadArgs head_fused{};
    if (fuse_head) {
        HeadArgs& a = head_fused;
        a = head_args(h, Ha2, hpart(0), true);
        // q.fwd0 carries the target rows (tile prologues) and, folded, the previous update's
        // alpha rows; the policy rows ride as extra workgroups of critic.adam (policy_head)
        a.nseg = 1;
        a.seg[0] = {0, B, 0, 0, noise_t, nullptr, W("ws.nlp_t")};
        // total_rows = Ra: merged_body appends the previous update's alpha rows at round4(Ra),
        // where their layer-2 outputs live (ws.Hl2 aliases Ha2 from row round4(Ra))
        a.total_rows = h->Ra;
        a.cache_row0 = 1 << 30;             // no backward cache from these rows (target, alpha)
        a.cache_row1 = 1 << 30;
        if (eo) {                           // SAC-EO expert rows: sample() into Xm, cached
            a.nseg = 2;
            a.seg[1] = {2 * B, 2 * B + h->ne, 1, 0, noise_e, Xm, nullptr};
            a.cache_row0 = B;
            a.cache_row1 = h->Ra;
        }
    } else {
        plan.push_back(actor_head_launch(h, slot, hpart(0)));
    }
    // ---- target / critic / model forward
    {
        std::vector<GemmProb> p0, p1;
        for (int k = 0; k < 4; ++k) {
            p0.push_back(critic_fwd_prob(h, qn[k], k < 2 ? Xt : Xq, "ws.Hq", k, 0));
            p1.push_back(critic_fwd_prob(h, qn[k], nullptr, "ws.Hq", k, 1));
        }
        if (fuse_head) {
            p0[0].headp = p0[1].headp = 1;  // the target tiles' prologue
            add_gemm(h, plan, "q.fwd0+actor.head", p0);
            Launch& L = plan.back();
            set_rows(L, GR_ACTOR_HEAD);
            L.gemm.head = head_fused;
            L.gemm.head_block0 = eo ? (2 * B) / 4 : ((h->Ra + 3) & ~3) / 4;
            L.gemm.row_blocks = eo ? (h->Ra + 3) / 4 - (2 * B) / 4 : 0;   // + the alpha rows (merged_body)
            L.grid += L.gemm.row_blocks;
            L.flops += 2.0 * B * H1 * Aout;
            L.bytes += 4.0 * B * (H1 + 6.0 * A);
            L.frees_slot = true;
            // the models' layer 0 on Xm (written by the rows above)
            for (int k = 0; eo && k < nm; ++k) p1.push_back(model_fwd_prob(h, Xm, k, 0));
            add_gemm(h, plan, "q.fwd1", p1);
            if (h->fwd2 && !eo) fuse_fwd2(h, plan, "q.fwd01+actor.head");
        } else {
            for (int k = 0; eo && k < nm; ++k) {
                p0.push_back(model_fwd_prob(h, Xm, k, 0));
                p1.push_back(model_fwd_prob(h, Xm, k, 1));
            }
            fwd_pair("q.fwd", p0, p1);
        }
    }
    // ---- critic backward.  By linearity Dq1 = g (.) M1 with M1 = ((w3 (.) act'(Hq2)) Wq1^T) (.) act'(Hq1)
    // independent of the per-row loss gradient g, so the dX GEMM (A generated from Hq2 and w3)
    // shares one launch with the q.head rows (target, g, loss rows, Dq2, expert MSE + Dm2), and
    // critic.adam applies g to layer 0 (row-scaled B).
    {
        std::vector<GemmProb> pb;
        for (int k = 0; k < 2; ++k) {
            GemmProb p = critic_dx_prob(h, qk(k), "ws.Hq", 2 + k, "ws.Dq", k, 1, true);
            p.wgen = W(qk(k) + ".l2");         // w3 column of W3_ext
            p.gen_act = c1;                    // act'(Hq2); the epilogue takes act'(Hq1)
            pb.push_back(p);
        }
        add_gemm(h, plan, "q.head+critic.bwd1", pb);
        Launch& L = plan.back();
        set_rows(L, GR_QHEAD);
        L.gemm.row_blocks = (B + 3) / 4;
        L.gemm.qh = q_head_args(h, 0, Hq2, W("ws.Dq2"), r_in, d_in);
        L.grid += L.gemm.row_blocks;
        L.flops += 2.0 * B * Hc1 * 4 + 2.0 * B * Hc1 * 2;
        L.bytes += 4.0 * (4.0 * B * Hc1 + 2.0 * B * Hc1 * 2);
        std::vector<GemmProb> pw;
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i <= 2; ++i) {
                GemmProb p = critic_dw_prob(h, k, Xq, i);
                if (i == 0) p.bscale = W("ws.gq") + (size_t)k * B;   // Dq1 = g (.) M1
                pw.push_back(p);
            }
        // (no k_dwl where rows ride along: the policy head rows)
        add_gemm(h, plan, "critic.adam", pw, {-1, fuse_head ? 0 : -1});
        if (fuse_head) {                    // the policy rows of actor.head (read from pi.q.fwd0 on)
            Launch& L = plan.back();
            HeadArgs a = head_fused;
            a.nseg = 1;
            a.seg[0] = {B, 2 * B, 0, 0, noise_pi, Xp, W("ws.nlp_p")};
            a.total_rows = 2 * B;
            a.cache_row0 = B;
            a.cache_row1 = h->Ra;
            L.name += "+actor.head";
            set_rows(L, GR_POLICY_HEAD);
            L.gemm.head = a;
            L.gemm.head_block0 = B / 4;
            L.gemm.row_blocks = (2 * B + 3) / 4 - B / 4;
            L.grid += L.gemm.row_blocks;
            L.flops += 2.0 * B * H1 * Aout;
            L.bytes += 4.0 * B * (H1 + 6.0 * A);
        }
        if (h->dp_ranks > 0) dp_split_adam(h, plan, "q0.l0", "q1.l2", "t0.l0", GRP_Q);
    }
    // ---- policy loss through the updated critics: the same linearity; pi.q.head's rows
    // (min, tie split, loss rows, g0 / g1) share the unscaled dX launch, actor.head.bwd applies
    // g0 / g1.  The SAC-EO world-model dX (needs q.head's Dm2) rides in the same launch.
    {
        std::vector<GemmProb> p0, p1;
        for (int k = 0; k < 2; ++k) {
            p0.push_back(critic_fwd_prob(h, qk(k), Xp, "ws.Hp", k, 0));
            p1.push_back(critic_fwd_prob(h, qk(k), nullptr, "ws.Hp", k, 1));
        }
        // the models' layer 1 on Hm1 (from q.fwd1)
        for (int k = 0; eo && fuse_head && k < nm; ++k) p0.push_back(model_fwd_prob(h, Xm, k, 1));
        if (eo) fwd_pair("pi.q.fwd", p0, p1);
        else fwd_pair2("pi.q.fwd", p0, p1);
        if (eo) {
            // SAC-EO: world-model layer 2 on the expert rows + MSE epilogue (needs Hm2 from q.fwd1),
            // riding in the pi.q.fwd0 launch (or, with the fused head, in pi.q.fwd1 = plan.back(): Hm2
            // comes from pi.q.fwd0)
            Launch& F0 = plan[plan.size() - (fuse_head ? 1 : 2)];
            const std::vector<GemmProb> pm = model_head_probs(h, MSE_EXPERT, se_raw, spe_raw);
            std::vector<Launch> one;
            add_gemm(h, one, "model.head", pm);
            if (!merge_gemm(F0.gemm, one[0].gemm)) { fprintf(stderr, "sacx: model.head merge\n"); abort(); }
            F0.name += "+model.head";
            F0.grid = F0.gemm.total_tiles;
            F0.flops += one[0].flops;
            F0.bytes += one[0].bytes;
        }
        std::vector<GemmProb> pb;
        for (int k = 0; k < 2; ++k) {
            GemmProb p = critic_dx_prob(h, qk(k), "ws.Hp", k, "ws.Dp", k, 1, true);
            p.wgen = W(qk(k) + ".l2");
            p.gen_act = c1;
            // partial action gradients instead of Dp1 (read by no one else)
            if (fold_hbw) part_action_grad(h, p, W(qk(k) + ".l0"), Hc0, W("ws.apart") + (size_t)k * B * tq * A);
            pb.push_back(p);
        }
        if (eo) {                            // Dm2 = dout . Wm2[:, :S]^T (.) act'(Hm2)
            const std::vector<GemmProb> pd = model_bwd_probs(h, 2);
            pb.insert(pb.end(), pd.begin(), pd.end());
        }
        add_gemm(h, plan, "pi.q.head+pi.q.bwd1", pb);
        {
            Launch& L = plan.back();
            set_rows(L, GR_PIQHEAD);
            L.gemm.row_blocks = (B + 3) / 4;
            L.gemm.qh = q_head_args(h, 1, Hp2, nullptr, nullptr, nullptr);
            L.grid += L.gemm.row_blocks;
            L.flops += 2.0 * B * Hc1 * 2 * 2;
            L.bytes += 4.0 * (2.0 * B * Hc1 * 2);
        }
        if (eo) {                            // Dm1 = Dm2 . Wm1^T (.) act'(Hm1), for actor.head.bwd
            std::vector<GemmProb> pd = model_bwd_probs(h, 1);
            const int tqm = (Hm0 + 15) / 16;
            // partial action gradients of the expert rows instead of Dm1
            for (int k = 0; fold_hbw && k < nm; ++k)
                part_action_grad(h, pd[k], W("m" + std::to_string(k) + ".l0"), Hm0, W("ws.mpart") + (size_t)k * half * A * tqm);
            add_gemm(h, plan, "model.bwd1", pd);
            if (fold_hbw) set_rows(plan.back(), GR_PIQHEAD);   // DX with the partial epilogue (no q-head rows)
        }
    }
    // ---- actor backward: the policy and expert rows, rows [B, B + Rb) of Xa and of the hidden buffers
    {
        if (fold_hbw) {
            // actor.head.bwd as the tile prologue of actor.bwd1, from the partials of pi.q.bwd1 / model.bwd1
            Launch& L = head_bwd_fold(h, plan, B, eo);
            L.flops += 2.0 * B * 2 * Hc0 * A + 2.0 * Rb * H1 * Aout;
            L.bytes += 4.0 * (2.0 * B * tq * A + 2.0 * Rb * H1);
        } else {
            plan.push_back(actor_head_bwd_launch(h, B, eo, W("ws.gp")));
        }
        // (the folded head backward is layer 1's dX already: the norm's backward alone follows it)
        const ActorPass bw = actor_pass_ws(h, Xa + (size_t)B * ldS, Rb, B, h->Ra);
        actor_bwd_chain(h, plan, bw, fold_hbw ? 0 : 1);
        add_gemm(h, plan, "actor.adam", actor_dw_probs(h, bw));
        if (h->dp_ranks > 0) dp_split_adam(h, plan, "actor.l0", "actor.logstd", "", GRP_PI);
    }
    // ---- alpha: updated actor on s, evaluate, Adam on alpha, statistics
    const size_t alpha_first = plan.size();
    // the alpha forward is folded into the next update's actor forward (merged_body): the same fusion as
    // the actor pair's, so merged_body folds one k_fwd2 launch into the other
    actor_fwd(actor_pass_ws(h, Xa + (size_t)B * ldS, B, Ra4, h->Ra), "alpha.fwd", "alpha.ln");
    plan.push_back(alpha_head_launch(h, slot, hpart(Ra4)));
    plan_alpha_final(h, plan, nm);
    // alpha.fwd .. alpha.final only feed the next update's q.head
    for (size_t i = alpha_first; i < plan.size(); ++i) plan[i].alpha_branch = true;
    xbf_wire(h, plan, slot);
    for (Launch& L : plan) pack_seeds(L, (int64_t)h->seed_bytes, h->seeds);
}

// ---------------------------------------------------------------- the generic update plan
// Nets of any depth (create_nn's layers list, nn_utils.py:100-138; SACX_GENERIC=1 also at two layers,
// the parity check of this plan against the fused one): the update of build_plan in the reference's
// order, with every Dense layer a problem of its depth level's forward, dX or dW + Adam launch and the
// heads on the row kernels -- k_actor_head (evaluate / sample), k_qhead (twin-Q target, critic loss and
// policy-loss gradients, writing the delta at the critics' last hidden layer), k_actor_bwd (the action
// gradient through the first layer of the critics / world models, the tanh-Gaussian backward, the
// delta at the actor's last hidden layer).  No folds and no linearity fusion: each delta is the
// loss-scaled one, the dW launches take unscaled rows.  merged_body folds the alpha branch exactly
// as in the fused plan (alpha.fwd<i> into actor.fwd<i>, alpha.head into actor.head, alpha.final into
// the first forward launch after it).
void build_plan_generic(sacx_handle* h, int slot) {
    std::vector<Launch>& plan = h->plan[slot];
    plan.clear();
    const int B = h->B, Hc1 = h->Hc1;
    const int nm = expert_split(h).nm;      // the expert term's models
    const int ldS = h->ldS, Rb = h->Rb;
    const bool eo = h->cfg.use_expert != 0;
    const int Da = h->nd[0].D(), Dc = h->nd[1].D(), Dm = eo ? h->nd[2].D() : 0;
    const std::string sl = "slot" + std::to_string(slot);
    auto W = [&](const std::string& n) { return h->f(n); };
    auto L_ = layer_name;
    float *Xa = W(sl + ".Xa"), *Xq = W(sl + ".Xq"), *Xt = W(sl + ".Xt"), *Xp = W(sl + ".Xp"), *Xm = W(sl + ".Xm");
    float *r_in = W(sl + ".r"), *d_in = W(sl + ".d"), *se_raw = W(sl + ".se_raw"), *spe_raw = W(sl + ".spe_raw");
    const char* qn[4] = {"t0", "t1", "q0", "q1"};
    const int Ra4 = (h->Ra + 3) & ~3;       // first row of the alpha rows in the actor chain's buffers

    plan_inputs(h, plan, slot);
    // ---- actor forward on all Ra rows of Xa (the layer-norm cache holds them all)
    actor_fwd_chain(h, plan, actor_pass_ws(h, Xa, h->Ra, 0, h->Ra), "actor.fwd", "actor.ln");
    // ---- actor head: evaluate(sp) -> target rows, evaluate(s) -> policy rows, sample(s_e) -> model rows
    plan.push_back(actor_head_launch(h, slot, nullptr));
    // ---- target / critic forward (t0, t1 on [sp | pi(sp)], q0, q1 on [s | a]; the world models' hidden
    // layers on the expert rows [s_e | pi(s_e)]), one launch per depth level
    for (int i = 0; i < std::max(Dc, Dm); ++i) {
        std::vector<GemmProb> ps;
        if (i < Dc)
            for (int k = 0; k < 4; ++k) ps.push_back(critic_fwd_prob(h, qn[k], k < 2 ? Xt : Xq, "ws.Hq", k, i));
        if (i < Dm)
            for (int k = 0; k < nm; ++k) ps.push_back(model_fwd_prob(h, Xm, k, i));
        add_gemm(h, plan, "q.fwd" + std::to_string(i), ps);
    }
    if (eo)     // the world models' head on the expert rows + the expert MSE (SAC_expert.py:319-332)
        add_gemm(h, plan, "model.head", model_head_probs(h, MSE_EXPERT, se_raw, spe_raw));
    {   // ---- q.head: min target, TD target, critic losses and the delta at the critics' last hidden layer
        Launch L{};
        L.kind = Launch::QHEAD;
        L.name = "q.head";
        L.qh = q_head_args(h, 0, W("ws.Hq2"), W("ws.Dq2"), r_in, d_in);
        L.grid = (B + 3) / 4;
        L.flops = 2.0 * B * Hc1 * 4;
        L.bytes = 4.0 * (4.0 * B * Hc1 + 2.0 * B * Hc1);
        plan.push_back(L);
    }
    // ---- critic backward (dX down to layer 0's output), then dW + Keras Adam + Polyak into t0 / t1
    for (int i = Dc - 1; i >= 1; --i) {
        std::vector<GemmProb> pb;
        for (int k = 0; k < 2; ++k) pb.push_back(critic_dx_prob(h, qn[2 + k], "ws.Hq", 2 + k, "ws.Dq", k, i));
        add_gemm(h, plan, "critic.bwd" + std::to_string(i), pb);
    }
    {
        std::vector<GemmProb> pw;
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i <= Dc; ++i) pw.push_back(critic_dw_prob(h, k, Xq, i));
        const int n = add_gemm_split(h, plan, "critic.adam", pw);
        if (h->dp_ranks > 0) dp_split_adam(h, plan, "q0.l0", L_("q1", Dc), "t0.l0", GRP_Q, n);
    }
    // ---- policy loss through the updated critics
    for (int i = 0; i < Dc; ++i) {
        std::vector<GemmProb> ps;
        for (int k = 0; k < 2; ++k) ps.push_back(critic_fwd_prob(h, qn[2 + k], Xp, "ws.Hp", k, i));
        add_gemm(h, plan, "pi.q.fwd" + std::to_string(i), ps);
    }
    {   // min, tie split, policy loss rows, the delta at the critics' last hidden layer (x d p / d Q_k)
        Launch L{};
        L.kind = Launch::QHEAD;
        L.name = "pi.q.head";
        L.qh = q_head_args(h, 1, W("ws.Hp2"), W("ws.Dp2"), nullptr, nullptr);
        L.grid = (B + 3) / 4;
        L.flops = 2.0 * B * Hc1 * 2;
        L.bytes = 4.0 * (4.0 * B * Hc1);
        plan.push_back(L);
    }
    for (int i = Dc - 1; i >= 1; --i) {
        std::vector<GemmProb> pb;
        for (int k = 0; k < 2; ++k) pb.push_back(critic_dx_prob(h, qn[2 + k], "ws.Hp", k, "ws.Dp", k, i));
        add_gemm(h, plan, "pi.q.bwd" + std::to_string(i), pb);
    }
    if (eo)     // the world models' backward to their layer-0 output (the expert rows' action gradient)
        for (int i = Dm; i >= 1; --i) add_gemm(h, plan, "model.bwd" + std::to_string(i), model_bwd_probs(h, i));
    // ---- actor backward: action gradients -> tanh-Gaussian backward -> the delta at the last hidden
    // layer (k_actor_bwd, from the loss-scaled deltas: gpol = null), dX to layer 0, dW + Adam
    plan.push_back(actor_head_bwd_launch(h, B, eo, nullptr));
    {   // the policy and expert rows: rows [B, B + Rb) of Xa and of the hidden buffers, [0, Rb) of the deltas
        const ActorPass bw = actor_pass_ws(h, Xa + (size_t)B * ldS, Rb, B, h->Ra);
        actor_bwd_chain(h, plan, bw, Da - 1);
        const int n = add_gemm_split(h, plan, "actor.adam", actor_dw_probs(h, bw));
        if (h->dp_ranks > 0) dp_split_adam(h, plan, "actor.l0", "actor.logstd", "", GRP_PI, n);
    }
    // ---- alpha: the updated actor on s, evaluate, Adam on alpha, statistics
    const size_t alpha_first = plan.size();
    actor_fwd_chain(h, plan, actor_pass_ws(h, Xa + (size_t)B * ldS, B, Ra4, h->Ra), "alpha.fwd", "alpha.ln");
    plan.push_back(alpha_head_launch(h, slot, nullptr));
    plan_alpha_final(h, plan, nm);
    for (size_t i = alpha_first; i < plan.size(); ++i) plan[i].alpha_branch = true;
    for (Launch& L : plan) pack_seeds(L, (int64_t)h->seed_bytes, h->seeds);
}

// ---------------------------------------------------------------- the BC update plans
// BC._update_actor (BC.py:309-363): actor.sample(s_e) through world models 0 / 1 (or model 0 alone),
// loss = mean(0.5 sum (sp_e - sp_pred)^2), Adam on the actor.  It is the expert term of the SAC-EO
// update with weight 1 and no policy rows (sac_oracle.py:608-628), so it runs the same kernels with a
// batch of zero replay rows: the expert rows are rows [0, ne) of every actor-side buffer, the row
// kernels see B = 0, and the world-model head takes weight 1 (MSE_BC) instead of ctl->epsilon.  No
// critic, target or alpha launch; bc_finalize writes the statistics row and advances the counters.
//   generic (any depth, layer norm, SACX_GENERIC=1): one GEMM launch per layer and direction, the heads
//     on the row kernels -- actor.fwd<i> (actor.ln) actor.head model.fwd<i> model.head model.bwd<i>
//     actor.head.bwd actor.bwd<i> (actor.ln.bwd) actor.adam bc.final;
//   folded (two-layer nets): the actor pair and the model pair as k_fwd2 launches (the actor's writing
//     the head's partial dots, the models' on the fit's pre-gathered-rows variant: layer 0 up to 512
//     wide), the head backward as actor.bwd1's tile prologue from model.bwd1's partial action gradients,
//     and the finalisation as one more workgroup of model.bwd2 (behind model.head, whose MSE partials it
//     sums; actor.adam then takes the advanced step, t_adv) -- 8 launches at the HalfCheetah shapes:
//     actor.fwd01 actor.head model.fwd01 model.head model.bwd2+bc.final model.bwd1
//     actor.head.bwd+actor.bwd1 actor.adam.
void build_plan_bc(sacx_handle* h, int slot) {
    std::vector<Launch>& plan = h->plan[slot];
    plan.clear();
    const int S = h->S, A = h->A, H1 = h->H1, ne = h->ne, Aout = h->Aout;
    const int Hm0 = h->Hm0;
    const ExpertSplit es = expert_split(h);
    const int nm = es.nm;                   // the expert term's models
    const bool fold = !h->deep;
    const int Da = h->nd[0].D(), Dm = h->nd[2].D();
    const std::string sl = "slot" + std::to_string(slot);
    auto W = [&](const std::string& n) { return h->f(n); };
    float* noise_e = h->f(sl + ".noise");
    float *Xa = W(sl + ".Xa"), *Xm = W(sl + ".Xm"), *se_raw = W(sl + ".se_raw"), *spe_raw = W(sl + ".spe_raw");

    plan_inputs(h, plan, slot);
    const size_t body0 = plan.size();
    // ---- actor forward on the expert rows: rows [0, ne) of every actor-side buffer
    const ActorPass ap = actor_pass_ws(h, Xa, ne, 0, ne);
    const bool head_part = fold && head_part_shape(h) && h->tile32_plan == 0;
    actor_fwd_chain(h, plan, ap, "actor.fwd", "actor.ln");
    if (head_part) {                         // the head's Ha2 . W3 as per-column-tile partials of the last layer (GR_HEAD_PART)
        head_part_dots(h, plan.back().gemm.probs[0], W("ws.hpart"));   // (two layers: the norm's launch is behind layer 0's)
        set_rows(plan.back(), GR_HEAD_PART);
    }
    if (fold && !h->ln && h->fwd2) fuse_fwd2(h, plan, "actor.fwd01");
    {   // ---- actor head: sample(s_e) into the models' input rows (their normaliser for the action columns)
        Launch L = actor_head_rows(h, head_part ? W("ws.hpart") : nullptr, ne, 0);
        L.head.nseg = 1;
        L.head.seg[0] = {0, ne, 1, 0, noise_e, Xm, nullptr};
        plan.push_back(L);
    }
    // ---- world models 0 / 1 forward on [s_e | pi(s_e)]
    for (int i = 0; i < Dm; ++i) {
        std::vector<GemmProb> ps;
        for (int k = 0; k < nm; ++k) ps.push_back(model_fwd_prob(h, Xm, k, i));
        add_gemm(h, plan, "model.fwd" + std::to_string(i), ps);
    }
    // the pair as one k_fwd2 launch (GR_PREGATHERED: layer 0 up to 512 wide)
    if (fold && h->fwd2 && S + A <= 32) fuse_fwd2(h, plan, "model.fwd01", true);
    const int mtn = (S + 15) / 16;
    // ---- the models' head + the MSE (BC.py:340-352), weight 1
    add_gemm(h, plan, "model.head", model_head_probs(h, MSE_EXPERT | MSE_BC, se_raw, spe_raw));
    FinalArgs fin{};
    fin.alpha = W("alpha"); fin.alpha_m = fin.alpha + h->p_stride; fin.alpha_v = fin.alpha + 2 * h->p_stride;
    fin.ctl = h->ctl();
    fin.ne = ne; fin.use_expert = SACX_EXPERT_BC; fin.nm = nm;
    fin.mse_rows = W("ws.mse"); fin.mse_tiles = mtn;
    fin.stats = W("stats"); fin.stats_cap = h->stats_cap;
    bool fin_folded = false;
    // ---- the models' backward down to their layer-0 output (the expert rows' action gradient)
    const int tqm = (Hm0 + 15) / 16;
    const bool fold_hbw = fold && fold_hbw_shape(h) && h->tile32_plan == 0;
    for (int i = Dm; i >= 1; --i) {
        std::vector<GemmProb> pb = model_bwd_probs(h, i);
        for (int k = 0; k < nm && i == 1 && fold_hbw; ++k)     // partial action gradients instead of Dm1
            part_action_grad(h, pb[k], W("m" + std::to_string(k) + ".l0"), Hm0, W("ws.mpart") + (size_t)k * es.half * A * tqm);
        add_gemm(h, plan, "model.bwd" + std::to_string(i), pb);
        Launch& L = plan.back();
        if (i == 1 && fold_hbw) set_rows(L, GR_PIQHEAD);   // DX with the partial epilogue (no q-head rows)
        if (fold && i == Dm && L.gemm.rowk == GR_NONE) {   // + the finalisation: one more workgroup
            L.name += "+bc.final";
            L.gemm.has_mfinal = 2;
            L.gemm.fin = fin;
            fin_folded = true;
        }
    }
    // ---- actor backward: tanh-Gaussian backward -> the delta at the last hidden layer, dX, dW + Adam
    if (fold_hbw) {                          // no policy rows (B = 0): the expert rows' partials alone
        Launch& L = head_bwd_fold(h, plan, 0, true);
        L.flops += 2.0 * ne * H1 * Aout;
        L.bytes += 4.0 * (ne * tqm * A + 2.0 * ne * H1);
    } else {
        plan.push_back(actor_head_bwd_launch(h, 0, true, nullptr));
    }
    // (the folded head backward is layer 1's dX already: the norm's backward alone follows it)
    actor_bwd_chain(h, plan, ap, fold_hbw ? 0 : Da - 1);
    {
        const size_t first = plan.size();
        add_gemm_split(h, plan, "actor.adam", actor_dw_probs(h, ap));
        for (size_t i = first; i < plan.size(); ++i) plan[i].gemm.t_adv = fin_folded ? 1 : 0;
    }
    if (!fin_folded) {
        Launch L{};
        L.kind = Launch::FINAL;
        L.name = "bc.final";
        L.fin = fin;
        L.grid = 1;
        L.block = 64;
        L.bytes = 4.0 * ne * mtn;
        plan.push_back(L);
    }
    // the update reads its slot from its first launch on, and no later update reads it
    plan[body0].frees_slot = true;
    for (Launch& L : plan) pack_seeds(L, (int64_t)h->seed_bytes, h->seeds);
}

// one world-model fitting step: gather -> 3 fwd GEMMs -> loss grads -> 2 dX GEMMs -> dW + Adam -> finalize
// the fitting plan of the selected seed (its arena block's pointers).  Folded (h->mfuse, the
// default): the loss and its gradient are model.fwd2's epilogue (mse = 2) and the finalisation is
// one extra workgroup of model.bwd2, so model.adam takes the already-advanced step counter (t_adv);
// the weights are bit-identical to the unfolded chain, the loss statistic sums in another order.
void build_model_plan(sacx_handle* h) {
    std::vector<Launch>& plan = h->mplans[h->sel];
    plan.clear();
    if (!h->cfg.use_expert) return;
    const int S = h->S, A = h->A, mb = h->mb, O = S + 1, ldQ = h->ldQ;
    const int nm = h->nm;
    const NetDims& nmd = h->nd[2];
    const int Dm = nmd.D(), Dr = h->srn ? h->nd[3].D() : 0;
    const int Lf = std::max(Dm, Dr);          // forward levels 0 .. Lf (a net's head at its own depth)
    // GaussianModel / --separate_reward_nn fits exist only in the folded form (their loss epilogues)
    const bool fuse = h->mfuse != 0 || h->gm || h->srn;
    const int Om = h->Om;             // model-net outputs (S + 1, or S beside a reward net)
    const int nt = (Om + 15) / 16;    // fit-loss partials per row (16-column tiles of model.fwd2)
    const int ldO = (int)r4(O);       // D3 row stride
    const int ntm = (mb + 15) / 16;   // GaussianModel: logstd-gradient partials per column (row tiles)
    // model.bwd2 generated on model.bwd1's operand loads (GR_GEN_BWD2) for narrow heads (S + 1 <= 32).
    // fp32 only: the generation is an fp32 MFMA, while model.bwd2 as a launch of its own is a bf16 GEMM
    // under config C5 -- the fold would leave the head's dX operands unrounded in this one variant
    // (every GEMM operand is rounded, whichever launch carries the GEMM).
    // Layer 1 a whole number of float4s wide: column tile 0 stores the generated D2 in 16-B pieces at row
    // stride Hm1, every lane of a 16-column slab one piece.  The kernel leaves out the pieces that begin past
    // the row (a last slab of Hm1 % 16 columns); a piece straddling the row's end -- Hm1 % 4 != 0 -- it cannot
    // split, and it would land on the next row's first columns (the last row's on the buffer behind ws.Df2)
    const bool bfold = fuse && h->mfuse >= 3 && O <= 32 && h->mtile != 2 && h->unaligned_b && !h->gm && !h->srn &&
                       Dm == 2 && !h->wide && !h->cfg.gemm_bf16 && nmd.h[1] % 4 == 0;
    auto W = [&](const std::string& n) { return h->f(n); };
    auto L_ = [](const std::string& net, int i) { return net + ".l" + std::to_string(i); };
    float *Xf = W("ws.Xf"), *Tf = W("ws.Tf"), *Of = W("ws.Of");
    float *Df3 = W("ws.Df3");
    MGatherArgs mg{};
    mg.replay = W("replay"); mg.cap = h->cap; mg.stride = h->stride; mg.S = S; mg.A = A; mg.mb = mb;
    mg.idx_ring = h->ptr<int32_t>("mfit.idx"); mg.idx_cap = h->mfit_cap; mg.ctl = h->ctl();
    mg.s_mean = W("mnorm.s_mean"); mg.s_den = W("mnorm.s_den"); mg.a_mean = W("mnorm.a_mean");
    mg.a_den = W("mnorm.a_den"); mg.d_mean = W("mnorm.d_mean"); mg.d_den = W("mnorm.d_den"); mg.r_norm = W("mnorm.r");
    mg.X = Xf; mg.ldQ = ldQ; mg.T = Tf; mg.nm = nm;
    mg.clip_d = h->cfg.delta_clip_loss; mg.clip_r = h->cfg.reward_clip_loss;
    // The minibatch rows: pre-gathered (SACX_MPRE, default) -- one k_mgather per block of <= MFIT_PRE steps
    // writes step j's normalised rows / targets into staging slot j before the block's steps, whose
    // launches read slot j (enqueue_fit_step moves their slot-0 pointers); or gathered per step, on
    // model.fwd0's operand loads (GR_GATHER: 16x16 tiles, whose rows are whole records; the reward nets'
    // layer 0 reads the gathered X, so --separate_reward_nn keeps the gather launch) or by its own launch
    const bool pre = h->mpre != 0;
    float* Xin = pre ? W("mfit.Xs") : Xf;     // what the steps read: slot 0 of the staging, or X / T
    float* Tin = pre ? W("mfit.Ts") : Tf;
    h->mpres[h->sel] = Launch{};
    h->mpres[h->sel].kind = Launch::RNG;      // (none)
    if (pre) {
        Launch L{};
        L.kind = Launch::MGATHER;
        L.name = "model.pregather";
        L.mg = mg;
        L.mg.X = Xin;
        L.mg.T = Tin;
        L.pre_steps = 1;                      // (the block's step count, set at enqueue)
        L.grid = (nm * mb + 3) / 4;
        L.bytes = 4.0 * nm * mb * (2.0 * S + A + 1 + ldQ + O);
        h->mpres[h->sel] = L;
    }
    const bool gfold = !pre && fuse && h->mfuse >= 2 && h->mtile != 2 && h->stride % 4 == 0 && ldQ % 4 == 0 && !h->srn &&
                       !h->wide;              // (GR_GATHER / GR_PREGATHERED and k_fwd2: layer 0 up to 512 wide)
    if (!gfold && !pre) {
        Launch L{};
        L.kind = Launch::MGATHER;
        L.name = "model.gather";
        L.mg = mg;
        L.grid = (nm * mb + 3) / 4;
        L.bytes = 4.0 * nm * mb * (2.0 * S + A + 1 + ldQ + O);
        plan.push_back(L);
    }
    // forward levels (f[i]: every net's layer i, the head at its depth), backward steps from the heads
    // (b[t]: the dX through layer D - t of each net of depth D > t), dW + Adam per net
    std::vector<std::vector<GemmProb>> f(Lf + 1), b(Lf);
    std::vector<GemmProb> w, wr;
    // net `net` of model k on its mb rows: the chains Hn / Dn, the head's N columns into `out` (row stride ldo)
    // and its delta in D3 (row stride ldd); its problems by level, its dW in layer order into `dw`
    auto add_net = [&](const std::string& net, int ndi, int k, const std::string& Hn, const std::string& Dn, int N, float* out,
                       int ldo, float* D3, int ldd, std::vector<GemmProb>& dw) {
        const size_t r0 = (size_t)k * mb;
        NetPass c = chain_pass(h, net, ndi, GRP_MODEL, Xin + r0 * ldQ, ldQ, S + A, mb, Hn, r0, Dn, r0);
        c.N = N; c.out = out + r0 * ldo; c.ldo = ldo; c.dout = D3 + r0 * ldd; c.lddo = ldd;
        const int D = c.nd->D();
        for (int i = 0; i <= D; ++i) f[i].push_back(net_fwd_prob(h, c, i));
        for (int i = D; i >= 1; --i) b[D - i].push_back(net_dx_prob(h, c, i));
        for (int i = 0; i <= D; ++i) dw.push_back(net_dw_prob(h, c, i));
    };
    for (int k = 0; k < nm; ++k) {
        const std::string n = "m" + std::to_string(k);
        const size_t r0 = (size_t)k * mb;
        add_net(n, 2, k, "ws.Hf", "ws.Df", Om, fuse ? Df3 : Of, fuse ? ldO : O, Df3, ldO, w);
        if (fuse) {   // MSEModel / GaussianModel.get_loss as the head's epilogue: C = d loss / d out, partials
            GemmProb& p = f[Dm].back();
            p.mse = MSE_FIT | (h->gm ? MSE_GAUSS : 0) | (h->lscale ? MSE_SCALE : 0) | (h->srn ? MSE_NOREW : 0);
            p.se_raw = Tin + r0 * O; p.ldp = O; p.part = W("ws.lf") + r0 * nt;
            p.grad_scale = 1.f / (float)mb; p.fcoef = h->cfg.reward_loss_coef;   // the reward column's
            if (h->gm) {
                p.spe_raw = W(n + ".logstd");
                p.ppart = W("ws.lgp") + (size_t)k * ntm * S;
            }
        }
        if (bfold) {   // layer 1's dX: A = D2 generated from H2, D3 and W2 on load; column tile 0 stores it for model.adam
            GemmProb& p = b[Dm - 1].back();
            p.A = W("ws.Hf2") + r0 * nmd.h[1]; p.wgen = W(L_(n, 2)); p.gen_act = nmd.act[1];
            p.gd = Df3 + r0 * ldO; p.gd_ld = ldO; p.g_o = O; p.gst = W("ws.Df2") + r0 * nmd.h[1]; p.gst_ld = nmd.h[1];
        }
    }
    // --separate_reward_nn (base_world_model.py:32-37, :72-74): the reward nets ride in the same
    // launches -- their hidden layers beside the model nets', the 1-wide head with the MSE loss
    // epilogue on the targets' reward column, their dX and (own launch) dW + Adam
    for (int k = 0; h->srn && k < nm; ++k) {
        const size_t r0 = (size_t)k * mb;
        add_net("r" + std::to_string(k), 3, k, "ws.Hrf", "ws.Drf", 1, W("ws.Drf3"), 4, W("ws.Drf3"), 4, wr);
        GemmProb& p = f[Dr].back();
        p.mse = MSE_FIT;                                // N = 1: column 0 is the reward column
        p.se_raw = Tin + r0 * O + S; p.ldp = O; p.part = W("ws.lf") + (size_t)nm * mb * nt + r0;
        p.grad_scale = 1.f / (float)mb; p.fcoef = h->cfg.reward_loss_coef;
    }
    // the fit's own tile shapes (SACX_MTILE): its 2 x 200 rows want 16x16 forward / dX tiles
    // (832 workgroups at 512 wide, against 224 as 32x32) whatever the update's batch made
    // h->tile32; the dW + Adam launch takes 32x32 tiles when its 16x16 ones exceed one round of
    // residency (HC 2,372 -> 610 tiles), the rule of add_gemm at tile32 = 2.  2: the handle's.
    // Under mtile 1 a launch takes 32x32 tiles (tile32 = 2) where mt32 names it: bit 2 the hidden forward
    // levels (not inside the k_fwd2 pair), bit 8 the last level's heads + loss epilogue (MSE heads only),
    // bit 4 the heads' dX (+ k_mfinal's workgroup), bit 1 the other dX levels; dW + Adam always
    const GemmTiles fit16{h->mtile == 2 ? h->tile32 : 0, h->dwl}, fit32{2, h->dwl};
    auto tiles_if = [&](bool t32) { return h->mtile == 1 && t32 ? fit32 : fit16; };
    auto has_head = [](const std::vector<GemmProb>& ps) {
        for (const auto& p : ps)
            if (p.mse) return true;
        return false;
    };
    int n_fwd0 = 1;                                  // launches of level 0
    for (int i = 0; i <= Lf; ++i) {
        const std::string name = "model.fwd" + std::to_string(i);
        if (i == 0) {
            // the gather folded into layer 0's operand loads: one launch (gfold needs !srn, so f[0] holds
            // nm <= SACX_MAX_MODELS problems); otherwise, with the reward nets' layer 0 beside the models',
            // up to 2 nm problems, GEMM_MAXP to a launch as at every other level
            if (gfold) {
                add_gemm(h, plan, name, f[0], fit16);
                Launch& F = plan.back();
                set_rows(F, GR_GATHER);         // (16x16 tiles: a row is a whole record)
                F.gemm.mg = mg;
                F.name = "model.gather+fwd0";
                F.bytes += 4.0 * nm * mb * (2.0 * S + A + 1 + O);
            } else {
                n_fwd0 = add_gemm_split(h, plan, name, f[0], fit16);
            }
            continue;
        }
        const bool in_pair = i == 1 && (gfold || pre) && h->mfwd2 && S + A <= 32;
        const bool t32 = !has_head(f[i]) ? (h->mt32 & 2) && !in_pair : i == Lf && (h->mt32 & 8) && !h->gm && !h->srn;
        const size_t first = plan.size();
        const int n_lv = add_gemm_split(h, plan, name, f[i], tiles_if(t32));
        // fuse_fwd2 pairs the plan's last two launches: layer 0 and layer 1, each ONE launch (a split level
        // -- more than GEMM_MAXP nets, which is more than k_fwd2's 4 -- keeps its launches as they are)
        const bool pair01 = i == 1 && n_fwd0 == 1 && n_lv == 1;
        // the gathered layer 0 and layer 1 as ONE k_fwd2 launch (SACX_MFWD2, default; K0 = S + A <= 32)
        if (pair01 && gfold && h->mfwd2) fuse_fwd2(h, plan, "model.gather+fwd01");
        // or, pre-gathered, layer 0 (GR_PREGATHERED: H0 <= 512, plain A) and layer 1 the same way
        if (pair01 && pre && h->mfwd2 && h->mtile != 2 && S + A <= 32 && !h->wide) fuse_fwd2(h, plan, "model.fwd01", true);
        if (i == Lf && fuse)       // (every launch of a split last level: model.fwd<i>+loss, model.fwd<i>.1+loss)
            for (size_t j = std::min(first, plan.size() - 1); j < plan.size(); ++j) plan[j].name += "+loss";
    }
    if (!fuse) {
        Launch L{};
        L.kind = Launch::MLOSS;
        L.name = "model.loss";
        L.ml.S = S; L.ml.mb = mb; L.ml.nm = nm; L.ml.T = Tin; L.ml.O = Of; L.ml.D3 = Df3; L.ml.ldD = ldO;
        L.ml.loss_rows = W("ws.lf");
        L.ml.reward_coef = h->cfg.reward_loss_coef;
        L.grid = (nm * mb + 3) / 4;
        L.bytes = 4.0 * nm * mb * O * 3;
        plan.push_back(L);
    }
    MFinalArgs mf{};
    mf.ctl = h->ctl(); mf.loss_rows = W("ws.lf"); mf.mb = mb; mf.nm = nm;
    mf.mstats = W("mstats"); mf.mstats_cap = h->stats_cap; mf.nt = fuse ? nt : 0;
    if (h->srn) mf.nt2 = 1;            // the reward heads' partials follow the model heads' in ws.lf
    if (h->gm) {                       // the logstd gradient and Adam (or its store for the global-norm clip)
        mf.lgpart = W("ws.lgp"); mf.ntm = ntm; mf.S = S; mf.lscale = h->lscale ? 1 : 0;
        mf.gstore = h->cfg.model_max_grad_norm > 0.f ? 1 : 0;
        mf.logstd = W("m0.logstd");
        mf.lstride = nm > 1 ? (int64_t)(h->off_of("m1.logstd") - h->off_of("m0.logstd")) / 4 : 0;
        for (int k = 1; k < nm; ++k)      // (build_layout gives every model the same block)
            if ((int64_t)(h->off_of("m" + std::to_string(k) + ".logstd") - h->off_of("m0.logstd")) / 4 != k * mf.lstride) {
                fprintf(stderr, "sacx: model parameter blocks differ\n");
                abort();
            }
    }
    for (int t = 0; t < Lf; ++t) {
        const std::string name = "model.bwd" + std::to_string(Lf - t);
        if (t == Lf - 1 && bfold) {      // model.bwd2 folded: model.bwd1 generates its A operand
            add_gemm(h, plan, name, b[t], fit16);
            Launch& B1 = plan.back();
            B1.name = "model.bwd2+bwd1+final";
            set_rows(B1, GR_GEN_BWD2);      // (16x16 tiles)
            B1.gemm.has_mfinal = 1;
            B1.gemm.mfin = mf;
            for (const GemmProb& q : b[0]) { B1.flops += gemm_flops(q); B1.bytes += gemm_bytes(q); }
            continue;
        }
        if (t == 0 && bfold) continue;   // (in the launch above)
        const size_t first = plan.size();
        add_gemm_split(h, plan, name, b[t], tiles_if((h->mt32 & (t == 0 ? 4 : 1)) != 0));
        if (t == 0 && fuse) {
            Launch& B2 = plan[first];
            B2.name += "+final";
            B2.gemm.has_mfinal = 1;
            B2.gemm.mfin = mf;
        }
    }
    int n_adam = add_gemm_split(h, plan, "model.adam", w, tiles_if(true));
    for (int j = 0; j < n_adam; ++j) plan[plan.size() - 1 - j].gemm.t_adv = fuse ? 1 : 0;
    if (!wr.empty()) {
        const int nr = add_gemm_split(h, plan, "reward.adam", wr, tiles_if(true));
        for (int j = 0; j < nr; ++j) plan[plan.size() - 1 - j].gemm.t_adv = 1;
        n_adam += nr;
    }
    for (Launch& L : plan)           // GaussianModel fits: the head epilogue has the 16x16 form only
        if (L.kind == Launch::GEMM && L.gemm.t32)
            for (int i = 0; i < L.gemm.nprob; ++i)
                if (L.gemm.probs[i].mse & (MSE_GAUSS | MSE_NOREW)) {
                    fprintf(stderr, "sacx: GaussianModel / reward-net fit heads need 16x16 tiles\n");
                    abort();
                }
    if (h->cfg.model_max_grad_norm > 0.f) {
        // --model_max_grad_norm (mbrl_onpolicy_alg.py:315-317): the dW launches store the
        // gradients (+3 p_stride; GaussianModel's logstd gradient from mfit_final); their global
        // norm gives one scale; Adam applies g * scale over the models' whole contiguous range
        store_grads(plan, n_adam);
        for (int a = 0; a < n_adam; ++a) {
            Launch& G = plan[plan.size() - 1 - a];
            const size_t at = G.name.find(".adam");
            G.name = G.name.substr(0, at) + ".grad" + G.name.substr(at + 5);
        }
        std::string last = L_("m" + std::to_string(nm - 1), Dm);
        if (h->gm) last = "m" + std::to_string(nm - 1) + ".logstd";
        if (h->srn) last = L_("r" + std::to_string(nm - 1), Dr);
        const uint64_t o0 = h->off_of("m0.l0");
        const SegInfo& sl = h->seg(last);
        const int64_t n = (int64_t)((sl.off + (uint64_t)(sl.rows * sl.cols) * 4 - o0) / 4);
        float* P = h->f("m0.l0");
        Launch N{};
        N.kind = Launch::GNORM;
        N.name = "model.gnorm";
        N.gn.g = P + 3 * h->p_stride; N.gn.n = n;
        N.gn.part = W("ws.gnorm"); N.gn.scale_out = W("ws.gnorm") + GNORM_PARTS;
        N.gn.clip = (float)((double)h->cfg.model_max_grad_norm * nm);    // max_norm * self.B
        N.grid = GNORM_PARTS;
        N.bytes = 4.0 * n;
        plan.push_back(N);
        plan.push_back(adam_apply_launch(h, "model.adam", P, n, GRP_MODEL, N.gn.scale_out, fuse ? 1 : 0));
    }
    if (!fuse) {
        Launch L{};
        L.kind = Launch::MFINAL;
        L.name = "model.final";
        L.mf = mf;
        L.grid = 1;
        L.block = 64;
        plan.push_back(L);
    }
}

void enqueue(const Launch& L, sacx_handle* h, hipStream_t s) {
    switch (L.kind) {
        case Launch::RNG: launch_rng(L.rng, s); break;
        case Launch::GATHER: launch_gather(L.gather, s); break;
        case Launch::GEMM: launch_gemm(L.gemm, s); break;
        case Launch::AHEAD: launch_actor_head(L.head, L.fin, s); break;
        case Launch::QHEAD: launch_qhead(L.qh, s); break;
        case Launch::ABWD: launch_actor_bwd(L.ab, s); break;
        case Launch::FINAL: launch_alpha_final(L.fin, s); break;
        case Launch::MGATHER: launch_mgather(L.mg, s, L.pre_steps); break;
        case Launch::MLOSS: launch_mloss(L.ml, s); break;
        case Launch::MFINAL: launch_mfinal(L.mf, s); break;
        case Launch::ALLREDUCE:
            if (h->dp_local) break;            // sacx_dp_local_step reduces over the ranks' handles
            if (ncclAllReduce(L.ar_buf, L.ar_buf, (size_t)L.ar_count, ncclFloat32, ncclSum, h->comm, s) != ncclSuccess)
                h->nccl_failed = true;
            break;
        case Launch::APPLY: launch_adam_apply(L.ap, s); break;
        case Launch::AAPPLY: launch_alpha_apply(L.fin, s); break;
        case Launch::GNORM: launch_gnorm(L.gn, s); break;
        case Launch::LNORM: launch_ln(L.ln, s); break;
        case Launch::PPOGATHER: launch_ppo_gather(L.pg, s); break;
        case Launch::PPOHEAD: launch_ppo_head(L.ph, s); break;
        case Launch::GNPART: launch_gnorm_part(L.gn, s); break;
        case Launch::PPOFINAL: launch_ppo_final(L.pf, s); break;
        case Launch::VCGATHER: launch_vc_gather(L.vg, s); break;
        case Launch::VCHEAD: launch_vc_head(L.vh, s); break;
        case Launch::VCFINAL: launch_vc_final(L.vf, s); break;
        case Launch::VCADAM: launch_vc_adam(L.va, s); break;
        case Launch::TRIN: launch_trpo_in(L.ti, s); break;
        case Launch::TRTAN: launch_trpo_tan(L.tt, s); break;
        case Launch::TRHEAD: launch_trpo_head(L.th, s); break;
        case Launch::TRACC: launch_trpo_acc(L.ta, s); break;
        case Launch::TRCG: launch_trpo_cg(L.tc, s); break;
    }
}

// A fit step's launches as step j of a pre-gathered block (SACX_MPRE): the pointers into slot 0 of the
// staging (the rows mfit.Xs the first layers and the layer-0 dW read, the targets mfit.Ts of the loss)
// moved to slot j
Launch fit_step_launch(const sacx_handle* h, const Launch& L, int j) {
    Launch C = L;
    if (!h->mpre || j == 0) return C;
    const float* x0 = h->f("mfit.Xs");
    const float* t0 = h->f("mfit.Ts");
    const int64_t xs = h->seg("mfit.Xs").cols, ts = h->seg("mfit.Ts").cols;
    auto mv = [&](const float*& p) {
        if (p >= x0 && p < x0 + xs) p += (size_t)j * xs;
        else if (p >= t0 && p < t0 + ts) p += (size_t)j * ts;
    };
    if (C.kind == Launch::GEMM) {
        for (int i = 0; i < C.gemm.nprob; ++i) {
            mv(C.gemm.probs[i].A);
            mv(C.gemm.probs[i].se_raw);
        }
    } else if (C.kind == Launch::MLOSS) {
        mv(C.ml.T);
    }
    return C;
}

// The pre-gather of a block of n fit steps (none without SACX_MPRE)
void enqueue_fit_pre(sacx_handle* h, int n, hipStream_t s) {
    if (!h->mpre || h->mpres[h->sel].kind != Launch::MGATHER) return;
    Launch P = h->mpres[h->sel];
    P.pre_steps = n;
    enqueue(P, h, s);
}

// Rebuilds every bf16 weight shadow from the fp32 weights (all seeds): at each entry point that
// runs the update plans, so that parameter writes from the host reach the bf16 forward tiles
void wbf_refresh(sacx_handle* h, hipStream_t s) {
    if (!h->wbf_live || h->wbf_mats.empty()) return;
    WbfArgs a{};
    for (const auto& m : h->wbf_mats) {
        if (a.nmat == WBF_MAXM) break;
        a.W[a.nmat] = reinterpret_cast<const float*>(h->arena0 + h->off_of(m.name));
        a.S[a.nmat] = reinterpret_cast<uint16_t*>(h->arena0 + h->off_of("wbf." + m.name));
        a.K[a.nmat] = m.K;
        a.N[a.nmat] = m.N;
        ++a.nmat;
    }
    a.sstride = (int64_t)h->seed_bytes;
    a.nseeds = h->seeds;
    launch_wbf_refresh(a, s);
}

// the sampler + gather launches of a slot (the update's inputs)
bool is_prologue(const Launch& L) { return L.kind == Launch::RNG || L.kind == Launch::GATHER; }

void enqueue_step(sacx_handle* h, int slot, bool with_rng, hipStream_t s) {
    if (!with_rng)   // caller-provided randoms: perm of this update
        launch_set_pseq(h->ctl0(), slot, (int64_t)h->seed_bytes, h->seeds, s);
    for (const Launch& L : h->plan[slot]) {
        if (L.kind == Launch::RNG && !with_rng) continue;
        enqueue(L, h, s);
    }
}

// The main-stream launches of update `slot` with the alpha branch (alpha.fwd, alpha.head,
// alpha.final) of the PREVIOUS update (prev_slot >= 0) folded in:
//   alpha.fwd   -> extra problems of this update's actor forward launch(es);
//   alpha.head  -> an extra segment (rows from round4(Ra)) of this update's actor.head;
//   alpha.final -> one extra workgroup of the first GEMM after actor.head (q.fwd).
// Each folded piece computes exactly what it computed standalone (bit-identical results);
// the update's own alpha branch is left out (folded into the next update, or the tail).
// Returns false if the plans do not line up (then the caller keeps the branch separate).
bool merged_body(sacx_handle* h, int slot, int prev_slot, std::vector<Launch>& out) {
    out.clear();
    std::vector<const Launch*> pg;
    const Launch *ph = nullptr, *pf = nullptr, *pln = nullptr;
    if (prev_slot >= 0)
        for (const Launch& L : h->plan[prev_slot]) {
            if (!L.alpha_branch) continue;
            if (L.kind == Launch::GEMM) pg.push_back(&L);
            else if (L.kind == Launch::AHEAD) ph = &L;
            else if (L.kind == Launch::FINAL) pf = &L;
            else if (L.kind == Launch::LNORM) pln = &L;
        }
    size_t gi = 0;
    // (a plan without an alpha branch -- BC -- has nothing to fold: the body is the update itself)
    if (pg.empty() && !ph && !pf && !pln) prev_slot = -1;
    bool head_done = prev_slot < 0, final_done = prev_slot < 0, ln_done = pln == nullptr;
    bool afin_next = false;    // the split alpha finalisation still has its q.head half to place
    for (const Launch& L : h->plan[slot]) {
        if (is_prologue(L) || L.alpha_branch) continue;
        Launch C = L;
        if (prev_slot >= 0) {
            if (C.kind == Launch::GEMM && !head_done && gi < pg.size() && C.name.rfind("actor.fwd", 0) == 0) {
                if (!merge_gemm(C.gemm, pg[gi]->gemm)) return false;
                C.name += "+alpha";
                ++gi;
            } else if (C.kind == Launch::LNORM && !ln_done && C.ln.mode == 0) {
                // the previous update's alpha rows through the layer norm in the same launch
                C.ln.nrange = 2;
                C.ln.r[2] = pln->ln.r[0];
                C.ln.r[3] = pln->ln.r[1];
                C.grid += pln->grid;
                C.name += "+alpha";
                ln_done = true;
            } else if (!head_done && ph && (C.kind == Launch::AHEAD || (C.kind == Launch::GEMM && C.gemm.rowk == GR_ACTOR_HEAD))) {
                // the head rows: a standalone actor.head, or the rows folded into q.fwd0 (as a k_fwd2 pair:
                // GR_PAIR_HEAD, the same value)
                HeadArgs& a = C.kind == Launch::AHEAD ? C.head : C.gemm.head;
                const HeadSeg& sg = ph->head.seg[0];
                if (a.nseg >= 4) return false;
                const int r0 = (a.total_rows + 3) & ~3;
                HeadSeg m = sg;
                m.r0 = r0;
                m.r1 = r0 + (sg.r1 - sg.r0);
                a.seg[a.nseg++] = m;
                a.total_rows = m.r1;
                a.alpha_mode = 1;
                a.alpha_row0 = r0;
                if (C.kind == Launch::AHEAD) {
                    C.fin = ph->fin;
                } else {
                    C.gemm.hfin = ph->fin;
                    int rb = (a.total_rows + 3) / 4 - C.gemm.head_block0;
                    if (C.gemm.mode == GM_FWD2) {
                        // k_fwd2's head workgroups hold NW / 4 groups of 4 rows; the ticketed alpha
                        // path needs the alpha rows to start a workgroup (its group 0 initialises the
                        // ticket flags and no group of an alpha workgroup may take the early return)
                        if ((r0 / 4 - C.gemm.head_block0) % (SACX_FWD2_HEAD_NW / 4) != 0) return false;
                        rb = (rb + SACX_FWD2_HEAD_NW / 4 - 1) / (SACX_FWD2_HEAD_NW / 4);
                    }
                    C.grid += rb - C.gemm.row_blocks;
                    C.gemm.row_blocks = rb;
                }
                C.name += "+alpha";
                head_done = true;
                if (C.kind == Launch::GEMM && C.gemm.mode == GM_FWD2 && pf) {
                    // k_fwd2 has no later forward launch to take it.  Split (SACX_AFIN, default): its
                    // first alpha block snapshots the finalisation's operands and the next launch's
                    // target rows finish the alpha step; else the last alpha block finalises (ticket)
                    // (qhead_block reads the snapshot unrelocated, and FinalArgs::pre shares its slot with
                    // the data-parallel alpha_g: one seed, no data-parallel ranks)
                    const bool split = h->afin && h->seeds == 1 && h->dp_ranks == 0 && !h->dp_local;
                    C.gemm.has_final = split ? 2 : 1;
                    C.gemm.fin = pf->fin;
                    if (split) {
                        C.gemm.fin.pre = h->ptr<AfinPre>("ws.afin");
                        afin_next = true;
                    } else {
                        C.name += ".final";
                    }
                    final_done = true;
                }
            } else if (afin_next && C.kind == Launch::GEMM && C.gemm.mode == GM_DX && C.gemm.rowk == GR_QHEAD) {
                // q.head+critic.bwd1: every target row block finishes the previous update's alpha step
                C.gemm.fin = pf->fin;
                C.gemm.fin.pre = h->ptr<AfinPre>("ws.afin");
                C.name += "+alpha.final";
                afin_next = false;
            } else if (C.kind == Launch::GEMM && head_done && !final_done && pf &&
                       C.gemm.mode == GM_FWD) {
                C.gemm.has_final = 1;
                C.gemm.fin = pf->fin;
                C.name += "+alpha.final";
                final_done = true;
            }
        }
        out.push_back(C);
    }
    return gi == pg.size() && head_done && final_done && ln_done && !afin_next;
}

// Every captured graph of the handle: what body(cap_stream) hands to the capture stream, instantiated
// into *out.  The body returns non-zero to abort, having reported its error (fail).  The capture is
// ended and the captured graph destroyed on every path, so a failure leaves the stream usable for the
// next capture; every HIP failure is reported with its error text.  upload: the exec goes to the
// stream's device now, so the first replay does not pay for it; nodes: the captured graph's node count.
template <class F>
int capture_graph(sacx_handle* h, const char* what, F&& body, hipGraphExec_t* out, bool upload = false,
                  int64_t* nodes = nullptr) {
    hipStream_t cs = h->cap_stream;
    (void)hipGetLastError();              // (an earlier call's error is that call's: not this capture's)
    HIPCHK(h, hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int rc = body(cs);
    const hipError_t le = hipGetLastError();
    hipGraph_t graph = nullptr;
    const hipError_t ee = hipStreamEndCapture(cs, &graph);
    const bool captured = rc == 0 && le == hipSuccess && ee == hipSuccess;
    hipGraphExec_t ex = nullptr;
    hipError_t ie = hipSuccess;
    if (captured) {
        size_t nn = 0;
        if (nodes && hipGraphGetNodes(graph, nullptr, &nn) == hipSuccess) *nodes = (int64_t)nn;
        ie = hipGraphInstantiateWithFlags(&ex, graph, 0);
    }
    if (graph) (void)hipGraphDestroy(graph);
    if (rc) return -1;
    if (!captured) return fail(h, std::string(what) + " graph capture: " + hipGetErrorString(le != hipSuccess ? le : ee));
    if (ie != hipSuccess) return fail(h, std::string(what) + " graph instantiate: " + hipGetErrorString(ie));
    if (upload) {
        const hipError_t ue = hipGraphUpload(ex, h->stream);
        if (ue != hipSuccess) {
            (void)hipGraphExecDestroy(ex);
            return fail(h, std::string(what) + " graph upload: " + hipGetErrorString(ue));
        }
    }
    *out = ex;
    return 0;
}

// `n` back-to-back runs of a launch list as one graph (each run finds its inputs through a device-side
// counter: the index rings of the PPO / critic steps)
int capture_plan(sacx_handle* h, const char* what, const std::vector<Launch>& plan, int n, hipGraphExec_t* out) {
    return capture_graph(h, what, [&](hipStream_t cs) {
        for (int j = 0; j < n; ++j)
            for (const Launch& L : plan) enqueue(L, h, cs);
        return 0;
    }, out);
}

// n_steps minibatch steps of `plan` (the PPO actor step, the critic step), each reading its mb indices
// from the device's index ring [cap, ld] at its control block's step counter, which *seq_host mirrors:
// it advances with every step handed to the stream, so a failure midway leaves the two in step.  The
// ring is filled a chunk of at most cap steps at a time; a chunk replays as graphs of 64, 8 and 1
// back-to-back steps, cached in `graphs` by (mb, steps), or runs as plain launches (SACX_STEP_EAGER).
// Packed learners (seq_hosts holds more than one counter): `ring` is learner 0's, learner k's sits
// k * seed_bytes behind it and takes idx[k][n_steps][mb] at its own counter; `plan` then runs them all.
int run_ring_steps(sacx_handle* h, const std::vector<Launch>& plan, int32_t* ring, int ld, int64_t cap,
                   const std::vector<int64_t*>& seq_hosts, std::map<std::pair<int, int>, hipGraphExec_t>& graphs,
                   const char* what, const int32_t* idx, int64_t n_steps, int mb, int32_t flags) {
    for (int64_t done = 0; done < n_steps;) {
        const int64_t chunk = std::min<int64_t>(n_steps - done, cap);
        HIPCHK(h, hipStreamSynchronize(h->stream));   // ring rows of earlier chunks are consumed
        for (size_t k = 0; k < seq_hosts.size(); ++k) {
            int32_t* rk = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ring) + k * h->seed_bytes);
            const int32_t* ik = idx + (int64_t)k * n_steps * mb;
            // the chunk's rows are contiguous modulo the ring: at most two copies
            const int64_t s0 = *seq_hosts[k] % cap;
            const int64_t first = std::min<int64_t>(chunk, cap - s0);
            HIPCHK(h, hipMemcpy2D(rk + s0 * ld, sizeof(int32_t) * ld, ik + done * mb, sizeof(int32_t) * mb, sizeof(int32_t) * mb,
                                  (size_t)first, hipMemcpyHostToDevice));
            if (chunk > first)
                HIPCHK(h, hipMemcpy2D(rk, sizeof(int32_t) * ld, ik + (done + first) * mb, sizeof(int32_t) * mb,
                                      sizeof(int32_t) * mb, (size_t)(chunk - first), hipMemcpyHostToDevice));
        }
        if (flags & SACX_STEP_EAGER) {
            for (int64_t j = 0; j < chunk; ++j)
                for (const Launch& L : plan) enqueue(L, h, h->stream);
            for (int64_t* q : seq_hosts) *q += chunk;
            HIPCHK(h, hipGetLastError());
        } else {
            for (int64_t j = 0; j < chunk;) {
                const int n = chunk - j >= 64 ? 64 : chunk - j >= 8 ? 8 : 1;
                auto it = graphs.find({mb, n});
                if (it == graphs.end()) {
                    hipGraphExec_t ex = nullptr;
                    if (capture_plan(h, what, plan, n, &ex)) return -1;
                    it = graphs.emplace(std::make_pair(mb, n), ex).first;
                }
                HIPCHK(h, hipGraphLaunch(it->second, h->stream));
                for (int64_t* q : seq_hosts) *q += n;
                j += n;
            }
        }
        done += chunk;
    }
    return 0;
}

// Captured chain of G updates on two streams (see the fork branch below):
//   cs: the updates, alpha branches folded one update later (merged_body) + a tail;
//   rs: sampler + gather, two updates ahead (slot double buffer).
// skip_kind >= 0 leaves that launch kind out (measurement only: sacx_time_graph)
// kt (measurement only, uncached): every k_gemm launch gets its own per-workgroup timestamp
// slots in kt->base, recorded in kt->spans as (offset, workgroups).
struct KTimeMap {
    uint64_t* base = nullptr;
    int64_t cap = 0, used = 0;
    std::vector<std::pair<int64_t, int>> spans;
    std::vector<std::string> names;
    std::vector<char> is_gemm;
    std::vector<std::pair<int, int>> rowspan;   // [first, end) workgroups that run row kernels
    std::vector<std::vector<int>> cls;          // k_fwd2: first workgroup of each problem pair's tiles
    bool rows = false;      // also stamp the row kernels (k_actor_head, k_actor_bwd): dump only
};

// Sampler batches [s, e) of a G-update call (sampler_sched.h): sizes ramp 1, 2, 4, ... up to nbatch,
// never crossing a multiple of nbatch; a graph of kSamplerGrowMinG updates or more on a handle
// with the grown schedule (h->grow) ramps 1, 4, 16, ... up to h->grow instead (see chain_body)
std::vector<std::pair<int, int>> sampler_batches(const sacx_handle* h, int G) {
    if (h->grow > h->nbatch && G >= kSamplerGrowMinG) return sampler_batches_grown(G, h->grow);
    return sampler_batches_fixed(G, h->nbatch);
}

// what get_graph captures; the caller has created the 3 G + 1 events
int chain_body(sacx_handle* h, int G, bool with_rng, int skip_kind, KTimeMap* kt) {
    auto emit = [&](const Launch& L, hipStream_t st) {
        const bool timed = kt && (L.kind == Launch::GEMM || (kt->rows && (L.kind == Launch::AHEAD || L.kind == Launch::ABWD)));
        if (timed) {
            Launch C = L;
            // (a k_fwd2 launch finalises alpha in its last alpha block, not in a workgroup of its own)
            const int fin_wg = C.gemm.has_final && C.gemm.mode != GM_FWD2 ? 1 : 0;
            // a k_gemm launch's slots: its workgroups -- but the has_mfinal workgroup has none, and k_fwd2
            // numbers its 2-D grid's tiles and rows itself (f2_slot)
            const int nwg1 = L.kind == Launch::GEMM
                                 ? (C.gemm.mode != GM_FWD2 && !C.gemm.has_mfinal
                                        ? gemm_workgroups(C.gemm)
                                        : C.gemm.total_tiles + fin_wg + (C.gemm.rowk ? C.gemm.row_blocks : 0))
                                 : (L.kind == Launch::AHEAD ? (C.head.total_rows + 3) / 4 : C.grid);
            const int nwg = nwg1 * h->seeds;   // slots of every seed (seed-major)
            if (kt->used + 2 * nwg <= kt->cap) {
                uint64_t* p = kt->base + kt->used;
                if (L.kind == Launch::GEMM) C.gemm.ktime = p;
                else if (L.kind == Launch::AHEAD) C.head.ktime = p;
                else C.ab.ktime = p;
                kt->spans.push_back({kt->used, nwg});
                kt->names.push_back(C.name);
                kt->is_gemm.push_back(L.kind == Launch::GEMM);
                if (L.kind != Launch::GEMM) kt->rowspan.push_back({0, 0});
                else if (C.gemm.rowk == GR_ACTOR_HEAD)     // (in any mode: head rows run ahead of the tiles)
                    kt->rowspan.push_back({fin_wg, fin_wg + C.gemm.row_blocks});
                else kt->rowspan.push_back({C.gemm.total_tiles + fin_wg, nwg1});
                std::vector<int> cb;
                if (L.kind == Launch::GEMM && C.gemm.mode == GM_FWD2) {
                    const int nn = C.gemm.nprob / 2, r0 = C.gemm.rowk == GR_PAIR_HEAD ? C.gemm.row_blocks : 0;
                    for (int i = 0; i < nn; ++i) cb.push_back(r0 + C.gemm.probs[nn + i].tile_begin);
                }
                kt->cls.push_back(cb);
                kt->used += 2 * nwg;
            }
            enqueue(C, h, st);
        } else {
            enqueue(L, h, st);
        }
    };
    hipStream_t cs = h->cap_stream, rs = h->rng_stream;
    hipEvent_t* evR = h->events.data();          // inputs of update j ready
    hipEvent_t* evS = h->events.data() + G;      // update j's body done
    hipEvent_t* evF = h->events.data() + 2 * G;  // alpha.final of update j done
    hipEvent_t evFork = h->events[3 * G];
    if (with_rng) {
        // cs: the updates, each with the previous update's alpha branch folded into its first
        //     launches (merged_body), plus the last update's alpha branch as a tail;
        // rs: sampler + gather of update j+2 into slot (j+2)%3 == (j-1)%3, once update j's
        //     actor.head (the last reader of that slot, through the folded alpha rows) has run.
        const bool merge = h->dp_ranks == 0;   // the DP mode keeps each alpha branch as its own launches
        HIPCHK(h, hipEventRecord(evFork, cs));
        HIPCHK(h, hipStreamWaitEvent(rs, evFork, 0));
        // Sampler batches [s, e): one k_rng launch draws updates s..e-1 in stream order and one
        // gather fills their slots s % nslot .. s % nslot + (e - s) - 1 -- consecutive slots (the
        // kernels address slot + u), so a batch never crosses a multiple of the largest batch
        // (nslot is one).  Sizes ramp 1, 2, 4, ... up to nbatch (long graphs of a cheap sampler:
        // 1, 4, 16, 64, sampler_sched.h) so the first update of the graph waits
        // for one update's draws only.  Slot u%nslot is last read through update u's folded
        // alpha rows in update u+1's actor.head, so batch [s, e) is drawn after the actor.head
        // of update e-nslot, and must be done before update s.  When e <= nslot its slots are
        // fresh at graph start: their last reader is update e-1-nslot < 0 of an earlier graph
        // (update 0 folds no alpha rows), complete before this graph starts.
        const std::vector<std::pair<int, int>> batches = sampler_batches(h, G);
        const int nslot = h->nslot;
        for (int b = 0; b < (int)batches.size(); ++b) {
            const int s0 = batches[b].first, n = batches[b].second - s0;
            if ((b + 1 < (int)batches.size() && batches[b + 1].first != batches[b].second) || n < 1 ||
                s0 % nslot + n > nslot || (s0 > 0 && sampler_emit_after(batches[b], nslot) >= s0))
                return fail(h, "internal: sampler batches");
        }
        auto prologue = [&](int b) {
            const int j0 = batches[b].first, n = batches[b].second - j0;
            for (const Launch& L : h->plan[j0 % nslot]) {
                if (!is_prologue(L)) continue;
                if ((int)L.kind == skip_kind) continue;   // ablation of the sampler (stale randoms)
                Launch C = L;
                if (C.kind == Launch::RNG) {
                    C.rng.reset_seq = (b == 0);
                    C.rng.nupd = n;
                    // the segmented sampler (k_mtj_*) where the chain waits for the draw: the ramp's
                    // batches; the batches drawn ahead stay on k_rng's one CU, which the chain's
                    // launches never miss (the segmented launches take CUs: Humanoid bf16 -2 %)
                    if (b >= h->mtj_ramp) C.rng.jmin = INT32_MAX;
                } else {
                    C.gather.nupd = n;
                }
                enqueue(C, h, b == 0 && h->g_inline0 ? cs : rs);
            }
            return hipEventRecord(evR[b], b == 0 && h->g_inline0 ? cs : rs);
        };
        std::vector<int> batch_of(G, -1), emit_after(batches.size(), -1);
        for (int b = 0; b < (int)batches.size(); ++b) {
            batch_of[batches[b].first] = b;
            emit_after[b] = sampler_emit_after(batches[b], nslot);   // <= 0: slots fresh at graph start
        }
        for (int b = 0; b < (int)batches.size(); ++b)
            if (emit_after[b] <= 0) {
                HIPCHK(h, prologue(b));
                emit_after[b] = -1;                             // drawn once: not again after update 0
                // batch 0 on the chain's stream (g_inline0): the side stream's draws continue after it
                if (b == 0 && h->g_inline0) HIPCHK(h, hipStreamWaitEvent(rs, evR[0], 0));
            }
        std::vector<Launch> body;
        for (int j = 0; j < G; ++j) {
            if (batch_of[j] >= 0) HIPCHK(h, hipStreamWaitEvent(cs, evR[batch_of[j]], 0));
            const int slot = j % nslot, prev = j > 0 ? (j - 1) % nslot : -1;
            const bool folded = merge && merged_body(h, slot, prev, body);
            if (!folded) {                    // plain order: previous alpha branch, then this body
                body.clear();
                if (prev >= 0)
                    for (const Launch& L : h->plan[prev])
                        if (L.alpha_branch) body.push_back(L);
                for (const Launch& L : h->plan[slot])
                    if (!is_prologue(L) && !L.alpha_branch) body.push_back(L);
            }
            std::vector<int> due;               // batches whose slots this update's actor.head frees
            for (int b = 0; b < (int)batches.size(); ++b)
                if (emit_after[b] == j) due.push_back(b);
            bool recorded = false;
            bool afin_skipped = false;          // ablation: the split finalisation's snapshot was never taken
            for (const Launch& L : body) {
                if ((int)L.kind == skip_kind) {
                    // ablation: the alpha.final folded into a skipped GEMM still runs
                    if (L.kind == Launch::GEMM && L.gemm.has_final) {
                        FinalArgs f = L.gemm.fin;
                        f.pre = nullptr;                 // (the split form's snapshot: finalise in place)
                        launch_alpha_final(f, cs);
                        afin_skipped = afin_skipped || L.gemm.has_final == 2;
                    }
                    continue;
                }
                if (afin_skipped && L.kind == Launch::GEMM && L.gemm.rowk == GR_QHEAD && L.gemm.fin.pre != nullptr) {
                    Launch C = L;                        // its q.head half: alpha is already final in place
                    C.gemm.fin.pre = nullptr;
                    afin_skipped = false;
                    emit(C, cs);
                    continue;
                }
                emit(L, cs);
                if (!due.empty() && !recorded && L.frees_slot) {
                    HIPCHK(h, hipEventRecord(evS[j], cs));
                    recorded = true;
                }
            }
            if (!due.empty()) {
                if (!recorded) HIPCHK(h, hipEventRecord(evS[j], cs));
                HIPCHK(h, hipStreamWaitEvent(rs, evS[j], 0));
                for (int b : due) HIPCHK(h, prologue(b));
            }
        }
        for (const Launch& L : h->plan[(G - 1) % nslot])   // tail: the last update's alpha branch
            if (L.alpha_branch && (int)L.kind != skip_kind) emit(L, cs);
        HIPCHK(h, hipEventRecord(evF[0], rs));
        HIPCHK(h, hipStreamWaitEvent(cs, evF[0], 0));    // join the sampler stream
    } else {
        if (skip_kind >= 0) return fail(h, "kernel ablation needs the forked sampler graph");
        for (int j = 0; j < G; ++j) enqueue_step(h, 0, with_rng, cs);
    }
    return 0;
}

// the SAC update graphs live in h->graphs: a key's graph, captured (and uploaded) on its first use
template <class F>
int cached_graph(sacx_handle* h, const std::tuple<int, int, int>& key, const char* what, F&& body, hipGraphExec_t* out) {
    auto it = h->graphs.find(key);
    if (it == h->graphs.end()) {
        hipGraphExec_t exec = nullptr;
        if (capture_graph(h, what, body, &exec, true)) return -1;
        it = h->graphs.emplace(key, exec).first;
    }
    *out = it->second;
    return 0;
}

int get_graph(sacx_handle* h, int G, bool with_rng, hipGraphExec_t* out, int skip_kind = -1,
              KTimeMap* kt = nullptr) {
    for (int i = (int)h->events.size(); i < 3 * G + 1; ++i) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->events.push_back(e);
    }
    auto body = [&](hipStream_t) { return chain_body(h, G, with_rng, skip_kind, kt); };
    if (kt) return capture_graph(h, "update", body, out, true);      // measurement only: uncached
    return cached_graph(h, std::make_tuple(G, with_rng ? 1 : 0, skip_kind), "update", body, out);
}

// The one-update graphs of the drop-in loop's speculative path: gather + update of slot `slot`
// (1 or 2), reading the randoms the speculative k_rng drew there -- not slot 0, so that slot 0
// keeps the randoms of the last update a caller observed: a cancelled draw leaves no trace in it
// -- with the alpha branch of the previous speculative update (slot `prev`, -1: none) folded in
// and the update's own alpha branch left out (deferred to the next one, or to settle()).
int get_spec_graph(sacx_handle* h, int slot, int prev, hipGraphExec_t* out) {
    const auto key = std::make_tuple(-1, 64 * slot + (prev + 1), -1);   // < 0: never a get_graph key
    return cached_graph(h, key, "speculative update", [&](hipStream_t cs) -> int {
        if (h->nslot <= slot || h->plan[slot].empty()) return fail(h, "internal: no spare slot for the speculative draw");
        std::vector<Launch> body;
        if (!merged_body(h, slot, prev, body)) {   // plans that do not fold: the branch, then the body
            std::vector<Launch> own;
            if (!merged_body(h, slot, -1, own)) return fail(h, "internal: speculative update body");
            body.clear();
            for (const Launch& L : h->plan[prev])
                if (L.alpha_branch) body.push_back(L);
            body.insert(body.end(), own.begin(), own.end());
        }
        if (h->cfg.use_expert)                     // plain SAC: the speculative draw gathered too
            for (const Launch& L : h->plan[slot])  // (the draw stamped pseq[slot] itself)
                if (L.kind == Launch::GATHER) enqueue(L, h, cs);
        for (const Launch& L : body) enqueue(L, h, cs);
        return 0;
    }, out);
}

// Single-stream segments (round 4).  A graph that forks the sampler onto a second stream pays
// two runtime costs the update chain does not: its host launch takes ~0.55 ms for 20 updates
// (0.12-0.31 ms for a single-stream graph of the same chain), and its FIRST replay takes
// ~0.17 ms longer on the device than later ones (a single-stream graph shows no such penalty;
// r04_first_replay_v1.txt, r04_single_stream_v1.txt).  A call of n <= nslot updates draws every
// input at its start anyway (all its slots are fresh), so it needs no dependency from the chain to
// the sampler: the sampler batches run as plain launches on the side stream, and the chain as one
// single-stream graph per batch segment [s, e), each behind its batch's event.  Segment graphs
// carry exactly the fork / join graph's main-stream launches: the previous segment's last alpha
// branch folded into their first update (merged_body), the call's last segment ending with the
// tail; so the results are bit-identical.  Keyed by (first slot, length, folds a previous
// branch, ends the call).
int get_seg_graph(sacx_handle* h, int s0, int n, bool has_prev, bool is_last, hipGraphExec_t* out) {
    const int nslot = h->nslot;
    // (first element -4: get_graph's keys start with G > 0, so a segment never replays a G-update graph)
    const auto key = std::make_tuple(-4, (s0 % nslot) * 1024 + n, (has_prev ? 2 : 0) + (is_last ? 1 : 0));
    return cached_graph(h, key, "segment", [&](hipStream_t cs) -> int {
        std::vector<Launch> body;
        for (int j = s0; j < s0 + n; ++j) {
            const int slot = j % nslot, prev = (j > s0 || has_prev) ? (j - 1 + nslot) % nslot : -1;
            if (!merged_body(h, slot, prev, body)) return fail(h, "internal: segment body");
            for (const Launch& L : body) enqueue(L, h, cs);
        }
        if (is_last)
            for (const Launch& L : h->plan[(s0 + n - 1) % nslot])
                if (L.alpha_branch) enqueue(L, h, cs);
        return 0;
    }, out);
}

constexpr int kSegMaxN = 32;

// whether step(n) takes the single-stream segments (SACX_SEGMENTS, default on)
// (2: every call, the mid-call sampler batches behind the end of the segment holding the update
// that frees their slots)
bool use_segments(const sacx_handle* h, int64_t n, int32_t flags) {
    const char* e = std::getenv("SACX_SEGMENTS");
    const int env = e ? std::atoi(e) : 1;
    // n = 1 keeps its fork / join graph: 115 vs 134 us per warm call (r04_segments_by_n_v1.txt;
    // from n = 2 on the segments win, 202 vs 209 us, 1,316 vs 1,375 us at n = 20)
    const int nmin = std::getenv("SACX_SEG_NMIN") ? std::atoi(std::getenv("SACX_SEG_NMIN")) : 2;
    // (short = at most kSegMaxN updates, whatever the ring: the 128-slot ring would hold longer calls,
    // but those keep their fork / join graph, measured only up to 32 updates as segments)
    return env != 0 && flags == 0 && h->dp_ranks == 0 && !h->dp_local && n >= nmin &&
           (n <= std::min(h->nslot, kSegMaxN) || (env == 2 && n <= (int64_t)1 << 24));
}

// The segments of step(n): every segment graph instantiated (prepare), or also launched (run):
// sampler batches as plain launches on the side stream, each segment behind its batch
// The sampler batches of a segmented call (n <= nslot: every slot fresh, all drawn at the call's
// start).  With the one-workgroup k_rng alone, sizes grow 1, 4, 16, ... (SACX_SEG_GROW, 0: the graphs'
// ramp 1, 2, 4, 8 aligned to nbatch): each batch still lands before its first update (a batch of k
// updates draws in ~1.5 + 11.5 k us against 61 us per update at HC), and the call has fewer segments,
// so fewer cross-stream waits and graph launches (20 updates: 3 segments instead of 6)
std::vector<std::pair<int, int>> segment_batches(const sacx_handle* h, int n) {
    static const int grow = [] { const char* e = std::getenv("SACX_SEG_GROW"); return e ? std::atoi(e) : 4; }();
    if (grow < 2 || h->rng_jump || h->rng_split || n > std::min(h->nslot, kSegMaxN))
        return sampler_batches_fixed(n, h->nbatch);
    std::vector<std::pair<int, int>> batches;
    for (int s0 = 0, sz = 1; s0 < n; sz *= grow) {
        const int k = std::min(sz, n - s0);
        batches.push_back({s0, s0 + k});
        s0 += k;
    }
    return batches;
}

// SACX_SEG_INLINE0 (default 1): batch 0 of a segmented call drawn on the bound stream
static int seg_inline0() {
    static const int v = [] { const char* e = std::getenv("SACX_SEG_INLINE0"); return e ? std::atoi(e) : 1; }();
    return v;
}

int run_segments(sacx_handle* h, int n, bool run) {
    const auto batches = segment_batches(h, n);
    const int nb = (int)batches.size(), nslot = h->nslot;
    // segment k = batch k; batch b is drawn at the start when its slots are fresh (e <= nslot),
    // else behind the end of the segment holding update e - nslot (the one that frees them)
    std::vector<int> due_seg(nb, -1);
    for (int b = 0, k = 0; b < nb; ++b) {
        const int u = batches[b].second - nslot;
        if (u <= 0) continue;
        while (batches[k].second <= u) ++k;
        due_seg[b] = k;
    }
    std::vector<hipGraphExec_t> gx(nb);
    for (int b = 0; b < nb; ++b)
        if (get_seg_graph(h, batches[b].first, batches[b].second - batches[b].first, b > 0, b + 1 == nb, &gx[b]))
            return -1;
    if (!run) return 0;
    const int nev = 2 * nb + 1;
    for (int i = (int)h->events.size(); i < nev; ++i) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->events.push_back(e);
    }
    hipEvent_t* evR = h->events.data();          // batch b drawn
    hipEvent_t* evE = h->events.data() + nb;     // segment k done
    hipStream_t rs = h->rng_stream;
    const int first_inline = seg_inline0();
    const int sig = h->seg_sig;
    if (sig && !h->sig_mem[0]) {
        int dev = 0, can = 0;
        HIPCHK(h, hipGetDevice(&dev));
        if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, dev) != hipSuccess || !can) {
            h->seg_sig = 0;
            return run_segments(h, n, run);
        }
        for (int w = 0; w < 2; ++w) {
            HIPCHK(h, hipExtMallocWithFlags((void**)&h->sig_mem[w], sizeof(uint64_t), hipMallocSignalMemory));
            HIPCHK(h, hipStreamWriteValue64(h->stream, h->sig_mem[w], 0, 0));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    const uint64_t base0 = h->sig_seq[0];
    auto draw = [&](int b, hipStream_t st) {
        const int j0 = batches[b].first, n_b = batches[b].second - j0;
        for (const Launch& L : h->plan[j0 % nslot]) {
            if (!is_prologue(L)) continue;
            Launch C = L;
            if (C.kind == Launch::RNG) {
                C.rng.reset_seq = (b == 0);
                C.rng.nupd = n_b;
            } else {
                C.gather.nupd = n_b;
            }
            enqueue(C, h, st);
        }
        if (sig == 0 || (b == 0 && st == h->stream && sig < 2)) return hipEventRecord(evR[b], st);
        const int w = st == h->stream ? 1 : 0;
        const hipError_t e = hipStreamWriteValue64(st, h->sig_mem[w], h->sig_seq[w] + 1, 0);
        if (e == hipSuccess) ++h->sig_seq[w];   // (the waits count on every queued write)
        return e;
    };
    auto wait_batch = [&](hipStream_t st, int b) {   // st waits for batch b's draw
        if (sig == 0 || (b == 0 && st == rs && sig < 2)) return hipStreamWaitEvent(st, evR[b], 0);
        // batch b's value: batch 0 (bound stream) is the one write of sig_mem[1] this call; side
        // stream batch b the (b - first)-th write of sig_mem[0] after this call's base
        const int w = b == 0 && first_inline ? 1 : 0;
        const uint64_t v = w ? h->sig_seq[1] : base0 + (uint64_t)(b - (first_inline ? 1 : 0)) + 1;
        return hipStreamWaitValue64(st, h->sig_mem[w], v, hipStreamWaitValueGte, ~0ull);
    };
    // the sampler follows the bound stream's earlier work but not this call's k_set_ctl (it writes
    // num_timesteps / ts_increment, which the sampler does not read): sacx_sac_step recorded
    // seg_start before launching it
    // SACX_SEG_INLINE0 (default 1): warm step(20) 1,296 vs 1,320 us, the driver's command +0.3 %
    // (r04_seg_inline0_v1.txt)
    if (first_inline) {
        // batch 0 on the bound stream itself, right before segment 0: no cross-stream hop on the
        // call's critical path; the side stream continues the draws after it
        HIPCHK(h, draw(0, h->stream));
        HIPCHK(h, wait_batch(rs, 0));
    } else {
        HIPCHK(h, hipStreamWaitEvent(rs, h->seg_start, 0));
    }
    for (int b = first_inline ? 1 : 0; b < nb; ++b)
        if (due_seg[b] < 0) HIPCHK(h, draw(b, rs));
    for (int k = 0; k < nb; ++k) {
        if (k > 0 || !first_inline) HIPCHK(h, wait_batch(h->stream, k));
        HIPCHK(h, hipGraphLaunch(gx[k], h->stream));
        bool rec = false;
        for (int b = 0; b < nb; ++b)
            if (due_seg[b] == k) {
                if (!rec) {
                    if (sig >= 2) {     // segment k done, as a write on the bound stream
                        HIPCHK(h, hipStreamWriteValue64(h->stream, h->sig_mem[1], h->sig_seq[1] + 1, 0));
                        ++h->sig_seq[1];
                        HIPCHK(h, hipStreamWaitValue64(rs, h->sig_mem[1], h->sig_seq[1], hipStreamWaitValueGte, ~0ull));
                    } else {
                        HIPCHK(h, hipEventRecord(evE[k], h->stream));
                        HIPCHK(h, hipStreamWaitEvent(rs, evE[k], 0));
                    }
                    rec = true;
                }
                HIPCHK(h, draw(b, rs));
            }
    }
    return 0;
}

// the deferred append, queued now (sacx_handle::app_defer)
// An append whose source rows are the pinned staging buffer: its workgroups (one per seed) bump
// done_host[1] once they have read them, and the next staging reuse polls that count (stage_begin)
// instead of waiting for an event marker recorded behind the launch (SACX_APP_CTR)
static int launch_staged_append(sacx_handle* h, AppendArgs g) {
    if (h->app_ctr) {
        g.done = h->done_dev + 1;
        launch_append(g, h->stream);
        if (hipGetLastError() != hipSuccess) return fail(h, "append launch");
        h->app_seq += (uint32_t)(g.nseeds > 1 ? g.nseeds : 1);
        h->app_ctr_pending = true;
        return 0;
    }
    launch_append(g, h->stream);
    if (hipGetLastError() != hipSuccess || hipEventRecord(h->pin_ev, h->stream) != hipSuccess)
        return fail(h, "append launch");
    h->pin_pending = true;
    return 0;
}

int flush_append(sacx_handle* h) {
    if (!h->app_pending) return 0;
    h->app_pending = false;
    return launch_staged_append(h, h->app_args);
}

// Queues a held append, runs a deferred alpha branch (the tail a one-update graph would have ended
// with), then undoes a queued speculative draw: the state every entry point but act / append / the
// speculative step(1) starts from.
int settle(sacx_handle* h, bool keep_rng_state = false) {
    if (flush_append(h)) return -1;
    h->ctl_known = false;
    if (h->alpha_pending >= 0) {
        const int slot = h->alpha_pending;
        h->alpha_pending = -1;
        for (const Launch& L : h->plan[slot])
            if (L.alpha_branch) enqueue(L, h, h->stream);
        HIPCHK(h, hipGetLastError());
    }
    return spec_cancel(h, keep_rng_state);
}

// The graphs sacx_sac_step(n_steps) replays: n_steps / G full graphs of G updates, then the
// remainder as ONE graph of exactly r updates (each graph pays its own sampler start-up and
// alpha tail, so one remainder graph beats a chain of power-of-two pieces).  Up to
// kMaxRemGraphs distinct remainder sizes are cached; beyond that a new remainder is split
// into cached powers of two.  The returned list is what sacx_sac_step launches and what
// sacx_prepare instantiates ahead of time.
constexpr int kMaxRemGraphs = 24;

int step_graph_list(sacx_handle* h, int64_t n_steps, bool ext, std::vector<std::pair<hipGraphExec_t, int64_t>>* out) {
    out->clear();
    const int G = ext ? 1 : h->graph_steps;
    const int64_t q = n_steps / G;
    int64_t r = n_steps % G;
    if (q > 0) {
        hipGraphExec_t g;
        if (get_graph(h, G, !ext, &g)) return -1;
        out->push_back({g, q});
    }
    if (r == 0) return 0;
    int n_rem = 0;
    for (const auto& kv : h->graphs)
        if (std::get<0>(kv.first) > 0 && std::get<0>(kv.first) != h->graph_steps && std::get<2>(kv.first) < 0) ++n_rem;
    const bool exact = h->graphs.count(std::make_tuple((int)r, ext ? 0 : 1, -1)) > 0 || n_rem < kMaxRemGraphs;
    if (exact) {
        hipGraphExec_t g;
        if (get_graph(h, (int)r, !ext, &g)) return -1;
        out->push_back({g, 1});
        return 0;
    }
    for (int p = 1 << 30; r > 0 && p >= 1; p >>= 1) {
        if (p > r) continue;
        hipGraphExec_t g;
        if (get_graph(h, p, !ext, &g)) return -1;
        out->push_back({g, 1});
        r -= p;
    }
    return 0;
}

}  // namespace

// ============================================================================ C ABI
extern "C" {

int sacx_create(const sacx_config* cfg, sacx_handle** out) {
    g_create_error.clear();
    if (!cfg || !out) {
        g_create_error = "null argument";
        return -1;
    }
    auto bad = [&](const char* m) {
        g_create_error = m;
        return -2;
    };
    if (cfg->abi_version != SACX_ABI_VERSION) return bad("abi_version mismatch");
    if (cfg->seeds < 0 || cfg->seeds > 64) return bad("seeds must be in [0, 64]");
    if (cfg->s_dim <= 0 || cfg->a_dim <= 0 || cfg->a_dim > 32) return bad("s_dim/a_dim out of range (a_dim <= 32)");
    if (cfg->activation < 0 || cfg->activation > 2) return bad("activation must be relu/tanh/elu");
    if (cfg->batch <= 0 || cfg->buffer_capacity <= 0) return bad("batch/buffer_capacity must be positive");
    if (cfg->buffer_capacity >= (int64_t(1) << 31)) return bad("buffer_capacity must be < 2^31");
    if (cfg->num_models < 0 || cfg->num_models > SACX_MAX_MODELS) return bad("num_models must be in [1, 8] (0 -> 2)");
    if (cfg->use_expert < SACX_EXPERT_OFF || cfg->use_expert > SACX_EXPERT_MODELS)
        return bad("use_expert must be SACX_EXPERT_OFF, SACX_EXPERT_EO, SACX_EXPERT_BC or SACX_EXPERT_MODELS");
    const bool models_only = cfg->use_expert == SACX_EXPERT_MODELS;
    if (models_only && cfg->actor_gaussian != SACX_ACTOR_GAUSSIAN_TRAIN)
        return bad("use_expert = SACX_EXPERT_MODELS (world models without an expert term) goes with "
                   "actor_gaussian = SACX_ACTOR_GAUSSIAN_TRAIN only");
    if (cfg->use_expert == SACX_EXPERT_BC) {
        if (cfg->gemm_bf16) return bad("BC (use_expert = SACX_EXPERT_BC) runs fp32 only (gemm_bf16 = 0)");
        if (cfg->seeds > 1) return bad("BC (use_expert = SACX_EXPERT_BC) runs one learner per handle (seeds <= 1)");
        if (cfg->actor_gaussian) return bad("BC (use_expert = SACX_EXPERT_BC) trains the squashed actor");
    }
    if (cfg->actor_gaussian < 0 || cfg->actor_gaussian > SACX_ACTOR_GAUSSIAN_TRAIN)
        return bad("actor_gaussian must be SACX_ACTOR_SQUASHED, SACX_ACTOR_GAUSSIAN or SACX_ACTOR_GAUSSIAN_TRAIN");
    if (cfg->actor_gaussian == SACX_ACTOR_GAUSSIAN_TRAIN) {
        if (cfg->actor_output_norm)
            return bad("trainable GaussianActor (SACX_ACTOR_GAUSSIAN_TRAIN): actor_output_norm has no backward (set it to 0)");
        if (cfg->gemm_bf16) return bad("trainable GaussianActor (SACX_ACTOR_GAUSSIAN_TRAIN) runs fp32 only (gemm_bf16 = 0)");
        if (cfg->seeds > 1)
            return bad("trainable GaussianActor (SACX_ACTOR_GAUSSIAN_TRAIN) runs one learner per handle (seeds <= 1)");
        if (cfg->use_expert && !models_only)
            return bad("trainable GaussianActor (SACX_ACTOR_GAUSSIAN_TRAIN): use_expert must be SACX_EXPERT_OFF "
                       "or SACX_EXPERT_MODELS (the expert_reg branch of the PPO step is not built)");
        if (cfg->buffer_capacity > (int64_t(1) << 24))
            return bad("trainable GaussianActor (SACX_ACTOR_GAUSSIAN_TRAIN): buffer_capacity (rollout rows) must be <= 2^24");
    }
    if (cfg->use_expert) {
        const int nmc = cfg->num_models > 0 ? cfg->num_models : 2;
        if (!models_only) {               // (SACX_EXPERT_MODELS: no expert rows, expert_batch / expert_capacity unused)
            if (cfg->expert_batch <= 0) return bad("expert_batch must be positive");
            // the expert term adds model 0's and model 1's rows elementwise (SAC_expert.py:329-332): the
            // first two sections of np.array_split(perm, num_models) must hold the same number of rows
            if (nmc == 2 && (cfg->expert_batch & 1))
                return bad("expert_batch must be even with 2 models (SAC_expert.py:329-332 adds equal halves)");
            if (nmc > 2 && cfg->expert_batch % nmc == 1)
                return bad("expert_batch % num_models == 1: the two array_split sections of the expert term differ in length");
            if (nmc >= 2 && cfg->expert_batch < nmc) return bad("expert_batch < num_models");
            if (cfg->expert_capacity < cfg->expert_batch) return bad("expert_capacity < expert_batch");
        }
        if (cfg->model_activation < 0 || cfg->model_activation > 2) return bad("model activation invalid");
        if (cfg->s_dim + 1 > 512) return bad("s_dim > 511 unsupported by the model MSE head");
    }
    for (int n = 0; n < 4; ++n)
        if (cfg->net_depth[n] < 0 || cfg->net_depth[n] > SACX_MAX_DEPTH) return bad("net_depth must be in [0, 4]");
    if (cfg->act_per_layer)
        for (int n = 0; n < 3; ++n)
            for (int l = 0; l < 2; ++l)
                if (cfg->act_layers[n][l] < 0 || cfg->act_layers[n][l] > 2) return bad("act_layers must be relu/tanh/elu");
    // every net's hidden layers: the ABI-8 lists, or the two of the older fields
    NetDims nd[4];
    bool wide = false;      // a used net has a hidden layer above 512
    {
        const int leg_w[4][2] = {{cfg->hidden[0], cfg->hidden[1]},
                                 {cfg->critic_hidden[0] > 0 ? cfg->critic_hidden[0] : cfg->hidden[0],
                                  cfg->critic_hidden[1] > 0 ? cfg->critic_hidden[1] : cfg->hidden[1]},
                                 {cfg->model_hidden[0], cfg->model_hidden[1]},
                                 {cfg->reward_hidden[0] > 0 ? cfg->reward_hidden[0] : 512,
                                  cfg->reward_hidden[1] > 0 ? cfg->reward_hidden[1] : 512}};
        for (int n = 0; n < 4; ++n) {
            if (cfg->net_depth[n] > 0) {
                for (int l = 0; l < cfg->net_depth[n]; ++l) {
                    nd[n].h.push_back(cfg->net_hidden[n][l]);
                    nd[n].act.push_back(cfg->net_acts[n][l]);
                }
                continue;
            }
            for (int l = 0; l < 2; ++l) {
                nd[n].h.push_back(leg_w[n][l]);
                int a = n == 3 ? cfg->reward_act_layers[l]
                               : cfg->act_per_layer ? cfg->act_layers[n][l] : (n == 2 ? cfg->model_activation : cfg->activation);
                nd[n].act.push_back(a);
            }
        }
        const bool used[4] = {true, true, cfg->use_expert != 0, cfg->use_expert && cfg->separate_reward_nn};
        for (int n = 0; n < 4; ++n) {
            if (!used[n]) continue;
            for (int l = 0; l < nd[n].D(); ++l) {
                if (nd[n].h[l] <= 0 || nd[n].h[l] > SACX_MAX_WIDTH)
                    return bad("hidden sizes must be in [1, 1024] (SACX_MAX_WIDTH: the row kernels walk a row in at "
                               "most two 512-column slabs)");
                static_assert(SACX_MAX_WIDTH == 1024, "the message above and k_sac.hip's WIDEQ name the bound");
                wide = wide || nd[n].h[l] > 512;
                if (nd[n].act[l] < 0 || nd[n].act[l] > 2) return bad("activations must be relu/tanh/elu");
            }
        }
    }
    if (cfg->actor_gaussian && cfg->actor_std_mult < 0.f) return bad("actor_std_mult must be positive");
    auto* h = new sacx_handle();
    h->cfg = *cfg;
    h->S = cfg->s_dim;
    h->A = cfg->a_dim;
    for (int n = 0; n < 4; ++n) h->nd[n] = nd[n];
    // the first and the last hidden layer of each net (one layer: both the same)
    h->H0 = nd[0].h.front();
    h->H1 = nd[0].h.back();
    h->Hc0 = nd[1].h.front();   // --critic_layers (nn_utils.py:86-138)
    h->Hc1 = nd[1].h.back();
    h->B = cfg->batch;
    h->cap = cfg->buffer_capacity;
    h->aact[0] = nd[0].act.front(); h->aact[1] = nd[0].act.back();
    h->cact[0] = nd[1].act.front(); h->cact[1] = nd[1].act.back();
    h->macts[0] = nd[2].act.front(); h->macts[1] = nd[2].act.back();
    h->Aout = cfg->per_state_std ? 2 * h->A : h->A;
    h->nm = cfg->use_expert ? (cfg->num_models > 0 ? cfg->num_models : 2) : 0;
    h->ne_perm = cfg->use_expert && !models_only ? cfg->expert_batch : 0;
    // the update's expert rows: every row with one model, else the first two array_split sections
    // (each ceil(ne / nm) rows here: their lengths agree, checked above)
    h->ne = h->nm <= 1 ? h->ne_perm : 2 * ((h->ne_perm + h->nm - 1) / h->nm);
    h->ecap = cfg->use_expert && !models_only ? cfg->expert_capacity : 0;
    h->models_only = models_only;
    h->Hm0 = cfg->use_expert ? nd[2].h.front() : 0;
    h->Hm1 = cfg->use_expert ? nd[2].h.back() : 0;
    h->gm = cfg->use_expert && cfg->gaussian_model;
    h->lscale = h->gm && cfg->scale_model_loss;
    h->srn = cfg->use_expert && cfg->separate_reward_nn;
    h->Om = h->srn ? h->S : h->S + 1;
    if (h->srn) {
        h->Hr0 = nd[3].h.front();
        h->Hr1 = nd[3].h.back();
        h->racts[0] = nd[3].act.front();
        h->racts[1] = nd[3].act.back();
    }
    // the fused plans are built for two hidden layers per net; any other depth takes the generic
    // plans (SACX_GENERIC=1 forces them at two layers too: their parity test)
    h->deep = nd[0].D() != 2 || nd[1].D() != 2 || (cfg->use_expert && nd[2].D() != 2) || (h->srn && nd[3].D() != 2);
    // a layer wider than 512 does too: the fused plans' row kernels and folds hold a row in 8
    // registers per lane, the generic plans' heads have the slab-walking wide variants
    h->wide = wide;
    h->deep = h->deep || wide;
    if (const char* e = std::getenv("SACX_GENERIC")) h->deep = h->deep || std::atoi(e) != 0;
    h->bc = cfg->use_expert == SACX_EXPERT_BC;
    h->mb = cfg->use_expert ? (cfg->model_batch > 0 ? cfg->model_batch : 200) : 0;
    h->ln = cfg->actor_layer_norm != 0;
    h->ppo = cfg->actor_gaussian == SACX_ACTOR_GAUSSIAN_TRAIN;
    h->ldS = (int)r4(h->S);
    h->ldQ = (int)r4(h->S + h->A);
    h->stride = (int)r4(2 * h->S + h->A + 2);
    h->Ra = 2 * h->B + h->ne;
    h->Rb = h->B + h->ne;
    h->n_norm = (3 * h->B + h->ne) * h->A;
    if (cfg->graph_steps > 0) h->graph_steps = cfg->graph_steps;
    if (h->graph_steps > 256) h->graph_steps = 256;
    if (h->graph_steps > 1 && (h->graph_steps & 1)) h->graph_steps += 1;
    if (cfg->stats_capacity > 0) h->stats_cap = cfg->stats_capacity;
    if (cfg->perm_capacity > 0) h->perm_cap = cfg->perm_capacity;
    if (h->Aout > 64) {
        delete h;
        return bad("action output > 64 unsupported");
    }
    if (const char* e = std::getenv("SACX_WBF")) h->wbf_enabled = std::atoi(e);
    h->seeds = cfg->seeds > 1 ? cfg->seeds : 1;
    h->plan_seeds = cfg->single_seed_plan ? 1 : h->seeds;
    build_layout(h);                                        // (its slot ring follows the seed count)
    h->seed_bytes = h->seeds > 1 ? (h->arena_bytes + 65535) & ~uint64_t(65535) : h->arena_bytes;
    *out = h;
    return 0;
}

void sacx_destroy(sacx_handle* h) {
    if (!h) return;
    if (h->rng_stream) (void)hipStreamSynchronize(h->rng_stream);
    if (h->act_ev) (void)hipEventDestroy(h->act_ev);
    if (h->seg_start) (void)hipEventDestroy(h->seg_start);
    for (uint64_t* p : h->sig_mem)
        if (p) (void)hipFree(p);
    for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second);
    for (auto& m : h->mgraphs)
        for (auto& kv : m) (void)hipGraphExecDestroy(kv.second);
    for (auto& kv : h->roll_graphs) (void)hipGraphExecDestroy(kv.second);
    for (auto& kv : h->ppo_graphs) (void)hipGraphExecDestroy(kv.second);
    for (auto& kv : h->vc_graphs) (void)hipGraphExecDestroy(kv.second);
    for (auto& kv : h->ppo_pk_graphs) (void)hipGraphExecDestroy(kv.second);
    for (auto& kv : h->vc_pk_graphs) (void)hipGraphExecDestroy(kv.second);
    if (h->trpo_graph) (void)hipGraphExecDestroy(h->trpo_graph);
    if (h->trpo_fgraph) (void)hipGraphExecDestroy(h->trpo_fgraph);
    for (auto e : h->events) (void)hipEventDestroy(e);
    if (h->pin) (void)hipHostFree(h->pin);
    if (h->done_host) (void)hipHostFree(h->done_host);
    if (h->pin_ev) (void)hipEventDestroy(h->pin_ev);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    if (h->rng_stream) (void)hipStreamDestroy(h->rng_stream);
    if (h->comm) (void)ncclCommDestroy(h->comm);
    delete h;
}

const char* sacx_last_error(const sacx_handle* h) {
    if (!h) return g_create_error.c_str();
    return h->err.c_str();
}

int64_t sacx_arena_bytes(const sacx_handle* h) { return h ? (int64_t)h->total_bytes() : -1; }

int64_t sacx_seed_stride(const sacx_handle* h) { return h ? (int64_t)h->seed_bytes : -1; }

int sacx_seed_select(sacx_handle* h, int32_t seed) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (seed < 0 || seed >= h->seeds) return fail(h, "seed out of range");
    h->sel = seed;
    h->arena = h->arena0 + (uint64_t)seed * h->seed_bytes;
    return 0;
}

int sacx_layout(const sacx_handle* h, sacx_segment* segs, int32_t cap, int32_t* n_out) {
    if (!h || !n_out) return -1;
    *n_out = (int32_t)h->segs.size();
    if (!segs) return 0;
    for (int i = 0; i < (int)h->segs.size() && i < cap; ++i) {
        const SegInfo& s = h->segs[i];
        std::memset(&segs[i], 0, sizeof(sacx_segment));
        std::strncpy(segs[i].name, s.name.c_str(), sizeof(segs[i].name) - 1);
        segs[i].offset = s.off;
        segs[i].rows = s.rows;
        segs[i].cols = s.cols;
        segs[i].dtype = s.dtype;
        segs[i].role = s.role;
    }
    return 0;
}

int sacx_bind(sacx_handle* h, void* arena, uint64_t bytes, void* stream) {
    if (!h) return -1;
    if (!arena || bytes < h->total_bytes()) return fail(h, "arena missing or too small");
    if (((uintptr_t)arena) & 255) return fail(h, "arena must be 256-byte aligned");
    if (h->bound) return fail(h, "handle already bound");
    h->arena = h->arena0 = static_cast<char*>(arena);
    h->sel = 0;
    h->stream = static_cast<hipStream_t>(stream);
    {   // ws.ones: the B-row scale of unscaled dW problems
        const SegInfo& so = h->seg("ws.ones");
        std::vector<float> ones((size_t)(so.rows * so.cols), 1.0f);
        for (int k = 0; k < h->seeds; ++k)
            HIPCHK(h, hipMemcpy(h->arena0 + (uint64_t)k * h->seed_bytes + so.off, ones.data(), ones.size() * sizeof(float),
                                hipMemcpyHostToDevice));
    }
    if (h->rng_jump) {   // rng.jc: the segmented sampler's jump coefficients
        const SegInfo& sj = h->seg("rng.jc");
        std::vector<int32_t> jc;
        int64_t used = 0;
        try {   // (a C entry point: no exception may leave it -- bad_alloc, or the charpoly search failing)
            jc.resize((size_t)mt_jump_lists_words(h->jsmax - 1, MTJ_CH));
            used = mt_jump_lists(h->jL, h->jsmax - 1, MTJ_CH, jc.data());
        } catch (const std::exception& e) {
            return fail(h, std::string("segmented sampler jump coefficients: ") + e.what());
        }
        for (int k = 0; k < h->seeds; ++k)
            HIPCHK(h, hipMemcpy(h->arena0 + (uint64_t)k * h->seed_bytes + sj.off, jc.data(), (size_t)used * sizeof(int32_t),
                                hipMemcpyHostToDevice));
    }
    // 32x32 forward / dX tiles once the launches are wide: seeds x batch >= 1024 rows (packed
    // seeds; Humanoid B = 1024: SAC-EO +5.6 %, model fit +8 %, SAC +1 %); a handle-level rule, so
    // the launches merged_body folds together always agree.  From 4,096 rows the dW + Adam
    // launches take 32x32 tiles too (tools/t32_dw.sh: Humanoid 4 seeds +3.5 %, 8 seeds +5 %,
    // bf16 4 seeds +8 %, HC 32 seeds +1.9 %; HC 8 / 16 seeds and one Humanoid seed even or worse)
    auto t32_of = [](int64_t rows) { return rows >= 4096 ? 1 : rows >= 1024 ? 2 : 0; };
    // (packed on-policy learners keep the one-learner handle's tiles: each learner's results are its own run's)
    h->tile32 = t32_of((int64_t)(h->learners > 1 ? 1 : h->seeds) * h->B);
    h->tile32_plan = t32_of((int64_t)h->plan_seeds * h->B);
    if (h->bc) h->tile32 = h->tile32_plan = 0;   // the BC update has the expert rows only, whatever the batch
    if (const char* e = std::getenv("SACX_T32")) h->tile32 = h->tile32_plan = std::atoi(e);
    // dW + Adam over >= 512 batch rows (Humanoid B = 1,024) on k_dwl: LDS-DMA staged 128-B row
    // pieces instead of the fragment-shaped column loads, bit-identical results
    if (const char* e = std::getenv("SACX_DWL")) h->dwl = std::atoi(e);
    if (const char* e = std::getenv("SACX_DW_ROUND")) h->dw_round_tiles = std::atoi(e);
    if (const char* e = std::getenv("SACX_MFUSE")) h->mfuse = std::atoi(e);
    if (const char* e = std::getenv("SACX_MTILE")) h->mtile = std::atoi(e);
    if (const char* e = std::getenv("SACX_MT32")) h->mt32 = std::atoi(e);
    if (const char* e = std::getenv("SACX_UNALIGNED")) h->unaligned_b = std::atoi(e);
    if (const char* e = std::getenv("SACX_FWD2")) h->fwd2 = std::atoi(e);
    if (const char* e = std::getenv("SACX_AFIN")) h->afin = std::atoi(e);
    if (const char* e = std::getenv("SACX_MFWD2")) h->mfwd2 = std::atoi(e);
    if (const char* e = std::getenv("SACX_MPRE")) h->mpre = std::atoi(e);
    if (const char* e = std::getenv("SACX_DWL_NH")) h->dwl_nh = std::atoi(e) == 2 ? 2 : 1;
    // Sampler batch: each batch start is a cross-stream wait on the chain (~1 us of gap), so a
    // cheap sampler takes 8 updates per launch (HC one seed, A/B x2: 13.55k vs 13.38k at 4);
    // an expensive one (Humanoid: 52k normals, 146 us per update) keeps 4, where the graph's
    // ramp and the sampler's lead over the chain favour smaller batches (5.80k vs 5.62k at 8)
    // (16 updates per k_rng launch measured within noise of 8 -- HC 2,000 updates 16.22k / 16.30k against
    // 16.15k / 16.17k, profiles/r06_ab_nbatch_v1.txt -- and slowed the profiled run: 10.2k updates/s
    // and 7.73 us per k_gemm / k_fwd2 launch under rocprofv3 against 16.1k and 6.92 at 8; SACX_NBATCH=16)
    h->nbatch = h->n_norm <= 16384 ? 8 : 4;
    // Long graphs of the cheap sampler (k_rng alone) grow their batches 1, 4, 16, 64 (sampler_sched.h):
    // every batch start costs the chain two cross-queue graph edges, and a 256-update graph has 7
    // batches instead of 35 (SACX_BATCH_GROW: the largest batch, 0 = batches of nbatch throughout;
    // a forced SACX_NBATCH keeps the fixed schedule).  HC 2,000 updates 17.43k against 16.25k on 32
    // slots with batches of 8; the 128-slot ring carries most of it (17.37k with batches of 8),
    // profiles/sampler_grow_ab_v1.txt
    int grow = h->n_norm <= 16384 ? 64 : 0;
    if (const char* e = std::getenv("SACX_BATCH_GROW")) grow = std::max(0, std::min(NSLOT / 2, std::atoi(e)));
    if (const char* e = std::getenv("SACX_NBATCH")) { // (k_rng alone takes batches up to half the ring)
        h->nbatch = std::max(1, std::min(h->rng_jump || h->rng_split ? NBATCH_MAX : NSLOT / 2, std::atoi(e)));
        grow = 0;
    }
    if (const char* e = std::getenv("SACX_MTJ_RAMP")) h->mtj_ramp = std::atoi(e);
    if (const char* e = std::getenv("SACX_MTJ_UNDER")) h->mtj_under = std::atoi(e);
    while (h->nslot % h->nbatch || h->nslot < 2 * h->nbatch) --h->nbatch;   // the ring holds whole batches
    h->grow = grow > 0 && !h->rng_jump && !h->rng_split ? sampler_grow_max(h->nslot, grow) : 0;
    if (h->dp_ranks > 0) {
        if (h->cfg.use_expert) return fail(h, "data-parallel mode covers plain SAC (use_expert = 0)");
        const int64_t d = (int64_t)(h->off_of("t0.l0") - h->off_of("q0.l0"));
        for (int l = 0; l <= h->nd[1].D(); ++l)
            for (int k = 0; k < 2; ++k)
                if ((int64_t)(h->off_of("t" + std::to_string(k) + ".l" + std::to_string(l)) -
                              h->off_of("q" + std::to_string(k) + ".l" + std::to_string(l))) != d)
                    return fail(h, "internal: target layout is not a fixed shift of the critics");
    }
    // the weight shadows feed the update plans' 32x32 bf16 forward tiles; the Adam epilogues
    // keep them current (not the data-parallel modes, whose Adam runs in k_adam_apply)
    h->wbf_attach = (!h->wbf_mats.empty() || !h->abf_segs.empty()) && h->tile32 > 0 && h->dp_ranks == 0;
    h->wbf_live = h->wbf_attach;
    // (a trainable GaussianActor handle has no SAC / BC update: its step plans are built per minibatch
    // size by build_ppo_plan, and cfg.batch only bounds them)
    for (int sl = 0; sl < h->nslot && !h->ppo; ++sl) {
        h->abf_written.clear();
        if (h->bc) build_plan_bc(h, sl);
        else if (h->deep) build_plan_generic(h, sl);
        else build_plan(h, sl);
    }
    h->abf_written.clear();
    h->wbf_attach = false;
    // q.head's expert rows (qhead_block's SAC-EO tail) hold a world-model row in 8 registers per lane,
    // and the wide q.head has no such rows: no plan may carry them beside a wide row
    for (int sl = 0; sl < h->nslot; ++sl)
        for (const Launch& L : h->plan[sl]) {
            const QHeadArgs* q = L.kind == Launch::QHEAD ? &L.qh
                                 : (L.kind == Launch::GEMM && gemm_rows_qhead(L.gemm.mode, L.gemm.rowk)) ? &L.gemm.qh : nullptr;
            if (q && q->ne > 0 && (q->Hm1 > 512 || q->H1 > 512))
                return fail(h, "internal: q.head with expert rows beside a hidden layer wider than 512");
        }
    for (int sl = 1; sl < h->nslot; ++sl) {
        if (h->plan[0].size() != h->plan[sl].size()) return fail(h, "internal: slot plans differ");
        for (size_t i = 0; i < h->plan[0].size(); ++i) {
            const Launch &a = h->plan[0][i], &b = h->plan[sl][i];
            if (a.kind != b.kind || a.name != b.name || a.grid != b.grid) return fail(h, "internal: slot plans differ at " + a.name);
        }
    }
    h->mplans.assign(h->seeds, {});
    h->mpres.assign(h->seeds, Launch{});
    h->mgraphs.assign(h->seeds, {});
    h->mfit_hosts.assign(h->seeds, 0);
    build_model_plan(h);                      // seed 0's; the others' on their first model_fit
    HIPCHK(h, hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    HIPCHK(h, hipStreamCreateWithFlags(&h->rng_stream, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&h->act_ev, hipEventDisableTiming));
    if (const char* e = std::getenv("SACX_SPEC")) h->spec_enabled = std::atoi(e) != 0;
    if (const char* e = std::getenv("SACX_ACT_RNG")) h->act_rng = std::atoi(e) != 0;
    if (const char* e = std::getenv("SACX_ACT_POLL")) h->act_poll = std::atoi(e) != 0;
    h->cur_size_host = 0;
    h->bound = true;
    return 0;
}

int sacx_resync(sacx_handle* h) {
    if (!h || !h->bound) return fail(h, "not bound");
    h->alpha_pending = -1;                   // the restored state is authoritative
    h->ctl_known = false;
    if (spec_cancel(h, true)) return -1;
    Ctl c{};
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(&c, h->ctl(), sizeof(Ctl), hipMemcpyDeviceToHost));
    h->seq_host = c.step_seq;
    h->cur_size_host = c.cur_size;
    h->mfit_hosts[h->sel] = c.mfit_seq;
    if (h->ppo) {                            // the step sequence (index ring position) and the table's rows
        PpoCtl pc{};
        HIPCHK(h, hipMemcpy(&pc, h->ptr<PpoCtl>("ppo.ctl"), sizeof(PpoCtl), hipMemcpyDeviceToHost));
        h->op().ppo_seq = pc.seq;
        h->op().ppo_rows = pc.n_rows;
    }
    if (h->vc > 0) {
        VcCtl vc{};
        HIPCHK(h, hipMemcpy(&vc, h->ptr<VcCtl>("vc.ctl"), sizeof(VcCtl), hipMemcpyDeviceToHost));
        h->op().vc_seq = vc.seq;
        for (int k = 0; k < MAX_MODELS; ++k) h->op().vc_rows[k] = vc.n_rows[k];
    }
    return 0;
}

int sacx_dp_unique_id(void* id_out, int32_t cap) {
    if (!id_out || cap < (int32_t)sizeof(ncclUniqueId)) return -1;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return -2;
    std::memcpy(id_out, &id, sizeof(id));
    return (int)sizeof(id);
}

int sacx_dp_init(sacx_handle* h, const void* id, int32_t nranks, int32_t rank) {
    if (!h) return -1;
    if (h->bound) return fail(h, "sacx_dp_init must precede sacx_bind");
    if (h->comm) return fail(h, "data-parallel communicator already set");
    if (h->seeds > 1) return fail(h, "data-parallel mode needs seeds = 1");
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return fail(h, "bad data-parallel arguments");
    if (h->cfg.use_expert) return fail(h, "data-parallel mode covers plain SAC (use_expert = 0)");
    if (h->ppo) return fail(h, "data-parallel mode covers plain SAC (not a trainable GaussianActor handle)");
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    const ncclResult_t r = ncclCommInitRank(&h->comm, nranks, uid, rank);
    if (r != ncclSuccess) return fail(h, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    h->dp_ranks = nranks;
    h->dp_rank = rank;
    return 0;
}

int sacx_dp_init_local(sacx_handle* h, int32_t nranks, int32_t rank) {
    if (!h) return -1;
    if (h->bound) return fail(h, "sacx_dp_init_local must precede sacx_bind");
    if (h->comm || h->dp_ranks) return fail(h, "data-parallel mode already set");
    if (h->seeds > 1) return fail(h, "data-parallel mode needs seeds = 1");
    if (nranks < 1 || nranks > DP_LOCAL_MAX || rank < 0 || rank >= nranks) return fail(h, "bad data-parallel arguments");
    if (h->cfg.use_expert) return fail(h, "data-parallel mode covers plain SAC (use_expert = 0)");
    if (h->ppo) return fail(h, "data-parallel mode covers plain SAC (not a trainable GaussianActor handle)");
    h->dp_ranks = nranks;
    h->dp_rank = rank;
    h->dp_local = true;
    return 0;
}

int sacx_dp_local_step(sacx_handle* const* hs, int32_t nranks, int64_t n_steps, int64_t num_timesteps,
                       int32_t ts_increment) {
    if (!hs || nranks < 1 || nranks > DP_LOCAL_MAX) return -1;
    sacx_handle* h0 = hs[0];
    for (int r = 0; r < nranks; ++r) {
        sacx_handle* h = hs[r];
        if (!h || !h->bound) return fail(h0, "rank handle not bound");
        if (!h->dp_local || h->dp_ranks != nranks || h->dp_rank != r)
            return fail(h0, "handles must be ranks 0..n-1 of one sacx_dp_init_local group, in rank order");
        if (h->stream != h0->stream) return fail(h0, "the ranks' handles must be bound to one stream");
    }
    if (n_steps <= 0) return 0;
    hipStream_t s = h0->stream;
    for (int r = 0; r < nranks; ++r)
        launch_set_ctl(hs[r]->ctl0(), num_timesteps, ts_increment, 0, 1, s);
    for (int64_t j = 0; j < n_steps; ++j) {
        std::vector<size_t> pos(nranks, 0);
        for (;;) {
            // every rank up to its next all-reduce (or its end), in rank order, on the one stream
            int at_ar = 0;
            for (int r = 0; r < nranks; ++r) {
                const std::vector<Launch>& pl = hs[r]->plan[0];
                while (pos[r] < pl.size() && pl[pos[r]].kind != Launch::ALLREDUCE) enqueue(pl[pos[r]++], hs[r], s);
                at_ar += pos[r] < pl.size();
            }
            if (at_ar == 0) break;
            if (at_ar != nranks) return fail(h0, "internal: the ranks' plans do not line up");
            DpSumArgs a{};
            a.nranks = nranks;
            a.n = hs[0]->plan[0][pos[0]].ar_count;
            for (int r = 0; r < nranks; ++r) {
                const Launch& L = hs[r]->plan[0][pos[r]];
                if (L.ar_count != a.n) return fail(h0, "internal: all-reduce sizes differ");
                a.buf[r] = L.ar_buf;
                ++pos[r];
            }
            launch_dp_sum(a, s);
        }
    }
    HIPCHK(h0, hipGetLastError());
    for (int r = 0; r < nranks; ++r) hs[r]->seq_host += n_steps;
    return 0;
}

int sacx_buffer_append(sacx_handle* h, const float* s, const float* a, const float* r, const float* sp,
                       const float* d, int64_t n) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (n <= 0) return 0;
    if (!s || !a || !r || !sp || !d) return fail(h, "null row pointer");
    if (flush_append(h)) return -1;           // appends stay in call order
    AppendArgs g{};
    g.replay = h->f("replay"); g.cap = h->cap; g.stride = h->stride; g.S = h->S; g.A = h->A;
    g.s = s; g.a = a; g.r = r; g.sp = sp; g.d = d; g.n = n; g.ctl = h->ctl();
    launch_append(g, h->stream);
    HIPCHK(h, hipGetLastError());
    h->cur_size_host = std::min<int64_t>(h->cur_size_host + n, h->cap);
    ++h->n_appends;
    return 0;
}

// Host-pointer variants for the env loop (one transition / one observation per call).  The
// rows go into one pinned, device-mapped buffer that the kernels read (k_append, the obs
// normaliser) and write (the action head) in place over PCIe: no DMA copy on either side,
// whose fixed cost exceeds the whole transfer at these sizes.
static int stage_alloc(sacx_handle* h) {
    if (!h->pin) {
        HIPCHK(h, hipHostMalloc((void**)&h->pin, sizeof(float) * 2 * STAGE_CAP, hipHostMallocMapped));
        HIPCHK(h, hipHostGetDevicePointer((void**)&h->pin_dev, h->pin, 0));
        HIPCHK(h, hipEventCreateWithFlags(&h->pin_ev, hipEventDisableTiming));
        HIPCHK(h, hipHostMalloc((void**)&h->done_host, 64, hipHostMallocMapped));
        HIPCHK(h, hipHostGetDevicePointer((void**)&h->done_dev, h->done_host, 0));
        __atomic_store_n(h->done_host, 0u, __ATOMIC_RELEASE);
        __atomic_store_n(h->done_host + 1, 0u, __ATOMIC_RELEASE);
        h->done_seq = 0;
    }
    return 0;
}

static inline void cpu_relax() {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
}

// The act_host rows' outputs are on the host once the counter reaches done_seq: spin on it (a
// few us) instead of waiting for the whole stream position (k_act_rng's sampler workgroup, the
// event's own latency).  An act queued behind a long stream prefix (step(G), a model fit) would
// keep spinning, so past ACT_SPIN the stream is waited for instead; a counter still short then
// is an error, and done_seq is resynchronised from the counter so later acts do not wait on it.
static constexpr auto ACT_SPIN = std::chrono::microseconds(2000);   // > one update graph (the drop-in cadence)
static int act_rows_wait(sacx_handle* h) {
    if (!h->act_poll) return hipEventSynchronize(h->act_ev) == hipSuccess ? 0 : fail(h, "act event");
    const uint32_t target = h->done_seq;
    auto reached = [&]() { return (int32_t)(__atomic_load_n(h->done_host, __ATOMIC_ACQUIRE) - target) >= 0; };
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t it = 1; !reached(); ++it) {
        cpu_relax();
        if ((it & 255) == 0 && std::chrono::steady_clock::now() - t0 > ACT_SPIN) {
            const hipError_t e = h->act_ev_live ? hipEventSynchronize(h->act_ev) : hipStreamSynchronize(h->stream);
            if (e != hipSuccess || !reached()) {
                h->done_seq = __atomic_load_n(h->done_host, __ATOMIC_ACQUIRE);
                return fail(h, e != hipSuccess ? "act event" : "act rows finished without their completion count");
            }
            break;
        }
    }
    return 0;
}
// the append half: waits until its last reader (a k_append) has finished
static int stage_begin(sacx_handle* h) {
    if (stage_alloc(h)) return -1;
    if (h->app_ctr_pending) {           // the held append's workgroup has read the rows
        const uint32_t target = h->app_seq;
        auto reached = [&]() { return (int32_t)(__atomic_load_n(h->done_host + 1, __ATOMIC_ACQUIRE) - target) >= 0; };
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t it = 1; !reached(); ++it) {
            cpu_relax();
            if ((it & 255) == 0 && std::chrono::steady_clock::now() - t0 > ACT_SPIN) {
                HIPCHK(h, hipStreamSynchronize(h->stream));
                if (!reached()) return fail(h, "held append finished without its completion count");
                break;
            }
        }
        h->app_ctr_pending = false;
    }
    if (h->pin_pending) HIPCHK(h, hipEventSynchronize(h->pin_ev));   // its last reader has finished
    h->pin_pending = false;
    return 0;
}

int sacx_buffer_append_host(sacx_handle* h, const float* s, const float* a, const float* r, const float* sp,
                            const float* d, int64_t n) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (n <= 0) return 0;
    if (!s || !a || !r || !sp || !d) return fail(h, "null row pointer");
    const int S = h->S, A = h->A;
    const int64_t per = 2 * S + A + 2, chunk = STAGE_CAP / per;
    if (chunk <= 0) return fail(h, "a transition is larger than the pinned staging buffer (use sacx_buffer_append)");
    if (flush_append(h)) return -1;           // (a held one first: appends stay in call order)
    // the drop-in cadence: hold the row for the next act's launch (sacx_handle::app_defer)
    const bool defer = n == 1 && h->app_defer && h->last_step_one && h->seeds == 1 && spec_mode(h) && h->act_rng;
    for (int64_t done = 0; done < n; done += chunk) {
        const int64_t m = std::min(chunk, n - done);
        if (stage_begin(h)) return -1;
        float* p = h->pin;
        std::memcpy(p, s + done * S, sizeof(float) * m * S);
        std::memcpy(p + m * S, a + done * A, sizeof(float) * m * A);
        std::memcpy(p + m * (S + A), r + done, sizeof(float) * m);
        std::memcpy(p + m * (S + A + 1), sp + done * S, sizeof(float) * m * S);
        std::memcpy(p + m * (2 * S + A + 1), d + done, sizeof(float) * m);
        const float* g = h->pin_dev;
        if (defer) {
            AppendArgs& ap = h->app_args;
            ap = AppendArgs{};
            ap.replay = h->f("replay"); ap.cap = h->cap; ap.stride = h->stride; ap.S = S; ap.A = A;
            ap.s = g; ap.a = g + m * S; ap.r = g + m * (S + A); ap.sp = g + m * (S + A + 1); ap.d = g + m * (2 * S + A + 1);
            ap.n = m; ap.ctl = h->ctl();
            h->app_pending = true;
            h->cur_size_host = std::min<int64_t>(h->cur_size_host + m, h->cap);
            ++h->n_appends;
            continue;
        }
        AppendArgs ag{};
        ag.replay = h->f("replay"); ag.cap = h->cap; ag.stride = h->stride; ag.S = S; ag.A = A;
        ag.s = g; ag.a = g + m * S; ag.r = g + m * (S + A); ag.sp = g + m * (S + A + 1); ag.d = g + m * (2 * S + A + 1);
        ag.n = m; ag.ctl = h->ctl();
        if (launch_staged_append(h, ag)) return -1;
        h->cur_size_host = std::min<int64_t>(h->cur_size_host + m, h->cap);
        ++h->n_appends;
    }
    return 0;
}

// The speculative draw (see sacx_handle::spec_live): the sampler launch of slot 1 or 2 for one
// update at the ring's current size, queued on the bound stream; it saves the state it starts
// from into "rng.spec" for spec_cancel.
static int spec_rng_args(sacx_handle* h, RngArgs* out) {
    const int slot = h->alpha_pending == 1 ? 2 : 1;    // not the slot a deferred alpha branch reads
    const Launch* R = nullptr;
    for (const Launch& L : h->plan[slot])
        if (L.kind == Launch::RNG) { R = &L; break; }
    if (!R) return fail(h, "internal: no sampler launch");
    RngArgs r = R->rng;
    // stamps pseq[slot] with the update that follows: step_seq, + 1 while a deferred
    // alpha.final has not counted the previous update yet
    r.reset_seq = h->alpha_pending >= 0 ? 2 : 1;
    h->spec_slot = slot;
    r.nupd = 1;
    r.size_fixed = 0;           // each seed's ring size, read on the device (final until the update)
    r.backup = reinterpret_cast<RngState*>(h->arena0 + h->off_of("rng.spec"));   // seed 0's (relocated per seed)
    *out = r;
    return 0;
}

// after the speculative sampler launch: plain SAC's gather too (SAC-EO's reads the permutation the
// caller pushes before the update), and the draw's bookkeeping
static int spec_after_rng(sacx_handle* h) {
    if (!h->cfg.use_expert)
        for (const Launch& L : h->plan[h->spec_slot])
            if (L.kind == Launch::GATHER) {
                if (!h->spec_polar_live) {
                    enqueue(L, h, h->stream);
                    continue;
                }
                Launch G = L;                  // + the draw's polar transform (sacx_handle::spec_polar)
                G.gather.pairs = h->ptr<uint32_t>("rng.spairs");
                G.gather.pairs_oi = h->ptr<int32_t>("rng.spairs_oi");
                for (const Launch& R : h->plan[h->spec_slot])
                    if (R.kind == Launch::RNG) G.gather.norm = R.rng.out_norm;
                G.gather.n_norm = h->n_norm;
                G.gather.polar_wgs = std::min(16, (h->spcap + 255) / 256);
                enqueue(G, h, h->stream);
            }
    h->spec_polar_live = false;
    HIPCHK(h, hipGetLastError());
    h->spec_live = true;
    h->spec_size = h->cur_size_host;
    h->spec_appends = h->n_appends;
    return 0;
}

static int spec_draw(sacx_handle* h) {
    RngArgs r;
    if (spec_rng_args(h, &r)) return -1;
    launch_rng(r, h->stream);
    return spec_after_rng(h);
}

// k_act_rows' arguments for n <= ACT_ROWS_MAX observation rows of the selected seed
static ActRowArgs act_rows_args(sacx_handle* h, const float* obs, float* noise, float* act_out) {
    ActRowArgs a{};
    a.obs = obs; a.s_mean = h->f("norm.s_mean"); a.s_den = h->f("norm.s_den");
    a.W0 = h->f("actor.l0"); a.W1 = h->f("actor.l1"); a.W3 = h->f("actor.l2"); a.logstd = h->f("actor.logstd");
    a.noise = noise; a.out = act_out;
    a.S = h->S; a.A = h->A; a.Aout = h->Aout; a.H0 = h->H0; a.H1 = h->H1;
    a.act0 = h->aact[0]; a.act1 = h->aact[1];
    a.mode = h->cfg.actor_gaussian ? 2 : 1;
    a.per_state_std = h->cfg.per_state_std;
    a.lim = h->cfg.act_limit;
    if (h->cfg.actor_gaussian) {
        a.logstd_init = logstd_init(h);
        a.output_norm = h->cfg.actor_output_norm;
    }
    return a;
}
static int actor_act(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, float* act_out,
                     uint32_t* done);
static bool act_rows_ok(const sacx_handle* h, int64_t n) {
    return n > 0 && n <= ACT_ROWS_MAX && !h->ln && h->nd[0].D() == 2 && h->S <= ACT_ROWS_DIM && h->H0 <= ACT_ROWS_DIM &&
           h->H1 <= ACT_ROWS_DIM && h->Aout <= 64;
}

int sacx_actor_act_host(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, float* act_out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (h->softmax) return fail(h, "a softmax handle samples on the host from sacx_ppo_dist's logits (discrete_actors.py:22-42)");
    if (n < 0 || (n > 0 && (!obs || !act_out))) return fail(h, "bad arguments");
    const int S = h->S, A = h->A;
    const int64_t chunk = std::min<int64_t>(ACT_CAP, STAGE_CAP / (S + A));
    if (chunk <= 0) return fail(h, "an observation row is larger than the pinned staging buffer (use sacx_actor_act)");
    const bool spec = h->last_step_one && spec_mode(h) && !h->spec_live && h->cur_size_host > 0;
    for (int64_t done = 0; done < n; done += chunk) {
        const int64_t m = std::min(chunk, n - done);
        if (stage_alloc(h)) return -1;
        float* p = h->pin + STAGE_CAP;          // the act half: its last reader was a synchronous act
        const float* g = h->pin_dev + STAGE_CAP;
        std::memcpy(p, obs + done * S, sizeof(float) * m * S);
        // (one seed's handle only: on a packed handle the act is the selected seed's rows while the
        // draw is every seed's, which spec_draw's own sampler launch covers)
        if (spec && deterministic && h->act_rng && h->seeds == 1 && done + m >= n && act_rows_ok(h, m)) {
            // the drop-in loop's act with the next update's draw beside the rows (k_act_rng)
            RngArgs r;
            if (spec_rng_args(h, &r)) return -1;
            ActRowArgs a = act_rows_args(h, g, nullptr, (float*)g + m * S);
            a.done = h->done_dev;
            const bool app = h->app_pending;  // the held append as one more workgroup: the draw then
            if (app) r.size_fixed = h->cur_size_host;   // takes the ring size from the host
            h->app_pending = false;
            if (h->spec_polar) {
                r.pairs = h->ptr<uint32_t>("rng.spairs");
                r.pairs_oi = h->ptr<int32_t>("rng.spairs_oi");
                r.pcap = h->spcap;
                h->spec_polar_live = true;
            }
            AppendArgs ag = h->app_args;
            if (app && h->app_ctr) {
                ag.done = h->done_dev + 1;
                ++h->app_seq;
                h->app_ctr_pending = true;
            }
            launch_act_rng(a, (int)m, r, h->stream, app ? &ag : nullptr, !h->spec_polar);
            HIPCHK(h, hipGetLastError());
            h->done_seq += (uint32_t)m;
            // no event markers behind the launch: each one held the next kernel back ~7-10 us on the
            // device (r06_dropin_ab_v2.txt).  The host polls the rows' count (act_poll) and the held
            // append's own count (stage_begin)
            h->act_ev_live = !(h->act_poll && h->app_ctr);
            if (h->act_ev_live) HIPCHK(h, hipEventRecord(h->act_ev, h->stream));
            if (app && !h->app_ctr) {
                HIPCHK(h, hipEventRecord(h->pin_ev, h->stream));
                h->pin_pending = true;
            }
            if (spec_after_rng(h)) return -1;
            if (act_rows_wait(h)) return -1;
            std::memcpy(act_out + done * A, p + m * S, sizeof(float) * m * A);
            continue;
        }
        if (flush_append(h)) return -1;
        const bool rows = act_rows_ok(h, m);     // k_act_rows: the host polls the rows' count
        const int rc = actor_act(h, g, m, deterministic, (float*)g + m * S, rows ? h->done_dev : nullptr);
        if (rc) return rc;
        if (rows) h->done_seq += (uint32_t)m;    // only once the launch that counts them is queued
        h->act_ev_live = !(rows && h->act_poll && h->app_ctr);   // (a marker holds the next launch back)
        if (h->act_ev_live) HIPCHK(h, hipEventRecord(h->act_ev, h->stream));
        // the drop-in loop steps next: its randoms are drawn while the host has the action
        if (done + m >= n && spec && spec_draw(h)) return -1;
        if (rows) {
            if (act_rows_wait(h)) return -1;
        } else {
            HIPCHK(h, hipEventSynchronize(h->act_ev));
        }
        std::memcpy(act_out + done * A, p + m * S, sizeof(float) * m * A);
    }
    return 0;
}

// Every seed of a packed handle at once (one launch chain for all): the env loop of K lock-step
// runs (sac_eo.train --runs K) hands over one row per run.  Arrays are [seeds, n, ...].
int sacx_buffer_append_host_seeds(sacx_handle* h, const float* s, const float* a, const float* r, const float* sp,
                                  const float* d, int64_t n) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (flush_append(h)) return -1;
    if (n <= 0) return 0;
    if (!s || !a || !r || !sp || !d) return fail(h, "null row pointer");
    const int S = h->S, A = h->A, K = h->seeds;
    const int64_t tot = (int64_t)K * n;
    if (tot * (2 * S + A + 2) > STAGE_CAP) return fail(h, "rows exceed the pinned staging buffer (append per seed)");
    if (stage_begin(h)) return -1;
    float* p = h->pin;
    std::memcpy(p, s, sizeof(float) * tot * S);
    std::memcpy(p + tot * S, a, sizeof(float) * tot * A);
    std::memcpy(p + tot * (S + A), r, sizeof(float) * tot);
    std::memcpy(p + tot * (S + A + 1), sp, sizeof(float) * tot * S);
    std::memcpy(p + tot * (2 * S + A + 1), d, sizeof(float) * tot);
    const float* g = h->pin_dev;
    AppendArgs ag{};
    ag.replay = h->f0("replay"); ag.cap = h->cap; ag.stride = h->stride; ag.S = S; ag.A = A;
    ag.s = g; ag.a = g + tot * S; ag.r = g + tot * (S + A); ag.sp = g + tot * (S + A + 1); ag.d = g + tot * (2 * S + A + 1);
    ag.n = n; ag.ctl = h->ctl0(); ag.sstride = (int64_t)h->seed_bytes; ag.nseeds = K;
    if (launch_staged_append(h, ag)) return -1;
    h->cur_size_host = std::min<int64_t>(h->cur_size_host + n, h->cap);   // every seed grows alike
    ++h->n_appends;
    return 0;
}

int sacx_actor_act_host_seeds(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, float* act_out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (h->softmax) return fail(h, "a softmax handle samples on the host from sacx_ppo_dist's logits (discrete_actors.py:22-42)");
    if (flush_append(h)) return -1;
    if (n <= 0 || !obs || !act_out) return fail(h, "bad arguments");
    const int S = h->S, A = h->A, K = h->seeds;
    if (n > ACT_ROWS_MAX || h->ln || h->nd[0].D() != 2 || S > ACT_ROWS_DIM || h->H0 > ACT_ROWS_DIM ||
        h->H1 > ACT_ROWS_DIM || h->Aout > 64)
        return fail(h, "sacx_actor_act_host_seeds: n <= 16 rows per seed, two hidden layers, no layer norm "
                       "(use per-seed calls)");
    const int64_t tot = (int64_t)K * n;
    if (tot * (S + A) > STAGE_CAP) return fail(h, "rows exceed the pinned staging buffer (act per seed)");
    if (stage_alloc(h)) return -1;
    float* const pa = h->pin + STAGE_CAP;          // the act half (acts are synchronous)
    float* const ga = h->pin_dev + STAGE_CAP;
    std::memcpy(pa, obs, sizeof(float) * tot * S);
    float* noise = deterministic ? nullptr : h->f0("act.noise");
    if (!deterministic && spec_cancel(h)) return -1;   // a draw from the streams: undo the speculative one
    if (!deterministic) {            // each seed's u = np.random.normal(size=(n, A)) from its own stream
        RngArgs r{};
        r.st = reinterpret_cast<RngState*>(h->f0("rng")); r.ctl = h->ctl0();
        r.n_int = 0; r.n_norm = (int32_t)n * A; r.out_idx = nullptr; r.out_norm = noise;
        r.slot = -1; r.reset_seq = 0; r.nupd = 1;
        r.sstride = (int64_t)h->seed_bytes; r.nseeds = K;
        launch_rng(r, h->stream);
    }
    ActRowArgs a{};
    a.obs = ga; a.s_mean = h->f0("norm.s_mean"); a.s_den = h->f0("norm.s_den");
    a.W0 = h->f0("actor.l0"); a.W1 = h->f0("actor.l1"); a.W3 = h->f0("actor.l2"); a.logstd = h->f0("actor.logstd");
    a.noise = noise; a.out = ga + tot * S;
    a.S = S; a.A = A; a.Aout = h->Aout; a.H0 = h->H0; a.H1 = h->H1;
    a.act0 = h->aact[0]; a.act1 = h->aact[1];
    a.mode = h->cfg.actor_gaussian ? 2 : 1;
    a.per_state_std = h->cfg.per_state_std;
    a.lim = h->cfg.act_limit;
    if (h->cfg.actor_gaussian) {
        a.logstd_init = logstd_init(h);
        a.output_norm = h->cfg.actor_output_norm;
    }
    a.sstride = (int64_t)h->seed_bytes; a.nseeds = K; a.m = (int32_t)n;
    a.done = h->done_dev;                   // every seed's rows count
    // lock-step drop-in cadence: every seed's next sampler draw, beside the action rows
    // (deterministic: k_act_rng) or queued behind them
    const bool spec = h->last_step_one && spec_mode(h) && !h->spec_live && h->cur_size_host > 0;
    if (spec && deterministic && h->act_rng) {
        RngArgs r;
        if (spec_rng_args(h, &r)) return -1;
        launch_act_rng(a, (int)n, r, h->stream);
        HIPCHK(h, hipGetLastError());
        h->done_seq += (uint32_t)(n * K);
        h->act_ev_live = !(h->act_poll && h->app_ctr);
        if (h->act_ev_live) HIPCHK(h, hipEventRecord(h->act_ev, h->stream));
        if (spec_after_rng(h)) return -1;
    } else {
        launch_act_rows(a, (int)n, h->stream);
        HIPCHK(h, hipGetLastError());
        h->done_seq += (uint32_t)(n * K);
        h->act_ev_live = !(h->act_poll && h->app_ctr);
        if (h->act_ev_live) HIPCHK(h, hipEventRecord(h->act_ev, h->stream));
        if (spec && spec_draw(h)) return -1;
    }
    if (act_rows_wait(h)) return -1;
    std::memcpy(act_out, pa + tot * S, sizeof(float) * tot * A);
    return 0;
}

int sacx_expert_set(sacx_handle* h, const float* s_e, const float* sp_e, int32_t n, float epsilon) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h)) return -1;             // alpha.final reads the epsilon this sets
    if (!h->cfg.use_expert) return fail(h, "handle was created without use_expert");
    if (h->models_only) return fail(h, "use_expert = SACX_EXPERT_MODELS: the handle holds no expert rows (sacx_expert_set)");
    if (n != h->ne_perm) return fail(h, "expert rows must equal expert_batch");
    const size_t bytes = sizeof(float) * (size_t)n * h->S;
    HIPCHK(h, hipMemcpyAsync(h->f("expert.s"), s_e, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->f("expert.sp"), sp_e, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    Ctl* c = h->ctl();
    const int64_t nn = n;
    HIPCHK(h, hipMemcpy(&c->n_expert, &nn, sizeof(nn), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(&c->epsilon, &epsilon, sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int sacx_perm_push(sacx_handle* h, const int32_t* perms, int64_t n_steps) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (!h->cfg.use_expert) return 0;
    if (h->models_only) return fail(h, "use_expert = SACX_EXPERT_MODELS: no expert permutations (sacx_perm_push)");
    if (n_steps > h->perm_cap) return fail(h, "n_steps exceeds perm_capacity");
    int32_t* ring = h->ptr<int32_t>("perm");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t j = 0; j < n_steps; ++j) {
        const int64_t slot = (h->seq_host + j) % h->perm_cap;
        HIPCHK(h, hipMemcpy(ring + slot * h->ne_perm, perms + j * h->ne_perm, sizeof(int32_t) * h->ne_perm,
                            hipMemcpyHostToDevice));
    }
    return 0;
}

int sacx_rng_seed(sacx_handle* h, uint32_t seed) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h, true)) return -1;
    RngState st{};
    for (int pos = 0; pos < 624; ++pos) {       // init_genrand (seeding.py:12 -> np.random.seed)
        st.key[pos] = seed;
        seed = 1812433253U * (seed ^ (seed >> 30)) + (uint32_t)pos + 1U;
    }
    st.pos = 624;
    st.has_gauss = 0;
    st.gauss = 0.0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(h->ptr<RngState>("rng"), &st, sizeof(st), hipMemcpyHostToDevice));
    return 0;
}

int sacx_rng_set_state(sacx_handle* h, const uint32_t key[624], int32_t pos, int32_t has_gauss, double gauss) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h, true)) return -1;
    if (pos < 0 || pos > 624) return fail(h, "pos out of range");
    RngState st{};
    std::memcpy(st.key, key, sizeof(st.key));
    st.pos = pos;
    st.has_gauss = has_gauss;
    st.gauss = gauss;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(h->ptr<RngState>("rng"), &st, sizeof(st), hipMemcpyHostToDevice));
    return 0;
}

int sacx_rng_get_state(sacx_handle* h, uint32_t key[624], int32_t* pos, int32_t* has_gauss, double* gauss) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h)) return -1;
    RngState st{};
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(&st, h->ptr<RngState>("rng"), sizeof(st), hipMemcpyDeviceToHost));
    std::memcpy(key, st.key, sizeof(st.key));
    *pos = st.pos;
    *has_gauss = st.has_gauss;
    *gauss = st.gauss;
    return 0;
}

int sacx_sac_step(sacx_handle* h, int64_t n_steps, int64_t num_timesteps, int32_t ts_increment, int32_t flags) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (h->dp_local) return fail(h, "in-process data-parallel ranks step together (sacx_dp_local_step)");
    if (h->ppo) return fail(h, "trainable GaussianActor handle: no SAC / BC step (sacx_ppo_steps trains it)");
    if (h->cfg.actor_gaussian) return fail(h, "GaussianActor handle: inference only (sacx_actor_act)");
    if (n_steps <= 0) return 0;
    // the drop-in loop's one-update steps: the randoms drawn speculatively after the previous
    // step are valid when the ring now holds the size they assumed (nothing else drew meanwhile:
    // every other consumer of the stream undid the draw)
    if (flush_append(h)) return -1;
    const bool spec_ok = spec_mode(h) && n_steps == 1 && flags == 0;
    const bool use_spec = spec_ok && h->spec_live && h->spec_appends == h->n_appends;
    if (!use_spec && settle(h)) return -1;
    h->last_step_one = spec_ok;
    // a deferred alpha.final (folded into this update) adds ts_increment to num_timesteps before
    // this update reads it
    const int prev = use_spec ? h->alpha_pending : -1;
    const bool segs = !use_spec && !(flags & SACX_STEP_EAGER) && use_segments(h, n_steps, flags);
    if (segs) {
        // (only the side-stream batch 0 waits for it: a marker on the bound stream otherwise costs the
        // call's first launches, r06_ab_seg_sig_v1.txt)
        if (!h->seg_start) HIPCHK(h, hipEventCreateWithFlags(&h->seg_start, hipEventDisableTiming));
        if (!seg_inline0()) HIPCHK(h, hipEventRecord(h->seg_start, h->stream));
    }
    wbf_refresh(h, h->stream);
    const int64_t nts_set = num_timesteps - (prev >= 0 ? ts_increment : 0);
    if (!(use_spec && h->ctl_skip && h->ctl_known && h->ctl_nts == nts_set && h->ctl_inc == ts_increment))
        launch_set_ctl(h->ctl0(), nts_set, ts_increment, (int64_t)h->seed_bytes, h->seeds, h->stream);
    h->ctl_known = false;
    const bool ext = (flags & SACX_STEP_EXTERNAL_RANDOMS) != 0;
    if (use_spec) {
        h->spec_live = false;
        ++h->spec_hits;
        hipGraphExec_t g;                 // gather + update, the randoms already in spec_slot
        if (get_spec_graph(h, h->spec_slot, prev, &g)) return -1;
        HIPCHK(h, hipGraphLaunch(g, h->stream));
        h->alpha_pending = h->spec_slot;
        // the control block after this chain: num_timesteps (the folded alpha.final added
        // ts_increment; this update's own is deferred into the next step)
        h->ctl_known = true;
        h->ctl_nts = num_timesteps;
        h->ctl_inc = ts_increment;
    } else if (flags & SACX_STEP_EAGER) {
        for (int64_t j = 0; j < n_steps; ++j) enqueue_step(h, 0, !ext, h->stream);
        HIPCHK(h, hipGetLastError());
    } else if (segs) {
        if (run_segments(h, (int)n_steps, true)) return -1;
    } else {
        std::vector<std::pair<hipGraphExec_t, int64_t>> gl;
        if (step_graph_list(h, n_steps, ext, &gl)) return -1;
        for (const auto& g : gl)
            for (int64_t i = 0; i < g.second; ++i) HIPCHK(h, hipGraphLaunch(g.first, h->stream));
    }
    h->seq_host += n_steps;
    if (h->nccl_failed) return fail(h, "ncclAllReduce failed");
    return 0;
}

int sacx_prepare(sacx_handle* h, int64_t n_steps, int32_t flags) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h)) return -1;
    if (n_steps <= 0 || (flags & SACX_STEP_EAGER)) return 0;
    if (use_segments(h, n_steps, flags)) {
        if (run_segments(h, (int)n_steps, false)) return -1;
    } else {
        std::vector<std::pair<hipGraphExec_t, int64_t>> gl;
        if (step_graph_list(h, n_steps, (flags & SACX_STEP_EXTERNAL_RANDOMS) != 0, &gl)) return -1;
    }
    if (spec_mode(h) && n_steps == 1 && flags == 0) {
        hipGraphExec_t g;                 // the drop-in loop's speculative path replays these
        for (int slot = 1; slot <= 2; ++slot)
            for (int prev : {-1, 3 - slot})
                if (get_spec_graph(h, slot, prev, &g)) return -1;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int sacx_model_fit(sacx_handle* h, const int32_t* idx, int64_t n_steps, int32_t flags) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h)) return -1;
    if (!h->cfg.use_expert) return fail(h, "handle was created without use_expert (no world models)");
    if (n_steps <= 0) return 0;
    if (!idx) return fail(h, "null index array");
    const int k = h->sel;                 // packed seeds: the selected seed's models and ring
    if (h->mplans[k].empty()) {
        build_model_plan(h);
    }
    const std::vector<Launch>& mplan = h->mplans[k];
    const int R2 = h->nm * h->mb;
    int32_t* ring = h->ptr<int32_t>("mfit.idx");
    // every step's launches read their minibatch rows from the index ring at ctl->mfit_seq, so a
    // graph of several steps replays them back to back (one graph launch per MFIT_GRAPH steps)
    auto graph_of = [&](int n, hipGraphExec_t* out) -> int {
        auto it = h->mgraphs[k].find(n);
        if (it == h->mgraphs[k].end()) {
            hipGraphExec_t ex = nullptr;
            if (capture_graph(h, "model-fit", [&](hipStream_t cs) {
                    enqueue_fit_pre(h, n, cs);     // (n <= MFIT_PRE)
                    for (int j = 0; j < n; ++j)
                        for (const Launch& L : mplan) enqueue(fit_step_launch(h, L, j), h, cs);
                    return 0;
                }, &ex))
                return -1;
            it = h->mgraphs[k].emplace(n, ex).first;
        }
        *out = it->second;
        return 0;
    };
    for (int64_t done = 0; done < n_steps;) {
        const int64_t chunk = std::min<int64_t>(n_steps - done, h->mfit_cap);
        HIPCHK(h, hipStreamSynchronize(h->stream));   // ring slots of earlier chunks are consumed
        // the chunk's slots are contiguous modulo the ring: at most two copies
        const int64_t s0 = (h->mfit_hosts[k] + done) % h->mfit_cap;
        const int64_t first = std::min<int64_t>(chunk, h->mfit_cap - s0);
        HIPCHK(h, hipMemcpy(ring + s0 * R2, idx + done * R2, sizeof(int32_t) * R2 * first, hipMemcpyHostToDevice));
        if (chunk > first)
            HIPCHK(h, hipMemcpy(ring, idx + (done + first) * R2, sizeof(int32_t) * R2 * (chunk - first),
                                hipMemcpyHostToDevice));
        const char* kdump = std::getenv("SACX_MFIT_KTIME");
        if ((flags & SACX_STEP_EAGER) && kdump) {
            // diagnostics: per-workgroup start / end stamps of every GEMM launch of each step, appended
            // to <file> as one line per launch and step: name, workgroups, span, mean / max workgroup,
            // last-start offset, gap to the previous launch's end (us)
            std::vector<int> nwg;
            int64_t tot = 0;
            for (const Launch& L : mplan) {
                const int n = L.kind == Launch::GEMM ? L.grid + (L.gemm.has_mfinal ? 1 : 0) : 0;
                nwg.push_back(n);
                tot += 2 * n;
            }
            uint64_t* kb = nullptr;
            HIPCHK(h, hipMalloc(&kb, sizeof(uint64_t) * std::max<int64_t>(1, tot)));
            std::vector<uint64_t> host((size_t)std::max<int64_t>(1, tot));
            FILE* f = std::fopen(kdump, "a");
            for (int64_t j = 0; j < chunk; ++j) {
                HIPCHK(h, hipMemsetAsync(kb, 0, sizeof(uint64_t) * std::max<int64_t>(1, tot), h->stream));
                if (j % MFIT_PRE == 0) enqueue_fit_pre(h, (int)std::min<int64_t>(MFIT_PRE, chunk - j), h->stream);
                int64_t o = 0;
                for (size_t i = 0; i < mplan.size(); ++i) {
                    Launch C = fit_step_launch(h, mplan[i], (int)(j % MFIT_PRE));
                    if (nwg[i] > 0) {
                        C.gemm.ktime = kb + o;
                        o += 2 * nwg[i];
                    }
                    enqueue(C, h, h->stream);
                }
                HIPCHK(h, hipStreamSynchronize(h->stream));
                HIPCHK(h, hipMemcpy(host.data(), kb, sizeof(uint64_t) * host.size(), hipMemcpyDeviceToHost));
                o = 0;
                uint64_t prev = 0;
                for (size_t i = 0; f && i < mplan.size(); ++i) {
                    if (nwg[i] == 0) continue;
                    uint64_t lo = UINT64_MAX, hi = 0, ls = 0, wmax = 0;
                    double wsum = 0.0;
                    int cnt = 0;
                    for (int b = 0; b < nwg[i]; ++b) {
                        const uint64_t t0 = host[o + 2 * b], t1 = host[o + 2 * b + 1];
                        if (t0 == 0 || t1 == 0) continue;           // (workgroups that return early stamp nothing)
                        lo = std::min(lo, t0); hi = std::max(hi, t1); ls = std::max(ls, t0);
                        wmax = std::max(wmax, t1 - t0); wsum += (double)(t1 - t0); ++cnt;
                    }
                    std::fprintf(f, "%s,%d,%.2f,%.2f,%.2f,%.2f,%.2f\n", mplan[i].name.c_str(), cnt, (hi - lo) * 0.01,
                                 wsum / std::max(1, cnt) * 0.01, wmax * 0.01, (ls - lo) * 0.01,
                                 prev ? ((double)lo - (double)prev) * 0.01 : 0.0);
                    prev = hi;
                    o += 2 * nwg[i];
                }
            }
            if (f) std::fclose(f);
            (void)hipFree(kb);
        } else if (flags & SACX_STEP_EAGER) {
            for (int64_t j = 0; j < chunk; ++j) {
                if (j % MFIT_PRE == 0) enqueue_fit_pre(h, (int)std::min<int64_t>(MFIT_PRE, chunk - j), h->stream);
                for (const Launch& L : mplan) enqueue(fit_step_launch(h, L, (int)(j % MFIT_PRE)), h, h->stream);
            }
            HIPCHK(h, hipGetLastError());
        } else {
            for (int64_t j = 0; j < chunk;) {
                const int n = chunk - j >= MFIT_GRAPH ? MFIT_GRAPH : chunk - j >= 8 ? 8 : 1;   // (<= MFIT_PRE)
                hipGraphExec_t ex = nullptr;
                if (graph_of(n, &ex)) return -1;
                HIPCHK(h, hipGraphLaunch(ex, h->stream));
                j += n;
            }
        }
        done += chunk;
    }
    h->mfit_hosts[k] += n_steps;
    return 0;
}

int sacx_settle(sacx_handle* h) {
    if (!h || !h->bound) return fail(h, "not bound");
    return settle(h);
}

int sacx_sync(sacx_handle* h) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h)) return -1;           // an observation point: the arena holds no speculative draw
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return 0;
}

int64_t sacx_spec_hits(const sacx_handle* h) { return h ? h->spec_hits : -1; }

int64_t sacx_rollout_launches(const sacx_handle* h) { return h ? h->roll_nodes : -1; }

static int launch_info(const std::vector<Launch>& plan, sacx_launch_info* out, int32_t cap, int32_t* n_out);

int sacx_plan_info(const sacx_handle* h, sacx_launch_info* out, int32_t cap, int32_t* n_out) {
    if (!h || !n_out) return -1;
    if (!h->bound) {
        *n_out = 0;
        return -1;
    }
    return launch_info(h->plan[0], out, cap, n_out);
}

int sacx_model_plan_info(const sacx_handle* h, sacx_launch_info* out, int32_t cap, int32_t* n_out) {
    if (!h || !n_out) return -1;
    if (!h->bound || h->mplans.empty()) {
        *n_out = 0;
        return h->bound ? 0 : -1;
    }
    return launch_info(h->mplans[h->sel], out, cap, n_out);
}

static int launch_info(const std::vector<Launch>& plan, sacx_launch_info* out, int32_t cap, int32_t* n_out) {
    *n_out = (int32_t)plan.size();
    if (!out) return 0;
    for (int i = 0; i < (int)plan.size() && i < cap; ++i) {
        std::memset(&out[i], 0, sizeof(sacx_launch_info));
        std::strncpy(out[i].name, plan[i].name.c_str(), sizeof(out[i].name) - 1);
        const bool bcf = plan[i].kind == Launch::FINAL && plan[i].fin.use_expert == SACX_EXPERT_BC;
        std::strncpy(out[i].kernel, bcf ? "k_bc_final" : kernel_family(plan[i].kind), sizeof(out[i].kernel) - 1);
        out[i].grid = plan[i].grid;
        out[i].block = plan[i].block;
        out[i].flops = plan[i].flops;
        out[i].bytes = plan[i].bytes;
    }
    return 0;
}

int sacx_profile(sacx_handle* h, int64_t n_steps, double* ms_per_launch, int32_t cap) {
    if (h && h->bound && settle(h)) return -1;
    if (!h || !h->bound) return fail(h, "not bound");
    wbf_refresh(h, h->stream);
    const auto& plan = h->plan[0];
    const int n = (int)plan.size();
    std::vector<hipEvent_t> ev(n + 1);
    for (auto& e : ev) HIPCHK(h, hipEventCreate(&e));
    std::vector<double> acc(n, 0.0);
    for (int64_t s = 0; s < n_steps; ++s) {
        launch_spin(3000.0, h->stream);   // the host queues the whole step while the GPU waits
        HIPCHK(h, hipEventRecord(ev[0], h->stream));
        for (int i = 0; i < n; ++i) {
            enqueue(plan[i], h, h->stream);
            HIPCHK(h, hipEventRecord(ev[i + 1], h->stream));
        }
        HIPCHK(h, hipEventSynchronize(ev[n]));
        for (int i = 0; i < n; ++i) {
            float ms = 0.f;
            HIPCHK(h, hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            acc[i] += ms;
        }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    h->seq_host += n_steps;
    for (int i = 0; i < n && i < cap; ++i) ms_per_launch[i] = acc[i];
    return 0;
}

// One GEMM launch outside any plan, enqueued at once on st (or captured by the caller)
static void gemm_now(sacx_handle* h, const std::string& name, const std::vector<GemmProb>& ps, hipStream_t st) {
    std::vector<Launch> pl;
    for (int n = add_gemm_split(h, pl, name, ps), j = 0; j < n; ++j) launch_gemm(pl[j].gemm, st);
}

// The eager passes: net `net` (widths h->nd[ndi]) on m rows of X (row stride ldX, K0 inputs), its hidden
// layers alternating between H1b and H2b (layer 0 -> H1b, layer 1 -> H2b, ...), the head's N columns into out
static NetPass eager_pass(sacx_handle* h, const std::string& net, int ndi, const float* X, int ldX, int K0, int m, float* H1b,
                          float* H2b, int N = 0, float* out = nullptr) {
    NetPass c{};
    c.net = net; c.nd = &h->nd[ndi]; c.X = X; c.ldx = ldX; c.K0 = K0; c.M = m;
    for (int i = 0; i < c.nd->D(); ++i) c.H.push_back((i & 1) ? H2b : H1b);
    c.N = c.ldo = N; c.out = out;
    return c;
}

// The pass's hidden layers; returns the buffer holding the last.  The actor's --actor_layer_norm puts
// Dense -> LayerNorm -> tanh on layer 0 (nn_utils.py:110-119).
static float* net_hidden(sacx_handle* h, const NetPass& c, hipStream_t st, bool ln = false) {
    for (int i = 0; i < c.nd->D(); ++i) {
        GemmProb p = net_fwd_prob(h, c, i);
        if (i == 0 && ln) p.act = ACT_NONE;
        gemm_now(h, c.net + ".fwd", {p}, st);
        if (i == 0 && ln) {
            LNArgs a{};
            a.mode = 0; a.H = c.nd->h[0]; a.Z = c.H[0]; a.nrange = 1; a.r[1] = c.M; a.gamma = h->f("actor.ln");
            launch_ln(a, st);
        }
    }
    return c.H.back();
}
// the head (with the pass's `out`)
static void net_head(sacx_handle* h, const NetPass& c, hipStream_t st) {
    gemm_now(h, c.net + ".out", {net_fwd_prob(h, c, c.nd->D())}, st);
}

static float* actor_hidden(sacx_handle* h, const float* X, int ldX, int m, float* H1b, float* H2b, hipStream_t st) {
    return net_hidden(h, eager_pass(h, "actor", 0, X, ldX, h->S, m, H1b, H2b), st, h->ln);
}

// n normals of np.random.normal from the global stream into out
static void noise_draw(sacx_handle* h, int64_t n, float* out, hipStream_t st) {
    RngArgs r{};
    r.st = h->ptr<RngState>("rng"); r.ctl = h->ctl();
    r.n_int = 0; r.n_norm = (int32_t)n; r.out_idx = nullptr; r.out_norm = out;
    r.slot = -1; r.reset_seq = 0; r.nupd = 1;
    launch_rng(r, st);
}

static int actor_act(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, float* act_out,
                     uint32_t* done);
int sacx_actor_act(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, float* act_out) {
    return actor_act(h, obs, n, deterministic, act_out, nullptr);
}
// done: the rows' completion counter (act_host; k_act_rows path only)
static int actor_act(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, float* act_out,
                     uint32_t* done) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (h->softmax) return fail(h, "a softmax handle samples on the host from sacx_ppo_dist's logits (discrete_actors.py:22-42)");
    if (!deterministic && spec_cancel(h)) return -1;   // a draw from the stream: undo the speculative one
    if (n < 0 || (n > 0 && (!obs || !act_out))) return fail(h, "bad arguments");
    const int S = h->S, A = h->A, ldS = h->ldS;
    auto W = [&](const std::string& nm) { return h->f(nm); };
    if (act_rows_ok(h, n)) {
        // the env loop's few rows: the noise draw, then one workgroup per row (k_act_rows)
        float* noise = deterministic ? nullptr : W("act.noise");
        if (!deterministic) noise_draw(h, n * A, noise, h->stream);   // u = np.random.normal(size=(n, A))
        ActRowArgs a = act_rows_args(h, obs, noise, act_out);
        a.done = done;
        launch_act_rows(a, (int)n, h->stream);
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    for (int64_t done = 0; done < n; done += ACT_CAP) {
        const int m = (int)std::min<int64_t>(ACT_CAP, n - done);
        float* noise = deterministic ? nullptr : W("act.noise");
        if (!deterministic) noise_draw(h, (int64_t)m * A, noise, h->stream);   // u = np.random.normal(size=(m, A))
        launch_obs_norm(obs + done * S, m, S, W("norm.s_mean"), W("norm.s_den"), W("act.X"), ldS, h->stream);
        HeadArgs a = head_args(h, actor_hidden(h, W("act.X"), ldS, m, W("act.H1"), W("act.H2"), h->stream), nullptr, false);
        a.nseg = 1;
        // SquashedGaussianActor.sample (mode 1) or GaussianActor.sample (mode 2)
        a.seg[0] = {0, m, h->cfg.actor_gaussian ? 2 : 1, 0, noise, nullptr, nullptr, act_out + done * A};
        if (h->cfg.actor_gaussian) {
            a.logstd_init = logstd_init(h);
            a.output_norm = h->cfg.actor_output_norm;
        }
        a.total_rows = m;
        a.cache_row0 = 1 << 30;
        a.alpha_mode = 0;
        FinalArgs f{};
        launch_actor_head(a, f, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- reference object methods
// model = true: the world models' normaliser set (MSEModel calls), else the update's (QCritic)
static NetIOArgs netio_base(sacx_handle* h, bool model = false) {
    auto W = [&](const std::string& nm) { return h->f(nm); };
    auto N = [&](const char* x) { return model ? W(mnorm(h, x)) : W(std::string("norm.") + x); };
    NetIOArgs g{};
    g.S = h->S; g.A = h->A;
    g.s_mean = N("s_mean"); g.s_den = N("s_den"); g.a_mean = N("a_mean"); g.a_den = N("a_den");
    g.d_mean = N("d_mean"); g.d_den = N("d_den"); g.r_norm = N("r"); g.ret_den = W("norm.ret_den");
    g.reward_coef = h->cfg.reward_loss_coef;
    return g;
}

int sacx_actor_evaluate(sacx_handle* h, const float* s, int64_t n, float* pi_out, float* nlp_out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h)) return -1;
    if (h->cfg.actor_gaussian) return fail(h, "GaussianActor handle: inference only (sacx_actor_act)");
    if (n < 0 || (n > 0 && (!s || !pi_out || !nlp_out))) return fail(h, "bad arguments");
    const int S = h->S, A = h->A, ldS = h->ldS;
    auto W = [&](const std::string& nm) { return h->f(nm); };
    for (int64_t done = 0; done < n; done += ACT_CAP) {
        const int m = (int)std::min<int64_t>(ACT_CAP, n - done);
        noise_draw(h, (int64_t)m * A, W("act.noise"), h->stream);   // u = np.random.normal(size=np.shape(a_mean)) (:351)
        launch_obs_norm(s + done * S, m, S, W("norm.s_mean"), W("norm.s_den"), W("act.X"), ldS, h->stream);
        HeadArgs a = head_args(h, actor_hidden(h, W("act.X"), ldS, m, W("act.H1"), W("act.H2"), h->stream), nullptr, false);
        a.nseg = 1;
        a.seg[0] = {0, m, 0, 0, W("act.noise"), nullptr, nlp_out + done, pi_out + done * A};   // mode 0: evaluate
        a.total_rows = m;
        a.cache_row0 = 1 << 30;
        FinalArgs f{};
        launch_actor_head(a, f, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int sacx_critic_forward(sacx_handle* h, int32_t net, const float* s, const float* a, int64_t n, int32_t value,
                        float* out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h)) return -1;
    if (net < 0 || net > 3) return fail(h, "net must be 0..3 (q0, q1, t0, t1)");
    if (n < 0 || (n > 0 && (!s || !a || !out))) return fail(h, "bad arguments");
    const int S = h->S, A = h->A, ldQ = h->ldQ;
    auto W = [&](const std::string& nm) { return h->f(nm); };
    static const char* names[4] = {"q0", "q1", "t0", "t1"};
    for (int64_t done = 0; done < n; done += ACT_CAP) {
        const int m = (int)std::min<int64_t>(ACT_CAP, n - done);
        NetIOArgs g = netio_base(h);
        g.mode = 0; g.n = m; g.ldX = ldQ; g.s = s + done * S; g.a = a + done * A; g.X = W("act.Xq");
        launch_net_io(g, h->stream);
        const NetPass c = eager_pass(h, names[net], 1, W("act.Xq"), ldQ, S + A, m, W("act.H1"), W("act.H2"), 1, W("act.Q"));
        net_hidden(h, c, h->stream);
        net_head(h, c, h->stream);
        g.mode = 1; g.O = W("act.Q"); g.ldO = 1; g.value = value ? 1 : 0; g.out0 = out + done;
        launch_net_io(g, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// The world model's GEMM launches on the m rows of roll.Xm (stream st): the model net roll.Xm ->
// M1 -> M2 -> roll.O [m, S+1] (its Om columns), and with --separate_reward_nn the reward net
// (base_world_model.py:72-74) in the same launches into roll.O's reward column.  Model k's rows
// start at row k * rstride of M1 / M2 / O / R1 / R2 (nk models on the same inputs: the diagnostics)
static void model_gemms(sacx_handle* h, const std::vector<int>& models, int m, int64_t rstride, hipStream_t st,
                        const char* tag) {
    const int S = h->S, O = S + 1;
    auto W = [&](const std::string& nm) { return h->f(nm); };
    const int Dm = h->nd[2].D(), Dr = h->srn ? h->nd[3].D() : 0, Lf = std::max(Dm, Dr);
    // the hidden layers alternate between the two buffers of each net (layer 0 -> M1 / R1, layer 1 ->
    // M2 / R2, ...): their row stride is the layer's width, so model i's rows start at i * rstride * width
    auto pass = [&](const std::string& net, int ndi, const char* b1, const char* b2, size_t mi, int N, float* out) {
        NetPass c = eager_pass(h, net, ndi, W("roll.Xm"), h->ldQ, S + h->A, m, W(b1), W(b2), N, out);
        for (int i = 0; i < c.nd->D(); ++i) c.H[i] += mi * rstride * c.nd->h[i];
        c.ldo = O;
        return c;
    };
    std::vector<std::vector<GemmProb>> lv(Lf + 1);
    for (size_t mi = 0; mi < models.size(); ++mi) {
        float* Oo = W("roll.O") + mi * rstride * O;
        const NetPass cm = pass("m" + std::to_string(models[mi]), 2, "roll.M1", "roll.M2", mi, h->Om, Oo);
        for (int i = 0; i <= Dm; ++i) lv[i].push_back(net_fwd_prob(h, cm, i));
        if (h->srn) {     // the reward net into roll.O's reward column (base_world_model.py:72-74)
            const NetPass cr = pass("r" + std::to_string(models[mi]), 3, "roll.R1", "roll.R2", mi, 1, Oo + S);
            for (int i = 0; i <= Dr; ++i) lv[i].push_back(net_fwd_prob(h, cr, i));
        }
    }
    for (int i = 0; i <= Lf; ++i) gemm_now(h, std::string(tag) + ".fwd" + std::to_string(i), lv[i], st);
}

// the model net on rows [c0, c0 + m) of (s, a): roll.Xm -> roll.M1 -> roll.M2 -> roll.O
static void model_net_chunk(sacx_handle* h, int32_t model, const float* s, const float* a, int m) {
    NetIOArgs g = netio_base(h, true);
    g.mode = 0; g.n = m; g.ldX = h->ldQ; g.s = s; g.a = a; g.X = h->f("roll.Xm");
    launch_net_io(g, h->stream);
    model_gemms(h, {model}, m, 0, h->stream, "model");
}

// GaussianModel noise (continuous_models.py:40, :61): np.random.normal(size=(m, S)) from the device
// stream into roll.mnoise (+ offset rows)
static void model_noise_draw(sacx_handle* h, int64_t rows, int64_t row0, hipStream_t st) {
    noise_draw(h, rows * h->S, h->f("roll.mnoise") + row0 * h->S, st);
}

int sacx_model_sample(sacx_handle* h, int32_t model, const float* s, const float* a, int64_t n,
                      int32_t stochastic, float delta_clip, float reward_clip, float* pred_out, float* sp_out,
                      float* r_out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h)) return -1;
    if (!h->cfg.use_expert) return fail(h, "the world models exist only with use_expert");
    if (model < 0 || model >= h->nm) return fail(h, "model index out of range (num_models)");
    if (n < 0 || (n > 0 && (!s || !a))) return fail(h, "bad arguments");
    const int S = h->S;
    const bool noisy = stochastic && h->gm;
    for (int64_t done = 0; done < n; done += ROLL_CAP) {
        const int m = (int)std::min<int64_t>(ROLL_CAP, n - done);
        model_net_chunk(h, model, s + done * S, a + done * h->A, m);
        if (noisy) model_noise_draw(h, m, 0, h->stream);   // chunks in row order: one draw of (n, S)
        NetIOArgs g = netio_base(h, true);
        g.mode = 2; g.n = m; g.s = s + done * S; g.O = h->f("roll.O"); g.ldO = S + 1;
        g.clip_d = delta_clip; g.clip_r = reward_clip;
        g.out0 = pred_out ? pred_out + done * (S + 1) : nullptr;
        g.out1 = sp_out ? sp_out + done * S : nullptr;
        g.out2 = r_out ? r_out + done : nullptr;
        if (noisy) {
            g.mlogstd = h->f("m" + std::to_string(model) + ".logstd");
            g.mnoise = h->f("roll.mnoise");
        }
        launch_net_io(g, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int sacx_model_forward(sacx_handle* h, int32_t model, const float* s, const float* a, int64_t n, float delta_clip,
                       float reward_clip, float* pred_out, float* sp_out, float* r_out) {
    return sacx_model_sample(h, model, s, a, n, 0, delta_clip, reward_clip, pred_out, sp_out, r_out);
}

int sacx_model_loss(sacx_handle* h, int32_t model, const float* s, const float* sp, const float* a, const float* r,
                    int64_t n, float delta_clip_loss, float reward_clip_loss, float* loss_out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h)) return -1;
    if (!h->cfg.use_expert) return fail(h, "the world models exist only with use_expert");
    if (model < 0 || model >= h->nm) return fail(h, "model index out of range (num_models)");
    if (n <= 0 || !s || !sp || !a || !r || !loss_out) return fail(h, "bad arguments");
    const int S = h->S, A = h->A;
    for (int64_t done = 0; done < n; done += ROLL_CAP) {
        const int m = (int)std::min<int64_t>(ROLL_CAP, n - done);
        model_net_chunk(h, model, s + done * S, a + done * A, m);      // _forward(s, a, clip=False)
        NetIOArgs g = netio_base(h, true);
        g.mode = 3; g.n = m; g.s = s + done * S; g.sp = sp + done * S; g.r = r + done;
        g.O = h->f("roll.O"); g.ldO = S + 1;
        g.clip_d = delta_clip_loss; g.clip_r = reward_clip_loss;
        g.out0 = h->f("roll.noise");           // running sum (workspace scalar)
        g.out1 = loss_out;
        if (h->gm) {                           // GaussianModel.get_loss (continuous_models.py:101-131)
            g.mlogstd = h->f("m" + std::to_string(model) + ".logstd");
            g.lscale = h->lscale ? 1 : 0;
        }
        g.first = done == 0; g.last = done + m >= n; g.n_total = n;
        launch_net_io(g, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

static int run_rollout(sacx_handle* h, int32_t model, const float* s_init, int64_t n, int32_t horizon,
                       int32_t deterministic, float delta_clip, float reward_clip, float* s_out, float* a_out,
                       float* r_out, float* sp_out, uint8_t* d_out);
// the launches of one rollout call on stream st (eager, or captured by sacx_rollout)
// s_init == nullptr (sacx_sim_collect): the n start states are the ring rows np.random.randint(rows held,
// size=n) names -- the draw rides in the first sampler launch, ahead of step 0's normals (alone when
// deterministic), and step 0's prep reads the indices
static void enqueue_rollout(sacx_handle* h, int32_t model, const float* s_init, int64_t n, int32_t horizon,
                     int32_t deterministic, float delta_clip, float reward_clip, float* s_out, float* a_out,
                     float* r_out, float* sp_out, uint8_t* d_out, hipStream_t st) {
    const bool collect = s_init == nullptr;
    auto draw = [&](int n_int, int n_norm, float* noise) {
        RngArgs r{};
        r.st = h->ptr<RngState>("rng"); r.ctl = h->ctl();
        r.n_int = n_int; r.n_norm = n_norm; r.out_idx = n_int ? h->ptr<int32_t>("roll.idx") : nullptr; r.out_norm = noise;
        r.slot = -1; r.reset_seq = 0; r.nupd = 1;
        launch_rng(r, st);
    };
    const int S = h->S, A = h->A, ldS = h->ldS, ldQ = h->ldQ;
    auto W = [&](const std::string& nm) { return h->f(nm); };
    const std::string mn = "m" + std::to_string(model);
    // steps outer, chunks inner: each step draws normal(size=(n, A)) in row order, exactly the
    // reference's one draw per step (samplers.py:92) however the rows are chunked
    for (int t = 0; t < horizon; ++t) {
        for (int64_t c0 = 0; c0 < n; c0 += ROLL_CAP) {
            const int m = (int)std::min<int64_t>(ROLL_CAP, n - c0);
            RollArgs ra{};
            ra.n = m; ra.S = S; ra.A = A; ra.H = horizon; ra.t = t; ra.ldS = ldS; ra.ldQ = ldQ;
            ra.s_init = collect ? nullptr : s_init + c0 * S;
            ra.s_out = s_out + c0 * horizon * S; ra.a_out = a_out + c0 * horizon * A;
            ra.r_out = r_out + c0 * horizon; ra.sp_out = sp_out + c0 * horizon * S; ra.d_out = d_out + c0 * horizon;
            ra.O = W("roll.O"); ra.a_raw = W("roll.A"); ra.X = W("roll.X"); ra.Xm = W("roll.Xm");
            ra.s_mean = W("norm.s_mean"); ra.s_den = W("norm.s_den");          // the actor's
            ra.ms_mean = W("mnorm.s_mean"); ra.ms_den = W("mnorm.s_den");      // the model's
            ra.d_mean = W("mnorm.d_mean"); ra.d_den = W("mnorm.d_den"); ra.r_norm = W("mnorm.r");
            ra.clip_d = delta_clip; ra.clip_r = reward_clip;
            if (h->gm) {               // GaussianModel.step: exp(logstd) * u (continuous_models.py:38-41)
                ra.mlogstd = W(mn + ".logstd");
                ra.mnoise = W("roll.mnoise");
            }
            ra.mode = 0;
            float* noise = deterministic ? nullptr : W("roll.noise");
            const bool first = collect && t == 0 && c0 == 0;
            if (collect && t == 0) {
                ra.idx = h->ptr<int32_t>("roll.idx") + c0; ra.replay = W("replay"); ra.cap = h->cap;
                ra.stride = h->stride; ra.ctl = h->ctl();
                // all n indices, then this chunk's normals, in the reference's order (get_states before
                // the first actor.sample); the prep reads them, so it follows the draw here
                if (first) draw((int)n, deterministic ? 0 : m * A, noise);
            }
            launch_roll(ra, st);
            ra.idx = nullptr;
            // actor.sample: u = np.random.normal(size=(m, A))
            if (!deterministic && !first) draw(0, m * A, noise);
            HeadArgs a = head_args(h, actor_hidden(h, W("roll.X"), ldS, m, W("roll.H1"), W("roll.H2"), st), nullptr, false);
            a.ma_mean = W("mnorm.a_mean"); a.ma_den = W("mnorm.a_den");
            a.nseg = 1;
            // sample(): raw action to roll.A, normalised clip(a) (= a: |lim tanh| <= lim) into
            // the action columns of the model input
            a.seg[0] = {0, m, 1, 0, noise, W("roll.Xm"), nullptr, W("roll.A")};
            if (h->models_only) {
                // GaussianActor.sample (continuous_actors.py:103-123; mode 2 as sacx_actor_act has it): the
                // raw action to roll.A, the normalised actor.clip(a) into the model input
                a.seg[0].mode = 2;
                a.logstd_init = logstd_init(h);
                a.output_norm = h->cfg.actor_output_norm;
            }
            a.total_rows = m;
            a.cache_row0 = 1 << 30;
            a.alpha_mode = 0;
            FinalArgs f{};
            launch_actor_head(a, f, st);
            model_gemms(h, {model}, m, 0, st, "roll.m");
            if (h->gm) model_noise_draw(h, m, 0, st);    // after the actor's draw (samplers.py:93-95)
            ra.mode = 1;
            launch_roll(ra, st);
        }
    }
}

int sacx_rollout(sacx_handle* h, int32_t model, const float* s_init, int64_t n, int32_t horizon,
                 int32_t deterministic, float delta_clip, float reward_clip, float* s_out, float* a_out,
                 float* r_out, float* sp_out, uint8_t* d_out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (h->softmax) return fail(h, "a softmax handle samples on the host from sacx_ppo_dist's logits (discrete_actors.py:22-42)");
    if (!h->cfg.use_expert) return fail(h, "rollout needs the world models (use_expert)");
    if (model < 0 || model >= h->nm) return fail(h, "model index out of range (num_models)");
    if (n < 0 || horizon < 0) return fail(h, "bad arguments");
    if (n == 0 || horizon == 0) return 0;
    if (!s_init || !s_out || !a_out || !r_out || !sp_out || !d_out) return fail(h, "null output");
    if (h->gm && n > ROLL_CAP)   // one step's draws: the actor's (n, A), then the model's (n, S)
        return fail(h, "GaussianModel rollout: at most 4096 trajectories per call (the draws of a step interleave)");
    if (settle(h)) return -1;
    return run_rollout(h, model, s_init, n, horizon, deterministic, delta_clip, reward_clip, s_out, a_out, r_out,
                       sp_out, d_out);
}

int sacx_sim_collect(sacx_handle* h, int32_t model, int64_t n, int32_t horizon, int32_t deterministic,
                     float delta_clip, float reward_clip, float* s_out, float* a_out, float* r_out, float* sp_out,
                     uint8_t* d_out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (h->softmax) return fail(h, "a softmax handle samples on the host from sacx_ppo_dist's logits (discrete_actors.py:22-42)");
    if (!h->cfg.use_expert) return fail(h, "sim_collect needs the world models (use_expert)");
    if (!h->models_only)
        return fail(h, "sim_collect: a use_expert = SACX_EXPERT_MODELS handle only (the ring holds the env data there)");
    if (model < 0 || model >= h->nm) return fail(h, "model index out of range (num_models)");
    if (n < 0 || horizon < 0) return fail(h, "sim_collect: n_traj and horizon must be >= 0");
    if (n > SIM_IDX_CAP) return fail(h, "sim_collect: at most 65536 trajectories per call");
    if (h->gm && n > ROLL_CAP)   // one step's draws: the actor's (n, A), then the model's (n, S)
        return fail(h, "GaussianModel rollout: at most 4096 trajectories per call (the draws of a step interleave)");
    if (flush_append(h)) return -1;
    if (settle(h)) return -1;
    if (h->cur_size_host <= 0) return fail(h, "sim_collect: the replay ring is empty (np.random.randint(0) raises)");
    if (n == 0 || horizon == 0) return 0;
    if (!s_out || !a_out || !r_out || !sp_out || !d_out) return fail(h, "null output");
    return run_rollout(h, model, nullptr, n, horizon, deterministic, delta_clip, reward_clip, s_out, a_out, r_out,
                       sp_out, d_out);
}

int sacx_model_losses_eval(sacx_handle* h, int32_t model, const float* s, const float* sp, const float* a,
                           const float* r, int64_t n, float* out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (settle(h)) return -1;
    if (!h->cfg.use_expert) return fail(h, "the world models exist only with use_expert");
    if (model < 0 || model >= h->nm) return fail(h, "model index out of range (num_models)");
    if (n <= 0 || !s || !sp || !a || !r || !out) return fail(h, "bad arguments");
    const int S = h->S, A = h->A;
    for (int64_t done = 0; done < n; done += ROLL_CAP) {
        const int m = (int)std::min<int64_t>(ROLL_CAP, n - done);
        model_net_chunk(h, model, s + done * S, a + done * A, m);      // _forward(s, a, clip=False)
        NetIOArgs g = netio_base(h, true);
        g.mode = 4; g.n = m; g.s = s + done * S; g.sp = sp + done * S; g.r = r + done;
        g.O = h->f("roll.O"); g.ldO = S + 1;
        g.out0 = h->f("roll.noise");           // the two running sums (workspace; ROLL_CAP * A >= 2 floats)
        g.out1 = out;
        g.first = done == 0; g.last = done + m >= n; g.n_total = n;
        launch_net_io(g, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// runs (or replays) the rollout's launches; s_init == nullptr: sacx_sim_collect
static int run_rollout(sacx_handle* h, int32_t model, const float* s_init, int64_t n, int32_t horizon,
                       int32_t deterministic, float delta_clip, float reward_clip, float* s_out, float* a_out,
                       float* r_out, float* sp_out, uint8_t* d_out) {
    // one captured graph per (model, shape, clips, pointers): the Python host keeps its
    // staging / output buffers per shape, so repeated calls replay (SACX_ROLL_GRAPH=0: eager)
    const char* rg = std::getenv("SACX_ROLL_GRAPH");
    if (rg && std::atoi(rg) == 0) {
        enqueue_rollout(h, model, s_init, n, horizon, deterministic, delta_clip, reward_clip, s_out, a_out, r_out,
                        sp_out, d_out, h->stream);
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    RollKey key{model, h->sel, n, horizon, deterministic, delta_clip, reward_clip, {s_init, s_out, a_out, r_out, sp_out, d_out}};
    hipGraphExec_t ge = nullptr;
    for (auto& kv : h->roll_graphs)
        if (std::memcmp(&kv.first, &key, sizeof(RollKey)) == 0) ge = kv.second;
    if (!ge) {
        auto body = [&](hipStream_t cs) {
            enqueue_rollout(h, model, s_init, n, horizon, deterministic, delta_clip, reward_clip, s_out, a_out, r_out,
                            sp_out, d_out, cs);
            return 0;
        };
        // (every node is a kernel launch: sacx_rollout_launches)
        if (capture_graph(h, "rollout", body, &ge, false, &h->roll_nodes)) return -1;
        if (h->roll_graphs.size() >= 4) {          // a few shapes live at once; drop the oldest
            (void)hipGraphExecDestroy(h->roll_graphs.front().second);
            h->roll_graphs.erase(h->roll_graphs.begin());
        }
        h->roll_graphs.push_back({key, ge});
    }
    HIPCHK(h, hipGraphLaunch(ge, h->stream));
    return 0;
}

int sacx_expert_diag(sacx_handle* h, const float* s_e, const float* a_e, const float* sp_e, int32_t n,
                     int32_t flags, float delta_clip, float* out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (!h->cfg.use_expert) return fail(h, "expert diagnostics need the world models (use_expert)");
    if (h->models_only) return fail(h, "use_expert = SACX_EXPERT_MODELS: no expert term to diagnose (sacx_expert_diag)");
    if (n <= 0 || n > 2048) return fail(h, "expert rows must be in [1, 2048]");
    const bool disc = (flags & SACX_DIAG_DISC) != 0, ea = (flags & SACX_DIAG_EXPERT_ACTIONS) != 0;
    if (disc && h->nm < 2) return fail(h, "_calc_disc compares two world models (num_models >= 2)");
    if (!s_e || !sp_e || !out || (ea && !a_e) || (!disc && !a_e)) return fail(h, "null argument");
    if (settle(h)) return -1;
    const int S = h->S, A = h->A, ldS = h->ldS, ldQ = h->ldQ;
    auto W = [&](const std::string& nm) { return h->f(nm); };
    DiagArgs d{};
    d.n = n; d.S = S; d.A = A; d.ldS = ldS; d.ldQ = ldQ;
    d.s_e = s_e; d.a_e = a_e; d.sp_e = sp_e; d.O = W("roll.O"); d.X = W("roll.X"); d.Xm = W("roll.Xm");
    d.s_mean = W("norm.s_mean"); d.s_den = W("norm.s_den");                 // the actor's
    d.ms_mean = W("mnorm.s_mean"); d.ms_den = W("mnorm.s_den");             // the models'
    d.a_mean = W("mnorm.a_mean"); d.a_den = W("mnorm.a_den");
    d.d_mean = W("mnorm.d_mean"); d.d_den = W("mnorm.d_den"); d.clip_d = delta_clip; d.out = out;
    // every model on the same n input rows: model k's rows land at [k n, (k+1) n)
    // (one model: its MSE twice, the mean is exact); _calc_disc reads models 0 and 1
    std::vector<int> all;
    for (int k = 0; k < std::max(2, h->nm); ++k) all.push_back(h->nm > 1 ? k : 0);
    d.nmod = (int)all.size();
    auto models = [&](bool two) {
        model_gemms(h, two ? std::vector<int>{0, 1} : all, n, n, h->stream, "diag.m");
    };
    // actor.sample(s_e, deterministic=False) (continuous_actors.py:270-306) into the action columns
    auto counterfactual = [&]() {
        RngArgs r{};
        r.st = h->ptr<RngState>("rng"); r.ctl = h->ctl();
        r.n_int = 0; r.n_norm = n * A; r.out_idx = nullptr; r.out_norm = W("roll.noise");
        r.slot = -1; r.reset_seq = 0; r.nupd = 1;
        launch_rng(r, h->stream);
        HeadArgs a = head_args(h, actor_hidden(h, W("roll.X"), ldS, n, W("roll.H1"), W("roll.H2"), h->stream), nullptr, false);
        a.ma_mean = W("mnorm.a_mean"); a.ma_den = W("mnorm.a_den");
        a.nseg = 1;
        a.seg[0] = {0, n, 1, 0, W("roll.noise"), W("roll.Xm"), nullptr, W("roll.A")};
        a.total_rows = n;
        a.cache_row0 = 1 << 30;
        FinalArgs f{};
        launch_actor_head(a, f, h->stream);
    };
    d.mode = 0;
    d.a_e = (disc && !ea) ? nullptr : a_e;
    launch_diag(d, h->stream);
    if (disc) {                      // _calc_disc (SAC_expert.py:427-460)
        if (!ea) counterfactual();
        models(true);
        if (h->gm) {                 // model.sample(deterministic=False): (n, S) for every model in order
            model_noise_draw(h, (int64_t)h->nm * n, 0, h->stream);
            d.mlogstd[0] = W("m0.logstd");
            d.mlogstd[1] = W("m1.logstd");
            d.mnoise = W("roll.mnoise");
        }
        d.mode = 3;
        launch_diag(d, h->stream);
    } else {                         // SAC_expert.py:579-608
        models(false);
        d.mode = 1;
        launch_diag(d, h->stream);
        if (!ea) {
            counterfactual();
            models(false);
        }
        d.mode = 2;                  // use_expert_actions: the counterfactual MSE is the data MSE
        launch_diag(d, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int sacx_time_kernels(sacx_handle* h, const char* kernel, int32_t n_replays, double* avg_us, double* us_per_update,
                      int64_t* n_launches) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (!kernel || std::strcmp(kernel, "k_gemm") != 0) return fail(h, "only k_gemm carries timestamps");
    if (settle(h)) return -1;
    wbf_refresh(h, h->stream);
    if (!avg_us || n_replays <= 0) return fail(h, "bad arguments");
    const int G = h->graph_steps;
    KTimeMap kt;
    kt.cap = (int64_t)G * 16 * 4096 * 2 * h->seeds;    // generous: <= 16 GEMM launches x 4096 WGs per update
    kt.rows = std::getenv("SACX_KTIME_DUMP") != nullptr;
    HIPCHK(h, hipMalloc(&kt.base, kt.cap * sizeof(uint64_t)));
    hipGraphExec_t g = nullptr;
    int rc = get_graph(h, G, true, &g, -1, &kt);
    double sum = 0.0;
    int64_t cnt = 0;
    std::vector<uint64_t> host((size_t)kt.used);
    for (int r = 0; rc == 0 && r < n_replays; ++r) {
        if (hipGraphLaunch(g, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
            hipMemcpy(host.data(), kt.base, host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(h, "timing replay failed");
            break;
        }
        // diagnostics: SACX_KTIME_DUMP=<file> appends one line per launch of the last replay:
        // name, span, mean / max workgroup duration, last-start offset, gap to the previous end (us)
        FILE* dump = nullptr;
        if (r == n_replays - 1)
            if (const char* path = std::getenv("SACX_KTIME_DUMP")) dump = std::fopen(path, "a");
        uint64_t prev_hi = 0;
        for (size_t si = 0; si < kt.spans.size(); ++si) {
            const auto& sp = kt.spans[si];
            uint64_t lo = UINT64_MAX, hi = 0, last_start = 0, wmax = 0, rmax = 0;
            double wsum = 0.0, rsum = 0.0;
            const int rb0 = kt.rowspan[si].first, rb1 = kt.rowspan[si].second;
            const int nt = sp.second - (rb1 - rb0) * h->seeds;
            const int per = sp.second / h->seeds;     // workgroups per seed (seed-major slots)
            for (int b = 0; b < sp.second; ++b) {
                const uint64_t t0 = host[sp.first + 2 * b], t1 = host[sp.first + 2 * b + 1];
                lo = std::min(lo, t0);
                hi = std::max(hi, t1);
                last_start = std::max(last_start, t0);
                const int bx = b % per;
                if (bx < rb0 || bx >= rb1) {
                    wmax = std::max(wmax, t1 - t0);
                    wsum += (double)(t1 - t0);
                } else {
                    rmax = std::max(rmax, t1 - t0);
                    rsum += (double)(t1 - t0);
                }
            }
            if (kt.is_gemm[si]) {
                sum += (double)(hi - lo) * 0.01;         // 100 MHz ticks -> us
                ++cnt;
            }
            if (dump)
                std::fprintf(dump, "%s,%d,%.2f,%.2f,%.2f,%.2f,%.2f,%.2f,%.2f\n", kt.names[si].c_str(), sp.second,
                             (hi - lo) * 0.01, wsum / std::max(1, nt) * 0.01, wmax * 0.01, (last_start - lo) * 0.01,
                             prev_hi ? ((double)lo - (double)prev_hi) * 0.01 : 0.0,
                             rb1 > rb0 ? rsum / ((rb1 - rb0) * h->seeds) * 0.01 : 0.0, rmax * 0.01);
            prev_hi = hi;
        }
        if (dump) std::fclose(dump);
        // SACX_KTIME_CLASSES=<file>: k_fwd2 launches' workgroups by problem pair (mean / max us)
        if (const char* path = std::getenv("SACX_KTIME_CLASSES"); path && r == n_replays - 1 && h->seeds == 1) {
            if (FILE* f = std::fopen(path, "a")) {
                for (size_t si = 0; si < kt.spans.size(); ++si) {
                    const auto& cb = kt.cls[si];
                    if (cb.empty()) continue;
                    const auto& sp = kt.spans[si];
                    std::fprintf(f, "%s", kt.names[si].c_str());
                    for (size_t c = 0; c < cb.size(); ++c) {
                        const int b0 = cb[c], b1 = c + 1 < cb.size() ? cb[c + 1] : sp.second;
                        double su = 0.0, mx = 0.0;
                        for (int b = b0; b < b1; ++b) {
                            const double d = (double)(host[sp.first + 2 * b + 1] - host[sp.first + 2 * b]) * 0.01;
                            su += d;
                            mx = std::max(mx, d);
                        }
                        std::fprintf(f, ",p%zu:%d:%.2f:%.2f", c, b1 - b0, su / std::max(1, b1 - b0), mx);
                    }
                    std::fprintf(f, "\n");
                }
                std::fclose(f);
            }
        }
    }
    if (g) (void)hipGraphExecDestroy(g);
    (void)hipFree(kt.base);
    if (rc) return rc;
    h->seq_host += (int64_t)n_replays * G;
    *avg_us = cnt ? sum / cnt : 0.0;
    if (us_per_update) *us_per_update = sum / ((double)n_replays * G);
    if (n_launches) *n_launches = cnt / n_replays;
    return 0;
}

int sacx_time_graph(sacx_handle* h, int64_t n_replays, const char* skip_kernel, double* ms_out) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (!ms_out || n_replays <= 0) return fail(h, "bad arguments");
    if (settle(h)) return -1;
    wbf_refresh(h, h->stream);
    int skip = -1;
    if (skip_kernel && skip_kernel[0]) {
        for (int k = Launch::RNG; k <= Launch::MFINAL; ++k)
            if (std::strcmp(kernel_family((Launch::Kind)k), skip_kernel) == 0) skip = k;
        if (skip < 0 || skip == Launch::GATHER) return fail(h, "unknown or non-removable kernel family");
    }
    hipGraphExec_t g;
    if (get_graph(h, h->graph_steps, true, &g, skip)) return -1;
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    HIPCHK(h, hipGraphLaunch(g, h->stream));   // warm
    HIPCHK(h, hipEventRecord(e0, h->stream));
    for (int64_t i = 0; i < n_replays; ++i) HIPCHK(h, hipGraphLaunch(g, h->stream));
    HIPCHK(h, hipEventRecord(e1, h->stream));
    HIPCHK(h, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_out = ms;
    h->seq_host += (n_replays + 1) * h->graph_steps;
    return 0;
}

// ---------------------------------------------------------------- PPO actor update
// One minibatch step of mb rows (ppo.py:122-147, :225-239) as a launch list:
//   ppo.gather     table rows by index -> normalised states, actions, adv (centred / scaled), nlp_old
//   actor.fwd<i>   the hidden layers (actor.ln behind layer 0), then the output layer as a plain GEMM
//   ppo.head       the distribution, nlp_cur, r, the clipped surrogate's branch, d loss / d output
//   actor.bwd<i>   dX from the output layer down (actor.ln.bwd behind layer 0's)
//   actor.grad     every dW (+ the logstd / layer-norm column sums) stored, not applied (EPI_STORE)
//   actor.gnorm    the gradient range's sum of squares by chunks
//   ppo.final      means, the clip scale, alpha's step, the statistics row, the counters
//   actor.adam     Keras Adam over the actor's parameter range at the device-read rate
static std::vector<Launch> make_ppo_plan(sacx_handle* h, int mb) {
    std::vector<Launch> plan;
    const int S = h->S, A = h->A, Aout = h->Aout, ldS = h->ldS;
    const int Da = h->nd[0].D();
    auto W = [&](const std::string& n) { return h->f(n); };
    PpoCtl* pctl = h->ptr<PpoCtl>("ppo.ctl");
    PpoPar* par = h->ptr<PpoPar>("ppo.par");
    float *X = W("ppo.X"), *O = W("ppo.O"), *acc = W("ppo.acc");
    ActorPass ap = actor_pass_ws(h, X, mb, 0, mb);           // the minibatch: rows [0, mb) of the update's workspace
    ap.O = O;
    {
        Launch L{};
        L.kind = Launch::PPOGATHER;
        L.name = "ppo.gather";
        PpoGatherArgs& g = L.pg;
        g.s = W("ppo.s"); g.a = W("ppo.a"); g.adv = W("ppo.adv"); g.nlp_old = W("ppo.nlp_old");
        g.idx_ring = h->ptr<int32_t>("ppo.idx"); g.idx_ld = h->B;
        g.ctl = pctl; g.par = par;
        g.s_mean = W("norm.s_mean"); g.s_den = W("norm.s_den");
        g.S = S; g.A = h->softmax ? 1 : A; g.mb = mb; g.ldS = ldS;      // (softmax: the one action-index column)
        g.X = X; g.Arow = W("ppo.A"); g.advn = W("ppo.advn"); g.nlpo = W("ppo.nlpo"); g.acc = acc;
        L.grid = (mb + PPO_GATHER_ROWS - 1) / PPO_GATHER_ROWS;
        L.bytes = 4.0 * mb * (S + ldS + 2.0 * A + 4);
        plan.push_back(L);
    }
    actor_fwd_chain(h, plan, ap, "actor.fwd", "actor.ln");
    {
        Launch L{};
        L.kind = Launch::PPOHEAD;
        L.name = "ppo.head";
        PpoHeadArgs& a = L.ph;
        a.d = ppo_dist(h, O); a.mb = mb;
        a.Arow = W("ppo.A"); a.advn = W("ppo.advn"); a.nlpo = W("ppo.nlpo");
        a.alpha = W("ppo.alpha"); a.par = par;
        a.D3 = ap.D3; a.E = ap.E; a.row_loss = W("ppo.rl"); a.row_ent = W("ppo.rl") + h->B;
        L.grid = (mb + 3) / 4;
        L.flops = 40.0 * mb * A;
        L.bytes = 4.0 * mb * (2.0 * Aout + 2.0 * A + 4);
        plan.push_back(L);
    }
    actor_bwd_chain(h, plan, ap, Da);
    store_grads(plan, add_gemm_split(h, plan, "actor.grad", actor_dw_probs(h, ap)));      // the clip comes first
    const ParamRange ar = actor_range(h);
    float* P = ar.P;
    const int64_t n = ar.n;
    {
        Launch N{};
        N.kind = Launch::GNPART;
        N.name = "actor.gnorm";
        N.gn.g = P + 3 * h->p_stride; N.gn.n = n; N.gn.part = W("ppo.gnorm");
        N.grid = GNORM_PARTS;
        N.bytes = 4.0 * n;
        plan.push_back(N);
    }
    {
        Launch L{};
        L.kind = Launch::PPOFINAL;
        L.name = "ppo.final";
        PpoFinalArgs& a = L.pf;
        a.mb = mb; a.row_loss = W("ppo.rl"); a.row_ent = W("ppo.rl") + h->B; a.gpart = W("ppo.gnorm");
        a.par = par; a.ctl = pctl; a.alpha = W("ppo.alpha"); a.acc = acc;
        a.stats = W("ppo.stats"); a.stats_cap = h->stats_cap;
        L.grid = 1;
        L.bytes = 4.0 * (2.0 * mb + GNORM_PARTS);
        plan.push_back(L);
    }
    {
        Launch U = adam_apply_launch(h, "actor.adam", P, n, GRP_PI, acc + PPO_ACC_SCALE, 1);   // ppo.final advanced t_pi
        U.ap.lr_dev = &par->actor_lr; U.ap.t_dev = &pctl->t_pi;
        plan.push_back(U);
    }
    return plan;
}
static const std::vector<Launch>& build_ppo_plan(sacx_handle* h, int mb) {
    auto it = h->ppo_plans.find(mb);
    if (it != h->ppo_plans.end()) return it->second;
    return h->ppo_plans.emplace(mb, make_ppo_plan(h, mb)).first->second;
}

// The plan of the packed steps (sacx_learners_init): `make`'s launch list on learner 0's arena block,
// whichever learner is selected, every launch at grid z = K (pack_seeds)
static const std::vector<Launch>& packed_plan(sacx_handle* h, std::map<int, std::vector<Launch>>& cache, int mb,
                                              std::vector<Launch> (*make)(sacx_handle*, int)) {
    auto it = cache.find(mb);
    if (it != cache.end()) return it->second;
    char* const sel_arena = h->arena;
    h->arena = h->arena0;
    std::vector<Launch> plan = make(h, mb);
    h->arena = sel_arena;
    for (Launch& L : plan) pack_seeds(L, (int64_t)h->seed_bytes, h->seeds);
    return cache.emplace(mb, std::move(plan)).first->second;
}
static int packed_check(sacx_handle* h, const char* one) {
    if (h->learners < 2)
        return fail(h, std::string("the handle holds one learner (sacx_learners_init was not called): use ") + one);
    return 0;
}

static int ppo_check(sacx_handle* h) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (!h->ppo)
        return fail(h, "not a trainable GaussianActor handle (actor_gaussian = SACX_ACTOR_GAUSSIAN_TRAIN): no PPO actor update");
    return 0;
}

// the actor on m <= ACT_CAP caller rows s: normalise, hidden layers, the output layer -> ppo.O [m, Aout]
static PpoDist ppo_forward(sacx_handle* h, const float* s, int m) {
    auto W = [&](const std::string& nm) { return h->f(nm); };
    launch_obs_norm(s, m, h->S, W("norm.s_mean"), W("norm.s_den"), W("act.X"), h->ldS, h->stream);
    const NetPass c = eager_pass(h, "actor", 0, W("act.X"), h->ldS, h->S, m, W("act.H1"), W("act.H2"), h->Aout, W("ppo.O"));
    net_hidden(h, c, h->stream, h->ln);
    net_head(h, c, h->stream);
    return ppo_dist(h, W("ppo.O"));
}

// the whole-rollout passes: n rows of s through the actor in chunks, k_ppo_rows on each; the
// prototype's row pointers are those of row 0 and move with the chunk
static int ppo_rows_pass(sacx_handle* h, const float* s, int64_t n, const PpoRowsArgs& proto) {
    const int S = h->S, A = h->A;
    for (int64_t done = 0; done < n; done += ACT_CAP) {
        const int m = (int)std::min<int64_t>(ACT_CAP, n - done);
        PpoRowsArgs r = proto;
        r.d = ppo_forward(h, s + done * S, m);
        r.m = m;
        auto mv = [&](auto*& p, int64_t w) { if (p) p += done * w; };
        mv(r.a, h->softmax ? 1 : A); mv(r.nlp_old, 1); mv(r.mean_ref, A); mv(r.ls_ref, A);
        mv(r.nlp_out, 1); mv(r.mean_out, A); mv(r.ls_out, A); mv(r.ent_out, 1); mv(r.kl_out, 1); mv(r.rdiff_out, 1);
        launch_ppo_rows(r, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int sacx_ppo_neglogp(sacx_handle* h, const float* s, const float* a, int64_t n, float* nlp_out) {
    if (ppo_check(h)) return -1;
    if (n < 0 || (n > 0 && (!s || !a || !nlp_out))) return fail(h, "bad arguments");
    PpoRowsArgs r{};
    r.a = a; r.nlp_out = nlp_out;
    return ppo_rows_pass(h, s, n, r);
}

int sacx_ppo_dist(sacx_handle* h, const float* s, int64_t n, float* mean_out, float* logstd_out, float* ent_out) {
    if (ppo_check(h)) return -1;
    if (n < 0 || (n > 0 && !s)) return fail(h, "bad arguments");
    if (h->softmax && logstd_out) return fail(h, "a softmax handle has no logstd: logstd_out must be NULL");
    PpoRowsArgs r{};
    r.mean_out = mean_out; r.ls_out = logstd_out; r.ent_out = ent_out;
    return ppo_rows_pass(h, s, n, r);
}

// SoftMaxActor.sample (discrete_actors.py:22-42) on the device: per chunk the uniform draw
// u = np.random.random(size=(m, A)) as Gumbel noise in act.noise (k_rng_unif), the logits, the pick.
// Few rows (act_rows_ok, as sacx_actor_act): one workgroup per row (k_softmax_rows); otherwise
// sacx_ppo_dist's chain into ppo.O and k_softmax_pick.  done: the rows' completion counter (_host form)
static int softmax_act(sacx_handle* h, const char* who, const float* obs, int64_t n, int32_t deterministic,
                       int32_t* act_out, double* u_out, uint32_t* done) {
    if (!h) return fail(h, "not bound");
    if (!h->softmax)
        return fail(h, std::string(who) + ": not a softmax handle (sacx_softmax_init); a Gaussian handle acts with sacx_actor_act");
    if (!h->bound) return fail(h, "not bound");
    if (n < 0 || (n > 0 && (!obs || !act_out))) return fail(h, std::string(who) + ": bad arguments");
    if (settle(h)) return -1;
    const int S = h->S, A = h->A;
    auto W = [&](const std::string& nm) { return h->f(nm); };
    float* const noise = deterministic ? nullptr : W("act.noise");
    auto draw = [&](int m, int64_t row0) {       // the chunk's rows of u, in stream order
        UnifArgs r{};
        r.st = h->ptr<RngState>("rng"); r.g_out = noise; r.u_out = u_out ? u_out + row0 * A : nullptr; r.n = m * A;
        launch_rng_unif(r, h->stream);
    };
    if (act_rows_ok(h, n)) {
        if (!deterministic) draw((int)n, 0);
        ActRowArgs a = act_rows_args(h, obs, noise, reinterpret_cast<float*>(act_out));
        a.done = done;
        launch_softmax_rows(a, (int)n, h->stream);
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    for (int64_t at = 0; at < n; at += ACT_CAP) {
        const int m = (int)std::min<int64_t>(ACT_CAP, n - at);
        if (!deterministic) draw(m, at);
        const PpoDist d = ppo_forward(h, obs + at * S, m);
        SoftmaxPickArgs p{};
        p.O = d.O; p.g = noise; p.out = act_out + at; p.m = m; p.A = A; p.ldO = h->Aout;
        launch_softmax_pick(p, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int sacx_softmax_act(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, int32_t* act_out,
                     double* u_out) {
    return softmax_act(h, "sacx_softmax_act", obs, n, deterministic, act_out, u_out, nullptr);
}

// host pointers: the rows through the act half of the pinned mapped buffer, synchronous
// (as sacx_actor_act_host; the indices come back in the same buffer, behind the observations)
int sacx_softmax_act_host(sacx_handle* h, const float* obs, int64_t n, int32_t deterministic, int32_t* act_out) {
    if (!h) return fail(h, "not bound");
    if (!h->softmax)
        return fail(h, "sacx_softmax_act_host: not a softmax handle (sacx_softmax_init); a Gaussian handle acts with sacx_actor_act");
    if (!h->bound) return fail(h, "not bound");
    if (n < 0 || (n > 0 && (!obs || !act_out))) return fail(h, "sacx_softmax_act_host: bad arguments");
    const int S = h->S;
    const int64_t chunk = std::min<int64_t>(ACT_CAP, STAGE_CAP / (S + 1));
    if (chunk <= 0) return fail(h, "an observation row is larger than the pinned staging buffer (use sacx_softmax_act)");
    for (int64_t at = 0; at < n; at += chunk) {
        const int64_t m = std::min(chunk, n - at);
        if (stage_alloc(h)) return -1;
        float* p = h->pin + STAGE_CAP;          // the act half: its last reader was a synchronous act
        float* g = h->pin_dev + STAGE_CAP;
        std::memcpy(p, obs + at * S, sizeof(float) * m * S);
        const bool rows = act_rows_ok(h, m);     // k_softmax_rows: the host polls the rows' count
        const int rc = softmax_act(h, "sacx_softmax_act_host", g, m, deterministic, reinterpret_cast<int32_t*>(g + m * S),
                                   nullptr, rows ? h->done_dev : nullptr);
        if (rc) return rc;
        if (rows) h->done_seq += (uint32_t)m;    // only once the launch that counts them is queued
        h->act_ev_live = !(rows && h->act_poll && h->app_ctr);
        if (h->act_ev_live) HIPCHK(h, hipEventRecord(h->act_ev, h->stream));
        if (rows) {
            if (act_rows_wait(h)) return -1;
        } else {
            HIPCHK(h, hipEventSynchronize(h->act_ev));
        }
        std::memcpy(act_out + at, p + m * S, sizeof(int32_t) * m);
    }
    return 0;
}

int sacx_ppo_kl(sacx_handle* h, const float* s, const float* mean_ref, const float* logstd_ref, int64_t n,
                float* kl_out) {
    if (ppo_check(h)) return -1;
    if (h->softmax && logstd_ref) return fail(h, "a softmax handle has no logstd: logstd_ref must be NULL");
    if (n < 0 || (n > 0 && (!s || !mean_ref || (!logstd_ref && !h->softmax) || !kl_out))) return fail(h, "bad arguments");
    PpoRowsArgs r{};
    r.mean_ref = mean_ref; r.ls_ref = logstd_ref; r.kl_out = kl_out;
    return ppo_rows_pass(h, s, n, r);
}

int sacx_ppo_begin(sacx_handle* h, const float* s, const float* a, const float* adv, int64_t n) {
    if (ppo_check(h)) return -1;
    if (!s || !a || !adv) return fail(h, "null rollout pointer");
    if (n < 1 || n > h->cap)
        return fail(h, "rollout rows " + std::to_string(n) + " outside [1, buffer_capacity = " + std::to_string(h->cap) + "]");
    const int S = h->S, A = h->A;
    auto W = [&](const std::string& nm) { return h->f(nm); };
    HIPCHK(h, hipMemcpyAsync(W("ppo.s"), s, sizeof(float) * (size_t)n * S, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(W("ppo.a"), a, sizeof(float) * (size_t)n * (h->softmax ? 1 : A), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(W("ppo.adv"), adv, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    launch_ppo_set(nullptr, PpoPar{}, h->ptr<PpoCtl>("ppo.ctl"), W("ppo.acc"), n, h->stream);
    {   // the gradient words of the actor's parameter range: the norm and Adam read all of it, the dW
        // launches write the weights' words only (not the padding between segments, nor logstd's with
        // per_state_std), so the rest must hold 0 whatever the caller's arena held before
        const ParamRange ar = actor_range(h);
        HIPCHK(h, hipMemsetAsync(ar.P + 3 * h->p_stride, 0, sizeof(float) * (size_t)ar.n, h->stream));
    }
    PpoRowsArgs r{};                  // neglogp_old, kl_info_ref, the entropy rows (ppo.py:44-46)
    r.a = W("ppo.a"); r.nlp_out = W("ppo.nlp_old"); r.mean_out = W("ppo.mean_ref");
    r.ls_out = h->softmax ? nullptr : W("ppo.ls_ref");
    r.ent_out = W("ppo.tmp");
    if (ppo_rows_pass(h, W("ppo.s"), n, r)) return -1;
    PpoReduceArgs q{};
    q.c[0] = W("ppo.tmp"); q.out[0] = W("ppo.log"); q.n = n; q.half0 = 1.f;
    launch_ppo_reduce(q, h->stream);
    HIPCHK(h, hipGetLastError());
    h->op().ppo_rows = n;
    return 0;
}

static PpoPar ppo_par_of(const sacx_ppo_params& q) {
    PpoPar par{};
    par.clip_lo = (float)(1.0 - (double)q.eps_ppo);
    par.clip_hi = (float)(1.0 + (double)q.eps_ppo);
    par.max_grad_norm = q.max_grad_norm;
    par.ent_targ = q.ent_targ; par.alpha_lr = q.alpha_lr; par.actor_lr = q.actor_lr;
    par.ent_reg = q.ent_reg != 0; par.adv_center = q.adv_center != 0; par.adv_scale = q.adv_scale != 0;
    return par;
}

int sacx_ppo_steps(sacx_handle* h, const int32_t* idx, int64_t n_steps, int32_t mb, const sacx_ppo_params* params,
                   int32_t flags) {
    if (ppo_check(h)) return -1;
    if (h->learners > 1)
        return fail(h, "the handle holds " + std::to_string(h->learners) + " learners: use sacx_ppo_steps_packed (the "
                       "one-learner step's graphs hold one learner's pointers)");
    if (n_steps <= 0) return 0;
    if (!idx || !params) return fail(h, "null index array or parameters");
    if (h->op().ppo_rows < 1) return fail(h, "no rollout table: call sacx_ppo_begin first");
    if (mb < 1 || mb > h->B)
        return fail(h, "minibatch rows " + std::to_string(mb) + " outside [1, batch = " + std::to_string(h->B) + "]");
    for (int64_t i = 0; i < n_steps * (int64_t)mb; ++i)
        if (idx[i] < 0 || idx[i] >= h->op().ppo_rows) return fail(h, "minibatch index outside the rollout table");
    if (!(params->eps_ppo >= 0.f) || !(params->actor_lr >= 0.f) || !(params->alpha_lr >= 0.f))
        return fail(h, "eps_ppo, actor_lr and alpha_lr must be non-negative");
    const std::vector<Launch>& plan = build_ppo_plan(h, mb);
    const PpoPar par = ppo_par_of(*params);
    launch_ppo_set(h->ptr<PpoPar>("ppo.par"), par, h->ptr<PpoCtl>("ppo.ctl"), h->f("ppo.acc"), -1, h->stream);
    return run_ring_steps(h, plan, h->ptr<int32_t>("ppo.idx"), h->B, PPO_IDX_CAP, {&h->op().ppo_seq}, h->ppo_graphs,
                          "PPO step", idx, n_steps, mb, flags);
}

int sacx_ppo_end(sacx_handle* h, float eps_ppo, double* out) {
    if (ppo_check(h)) return -1;
    if (!out) return fail(h, "null output");
    if (h->op().ppo_rows < 1) return fail(h, "no rollout table: call sacx_ppo_begin first");
    auto W = [&](const std::string& nm) { return h->f(nm); };
    const int64_t n = h->op().ppo_rows;
    PpoRowsArgs r{};                  // neglogp_cur over all rows -> |r - 1|; kl against the reference (ppo.py:91-95)
    r.a = W("ppo.a"); r.nlp_old = W("ppo.nlp_old"); r.rdiff_out = W("ppo.tmp");
    r.mean_ref = W("ppo.mean_ref"); r.ls_ref = h->softmax ? nullptr : W("ppo.ls_ref"); r.kl_out = W("ppo.tmp") + h->cap;
    if (ppo_rows_pass(h, W("ppo.s"), n, r)) return -1;
    float* lg = W("ppo.log");
    PpoReduceArgs q{};
    q.c[0] = W("ppo.tmp"); q.out[0] = lg + 1; q.half0 = 0.5f;          // tv
    q.c[1] = W("ppo.tmp") + h->cap; q.out[1] = lg + 2;                 // kl
    q.c[2] = W("ppo.tmp"); q.out[2] = lg + 3; q.count2 = 1; q.thr = eps_ppo;   // outside_clip
    q.n = n;
    launch_ppo_reduce(q, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float lh[8], ah[8], al[3];
    PpoCtl pc{};
    HIPCHK(h, hipMemcpy(lh, lg, sizeof(lh), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(ah, W("ppo.acc"), sizeof(ah), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(al, W("ppo.alpha"), sizeof(al), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(&pc, h->ptr<PpoCtl>("ppo.ctl"), sizeof(pc), hipMemcpyDeviceToHost));
    out[0] = lh[0]; out[1] = lh[1]; out[2] = lh[2];
    out[3] = (double)lh[3] / (double)n;      // np.mean of booleans (ppo.py:103): the count over n in f64
    // ppo.py:86-89: the f32 sums over the steps divided by their count
    out[4] = pc.n_steps > 0 ? (double)(float)((double)ah[PPO_ACC_PRE] / (double)pc.n_steps) : 0.0;
    out[5] = pc.n_steps > 0 ? (double)(float)((double)ah[PPO_ACC_POST] / (double)pc.n_steps) : 0.0;
    out[6] = al[0];
    out[7] = (double)pc.n_steps;
    return 0;
}

int sacx_ppo_plan_info(sacx_handle* h, int32_t mb, sacx_launch_info* out, int32_t cap, int32_t* n_out) {
    if (ppo_check(h)) return -1;
    if (!n_out) return fail(h, "null output");
    if (mb < 1 || mb > h->B) return fail(h, "minibatch rows outside [1, batch]");
    return launch_info(build_ppo_plan(h, mb), out, cap, n_out);
}

// ---------------------------------------------------------------- VCritics: value, GAE, the critic update
// The critic side of MBRLOnPolicyAlg._update_actor_critic on a trainable GaussianActor handle:
// VCritic._forward / value / get_loss (critics.py:30-49), gae / gae_batch (buffer_utils.py:8-83),
// BaseOnPolicyAlg._update_critics / _apply_critic_grads (base_onpolicy_alg.py:219-283).
int sacx_vcritic_init(sacx_handle* h, int32_t n_critics) {
    if (!h) return -1;
    if (h->bound) return fail(h, "sacx_vcritic_init must precede sacx_bind");
    if (!h->ppo)
        return fail(h, "not a trainable GaussianActor handle (actor_gaussian = SACX_ACTOR_GAUSSIAN_TRAIN): no VCritics");
    if (h->vc > 0) return fail(h, "sacx_vcritic_init was already called on this handle");
    if (h->learners > 0) return fail(h, "sacx_vcritic_init must precede sacx_learners_init");
    if (n_critics < 1 || n_critics > SACX_MAX_MODELS)
        return fail(h, "n_critics " + std::to_string(n_critics) + " outside [1, SACX_MAX_MODELS = " +
                           std::to_string(SACX_MAX_MODELS) + "]");
    static_assert(SACX_MAX_MODELS == MAX_MODELS, "VcCtl::n_rows and the statistics row hold one slot per critic");
    static_assert(sizeof(VcCtl) == 128 && sizeof(VcPar) == 64, "vc.ctl is 16 int64, vc.par 16 words");
    const int F = SACX_F32, S = h->S, B = h->B, nc = n_critics;
    const int64_t cap = h->cap;
    const NetDims& nd = h->nd[1];           // critic_layers / critic_activations (init_critic.py:10-21)
    // behind the ppo.* segments: every segment of the handle as it was keeps its offset
    uint64_t o0 = 0;
    for (int k = 0; k < nc; ++k) {
        int in = S;
        for (int l = 0; l <= nd.D(); ++l) {
            const int out = l < nd.D() ? nd.h[l] : 1;
            const uint64_t o = h->add("v" + std::to_string(k) + ".l" + std::to_string(l), in + 1, out, F, SACX_ROLE_PARAM);
            if (k == 0 && l == 0) o0 = o;
            in = out;
        }
    }
    h->arena_bytes = (h->arena_bytes + 255) & ~uint64_t(255);
    h->vc_pstride = (int64_t)((h->arena_bytes - o0) / 4);
    h->add("vc.adam_m", 1, h->vc_pstride, F, SACX_ROLE_STATE);      // at +1, +2, +3 vc_pstride of v0.l0
    h->add("vc.adam_v", 1, h->vc_pstride, F, SACX_ROLE_STATE);
    h->add("vc.grad", 1, h->vc_pstride, F, SACX_ROLE_WORK);
    h->add("vc.ctl", 1, 16, SACX_I64, SACX_ROLE_STATE);
    h->add("vc.par", 1, 16, F, SACX_ROLE_WORK);
    h->add("vc.s", (int64_t)nc * cap, S, F, SACX_ROLE_STATE);       // critic k's table: rows [k cap, k cap + n_k)
    h->add("vc.rtg", nc, cap, F, SACX_ROLE_STATE);
    h->add("vc.stats", h->stats_cap, VC_STAT_COLS, F, SACX_ROLE_STATE);
    h->add("vc.idx", VC_IDX_CAP, B, SACX_I32, SACX_ROLE_WORK);
    h->add("vc.loss", 1, MAX_MODELS, F, SACX_ROLE_WORK);            // the whole-table losses (sacx_vcritic_end)
    // a step's rows: critic k's minibatch is rows [k mb, (k + 1) mb)
    const int64_t R = (int64_t)nc * B;
    h->add("vc.X", R, h->ldS, F, 0);
    h->add("vc.T", 1, R, F, 0);
    h->add("vc.O", R, 1, F, 0);
    h->add("vc.G", R, 1, F, 0);
    h->add("vc.sq", 1, R, F, 0);
    for (int l = 0; l < nd.D(); ++l) {
        h->add("vc.H" + std::to_string(l), R, nd.h[l], F, 0);
        h->add("vc.D" + std::to_string(l), R, nd.h[l], F, 0);
    }
    // the whole-table passes and the GAE scan
    h->add("vc.tmp", 1, cap, F, 0);
    h->add("vc.gv", 2, cap, F, 0);                                  // value(s), value(sp) of sacx_gae
    h->add("vc.gagg", (cap + GAE_TILE - 1) / GAE_TILE, 2, SACX_F64, 0);
    h->arena_bytes = (h->arena_bytes + 255) & ~uint64_t(255);
    h->seed_bytes = h->arena_bytes;         // (one learner per trainable handle)
    h->vc = nc;
    return 0;
}

static int vc_check(sacx_handle* h) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (!h->ppo)
        return fail(h, "not a trainable GaussianActor handle (actor_gaussian = SACX_ACTOR_GAUSSIAN_TRAIN): no VCritics");
    if (h->vc < 1) return fail(h, "the handle has no VCritics (sacx_vcritic_init was not called)");
    return 0;
}
static int vc_check_critic(sacx_handle* h, int32_t critic) {
    if (vc_check(h)) return -1;
    if (critic < 0 || critic >= h->vc)
        return fail(h, "critic " + std::to_string(critic) + " outside [0, " + std::to_string(h->vc) + ")");
    return 0;
}

// One minibatch step of mb rows per critic (base_onpolicy_alg.py:269-283) as a launch list:
//   vc.gather    every critic's table rows by the step's indices -> normalised states, rtg / ret_den
//   v.fwd<i>     the hidden layers, then the output layer (N = 1), one problem per critic
//   vc.head      g = (v - rtg_n) / mb, the rows' squared differences
//   v.bwd<i>     dX from the output layer down
//   v.grad[.j]   every dW stored, not applied (EPI_STORE; the fused epilogue takes its rate and
//                iteration count from ctl / the plan's constants, which cannot point at vc.*): the
//                n_critics x (layers + 1) problems, GEMM_MAXP to a launch -- the one stage whose
//                launch count grows with the critics (two layers: 1 launch up to 2 critics, 2 up to 5, 3 up to 8)
//   vc.final     each critic's loss, their sum, the statistics row, the counters
//   v.adam       one Keras Adam over the critics' parameter range at the device-read rate
static std::vector<Launch> make_vc_plan(sacx_handle* h, int mb) {
    std::vector<Launch> plan;
    const int S = h->S, ldS = h->ldS, nc = h->vc;
    const NetDims& nd = h->nd[1];
    const int D = nd.D();
    auto W = [&](const std::string& n) { return h->f(n); };
    VcCtl* ctl = h->ptr<VcCtl>("vc.ctl");
    VcPar* par = h->ptr<VcPar>("vc.par");
    float *X = W("vc.X"), *O = W("vc.O"), *G = W("vc.G"), *T = W("vc.T"), *sq = W("vc.sq");
    const int rows = nc * mb;
    std::vector<NetPass> cs;                // critic k: slab k (mb rows) of vc.X, vc.H<i> / vc.D<i>, vc.O and vc.G
    for (int k = 0; k < nc; ++k) {
        NetPass c{};
        c.net = "v" + std::to_string(k); c.nd = &nd; c.group = GRP_Q;
        c.X = X + (size_t)k * mb * ldS; c.ldx = ldS; c.K0 = S; c.M = mb;
        for (int i = 0; i < D; ++i) {
            c.H.push_back(W("vc.H" + std::to_string(i)) + (size_t)k * mb * nd.h[i]);
            c.D.push_back(W("vc.D" + std::to_string(i)) + (size_t)k * mb * nd.h[i]);
        }
        c.N = c.ldo = c.lddo = 1; c.out = O + (size_t)k * mb; c.dout = G + (size_t)k * mb;
        cs.push_back(c);
    }
    {
        Launch L{};
        L.kind = Launch::VCGATHER;
        L.name = "vc.gather";
        VcGatherArgs& g = L.vg;
        g.s = W("vc.s"); g.s_stride = h->cap * S; g.rtg = W("vc.rtg"); g.rtg_stride = h->cap;
        g.idx_ring = h->ptr<int32_t>("vc.idx"); g.idx_ld = h->B; g.ctl = ctl;
        g.s_mean = W("norm.s_mean"); g.s_den = W("norm.s_den"); g.ret_den = W("norm.ret_den");
        g.S = S; g.ldS = ldS; g.mb = mb; g.nc = nc; g.X = X; g.T = T;
        L.grid = (rows + VC_GATHER_ROWS - 1) / VC_GATHER_ROWS;
        L.bytes = 4.0 * rows * (S + ldS + 3);
        plan.push_back(L);
    }
    for (int i = 0; i <= D; ++i) {
        std::vector<GemmProb> ps;
        for (const NetPass& c : cs) ps.push_back(net_fwd_prob(h, c, i));
        add_gemm(h, plan, "v.fwd" + std::to_string(i), ps);
    }
    {
        Launch L{};
        L.kind = Launch::VCHEAD;
        L.name = "vc.head";
        VcHeadArgs& a = L.vh;
        a.O = O; a.T = T; a.rows = rows; a.mb = mb; a.G = G; a.sq = sq;
        L.grid = (rows + 255) / 256;
        L.flops = 4.0 * rows;
        L.bytes = 16.0 * rows;
        plan.push_back(L);
    }
    for (int i = D; i >= 1; --i) {
        std::vector<GemmProb> ps;
        for (const NetPass& c : cs) ps.push_back(net_dx_prob(h, c, i));
        add_gemm(h, plan, "v.bwd" + std::to_string(i), ps);
    }
    {
        std::vector<GemmProb> pw;
        for (const NetPass& c : cs)
            for (int i = 0; i <= D; ++i) pw.push_back(net_dw_prob(h, c, i));
        const int n_dw = add_gemm_split(h, plan, "v.grad", pw);
        store_grads(plan, n_dw);               // the gradients go to +3 vc_pstride of the critics' own range
        for (int j = 0; j < n_dw; ++j) plan[plan.size() - 1 - j].gemm.p_stride = h->vc_pstride;
    }
    {
        Launch L{};
        L.kind = Launch::VCFINAL;
        L.name = "vc.final";
        VcFinalArgs& a = L.vf;
        a.sq = sq; a.mb = mb; a.nc = nc; a.ctl = ctl; a.stats = W("vc.stats"); a.stats_cap = h->stats_cap;
        L.grid = 1;
        L.bytes = 4.0 * rows;
        plan.push_back(L);
    }
    {
        Launch U{};
        U.kind = Launch::VCADAM;
        U.name = "v.adam";
        VcAdamArgs& a = U.va;
        const SegInfo& sl = h->seg(layer_name(cs.back().net, D));
        a.P = W("v0.l0");
        a.n = (int64_t)((sl.off + (uint64_t)(sl.rows * sl.cols) * 4 - h->off_of("v0.l0")) / 4);
        a.p_stride = h->vc_pstride; a.lr_dev = &par->critic_lr; a.t_dev = &ctl->t; a.t_adv = 1;   // vc.final advanced t
        U.grid = (int)((a.n + 255) / 256);
        U.bytes = 4.0 * a.n * 7;
        plan.push_back(U);
    }
    return plan;
}
static const std::vector<Launch>& build_vc_plan(sacx_handle* h, int mb) {
    auto it = h->vc_plans.find(mb);
    if (it != h->vc_plans.end()) return it->second;
    return h->vc_plans.emplace(mb, make_vc_plan(h, mb)).first->second;
}

// critic `critic` on m <= ACT_CAP caller rows s: normalise, hidden layers, the output layer -> act.Q [m]
static void vc_forward(sacx_handle* h, int critic, const float* s, int m) {
    auto W = [&](const std::string& nm) { return h->f(nm); };
    launch_obs_norm(s, m, h->S, W("norm.s_mean"), W("norm.s_den"), W("act.X"), h->ldS, h->stream);
    const NetPass c = eager_pass(h, "v" + std::to_string(critic), 1, W("act.X"), h->ldS, h->S, m, W("act.H1"), W("act.H2"), 1, W("act.Q"));
    net_hidden(h, c, h->stream);
    net_head(h, c, h->stream);
}

// the whole-table passes: n rows of s through critic `critic` in chunks of ACT_CAP, k_vc_rows on each
// (out: the [n] outputs, x ret_den with value; sq: (rtg / ret_den - v)^2 per row)
static int vc_rows_pass(sacx_handle* h, int critic, const float* s, int64_t n, int value, float* out, const float* rtg,
                        float* sq) {
    for (int64_t done = 0; done < n; done += ACT_CAP) {
        const int m = (int)std::min<int64_t>(ACT_CAP, n - done);
        vc_forward(h, critic, s + done * h->S, m);
        VcRowsArgs r{};
        r.Q = h->f("act.Q"); r.m = m; r.value = value; r.ret_den = h->f("norm.ret_den");
        r.rtg = rtg ? rtg + done : nullptr; r.out = out ? out + done : nullptr; r.sq = sq ? sq + done : nullptr;
        launch_vc_rows(r, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int sacx_vcritic_value(sacx_handle* h, int32_t critic, const float* s, int64_t n, int32_t value, float* out) {
    if (vc_check_critic(h, critic)) return -1;
    if (n < 0 || (n > 0 && (!s || !out))) return fail(h, "bad arguments");
    return vc_rows_pass(h, critic, s, n, value ? 1 : 0, out, nullptr, nullptr);
}

static int gae_launch(sacx_handle* h, const float* v_s, const float* v_sp, const float* r, const float* d,
                      const int32_t* traj, int64_t n, double gamma, double lam, float* adv, float* rtg, float* rtg_sp) {
    GaeArgs g{};
    g.v_s = v_s; g.v_sp = v_sp; g.r = r; g.d = d; g.traj = traj; g.n = n;
    g.gamma = gamma; g.gl = gamma * lam;
    g.agg = h->ptr<double>("vc.gagg"); g.tiles = (int32_t)((n + GAE_TILE - 1) / GAE_TILE);
    g.adv = adv; g.rtg = rtg; g.rtg_sp = rtg_sp;
    launch_gae(g, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

static int gae_args_check(sacx_handle* h, const void* r, const void* d, const void* traj, int64_t n, double gamma,
                          const void* adv, const void* rtg, const void* rtg_sp) {
    if (!r || !d || !traj || !adv || !rtg || !rtg_sp) return fail(h, "null pointer");
    if (n < 1 || n > h->cap)
        return fail(h, "rows " + std::to_string(n) + " outside [1, buffer_capacity = " + std::to_string(h->cap) + "]");
    if (!(gamma > 0.0)) return fail(h, "gamma must be positive (rtg_sp divides by it)");
    return 0;
}

int sacx_gae_values(sacx_handle* h, const float* v_s, const float* v_sp, const float* r, const float* d,
                    const int32_t* traj, int64_t n, double gamma, double lam, float* adv_out, float* rtg_out,
                    float* rtg_sp_out) {
    if (vc_check(h)) return -1;
    if (!v_s || !v_sp) return fail(h, "null pointer");
    if (gae_args_check(h, r, d, traj, n, gamma, adv_out, rtg_out, rtg_sp_out)) return -1;
    return gae_launch(h, v_s, v_sp, r, d, traj, n, gamma, lam, adv_out, rtg_out, rtg_sp_out);
}

int sacx_gae(sacx_handle* h, int32_t critic, const float* s, const float* r, const float* sp, const float* d,
             const int32_t* traj, int64_t n, double gamma, double lam, float* adv_out, float* rtg_out, float* rtg_sp_out) {
    if (vc_check_critic(h, critic)) return -1;
    if (!s || !sp) return fail(h, "null pointer");
    if (gae_args_check(h, r, d, traj, n, gamma, adv_out, rtg_out, rtg_sp_out)) return -1;
    float* gv = h->f("vc.gv");
    if (vc_rows_pass(h, critic, s, n, 1, gv, nullptr, nullptr)) return -1;
    if (vc_rows_pass(h, critic, sp, n, 1, gv + h->cap, nullptr, nullptr)) return -1;
    return gae_launch(h, gv, gv + h->cap, r, d, traj, n, gamma, lam, adv_out, rtg_out, rtg_sp_out);
}

// 0.5 mean((rtg / ret_den - v)^2) of critic `critic` over n rows -> dst (device), through vc.tmp
static int vc_loss_pass(sacx_handle* h, int critic, const float* s, const float* rtg, int64_t n, float* dst) {
    if (vc_rows_pass(h, critic, s, n, 0, nullptr, rtg, h->f("vc.tmp"))) return -1;
    VcReduceArgs q{};
    q.sq = h->f("vc.tmp"); q.n = n; q.out = dst;
    launch_vc_reduce(q, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int sacx_vcritic_loss(sacx_handle* h, int32_t critic, const float* s, const float* rtg, int64_t n, float* loss_out) {
    if (vc_check_critic(h, critic)) return -1;
    if (!s || !rtg || !loss_out) return fail(h, "null pointer");
    if (n < 1 || n > h->cap)
        return fail(h, "rows " + std::to_string(n) + " outside [1, buffer_capacity = " + std::to_string(h->cap) + "]");
    return vc_loss_pass(h, critic, s, rtg, n, loss_out);
}

int sacx_vcritic_begin(sacx_handle* h, int32_t critic, const float* s, const float* rtg, int64_t n) {
    if (vc_check_critic(h, critic)) return -1;
    if (!s || !rtg) return fail(h, "null table pointer");
    if (n < 1 || n > h->cap)
        return fail(h, "table rows " + std::to_string(n) + " outside [1, buffer_capacity = " + std::to_string(h->cap) + "]");
    const int S = h->S;
    HIPCHK(h, hipMemcpyAsync(h->f("vc.s") + (size_t)critic * h->cap * S, s, sizeof(float) * (size_t)n * S,
                             hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->f("vc.rtg") + (size_t)critic * h->cap, rtg, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice,
                             h->stream));
    launch_vc_set(nullptr, VcPar{}, h->ptr<VcCtl>("vc.ctl"), critic, n, h->stream);
    // the gradient words of the critics' parameter range: Adam reads all of it, the dW launches write
    // the weights' words only (not the padding between segments)
    HIPCHK(h, hipMemsetAsync(h->f("vc.grad"), 0, sizeof(float) * (size_t)h->vc_pstride, h->stream));
    HIPCHK(h, hipGetLastError());
    h->op().vc_rows[critic] = n;
    return 0;
}

int sacx_vcritic_steps(sacx_handle* h, const int32_t* idx, int64_t n_steps, int32_t mb, float critic_lr, int32_t flags) {
    if (vc_check(h)) return -1;
    if (h->learners > 1)
        return fail(h, "the handle holds " + std::to_string(h->learners) + " learners: use sacx_vcritic_steps_packed (the "
                       "one-learner step's graphs hold one learner's pointers)");
    if (n_steps <= 0) return 0;
    if (!idx) return fail(h, "null index array");
    int64_t n_min = h->op().vc_rows[0];
    for (int k = 0; k < h->vc; ++k) {
        if (h->op().vc_rows[k] < 1) return fail(h, "critic " + std::to_string(k) + " has no table: call sacx_vcritic_begin first");
        n_min = std::min(n_min, h->op().vc_rows[k]);
    }
    if (mb < 1 || mb > h->B)
        return fail(h, "minibatch rows " + std::to_string(mb) + " outside [1, batch = " + std::to_string(h->B) + "]");
    for (int64_t i = 0; i < n_steps * (int64_t)mb; ++i)
        if (idx[i] < 0 || idx[i] >= n_min) return fail(h, "minibatch index outside the shortest critic table");
    if (!(critic_lr >= 0.f)) return fail(h, "critic_lr must be non-negative");
    const std::vector<Launch>& plan = build_vc_plan(h, mb);
    VcPar par{};
    par.critic_lr = critic_lr;
    launch_vc_set(h->ptr<VcPar>("vc.par"), par, h->ptr<VcCtl>("vc.ctl"), -1, 0, h->stream);
    return run_ring_steps(h, plan, h->ptr<int32_t>("vc.idx"), h->B, VC_IDX_CAP, {&h->op().vc_seq}, h->vc_graphs,
                          "critic step", idx, n_steps, mb, flags);
}

int sacx_vcritic_end(sacx_handle* h, double* out) {
    if (vc_check(h)) return -1;
    if (!out) return fail(h, "null output");
    for (int k = 0; k < h->vc; ++k)
        if (h->op().vc_rows[k] < 1) return fail(h, "critic " + std::to_string(k) + " has no table: call sacx_vcritic_begin first");
    float* ls = h->f("vc.loss");
    for (int k = 0; k < h->vc; ++k)
        if (vc_loss_pass(h, k, h->f("vc.s") + (size_t)k * h->cap * h->S, h->f("vc.rtg") + (size_t)k * h->cap, h->op().vc_rows[k], ls + k))
            return -1;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float lh[MAX_MODELS];
    VcCtl vc{};
    HIPCHK(h, hipMemcpy(lh, ls, sizeof(lh), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(&vc, h->ptr<VcCtl>("vc.ctl"), sizeof(vc), hipMemcpyDeviceToHost));
    for (int k = 0; k < MAX_MODELS; ++k) out[k] = k < h->vc ? (double)lh[k] : 0.0;
    out[MAX_MODELS] = (double)vc.t;
    return 0;
}

int sacx_vcritic_plan_info(sacx_handle* h, int32_t mb, sacx_launch_info* out, int32_t cap, int32_t* n_out) {
    if (vc_check(h)) return -1;
    if (!n_out) return fail(h, "null output");
    if (mb < 1 || mb > h->B) return fail(h, "minibatch rows outside [1, batch]");
    return launch_info(build_vc_plan(h, mb), out, cap, n_out);
}

// ---------------------------------------------------------------- TRPO actor update
// TRPO.update (trpo.py:34-317, the expert_reg is None branch with grad_final := neg_pg) on a trainable
// GaussianActor handle: the surrogate gradient and every Fisher-vector product as whole-table passes in
// chunks of trpo_chunk rows, conjugate gradient on device vectors without a host round trip, the
// backtracking line search with one synchronisation per trial.
int sacx_trpo_init(sacx_handle* h) {
    if (!h) return -1;
    if (h->bound) return fail(h, "sacx_trpo_init must precede sacx_bind");
    if (!h->ppo)
        return fail(h, "not a trainable GaussianActor handle (actor_gaussian = SACX_ACTOR_GAUSSIAN_TRAIN): no TRPO update");
    if (h->trpo) return fail(h, "sacx_trpo_init was already called on this handle");
    if (h->learners > 0)
        return fail(h, "a handle with sacx_learners_init runs no TRPO update: its conjugate gradient and line search are one "
                       "learner per handle");
    static_assert(sizeof(TrpoPar) == 64, "trpo.par is 16 words");
    const int F = SACX_F32, A = h->A, Aout = h->Aout;
    const NetDims& na = h->nd[0];
    const int64_t cap = h->cap;
    const int C = (int)std::min<int64_t>(cap, TRPO_CHUNK);
    const int64_t nv = actor_range(h).n;
    int wmax = std::max(Aout, h->ldS);
    for (int w : na.h) wmax = std::max(wmax, w);
    // behind everything the handle holds: every earlier segment keeps its offset
    h->add("trpo.par", 1, 16, F, SACX_ROLE_WORK);
    h->add("trpo.sc", 1, 16, SACX_F64, SACX_ROLE_WORK);
    h->add("trpo.log", 1, 8, F, SACX_ROLE_WORK);
    h->add("trpo.done", 1, TRPO_CG_MAX + 2, SACX_I32, SACX_ROLE_WORK);
    h->add("trpo.rr", TRPO_CG_MAX + 1, TRPO_PARTS, SACX_F64, SACX_ROLE_WORK);
    h->add("trpo.pz", 1, TRPO_PARTS, SACX_F64, SACX_ROLE_WORK);
    h->add("trpo.vec", TRPO_VECS, r4(nv), F, SACX_ROLE_WORK);      // b, x, r, p, z, the saved weights, the step
    h->add("trpo.zero", 1, wmax, F, SACX_ROLE_WORK);                // the bias of the t_in . W problems
    h->add("trpo.ones", 1, C + 4, F, SACX_ROLE_WORK);               // the row scale of the dW problems
    h->add("trpo.adv", 2, cap, F, SACX_ROLE_WORK);                  // the advantages normalised once / twice
    h->add("trpo.ev", 3, cap, F, SACX_ROLE_WORK);                   // per row r adv, |r - 1|, kl
    // a chunk's rows
    h->add("trpo.X", C, h->ldS, F, 0);
    for (int l = 0; l < na.D(); ++l) {
        h->add("trpo.H" + std::to_string(l), C, na.h[l], F, 0);
        h->add("trpo.T" + std::to_string(l), C, na.h[l], F, 0);
        h->add("trpo.D" + std::to_string(l), C, na.h[l], F, 0);
    }
    h->add("trpo.G", 2 * (int64_t)C, wmax, F, 0);                   // the two halves of a layer's tangent
    h->add("trpo.O", C, Aout, F, 0);
    h->add("trpo.D3", C, Aout, F, 0);
    h->add("trpo.E", C, A, F, 0);
    if (h->ln) {
        h->add("trpo.xhat", C, h->H0, F, 0);
        h->add("trpo.rstd", 1, C, F, 0);
        h->add("trpo.gy", C, h->H0, F, 0);
        h->add("trpo.gb", C, h->H0, F, 0);
    }
    h->arena_bytes = (h->arena_bytes + 255) & ~uint64_t(255);
    h->seed_bytes = h->arena_bytes;         // (one learner per trainable handle)
    h->trpo = true;
    h->trpo_chunk = C;
    h->trpo_nv = nv;
    return 0;
}

// ---------------------------------------------------------------- SoftMaxActor on the trainable handle
// discrete_actors.py:8-117 with _nn = create_nn(s_dim, a_dim, ...): the actor net's A outputs are logits,
// and sacx_ppo_* / sacx_trpo_* carry the categorical neglogp, entropy and kl (k_ppo_head, k_ppo_rows,
// k_trpo_head in their softmax mode).  The layout stays the handle's own: actor.logstd keeps its words,
// outside the trainable range.
int sacx_softmax_init(sacx_handle* h) {
    if (!h) return -1;
    if (h->bound) return fail(h, "sacx_softmax_init must precede sacx_bind");
    if (!h->ppo)
        return fail(h, "not a trainable GaussianActor handle (actor_gaussian = SACX_ACTOR_GAUSSIAN_TRAIN): no SoftMaxActor");
    if (h->softmax) return fail(h, "sacx_softmax_init was already called on this handle");
    if (h->cfg.per_state_std) return fail(h, "a softmax handle has no std: per_state_std must be 0");
    if (h->models_only)
        return fail(h, "SACX_EXPERT_MODELS: the world models take continuous actions, the reference defines no encoding "
                       "of a discrete one");
    if (h->cfg.use_expert) return fail(h, "a softmax handle needs use_expert = SACX_EXPERT_OFF");
    h->softmax = true;
    if (h->trpo) h->trpo_nv = actor_range(h).n;     // the flat vectors hold the net only
    return 0;
}

// ---------------------------------------------------------------- packed on-policy learners
// The reference's --runs K (train.py:148-152) for the on-policy loop: K independent learners, each the
// one-learner handle's layout byte for byte, in K arena blocks seed_bytes apart.  Their PPO minibatch
// steps (ppo.py:55-83) and critic steps (base_onpolicy_alg.py:219-283) run in the same launches, grid
// z = learner; everything else addresses the learner chosen with sacx_seed_select.
int sacx_learners_init(sacx_handle* h, int32_t K) {
    if (!h) return -1;
    if (h->bound) return fail(h, "sacx_learners_init must precede sacx_bind");
    if (!h->ppo)
        return fail(h, "not a trainable GaussianActor handle (actor_gaussian = SACX_ACTOR_GAUSSIAN_TRAIN): no packed learners");
    if (h->learners > 0) return fail(h, "sacx_learners_init was already called on this handle");
    if (h->trpo)
        return fail(h, "a handle with sacx_trpo_init holds one learner: TRPO's conjugate gradient and line search are not packed");
    if (K < 2 || K > SACX_MAX_LEARNERS)
        return fail(h, "learners " + std::to_string(K) + " outside [2, SACX_MAX_LEARNERS = " + std::to_string(SACX_MAX_LEARNERS) + "]");
    h->learners = h->seeds = K;
    h->plan_seeds = 1;                      // (every shape decision is the one-learner handle's)
    h->seed_bytes = (h->arena_bytes + 65535) & ~uint64_t(65535);
    h->onp.assign((size_t)K, sacx_handle::OnPolicyHost{});
    return 0;
}

// A segment of learner k.  The step parameters go to each learner's block with one k_ppo_set / k_vc_set
// launch per learner: they differ between learners (adaptlr, ppo.py:109-117) and ride as kernel
// arguments, in stream order in front of the steps, as the one-learner call's do
static void* learner_seg(const sacx_handle* h, const std::string& seg, int k) {
    return h->arena0 + (uint64_t)k * h->seed_bytes + h->off_of(seg);
}

int sacx_ppo_steps_packed(sacx_handle* h, const int32_t* idx, int64_t n_steps, int32_t mb, const sacx_ppo_params* params,
                          int32_t flags) {
    if (ppo_check(h)) return -1;
    if (packed_check(h, "sacx_ppo_steps")) return -1;
    if (n_steps <= 0) return 0;
    if (!idx || !params) return fail(h, "null index array or parameters");
    if (mb < 1 || mb > h->B)
        return fail(h, "minibatch rows " + std::to_string(mb) + " outside [1, batch = " + std::to_string(h->B) + "]");
    const int K = h->learners;
    for (int k = 0; k < K; ++k) {
        const int64_t rows = h->onp[k].ppo_rows;
        if (rows < 1) return fail(h, "learner " + std::to_string(k) + " has no rollout table: call sacx_ppo_begin on it first");
        const int32_t* ik = idx + (int64_t)k * n_steps * mb;
        for (int64_t i = 0; i < n_steps * (int64_t)mb; ++i)
            if (ik[i] < 0 || ik[i] >= rows)
                return fail(h, "learner " + std::to_string(k) + ": minibatch index outside its rollout table");
        if (!(params[k].eps_ppo >= 0.f) || !(params[k].actor_lr >= 0.f) || !(params[k].alpha_lr >= 0.f))
            return fail(h, "learner " + std::to_string(k) + ": eps_ppo, actor_lr and alpha_lr must be non-negative");
    }
    const std::vector<Launch>& plan = packed_plan(h, h->ppo_pk_plans, mb, make_ppo_plan);
    std::vector<int64_t*> seqs;
    for (int k = 0; k < K; ++k) {
        launch_ppo_set(static_cast<PpoPar*>(learner_seg(h, "ppo.par", k)), ppo_par_of(params[k]),
                       static_cast<PpoCtl*>(learner_seg(h, "ppo.ctl", k)), static_cast<float*>(learner_seg(h, "ppo.acc", k)), -1,
                       h->stream);
        seqs.push_back(&h->onp[k].ppo_seq);
    }
    return run_ring_steps(h, plan, static_cast<int32_t*>(learner_seg(h, "ppo.idx", 0)), h->B, PPO_IDX_CAP, seqs,
                          h->ppo_pk_graphs, "packed PPO step", idx, n_steps, mb, flags);
}

int sacx_vcritic_steps_packed(sacx_handle* h, const int32_t* idx, int64_t n_steps, int32_t mb, const float* critic_lr,
                              int32_t flags) {
    if (vc_check(h)) return -1;
    if (packed_check(h, "sacx_vcritic_steps")) return -1;
    if (n_steps <= 0) return 0;
    if (!idx || !critic_lr) return fail(h, "null index array or rates");
    if (mb < 1 || mb > h->B)
        return fail(h, "minibatch rows " + std::to_string(mb) + " outside [1, batch = " + std::to_string(h->B) + "]");
    const int K = h->learners;
    for (int k = 0; k < K; ++k) {
        int64_t n_min = h->onp[k].vc_rows[0];
        for (int c = 0; c < h->vc; ++c) {
            if (h->onp[k].vc_rows[c] < 1)
                return fail(h, "learner " + std::to_string(k) + ": critic " + std::to_string(c) +
                                   " has no table: call sacx_vcritic_begin on it first");
            n_min = std::min(n_min, h->onp[k].vc_rows[c]);
        }
        const int32_t* ik = idx + (int64_t)k * n_steps * mb;
        for (int64_t i = 0; i < n_steps * (int64_t)mb; ++i)
            if (ik[i] < 0 || ik[i] >= n_min)
                return fail(h, "learner " + std::to_string(k) + ": minibatch index outside its shortest critic table");
        if (!(critic_lr[k] >= 0.f)) return fail(h, "learner " + std::to_string(k) + ": critic_lr must be non-negative");
    }
    const std::vector<Launch>& plan = packed_plan(h, h->vc_pk_plans, mb, make_vc_plan);
    std::vector<int64_t*> seqs;
    for (int k = 0; k < K; ++k) {
        VcPar par{};
        par.critic_lr = critic_lr[k];
        launch_vc_set(static_cast<VcPar*>(learner_seg(h, "vc.par", k)), par, static_cast<VcCtl*>(learner_seg(h, "vc.ctl", k)), -1, 0,
                      h->stream);
        seqs.push_back(&h->onp[k].vc_seq);
    }
    return run_ring_steps(h, plan, static_cast<int32_t*>(learner_seg(h, "vc.idx", 0)), h->B, VC_IDX_CAP, seqs, h->vc_pk_graphs,
                          "packed critic step", idx, n_steps, mb, flags);
}

static int trpo_check(sacx_handle* h) {
    if (!h || !h->bound) return fail(h, "not bound");
    if (!h->ppo)
        return fail(h, "not a trainable GaussianActor handle (actor_gaussian = SACX_ACTOR_GAUSSIAN_TRAIN): no TRPO update");
    if (!h->trpo) return fail(h, "the handle has no TRPO update (sacx_trpo_init was not called)");
    return 0;
}

// One chunk of a whole-table pass as a launch list.  mode 0: the surrogate gradient (rows row0 .. row0 + m),
// 1: a Fisher-vector product (rows row0 + i * stride; dir = the direction over the flat range),
// 2: the line search's evaluation (forward and head only).  Modes 0 and 1 end in the chunk's dW stored
// (EPI_STORE) into the gradient words of the actor's range and k_trpo_acc adding them to `out`.
//   trpo.in -> actor.fwd<i> (+ actor.ln) -> [actor.tan<i> + trpo.tan<i> per hidden layer, actor.tan<D>]
//   -> trpo.head -> actor.bwd<i> (+ actor.ln.bwd) -> actor.grad -> trpo.acc
static void trpo_chunk_plan(sacx_handle* h, std::vector<Launch>& plan, int mode, int64_t row0, int m, int64_t stride,
                            const float* dir, float* out, bool first, bool last) {
    const int S = h->S, A = h->A, Aout = h->Aout, ldS = h->ldS, C = h->trpo_chunk;
    const NetDims& na = h->nd[0];
    const int Da = na.D();
    auto W = [&](const std::string& n) { return h->f(n); };
    auto L_ = layer_name;
    auto Tb = [&](int i) { return W("trpo.T" + std::to_string(i)); };
    float* P0 = W("actor.l0");
    auto dir_of = [&](const std::string& seg) { return dir + (W(seg) - P0); };     // the direction's words of a segment
    const GemmTiles tl{0, 0};               // 16 x 16 tiles, k_gemm: the tiles the PPO step's tests pin
    float *X = W("trpo.X"), *O = W("trpo.O");
    float *G0 = W("trpo.G"), *G1 = W("trpo.G") + (size_t)C * h->seg("trpo.G").cols;
    TrpoPar* par = h->ptr<TrpoPar>("trpo.par");
    ActorPass ap{};                         // the chunk's rows: rows [0, m) of the trpo.* buffers
    ap.X = X; ap.ldx = ldS; ap.M = m; ap.cache_rows = m; ap.O = O;
    for (int i = 0; i < Da; ++i) {
        ap.H.push_back(W("trpo.H" + std::to_string(i)));
        ap.D.push_back(W("trpo.D" + std::to_string(i)));
    }
    ap.D3 = W("trpo.D3"); ap.E = W("trpo.E");
    if (h->ln) {
        ap.xhat = W("trpo.xhat"); ap.rstd = W("trpo.rstd"); ap.gy = W("trpo.gy"); ap.gb = W("trpo.gb");
    }
    auto Hb = [&](int i) { return ap.H[i]; };
    {
        Launch L{};
        L.kind = Launch::TRIN;
        L.name = "trpo.in";
        L.ti.s = W("ppo.s"); L.ti.row0 = row0; L.ti.stride = stride;
        L.ti.s_mean = W("norm.s_mean"); L.ti.s_den = W("norm.s_den");
        L.ti.S = S; L.ti.ldS = ldS; L.ti.m = m; L.ti.X = X;
        L.grid = (m + 63) / 64;
        L.bytes = 4.0 * m * (S + ldS);
        plan.push_back(L);
    }
    actor_fwd_chain(h, plan, ap, "actor.fwd", "actor.ln", tl);
    if (mode == 1) {
        // the tangent forward: per layer h_in . V + v_b and t_in . W as the two problems of one launch
        // (V_ext = the direction's words of the layer, so its bias row is v_b; the second problem's bias
        // is trpo.zero), then t_out = act'(h_out) (.) (G0 + G1); layer 0's input has no tangent
        for (int i = 0; i <= Da; ++i) {
            const float* in = i == 0 ? X : Hb(i - 1);
            const int ldi = i == 0 ? ldS : na.h[i - 1], K = i == 0 ? S : na.h[i - 1];
            const int N = i < Da ? na.h[i] : Aout;
            std::vector<GemmProb> ps;
            ps.push_back(prob_fwd(in, ldi, m, K, dir_of(L_("actor", i)), N, G0, ACT_NONE));
            if (i > 0) {
                GemmProb p = prob_fwd(Tb(i - 1), K, m, K, W(L_("actor", i)), N, G1, ACT_NONE);
                p.bias = W("trpo.zero");
                ps.push_back(p);
            }
            add_gemm(h, plan, "actor.tan" + std::to_string(i), ps, tl);
            if (i == Da) break;
            Launch L{};
            L.kind = Launch::TRTAN;
            L.name = "trpo.tan" + std::to_string(i);
            TrTanArgs& a = L.tt;
            a.G0 = G0; a.G1 = i > 0 ? G1 : nullptr; a.Hout = Hb(i); a.T = Tb(i);
            a.m = m; a.H = N; a.act = na.act[i]; a.ln = (i == 0 && h->ln) ? 1 : 0;
            if (a.ln) {
                a.xhat = W("trpo.xhat"); a.rstd = W("trpo.rstd"); a.gamma = W("actor.ln"); a.vgamma = dir_of("actor.ln");
            }
            L.grid = a.ln ? (m + 3) / 4 : (int)(((int64_t)m * N + 255) / 256);
            L.bytes = 4.0 * m * N * 4;
            plan.push_back(L);
        }
    }
    {
        Launch L{};
        L.kind = Launch::TRHEAD;
        L.name = "trpo.head";
        TrHeadArgs& a = L.th;
        a.d = ppo_dist(h, O);
        a.mode = mode; a.m = m; a.row0 = row0;
        a.a = W("ppo.a"); a.nlp_old = W("ppo.nlp_old"); a.mean_ref = W("ppo.mean_ref"); a.ls_ref = W("ppo.ls_ref");
        // the gradient takes the advantages normalised once, the line search twice (trpo.py:244-250)
        a.adv = W("trpo.adv") + (mode == 2 ? (size_t)h->cap : 0);
        a.alpha = W("ppo.alpha"); a.par = par;
        a.TO0 = G0; a.TO1 = G1; a.vls = (dir && !h->softmax) ? dir_of("actor.logstd") : nullptr;
        a.D3 = ap.D3; a.E = ap.E;
        a.o_radv = W("trpo.ev"); a.o_rdiff = W("trpo.ev") + h->cap; a.o_kl = W("trpo.ev") + 2 * (size_t)h->cap;
        L.grid = (m + 3) / 4;
        L.flops = 40.0 * m * A;
        L.bytes = 4.0 * m * (3.0 * Aout + 2.0 * A + 4);
        plan.push_back(L);
    }
    if (mode != 2) {
        actor_bwd_chain(h, plan, ap, Da, tl);
        std::vector<GemmProb> pw = actor_dw_probs(h, ap);
        for (GemmProb& p : pw) p.bscale = W("trpo.ones");       // the chunk's row scale
        store_grads(plan, add_gemm_split(h, plan, "actor.grad", pw, tl));   // stored at +3 p_stride, as the PPO step's
        Launch L{};
        L.kind = Launch::TRACC;
        L.name = "trpo.acc";
        TrAccArgs& a = L.ta;
        a.g = P0 + 3 * h->p_stride; a.dst = out; a.x = mode == 1 ? dir : nullptr; a.n = h->trpo_nv;
        a.first = first; a.last = last; a.sign = mode == 0 ? -1.f : 1.f; a.par = par;
        L.grid = (int)((h->trpo_nv + 255) / 256);
        L.bytes = 4.0 * h->trpo_nv * 3;
        plan.push_back(L);
    }
}

// a whole-table pass: every chunk's launches in chunk order
static void trpo_pass_plan(sacx_handle* h, std::vector<Launch>& plan, int mode, int64_t n, int64_t stride, const float* dir,
                           float* out) {
    const int64_t rows = (n + stride - 1) / stride;         // len(s_all[::stride])
    const int C = h->trpo_chunk;
    for (int64_t done = 0; done < rows; done += C) {
        const int m = (int)std::min<int64_t>(C, rows - done);
        trpo_chunk_plan(h, plan, mode, done * stride, m, stride, dir, out, done == 0, done + C >= rows);
    }
}

static TrCgArgs trpo_cg_args(sacx_handle* h, int phase, int it) {
    TrCgArgs a{};
    a.phase = phase; a.it = it; a.n = h->trpo_nv;
    a.vec = h->f("trpo.vec"); a.vstride = h->seg("trpo.vec").cols;
    a.rr = h->ptr<double>("trpo.rr"); a.pz = h->ptr<double>("trpo.pz");
    a.done = h->ptr<int32_t>("trpo.done"); a.sc = h->ptr<double>("trpo.sc");
    a.par = h->ptr<TrpoPar>("trpo.par");
    a.W = h->f("actor.l0");
    const bool ls = !h->cfg.per_state_std && !h->softmax;       // a state-independent logstd in the range
    a.ls_off = ls ? (int64_t)(h->f("actor.logstd") - h->f("actor.l0")) : 0;
    a.ls_n = ls ? h->A : 0;
    a.ls_floor = (float)std::log(1e-3);
    return a;
}
static Launch trpo_cg_launch(sacx_handle* h, int phase, int it, const char* name) {
    Launch L{};
    L.kind = Launch::TRCG;
    L.name = name;
    L.tc = trpo_cg_args(h, phase, it);
    L.grid = phase == TRC_GMAX ? 1 : TRPO_PARTS;
    L.bytes = 4.0 * h->trpo_nv * 3;
    return L;
}

static float* trpo_vec(sacx_handle* h, int k) { return h->f("trpo.vec") + (size_t)k * h->seg("trpo.vec").cols; }

static int trpo_par_check(sacx_handle* h, const sacx_trpo_params* q) {
    if (!q) return fail(h, "null parameters");
    if (!(q->delta >= 0.f) || !(q->trust_damp >= 0.f) || !(q->alpha_lr >= 0.f) || !(q->kl_maxfactor >= 0.f))
        return fail(h, "delta, trust_damp, kl_maxfactor and alpha_lr must be non-negative");
    if (q->cg_it < 1 || q->cg_it > TRPO_CG_MAX)
        return fail(h, "cg_it " + std::to_string(q->cg_it) + " outside [1, " + std::to_string(TRPO_CG_MAX) + "]");
    if (q->trust_sub < 1) return fail(h, "trust_sub must be at least 1");
    return 0;
}

static void trpo_par_set(sacx_handle* h, const sacx_trpo_params* q, int64_t n, hipStream_t st) {
    TrpoPar p{};
    p.delta = q->delta; p.damp = q->trust_damp; p.ent_targ = q->ent_targ; p.alpha_lr = q->alpha_lr;
    p.inv_n = (float)(1.0 / (double)n);
    p.inv_nsub = (float)(1.0 / (double)((n + q->trust_sub - 1) / q->trust_sub));
    p.ent_reg = q->ent_reg != 0; p.adv_center = q->adv_center != 0; p.adv_scale = q->adv_scale != 0;
    launch_trpo_set(h->ptr<TrpoPar>("trpo.par"), p, st);
}

int sacx_trpo_begin(sacx_handle* h, const float* s, const float* a, const float* adv, int64_t n,
                    const sacx_trpo_params* params) {
    if (trpo_check(h)) return -1;
    if (trpo_par_check(h, params)) return -1;
    h->trpo_rows = 0;
    // the table, neglogp_old, the reference distribution and the mean entropy (trpo.py:37, :240-241)
    if (sacx_ppo_begin(h, s, a, adv, n)) return -1;
    auto W = [&](const std::string& nm) { return h->f(nm); };
    trpo_par_set(h, params, n, h->stream);
    launch_trpo_fill(W("trpo.zero"), h->seg("trpo.zero").cols, 0.f, h->stream);
    launch_trpo_fill(W("trpo.ones"), h->seg("trpo.ones").cols, 1.f, h->stream);
    TrAdvArgs q{};
    q.src = W("ppo.adv"); q.dst = W("trpo.adv"); q.n = n; q.par = h->ptr<TrpoPar>("trpo.par");
    launch_trpo_advnorm(q, h->stream);
    q.src = W("trpo.adv"); q.dst = W("trpo.adv") + h->cap;         // _backtrack normalises once more (:244-250)
    launch_trpo_advnorm(q, h->stream);
    std::vector<Launch> plan;
    trpo_pass_plan(h, plan, 0, n, 1, nullptr, trpo_vec(h, TRV_B));
    plan.push_back(trpo_cg_launch(h, TRC_GMAX, 0, "trpo.gmax"));
    for (const Launch& L : plan) enqueue(L, h, h->stream);
    TrAlphaArgs al{};               // behind the gradient: it takes the alpha from before this step
    al.alpha = W("ppo.alpha"); al.ctl = h->ptr<PpoCtl>("ppo.ctl"); al.ent = W("ppo.log"); al.par = h->ptr<TrpoPar>("trpo.par");
    launch_trpo_alpha(al, h->stream);
    HIPCHK(h, hipGetLastError());
    h->trpo_rows = n;
    h->trpo_sub = params->trust_sub;
    return 0;
}

int sacx_trpo_grad(sacx_handle* h, float* out_dev) {
    if (trpo_check(h)) return -1;
    if (!out_dev) return fail(h, "null output");
    if (h->trpo_rows < 1) return fail(h, "no rollout table: call sacx_trpo_begin first");
    HIPCHK(h, hipMemcpyAsync(out_dev, trpo_vec(h, TRV_B), sizeof(float) * (size_t)h->trpo_nv, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

int sacx_trpo_fvp(sacx_handle* h, const float* x_dev, float* out_dev, int32_t flags) {
    if (trpo_check(h)) return -1;
    if (!x_dev || !out_dev) return fail(h, "null vector");
    if (h->trpo_rows < 1) return fail(h, "no rollout table: call sacx_trpo_begin first");
    const size_t nb = sizeof(float) * (size_t)h->trpo_nv;
    HIPCHK(h, hipMemcpyAsync(trpo_vec(h, TRV_P), x_dev, nb, hipMemcpyDeviceToDevice, h->stream));
    if (flags & SACX_STEP_EAGER) {
        std::vector<Launch> plan;
        trpo_pass_plan(h, plan, 1, h->trpo_rows, h->trpo_sub, trpo_vec(h, TRV_P), trpo_vec(h, TRV_Z));
        for (const Launch& L : plan) enqueue(L, h, h->stream);
        HIPCHK(h, hipGetLastError());
    } else {
        const std::pair<int64_t, int32_t> key{h->trpo_rows, h->trpo_sub};
        if (!h->trpo_fgraph || h->trpo_fkey != key) {
            if (h->trpo_fgraph) (void)hipGraphExecDestroy(h->trpo_fgraph);
            h->trpo_fgraph = nullptr;
            std::vector<Launch> plan;
            trpo_pass_plan(h, plan, 1, h->trpo_rows, h->trpo_sub, trpo_vec(h, TRV_P), trpo_vec(h, TRV_Z));
            if (capture_plan(h, "TRPO Fisher product", plan, 1, &h->trpo_fgraph)) return -1;
            h->trpo_fkey = key;
        }
        HIPCHK(h, hipGraphLaunch(h->trpo_fgraph, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(out_dev, trpo_vec(h, TRV_Z), nb, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// update_utils.cg from x = 0, then vFv = x . F(x), eta = sqrt(2 delta / vFv), step = eta x: one launch
// list, no host round trip (the break is the done flag of each iteration)
static void trpo_solve_plan(sacx_handle* h, std::vector<Launch>& plan, int cg_it) {
    float *p = trpo_vec(h, TRV_P), *x = trpo_vec(h, TRV_X), *z = trpo_vec(h, TRV_Z);
    plan.push_back(trpo_cg_launch(h, TRC_INIT, 0, "trpo.cg.init"));
    for (int it = 0; it < cg_it; ++it) {
        trpo_pass_plan(h, plan, 1, h->trpo_rows, h->trpo_sub, p, z);
        plan.push_back(trpo_cg_launch(h, TRC_DOT, it, "trpo.cg.dot"));
        plan.push_back(trpo_cg_launch(h, TRC_UPD1, it, "trpo.cg.xr"));
        plan.push_back(trpo_cg_launch(h, TRC_UPD2, it, "trpo.cg.p"));
    }
    trpo_pass_plan(h, plan, 1, h->trpo_rows, h->trpo_sub, x, z);
    plan.push_back(trpo_cg_launch(h, TRC_DOTX, 0, "trpo.vfv"));
    plan.push_back(trpo_cg_launch(h, TRC_SCALE, 0, "trpo.scale"));
}

int sacx_trpo_step(sacx_handle* h, const sacx_trpo_params* params, int32_t flags, double* out) {
    if (trpo_check(h)) return -1;
    if (trpo_par_check(h, params)) return -1;
    if (!out) return fail(h, "null output");
    if (h->trpo_rows < 1) return fail(h, "no rollout table: call sacx_trpo_begin first");
    if (params->trust_sub != h->trpo_sub) return fail(h, "trust_sub differs from sacx_trpo_begin's");
    const int64_t n = h->trpo_rows;
    auto W = [&](const std::string& nm) { return h->f(nm); };
    trpo_par_set(h, params, n, h->stream);
    double sc[16];
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(sc, h->ptr<double>("trpo.sc"), sizeof(sc), hipMemcpyDeviceToHost));
    // np.allclose(pg_vec, 0) or delta == 0 (trpo.py:179): the zero step
    const bool zero = !(sc[TRS_GMAX] > 1e-8) && sc[TRS_GMAX] == sc[TRS_GMAX];
    if (zero || params->delta == 0.f) {
        launch_trpo_cg(trpo_cg_args(h, TRC_ZERO, 0), h->stream);
    } else {
        if (flags & SACX_STEP_EAGER) {
            std::vector<Launch> plan;
            trpo_solve_plan(h, plan, params->cg_it);
            for (const Launch& L : plan) enqueue(L, h, h->stream);
            HIPCHK(h, hipGetLastError());
        } else {
            const std::tuple<int64_t, int32_t, int32_t> key{n, h->trpo_sub, params->cg_it};
            if (!h->trpo_graph || h->trpo_gkey != key) {
                if (h->trpo_graph) (void)hipGraphExecDestroy(h->trpo_graph);
                h->trpo_graph = nullptr;
                std::vector<Launch> plan;
                trpo_solve_plan(h, plan, params->cg_it);
                if (capture_plan(h, "TRPO solve", plan, 1, &h->trpo_graph)) return -1;
                h->trpo_gkey = key;
            }
            HIPCHK(h, hipGraphLaunch(h->trpo_graph, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(sc, h->ptr<double>("trpo.sc"), sizeof(sc), hipMemcpyDeviceToHost));
        // the reference divides by vFv and accepts the NaNs that follow; here the update is refused
        // with the weights untouched
        if (!(sc[TRS_VFV] > 0.0) || !(sc[TRS_ETA] == sc[TRS_ETA]) || std::isinf(sc[TRS_ETA]))
            return fail(h, "TRPO: the step is degenerate (vFv = " + std::to_string(sc[TRS_VFV]) +
                               " is not positive, or not finite); the weights are unchanged");
    }
    // _backtrack (trpo.py:229-317)
    const size_t nb = sizeof(float) * (size_t)h->trpo_nv;
    HIPCHK(h, hipMemcpyAsync(trpo_vec(h, TRV_SAVED), W("actor.l0"), nb, hipMemcpyDeviceToDevice, h->stream));
    std::vector<Launch> eval;
    trpo_pass_plan(h, eval, 2, n, 1, nullptr, nullptr);
    float lg[8];
    auto evaluate = [&]() -> int {          // tv, kl, mean(r adv) with the weights as they stand
        for (const Launch& L : eval) enqueue(L, h, h->stream);
        PpoReduceArgs q{};
        float* ev = W("trpo.ev");
        float* lo = W("trpo.log");
        q.c[0] = ev + h->cap; q.out[0] = lo; q.half0 = 0.5f;        // tv
        q.c[1] = ev + 2 * (size_t)h->cap; q.out[1] = lo + 1;        // kl
        q.c[2] = ev; q.out[2] = lo + 2;                             // surr
        q.n = n;
        launch_ppo_reduce(q, h->stream);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(lg, lo, sizeof(lg), hipMemcpyDeviceToHost));
        return 0;
    };
    auto apply = [&](int add) {
        TrCgArgs a = trpo_cg_args(h, TRC_APPLY, 0);
        a.add = add;
        launch_trpo_cg(a, h->stream);
    };
    if (evaluate()) return -1;
    const float surr_before = lg[2];
    apply(1);
    if (evaluate()) return -1;
    const float tv_pre = lg[0], kl_pre = lg[1];
    float tv = lg[0], kl = lg[1], improve = lg[2] - surr_before;
    const float kl_max = (float)((double)params->kl_maxfactor * (double)params->delta);
    double adj = 1.0;
    bool ok = false;
    for (int t = 0; t < 10; ++t) {
        if (!(kl > kl_max) && !(improve < 0.f)) {
            ok = true;
            break;
        }
        adj = adj / std::sqrt(2.0);
        launch_trpo_cg(trpo_cg_args(h, TRC_SHRINK, 0), h->stream);
        apply(1);
        if (evaluate()) return -1;
        tv = lg[0]; kl = lg[1]; improve = lg[2] - surr_before;
    }
    if (!ok) {                              // no policy update
        adj = 0.0;
        apply(0);
        if (evaluate()) return -1;
        tv = lg[0]; kl = lg[1]; improve = lg[2] - surr_before;
    }
    float ent = 0.f, alpha = 0.f;
    HIPCHK(h, hipMemcpy(&ent, W("ppo.log"), sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(&alpha, W("ppo.alpha"), sizeof(float), hipMemcpyDeviceToHost));
    out[0] = ent; out[1] = tv_pre; out[2] = kl_pre; out[3] = tv; out[4] = kl; out[5] = adj; out[6] = improve; out[7] = alpha;
    return 0;
}

int sacx_trpo_plan_info(sacx_handle* h, int64_t rows, sacx_launch_info* out, int32_t cap, int32_t* n_out) {
    if (trpo_check(h)) return -1;
    if (!n_out) return fail(h, "null output");
    if (rows < 1 || rows > h->cap) return fail(h, "rows outside [1, buffer_capacity]");
    std::vector<Launch> plan;
    trpo_pass_plan(h, plan, 1, rows, 1, trpo_vec(h, TRV_P), trpo_vec(h, TRV_Z));
    return launch_info(plan, out, cap, n_out);
}

}  // extern "C"
