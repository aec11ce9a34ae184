// The critic side of the on-policy loop on a trainable GaussianActor handle (sacx_vcritic_*, sacx_gae*):
// VCritic._forward / value / get_loss (critics.py:30-49), gae / gae_batch (buffer_utils.py:8-83) and
// BaseOnPolicyAlg._update_critics / _apply_critic_grads (base_onpolicy_alg.py:219-283).  The kernels are
// k_vcritic.hip's (a translation unit of its own); the matrix work is the grouped GEMM launches of k_sac.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "sacx_internal.h"

namespace sacx {

#define GAE_TILE 2048               // rows per workgroup of the GAE scan: 256 threads x GAE_ROWS rows
#define GAE_ROWS 8
#define VC_IDX_CAP 1024             // minibatch steps the index ring holds
#define VC_GATHER_ROWS 64           // rows per workgroup of k_vc_gather
#define VC_STAT_COLS (MAX_MODELS + 2)   // the summed loss, each critic's loss, the step number
#define VC_THREADS 1024             // the one-workgroup reductions

// Segment "vc.ctl" (int64 x 16)
struct VcCtl {
    int64_t seq;                    // minibatch steps run (index / statistics ring position)
    int64_t t;                      // iterations of the critics' one Adam (persists across calls)
    int64_t n_rows[MAX_MODELS];     // rows of each critic's table (sacx_vcritic_begin; 0: none)
    int64_t pad[6];
};
// Segment "vc.par" (float x 16): the step's run-time parameters, written in stream order at each
// sacx_vcritic_steps call (never constants of a captured graph)
struct VcPar {
    float critic_lr;
    float pad[15];
};

// k_vc_gather: the step's minibatch rows by index from every critic's table -> row k * mb + i of X
// (normalised states, pad columns 0) and T (rtg / ret_den); the same indices for every critic
struct VcGatherArgs {
    const float* s; int64_t s_stride;       // critic k's table: s + k * s_stride, [n_k, S]
    const float* rtg; int64_t rtg_stride;   // rtg + k * rtg_stride, [n_k]
    const int32_t* idx_ring; int32_t idx_ld;    // [VC_IDX_CAP, idx_ld]
    const VcCtl* ctl;
    const float *s_mean, *s_den, *ret_den;
    int32_t S, ldS, mb, nc;
    float* X;                       // [nc * mb, ldS]
    float* T;                       // [nc * mb]
    // packed learners (sacx_vcritic_steps_packed): the K learners' arena blocks sit sstride bytes apart,
    // grid z = learner, every pointer above moves by blockIdx.z * sstride
    int64_t sstride;
    int32_t nseeds;
};

// k_vc_head: per row g = (v - rtg_n) / mb (d loss / d output) and the row's squared difference
struct VcHeadArgs {
    const float *O, *T;             // [rows] the output layer's rows, the normalised targets
    int32_t rows, mb;
    float* G;                       // [rows]
    float* sq;                      // [rows]
    int64_t sstride;                // packed learners, as VcGatherArgs
    int32_t nseeds;
};

// k_vc_final: one workgroup -- each critic's 0.5 * mean of its mb squared differences (a fixed order),
// their sum in critic order, the statistics row, the counters
struct VcFinalArgs {
    const float* sq;
    int32_t mb, nc;
    VcCtl* ctl;
    float* stats; int32_t stats_cap;
    int64_t sstride;                // packed learners, as VcGatherArgs
    int32_t nseeds;
};

// k_vc_adam: Keras Adam over the critics' parameter range (m, v, gradient at +1, +2, +3 p_stride), the
// rate and the iteration count read from the device; the project's Adam arithmetic (k_adam_apply's)
struct VcAdamArgs {
    float* P; int64_t n; int64_t p_stride;
    const float* lr_dev;
    const int64_t* t_dev; int32_t t_adv;    // the count used is t_dev[0] + 1 - t_adv
    int64_t sstride;                // packed learners, as VcGatherArgs
    int32_t nseeds;
};

// k_vc_rows: a chunk of the whole-table passes -- out[i] = Q[i] (x ret_den with value), and / or
// sq[i] = (rtg[i] / ret_den - Q[i])^2
struct VcRowsArgs {
    const float* Q; int32_t m, value;
    const float* ret_den;
    const float* rtg;               // nullable
    float* out;                     // nullable
    float* sq;                      // nullable
};
// k_vc_reduce: one workgroup -- out[0] = 0.5 * sum(sq[0, n)) / n in a fixed order
struct VcReduceArgs {
    const float* sq; int64_t n; float* out;
};

// The GAE scan (buffer_utils.py:11-42 on given values, f64): launch 1 writes each tile's aggregate
// affine map, launch 2 composes the aggregates to the right of its tile into the carry, scans its
// tile again and stores the three f32 outputs
struct GaeArgs {
    const float *v_s, *v_sp, *r, *d;
    const int32_t* traj;
    int64_t n;
    double gamma, gl;               // gamma, gamma * lam
    double* agg;                    // [tiles, 2] (a, b)
    int32_t tiles;
    float *adv, *rtg, *rtg_sp;
};

void launch_vc_gather(const VcGatherArgs& a, hipStream_t s);
void launch_vc_head(const VcHeadArgs& a, hipStream_t s);
void launch_vc_final(const VcFinalArgs& a, hipStream_t s);
void launch_vc_adam(const VcAdamArgs& a, hipStream_t s);
void launch_vc_rows(const VcRowsArgs& a, hipStream_t s);
void launch_vc_reduce(const VcReduceArgs& a, hipStream_t s);
void launch_gae(const GaeArgs& a, hipStream_t s);
// host values into the arena in stream order: dst != null: *dst = v; critic >= 0: its table's row count
void launch_vc_set(VcPar* dst, const VcPar& v, VcCtl* ctl, int32_t critic, int64_t n, hipStream_t s);

}  // namespace sacx
