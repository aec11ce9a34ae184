// The TRPO actor update of a trainable GaussianActor handle (sacx_trpo_*; trpo.py:34-317, the
// expert_reg is None branch with grad_final := neg_pg; update_utils.py:4-24; continuous_actors.py:
// 201-234).  The kernels are k_trpo.hip's (a translation unit of its own); the matrix work is the
// grouped GEMM launches of k_sac.hip.
//
// Whole-table passes move TRPO_CHUNK rows at a time through the actor; a pass that ends in a
// gradient (the surrogate gradient, a Fisher-vector product) stores each chunk's dW and adds it
// to the result in chunk order (k_trpo_acc), so two runs add the same numbers in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "sacx_internal.h"

namespace sacx {

#define TRPO_CHUNK 4096             // rows per launch chain of a whole-table pass
#define TRPO_PARTS 128              // the fixed partition of the flat range (dot products, vector updates)
#define TRPO_CG_MAX 255             // cg_it bound (the per-iteration residual partials and flags)
#define TRPO_VECS 7                 // b (pg_vec), x, r, p, z, saved weights, step
enum { TRV_B = 0, TRV_X, TRV_R, TRV_P, TRV_Z, TRV_SAVED, TRV_STEP };

// Segment "trpo.par" (16 words): the update's run-time parameters, written in stream order
// (never constants of a captured graph)
struct TrpoPar {
    float delta, damp, ent_targ, alpha_lr;
    float inv_n, inv_nsub;          // 1 / rows of the table, 1 / rows of s_all[::trust_sub]
    int32_t ent_reg, adv_center, adv_scale;
    int32_t pad[7];
};
// Segment "trpo.sc" (f64 x 16): [0] max |pg_vec|, [1] vFv, [2] eta, [3] CG iterations run,
// [4] the last residual r.r
enum { TRS_GMAX = 0, TRS_VFV, TRS_ETA, TRS_ITERS, TRS_RR };

// k_trpo_in: table rows row0 + i * stride (i < m) -> normalised state rows X [m, ldS] (pad columns 0)
struct TrInArgs {
    const float* s; int64_t row0, stride;
    const float *s_mean, *s_den;
    int32_t S, ldS, m;
    float* X;
};

// k_trpo_advnorm: one workgroup -- dst = the table centred / scaled by the population statistics of
// src (mean, std + 1e-8 of the uncentred rows; trpo.py:40-47, :244-250)
struct TrAdvArgs {
    const float* src; float* dst; int64_t n;
    const TrpoPar* par;
};

// k_trpo_tan: t_out = act'(h_out) (.) (G0 + G1) on a chunk's rows (G1 null: layer 0, whose input has
// no tangent).  ln: layer 0 under layer norm -- G0 is the pre-norm tangent, the norm's tangent rule
// t_xhat = rstd (tz - mean(tz) - xhat mean(tz xhat)), ty = gamma t_xhat + v_gamma xhat + v_beta,
// then tanh' (one wave per row, H <= 1,024)
struct TrTanArgs {
    const float *G0, *G1, *Hout;
    float* T;
    int32_t m, H, act, ln;
    const float *xhat, *rstd, *gamma, *vgamma;     // ln (v_beta = vgamma + H)
};

// k_trpo_head: one wave per row, lane = action dimension.
//   mode 0 (the surrogate gradient, trpo.py:52-63): d loss / d O and d loss / d logstd of
//          loss = mean(-r adv) - alpha (mean(ent) - ent_targ), scaled by 1 / n
//   mode 1 (the Fisher product): the output tangent TO0 + TO1 -> (t_mean, t_ls) -> M / n_sub times it,
//          back through the head: D3 [m, Aout] and E [m, A] as mode 0 leaves them
//   mode 2 (the line search's evaluation): per row r adv, |r - 1|, kl against the reference
// On a softmax handle (d.softmax) lane = logit: mode 0 writes d loss / d logits, mode 1
// u = p (t - sum_j p_j t_j) / n_sub (M = diag(p) - p p^T at the reference point), mode 2 the categorical
// kl (discrete_actors.py:68-96); a is one index per row, mean_ref the reference logits, E is not written
struct TrHeadArgs {
    PpoDist d;
    int32_t mode, m;
    int64_t row0;                   // the chunk's first table row (modes 0, 2: a, adv, nlp_old, the reference)
    const float *a, *adv, *nlp_old, *mean_ref, *ls_ref;
    const float* alpha;             // ppo.alpha[0]
    const TrpoPar* par;
    const float *TO0, *TO1;         // mode 1: the two halves of the output layer's tangent [m, Aout]
    const float* vls;               // mode 1: the direction's logstd entries [A] (state-independent std)
    float *D3, *E;
    float *o_radv, *o_rdiff, *o_kl; // mode 2: table-indexed outputs
};

// k_trpo_acc: dst (+)= g over the flat range, chunk by chunk; on the last chunk
// dst = sign * sum + damp * x (x null: no damping term)
struct TrAccArgs {
    const float* g; float* dst; const float* x;
    int64_t n;
    int32_t first, last;
    float sign;
    const TrpoPar* par;
};

// k_trpo_cg: the vector side of update_utils.cg on the flat range, TRPO_PARTS workgroups, each its own
// contiguous slice; every dot product is TRPO_PARTS f64 partials summed in index order by whoever
// reads it.  A launch boundary is the only ordering between phases.
enum { TRC_INIT = 0, TRC_DOT, TRC_UPD1, TRC_UPD2, TRC_DOTX, TRC_SCALE, TRC_GMAX, TRC_APPLY, TRC_SHRINK, TRC_ZERO };
struct TrCgArgs {
    int32_t phase, it;
    int64_t n;
    float* vec; int64_t vstride;    // trpo.vec: TRPO_VECS vectors vstride floats apart
    double* rr;                     // [TRPO_CG_MAX + 1, TRPO_PARTS] r.r partials of each iteration
    double* pz;                     // [TRPO_PARTS] p.z / x.z partials
    int32_t* done;                  // [TRPO_CG_MAX + 2]
    double* sc;                     // trpo.sc
    const TrpoPar* par;
    // TRC_APPLY: W = saved + step (add != 0) or saved, the state-independent logstd words
    // [ls_off, ls_off + ls_n) floored at ls_floor (GaussianActor.set_weights)
    float* W; int64_t ls_off; int32_t ls_n, add; float ls_floor;
};

// k_trpo_alpha: one thread -- alpha's Keras Adam with gradient mean(ent) - ent_targ, then max(alpha, 0)
struct TrAlphaArgs {
    float* alpha;                   // ppo.alpha [3]
    PpoCtl* ctl;
    const float* ent;               // ppo.log[0]
    const TrpoPar* par;
};

void launch_trpo_in(const TrInArgs& a, hipStream_t s);
void launch_trpo_advnorm(const TrAdvArgs& a, hipStream_t s);
void launch_trpo_tan(const TrTanArgs& a, hipStream_t s);
void launch_trpo_head(const TrHeadArgs& a, hipStream_t s);
void launch_trpo_acc(const TrAccArgs& a, hipStream_t s);
void launch_trpo_cg(const TrCgArgs& a, hipStream_t s);
void launch_trpo_alpha(const TrAlphaArgs& a, hipStream_t s);
void launch_trpo_set(TrpoPar* dst, const TrpoPar& v, hipStream_t s);
void launch_trpo_fill(float* p, int64_t n, float v, hipStream_t s);

}  // namespace sacx
