// gfx950 kernels of the TRPO actor update (trpo.h): the rows around the grouped GEMM launches of the
// whole-table passes (states in, the tangent rule of a layer, the head in its three modes), the
// chunk-ordered gradient accumulation, and the vector side of conjugate gradient and the line search.
#include "trpo.h"

namespace sacx {

namespace {

#define TR_LOG2PI_F 0x1.d67f1ep+0f      // f32 log(f32(2 pi)), as the PPO rows
#define TR_SOFTPLUS_THR -0x1.be2804p+3f // log(FLT_EPSILON) + 2 (TF softplus_op.h)

// a wave's sum in a fixed order (xor butterfly over 64 lanes): every lane gets the same bits
__device__ __forceinline__ float tr_wave_sum(float v) {
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double tr_wave_sum_d(double v) {
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float tr_wave_max(float v) {
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// the wave sums of a workgroup of NW waves added in wave order: every thread gets the same bits
template <int NW>
__device__ __forceinline__ double tr_block_sum_d(double v, double* red) {
    const double w = tr_wave_sum_d(v);
    __syncthreads();                // (red may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    double t = red[0];
    for (int i = 1; i < NW; ++i) t = t + red[i];
    return t;
}

__device__ __forceinline__ float tr_softplus(float x) {
    if (x > -TR_SOFTPLUS_THR) return x;
    if (x < TR_SOFTPLUS_THR) return expf(x);
    return log1pf(expf(x));
}

__device__ __forceinline__ float tr_dact(float h, int act) {
    switch (act) {
        case ACT_RELU: return h > 0.f ? 1.f : 0.f;
        case ACT_TANH: return 1.f - h * h;
        case ACT_ELU: return h < 0.f ? h + 1.f : 1.f;
        default: return 1.f;
    }
}

// GaussianActor._forward's column (continuous_actors.py:83-95), as the PPO rows compute it
struct TrCol {
    float mean, ls, inv_sp, sden;
    bool pass;
};
__device__ __forceinline__ TrCol tr_col(const PpoDist& d, int row, int lane, bool jok) {
    TrCol c;
    const float* o = d.O + (size_t)row * d.Aout;
    c.mean = jok ? o[lane] : 0.f;
    c.inv_sp = 1.f;
    c.sden = 1.f;
    float lun;
    if (d.per_state_std) {
        const float raw = jok ? o[d.A + lane] : 0.f;
        const float sp = tr_softplus(raw);
        lun = logf(sp) + d.logstd_init;
        c.inv_sp = 1.f / sp;
        c.sden = expf(-raw) + 1.f;
    } else {
        lun = (jok ? d.logstd[lane] : 0.f) + d.logstd_init;
    }
    const float fl = logf(1e-3f);
    c.pass = lun >= fl;             // TF maximum: ties go to the first argument
    c.ls = c.pass ? lun : fl;
    return c;
}

// SoftMaxActor's row (discrete_actors.py:47-96), as the PPO rows compute it: lane j < A holds logit j,
// everything on the max-shifted logits, log p = (l - max) - log(sum exp(l - max))
struct TrSm {
    float p, logp;
};
__device__ __forceinline__ TrSm tr_sm(float l, bool jok) {
    const float m = tr_wave_max(jok ? l : -INFINITY);
    const float x = jok ? l - m : 0.f;
    const float e = jok ? expf(x) : 0.f;
    const float z = tr_wave_sum(e);
    return TrSm{e / z, x - logf(z)};
}
// the categorical kl (:68-96) from the f32 logits with the arithmetic in f64, as the PPO rows compute it
// (the two log-sum-exps cancel down to a kl of 1e-4 .. 1e-2: f32 leaves 1e-7 absolute on each)
__device__ __forceinline__ float tr_sm_kl(float l, float lref, bool jok) {
    const float m = tr_wave_max(jok ? l : -INFINITY), mr = tr_wave_max(jok ? lref : -INFINITY);
    const double x = jok ? (double)l - (double)m : 0.0, xr = jok ? (double)lref - (double)mr : 0.0;
    const double e = jok ? exp(x) : 0.0, er = jok ? exp(xr) : 0.0;
    const double z = tr_wave_sum_d(e), zr = tr_wave_sum_d(er);
    return (float)tr_wave_sum_d(jok ? (e / z) * ((x - log(z)) - (xr - log(zr))) : 0.0);
}

// the sum of TRPO_PARTS f64 partials in index order (every caller the same bits)
__device__ __forceinline__ double tr_parts_sum(const double* p) {
    double t = 0.0;
    for (int i = 0; i < TRPO_PARTS; ++i) t = t + p[i];
    return t;
}

}  // namespace

// ==================================================================== rows in
__global__ __launch_bounds__(256) void k_trpo_in(TrInArgs g) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = 0; q < 16; ++q) {
        const int i = blockIdx.x * 64 + wave * 16 + q;
        if (i >= g.m) break;
        const float* s = g.s + (size_t)(g.row0 + (int64_t)i * g.stride) * g.S;
        for (int c = lane; c < g.ldS; c += 64)
            g.X[(size_t)i * g.ldS + c] = c < g.S ? (s[c] - g.s_mean[c]) / g.s_den[c] : 0.f;
    }
}

__global__ __launch_bounds__(1024) void k_trpo_advnorm(TrAdvArgs g) {
    __shared__ double red[16];
    // np.mean / np.std of the uncentred table (trpo.py:40-41): f32 rows, the sums in f64
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < g.n; i += 1024) acc = acc + (double)g.src[i];
    const float mean = (float)(tr_block_sum_d<16>(acc, red) / (double)g.n);
    double acc2 = 0.0;
    for (int64_t i = threadIdx.x; i < g.n; i += 1024) {
        const float d = g.src[i] - mean;
        acc2 = acc2 + (double)(d * d);
    }
    const float sd = sqrtf((float)(tr_block_sum_d<16>(acc2, red) / (double)g.n)) + 1e-8f;
    const int center = g.par->adv_center, scale = g.par->adv_scale;
    for (int64_t i = threadIdx.x; i < g.n; i += 1024) {
        float x = g.src[i];
        if (center) x = x - mean;
        if (scale) x = x / sd;
        g.dst[i] = x;
    }
}

// ==================================================================== a layer's tangent
__global__ __launch_bounds__(256) void k_trpo_tan(TrTanArgs g) {
    const int H = g.H;
    if (!g.ln) {
        const int64_t tot = (int64_t)g.m * H;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
            float pre = g.G0[i];
            if (g.G1 != nullptr) pre = pre + g.G1[i];
            g.T[i] = tr_dact(g.Hout[i], g.act) * pre;
        }
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= g.m) return;
    const float inv_h = 1.f / (float)H;
    const float* tz = g.G0 + (size_t)row * H;
    const float* xh = g.xhat + (size_t)row * H;
    const float rstd = g.rstd[row];
    float s1 = 0.f, s2 = 0.f;
    for (int j = lane; j < H; j += 64) {
        s1 = s1 + tz[j];
        s2 = s2 + tz[j] * xh[j];
    }
    const float m1 = tr_wave_sum(s1) * inv_h, m2 = tr_wave_sum(s2) * inv_h;
    for (int j = lane; j < H; j += 64) {
        const float txh = rstd * ((tz[j] - m1) - xh[j] * m2);
        const float ty = (g.gamma[j] * txh + g.vgamma[j] * xh[j]) + g.vgamma[H + j];
        const float hh = g.Hout[(size_t)row * H + j];
        g.T[(size_t)row * H + j] = (1.f - hh * hh) * ty;
    }
}

// ==================================================================== the head
__global__ __launch_bounds__(256) void k_trpo_head(TrHeadArgs g) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= g.m) return;
    const int A = g.d.A, Aout = g.d.Aout;
    const bool jok = lane < A;
    if (g.d.softmax) {
        const int64_t trow = g.row0 + row;
        const float l = jok ? g.d.O[(size_t)row * Aout + lane] : 0.f;
        const TrSm sm = tr_sm(l, jok);
        if (g.mode == 1) {
            // u = M t / n_sub with M = diag(p) - p p^T: the Hessian of the mean kl at cur = ref
            const float t = jok ? g.TO0[(size_t)row * Aout + lane] + g.TO1[(size_t)row * Aout + lane] : 0.f;
            const float pt = tr_wave_sum(jok ? sm.p * t : 0.f);
            if (jok) g.D3[(size_t)row * Aout + lane] = (sm.p * (t - pt)) * g.par->inv_nsub;
            return;
        }
        const float af = g.a[trow];
        const int ai = (af >= 0.f && af < (float)A) ? (int)af : -1;     // outside [0, A): tf.one_hot's zero row
        const float nlp = 0.f - tr_wave_sum(lane == ai ? sm.logp : 0.f);
        const float r = expf(g.nlp_old[trow] - nlp);
        const float adv = g.adv[trow];
        if (g.mode == 0) {
            const float inv_n = g.par->inv_n;
            const float gn = ai >= 0 ? (adv * r) * inv_n : 0.f;
            const float ent = 0.f - tr_wave_sum(jok ? sm.p * sm.logp : 0.f);
            const float dent = -(sm.p * (sm.logp + ent));
            if (jok) g.D3[(size_t)row * Aout + lane] = gn * (sm.p - (lane == ai ? 1.f : 0.f)) - (g.alpha[0] * inv_n) * dent;
            return;
        }
        const float kl = tr_sm_kl(l, jok ? g.mean_ref[(size_t)trow * A + lane] : 0.f, jok);
        if (lane == 0) {
            g.o_radv[trow] = r * adv;
            g.o_rdiff[trow] = fabsf(r - 1.f);
            g.o_kl[trow] = kl;
        }
        return;
    }
    const TrCol c = tr_col(g.d, row, lane, jok);
    const int64_t tr = g.row0 + row;
    if (g.mode == 1) {
        // J x at the head: t_mean, t_ls (masked where the floor holds); u = M t / n_sub; back through
        // the head's own Jacobian (d ls / d raw by LogGrad and SoftplusGrad, as the PPO head)
        const float* t0 = g.TO0 + (size_t)row * Aout;
        const float* t1 = g.TO1 + (size_t)row * Aout;
        const float tm = jok ? t0[lane] + t1[lane] : 0.f;
        float tl;
        if (g.d.per_state_std) {
            const float traw = jok ? t0[A + lane] + t1[A + lane] : 0.f;
            tl = (traw * c.inv_sp) / c.sden;
        } else {
            tl = jok ? g.vls[lane] : 0.f;
        }
        tl = c.pass ? tl : 0.f;
        const float inv = g.par->inv_nsub;
        const float um = (tm / expf(2.f * c.ls)) * inv;
        float ul = (2.f * tl) * inv;
        ul = c.pass ? ul : 0.f;
        if (jok) {
            g.D3[(size_t)row * Aout + lane] = um;
            if (g.d.per_state_std) g.D3[(size_t)row * Aout + A + lane] = (ul * c.inv_sp) / c.sden;
            else g.E[(size_t)row * A + lane] = ul;
        }
        return;
    }
    const float a = jok ? g.a[(size_t)tr * A + lane] : 0.f;
    const float sd = expf(c.ls);
    const float z = (a - c.mean) / sd;
    const float nlp = 0.5f * tr_wave_sum(jok ? (z * z + 2.f * c.ls) + TR_LOG2PI_F : 0.f);
    const float r = expf(g.nlp_old[tr] - nlp);
    const float adv = g.adv[tr];
    if (g.mode == 0) {
        // trpo.py:52-63: loss = mean(-r adv) - alpha (mean(ent) - ent_targ)
        const float inv_n = g.par->inv_n;
        const float gn = (adv * r) * inv_n;                     // d loss / d nlp_cur (dr / dnlp = -r)
        const float alpha = g.alpha[0];
        const float dmean = gn * (-(z / sd));                   // d nlp / d mean = -(a - mean) / sd^2
        float dls = gn * (1.f - z * z) - alpha * inv_n;         // d nlp / d ls = 1 - z^2, d ent / d ls = 1
        dls = c.pass ? dls : 0.f;
        if (jok) {
            g.D3[(size_t)row * Aout + lane] = dmean;
            if (g.d.per_state_std) g.D3[(size_t)row * Aout + A + lane] = (dls * c.inv_sp) / c.sden;
            else g.E[(size_t)row * A + lane] = dls;
        }
        return;
    }
    // mode 2: the line search's figures (trpo.py:252-265); the kl in the PPO rows' form
    const float mr = jok ? g.mean_ref[(size_t)tr * A + lane] : 0.f;
    const float lr = jok ? g.ls_ref[(size_t)tr * A + lane] : 0.f;
    const float dm = c.mean - mr;
    const float dl = c.ls - lr;
    const float vec = (dm * dm) / expf(2.f * c.ls) + (expm1f(-2.f * dl) + 2.f * dl);
    const float kl = 0.5f * tr_wave_sum(jok ? vec : 0.f);
    if (lane == 0) {
        g.o_radv[tr] = r * adv;
        g.o_rdiff[tr] = fabsf(r - 1.f);
        g.o_kl[tr] = kl;
    }
}

// ==================================================================== chunk-ordered accumulation
__global__ __launch_bounds__(256) void k_trpo_acc(TrAccArgs g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    float v = g.g[i];
    if (!g.first) v = g.dst[i] + v;
    if (g.last) {
        v = v * g.sign;
        if (g.x != nullptr) v = v + g.par->damp * g.x[i];
    }
    g.dst[i] = v;
}

// ==================================================================== conjugate gradient, the step
__global__ __launch_bounds__(256) void k_trpo_cg(TrCgArgs g) {
    __shared__ double red[4];
    const int64_t per = (g.n + TRPO_PARTS - 1) / TRPO_PARTS;
    const int64_t i0 = (int64_t)blockIdx.x * per;
    const int64_t i1 = i0 + per < g.n ? i0 + per : g.n;
    float* b = g.vec + TRV_B * g.vstride;
    float* x = g.vec + TRV_X * g.vstride;
    float* r = g.vec + TRV_R * g.vstride;
    float* p = g.vec + TRV_P * g.vstride;
    float* z = g.vec + TRV_Z * g.vstride;
    float* saved = g.vec + TRV_SAVED * g.vstride;
    float* step = g.vec + TRV_STEP * g.vstride;
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    switch (g.phase) {
        case TRC_GMAX: {            // np.allclose(pg_vec, 0): max |b| (one workgroup)
            __shared__ float mred[4];
            float m = 0.f;
            for (int64_t i = threadIdx.x; i < g.n; i += 256) {
                const float v = fabsf(b[i]);
                m = (v > m || v != v) ? v : m;      // (a NaN gradient is not a zero one)
            }
            m = tr_wave_max(m);
            if ((threadIdx.x & 63) == 0) mred[threadIdx.x >> 6] = m;
            __syncthreads();
            if (threadIdx.x == 0) g.sc[TRS_GMAX] = (double)fmaxf(fmaxf(mred[0], mred[1]), fmaxf(mred[2], mred[3]));
            return;
        }
        case TRC_ZERO:              // the zero step (trpo.py:179-180)
            for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) step[i] = 0.f;
            if (lead) { g.sc[TRS_VFV] = 0.0; g.sc[TRS_ETA] = 0.0; g.sc[TRS_ITERS] = 0.0; g.sc[TRS_RR] = 0.0; }
            return;
        case TRC_INIT: {            // x = 0, r = p = b, r.r
            double acc = 0.0;
            for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
                const float v = b[i];
                x[i] = 0.f; r[i] = v; p[i] = v;
                acc = acc + (double)v * (double)v;
            }
            const double s = tr_block_sum_d<4>(acc, red);
            if (threadIdx.x == 0) g.rr[blockIdx.x] = s;
            if (lead) { g.done[0] = 0; g.sc[TRS_ITERS] = 0.0; }
            return;
        }
        case TRC_DOT: case TRC_DOTX: {      // p.z (an iteration), x.z (vFv)
            if (g.phase == TRC_DOT && g.done[g.it]) return;
            const float* u = g.phase == TRC_DOT ? p : x;
            double acc = 0.0;
            for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) acc = acc + (double)u[i] * (double)z[i];
            const double s = tr_block_sum_d<4>(acc, red);
            if (threadIdx.x == 0) g.pz[blockIdx.x] = s;
            return;
        }
        case TRC_UPD1: {            // v = r.r / p.z; x += v p; r -= v z; the new r.r
            if (g.done[g.it]) return;
            const double rr = tr_parts_sum(g.rr + (size_t)g.it * TRPO_PARTS);
            const float v = (float)(rr / tr_parts_sum(g.pz));
            double acc = 0.0;
            for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
                x[i] = x[i] + v * p[i];
                const float rn = r[i] - v * z[i];
                r[i] = rn;
                acc = acc + (double)rn * (double)rn;
            }
            const double s = tr_block_sum_d<4>(acc, red);
            if (threadIdx.x == 0) g.rr[(size_t)(g.it + 1) * TRPO_PARTS + blockIdx.x] = s;
            return;
        }
        case TRC_UPD2: {            // mu = new / old; p = r + mu p; the break as a flag
            if (g.done[g.it]) {
                if (lead) g.done[g.it + 1] = 1;
                return;
            }
            const double old = tr_parts_sum(g.rr + (size_t)g.it * TRPO_PARTS);
            const double nw = tr_parts_sum(g.rr + (size_t)(g.it + 1) * TRPO_PARTS);
            const float mu = (float)(nw / old);
            for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) p[i] = r[i] + mu * p[i];
            if (lead) {
                g.done[g.it + 1] = nw < 1e-10 ? 1 : 0;
                g.sc[TRS_ITERS] = (double)(g.it + 1);
                g.sc[TRS_RR] = nw;
            }
            return;
        }
        case TRC_SCALE: {           // vFv = x.F(x); eta = sqrt(2 delta / vFv); step = eta x
            const double vfv = tr_parts_sum(g.pz);
            const double eta = sqrt(2.0 * (double)g.par->delta / vfv);
            const float e = (float)eta;
            for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) step[i] = e * x[i];
            if (lead) { g.sc[TRS_VFV] = vfv; g.sc[TRS_ETA] = eta; }
            return;
        }
        case TRC_SHRINK:            // eta_v_flat / sqrt(2) (trpo.py:280-282)
            for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) step[i] = step[i] / 0x1.6a09e6p+0f;
            return;
        case TRC_APPLY:             // GaussianActor.set_weights (continuous_actors.py:211-234)
            for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
                float w = saved[i];
                if (g.add) w = w + step[i];
                if (i >= g.ls_off && i < g.ls_off + g.ls_n) w = fmaxf(w, g.ls_floor);
                g.W[i] = w;
            }
            return;
    }
}

__global__ __launch_bounds__(64) void k_trpo_alpha(TrAlphaArgs g) {
    if (threadIdx.x != 0 || !g.par->ent_reg) return;
    const int64_t t = g.ctl->t_alpha + 1;
    const float tt = (float)t;
    const float lr_t = g.par->alpha_lr * sqrtf(1.f - powf(0.999f, tt)) / (1.f - powf(0.9f, tt));
    const float gr = g.ent[0] - g.par->ent_targ;
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-7f;
    float mm = g.alpha[1], vv = g.alpha[2];
    mm = mm + (gr - mm) * (1.f - b1);
    vv = vv + (gr * gr - vv) * (1.f - b2);
    g.alpha[0] = fmaxf(g.alpha[0] - (mm * lr_t) / (sqrtf(vv) + eps), 0.f);
    g.alpha[1] = mm;
    g.alpha[2] = vv;
    g.ctl->t_alpha = t;
}

__global__ __launch_bounds__(64) void k_trpo_set(TrpoPar* dst, TrpoPar v) {
    if (threadIdx.x == 0) *dst = v;
}

__global__ __launch_bounds__(256) void k_trpo_fill(float* p, int64_t n, float v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// ==================================================================== launchers
void launch_trpo_in(const TrInArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_trpo_in, dim3((a.m + 63) / 64), dim3(256), 0, s, a);
}
void launch_trpo_advnorm(const TrAdvArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_trpo_advnorm, dim3(1), dim3(1024), 0, s, a);
}
void launch_trpo_tan(const TrTanArgs& a, hipStream_t s) {
    const int64_t tot = (int64_t)a.m * a.H;
    const unsigned grid = a.ln ? (unsigned)((a.m + 3) / 4) : (unsigned)((tot + 255) / 256);
    hipLaunchKernelGGL(k_trpo_tan, dim3(grid), dim3(256), 0, s, a);
}
void launch_trpo_head(const TrHeadArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_trpo_head, dim3((a.m + 3) / 4), dim3(256), 0, s, a);
}
void launch_trpo_acc(const TrAccArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_trpo_acc, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
}
void launch_trpo_cg(const TrCgArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_trpo_cg, dim3(a.phase == TRC_GMAX ? 1 : TRPO_PARTS), dim3(256), 0, s, a);
}
void launch_trpo_alpha(const TrAlphaArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_trpo_alpha, dim3(1), dim3(64), 0, s, a);
}
void launch_trpo_set(TrpoPar* dst, const TrpoPar& v, hipStream_t s) {
    hipLaunchKernelGGL(k_trpo_set, dim3(1), dim3(64), 0, s, dst, v);
}
void launch_trpo_fill(float* p, int64_t n, float v, hipStream_t s) {
    hipLaunchKernelGGL(k_trpo_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n, v);
}

}  // namespace sacx
