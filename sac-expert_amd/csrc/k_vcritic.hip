// gfx950 kernels of the critic side of the on-policy loop (vcritic.h): the rows around the grouped
// GEMM launches of a critic step, the whole-table passes, and the segmented f64 GAE scan.
#include "vcritic.h"

namespace sacx {

namespace {

// a wave's sum in a fixed order (xor butterfly over 64 lanes): every lane gets the same bits
__device__ __forceinline__ float vc_wave_sum(float v) {
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// the wave sums of a workgroup of NW waves added in wave order: every thread gets the same bits
template <int NW>
__device__ __forceinline__ float vc_block_sum(float v, float* red) {
    const float w = vc_wave_sum(v);
    __syncthreads();                // (red may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    float t = red[0];
    for (int i = 1; i < NW; ++i) t = t + red[i];
    return t;
}

// Packed learners (sacx_vcritic_steps_packed): grid z is the learner, and each arena pointer of the
// (learner-0) launch arguments moves by blockIdx.z * sstride -- k_sac.hip's seed_off / reloc idiom.  PK
// false is the one-learner launch: no relocation is compiled in.
__device__ __forceinline__ int64_t vc_seed_off(int64_t sstride) { return (int64_t)blockIdx.z * sstride; }
template <class T>
__device__ __forceinline__ T* vc_sr(T* p, int64_t so) {
    return p ? reinterpret_cast<T*>(reinterpret_cast<unsigned long long>(p) + (unsigned long long)so) : p;
}
__device__ __forceinline__ void reloc(VcGatherArgs& g, int64_t so) {
    g.s = vc_sr(g.s, so); g.rtg = vc_sr(g.rtg, so); g.idx_ring = vc_sr(g.idx_ring, so); g.ctl = vc_sr(g.ctl, so);
    g.s_mean = vc_sr(g.s_mean, so); g.s_den = vc_sr(g.s_den, so); g.ret_den = vc_sr(g.ret_den, so);
    g.X = vc_sr(g.X, so); g.T = vc_sr(g.T, so);
}
__device__ __forceinline__ void reloc(VcHeadArgs& g, int64_t so) {
    g.O = vc_sr(g.O, so); g.T = vc_sr(g.T, so); g.G = vc_sr(g.G, so); g.sq = vc_sr(g.sq, so);
}
__device__ __forceinline__ void reloc(VcFinalArgs& g, int64_t so) {
    g.sq = vc_sr(g.sq, so); g.ctl = vc_sr(g.ctl, so); g.stats = vc_sr(g.stats, so);
}
__device__ __forceinline__ void reloc(VcAdamArgs& a, int64_t so) {
    a.P = vc_sr(a.P, so); a.lr_dev = vc_sr(a.lr_dev, so); a.t_dev = vc_sr(a.t_dev, so);
}
inline unsigned vc_seeds_z(int n) { return n > 1 ? (unsigned)n : 1u; }

}  // namespace

// ==================================================================== the critic step's rows
template <bool PK>
__global__ __launch_bounds__(256) void k_vc_gather(VcGatherArgs g) {
    if constexpr (PK) reloc(g, vc_seed_off(g.sstride));
    const int mb = g.mb, S = g.S, ldS = g.ldS, rows = g.nc * g.mb;
    const int32_t* idx = g.idx_ring + (size_t)(g.ctl->seq % VC_IDX_CAP) * g.idx_ld;
    const float rden = g.ret_den[0];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int RW = VC_GATHER_ROWS / 4;      // rows per wave
    for (int q = 0; q < RW; ++q) {
        const int j = blockIdx.x * VC_GATHER_ROWS + wave * RW + q;
        if (j >= rows) break;
        const int k = j / mb, i = j - k * mb;
        const int64_t n = g.ctl->n_rows[k];
        if (n < 1) continue;        // (no table: the host refuses the step before it gets here)
        // an index outside the table is clamped into it (the host checks every index it uploads)
        int64_t r = idx[i];
        r = r < 0 ? 0 : (r >= n ? n - 1 : r);
        const float* s = g.s + (size_t)k * g.s_stride + (size_t)r * S;
        for (int c = lane; c < ldS; c += 64) g.X[(size_t)j * ldS + c] = c < S ? (s[c] - g.s_mean[c]) / g.s_den[c] : 0.f;
        if (lane == 0) g.T[j] = g.rtg[(size_t)k * g.rtg_stride + r] / rden;
    }
}

template <bool PK>
__global__ __launch_bounds__(256) void k_vc_head(VcHeadArgs g) {
    if constexpr (PK) reloc(g, vc_seed_off(g.sstride));
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= g.rows) return;
    // critics.py:42-49: 0.5 mean((rtg_n - v_n)^2); d / d v_n = -(rtg_n - v_n) / mb
    const float diff = g.T[j] - g.O[j];
    g.G[j] = (diff * -1.f) * (1.f / (float)g.mb);
    g.sq[j] = diff * diff;
}

template <bool PK>
__global__ __launch_bounds__(256) void k_vc_final(VcFinalArgs g) {
    if constexpr (PK) reloc(g, vc_seed_off(g.sstride));
    __shared__ float red[4];
    float loss[MAX_MODELS];
    float sum = 0.f;                // v_loss_all = 0.0, += each critic's loss (base_onpolicy_alg.py:273-280)
#pragma unroll
    for (int k = 0; k < MAX_MODELS; ++k) {
        loss[k] = 0.f;
        if (k < g.nc) {
            float acc = 0.f;
            for (int i = threadIdx.x; i < g.mb; i += 256) acc = acc + g.sq[(size_t)k * g.mb + i];
            loss[k] = 0.5f * (vc_block_sum<4>(acc, red) / (float)g.mb);
            sum = sum + loss[k];
        }
    }
    if (threadIdx.x != 0) return;
    VcCtl* ctl = g.ctl;
    const int64_t seq = ctl->seq;
    float* st = g.stats + (size_t)(seq % g.stats_cap) * VC_STAT_COLS;
    st[0] = sum;
#pragma unroll
    for (int k = 0; k < MAX_MODELS; ++k) st[1 + k] = loss[k];
    st[1 + MAX_MODELS] = (float)(seq + 1);
    ctl->seq = seq + 1;
    ctl->t = ctl->t + 1;            // (the Adam launch behind this one takes the advanced count: t_adv)
}

template <bool PK>
__global__ __launch_bounds__(256) void k_vc_adam(VcAdamArgs a) {
    if constexpr (PK) reloc(a, vc_seed_off(a.sstride));
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const float tt = (float)(a.t_dev[0] + 1 - a.t_adv);
    const float lr_t = a.lr_dev[0] * sqrtf(1.f - powf(0.999f, tt)) / (1.f - powf(0.9f, tt));
    float* P = a.P + i;
    const float gr = P[3 * a.p_stride];
    const float e0 = P[0], e1 = P[a.p_stride], e2 = P[2 * a.p_stride];
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-7f;
    const float mm1 = e1 + (gr - e1) * (1.f - b1);
    const float vv1 = e2 + (gr * gr - e2) * (1.f - b2);
    P[0] = e0 - (mm1 * lr_t) / (sqrtf(vv1) + eps);
    P[a.p_stride] = mm1;
    P[2 * a.p_stride] = vv1;
}

__global__ __launch_bounds__(64) void k_vc_set(VcPar* dst, VcPar v, VcCtl* ctl, int32_t critic, int64_t n) {
    if (threadIdx.x != 0) return;
    if (dst != nullptr) *dst = v;
    if (critic >= 0 && critic < MAX_MODELS) ctl->n_rows[critic] = n;
}

// ==================================================================== the whole-table passes
__global__ __launch_bounds__(256) void k_vc_rows(VcRowsArgs g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.m) return;
    const float q = g.Q[i], rden = g.ret_den[0];
    if (g.out != nullptr) g.out[i] = g.value ? q * rden : q;     // critics.py:36-40
    if (g.sq != nullptr) {
        const float diff = g.rtg[i] / rden - q;
        g.sq[i] = diff * diff;
    }
}

__global__ __launch_bounds__(VC_THREADS) void k_vc_reduce(VcReduceArgs g) {
    __shared__ float red[VC_THREADS / 64];
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < g.n; i += VC_THREADS) acc = acc + g.sq[i];
    const float s = vc_block_sum<VC_THREADS / 64>(acc, red);
    if (threadIdx.x == 0) g.out[0] = 0.5f * (s / (float)g.n);
}

// ==================================================================== the GAE scan
// adv_t = delta_t + gamma lam adv_{t+1} within a trajectory is the suffix composition of the affine
// maps m_t: y -> b_t + a_t y with b_t = delta_t and a_t = gamma lam, or 0 at a trajectory's last row
// (the restart of gae_batch's sections).  (l o r)(y) = l(r(y)): l is the EARLIER row.
namespace {

struct Aff {
    double a, b;
};
__device__ __forceinline__ Aff aff_comp(const Aff& l, const Aff& r) { return Aff{l.a * r.a, l.b + l.a * r.b}; }
__device__ __forceinline__ Aff aff_shfl_down(const Aff& x, int off) {
    return Aff{__shfl_down(x.a, off, 64), __shfl_down(x.b, off, 64)};    // (two dwords per double)
}

// the map of row t (t < n)
__device__ __forceinline__ Aff gae_row(const GaeArgs& g, int64_t t, float& vs, float& r) {
    vs = g.v_s[t];
    r = g.r[t];
    const double delta = (double)r + g.gamma * (1.0 - (double)g.d[t]) * (double)g.v_sp[t] - (double)vs;
    const bool last = t + 1 >= g.n || g.traj[t + 1] != g.traj[t];
    return Aff{last ? 0.0 : g.gl, delta};
}

// The 256 threads' maps (thread order = row order) composed over the workgroup: returns the
// composition of every thread BEHIND this one (exclusive suffix; the identity for the last), and in
// `total` the composition of all 256.  sh: 4 maps.
__device__ __forceinline__ Aff aff_suffix_256(const Aff& mine, Aff* sh, Aff& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Aff x = mine;                   // inclusive suffix within the wave
    for (int off = 1; off < 64; off <<= 1) {
        const Aff y = aff_shfl_down(x, off);
        if (lane + off < 64) x = aff_comp(x, y);
    }
    Aff ex = aff_shfl_down(x, 1);   // lanes lane + 1 .. 63
    if (lane == 63) ex = Aff{1.0, 0.0};
    __syncthreads();                // (sh may still be read from a previous call)
    if (lane == 0) sh[wave] = x;
    __syncthreads();
    Aff tail{1.0, 0.0};             // the waves behind this one, in order
    for (int w = 3; w > wave; --w) tail = aff_comp(sh[w], tail);
    total = aff_comp(sh[0], aff_comp(sh[1], aff_comp(sh[2], sh[3])));
    return aff_comp(ex, tail);
}

}  // namespace

// launch 1: each tile's aggregate map
__global__ __launch_bounds__(256) void k_gae_tiles(GaeArgs g) {
    __shared__ Aff sh[4];
    const int64_t t0 = (int64_t)blockIdx.x * GAE_TILE + (int64_t)threadIdx.x * GAE_ROWS;
    Aff m{1.0, 0.0};
#pragma unroll
    for (int i = GAE_ROWS - 1; i >= 0; --i) {
        const int64_t t = t0 + i;
        if (t < g.n) {
            float vs, r;
            m = aff_comp(gae_row(g, t, vs, r), m);
        }
    }
    Aff total;
    (void)aff_suffix_256(m, sh, total);
    if (threadIdx.x == 0) {
        g.agg[2 * (size_t)blockIdx.x] = total.a;
        g.agg[2 * (size_t)blockIdx.x + 1] = total.b;
    }
}

// launch 2: the carry from the tiles to the right, the tile's scan, the outputs
__global__ __launch_bounds__(256) void k_gae_apply(GaeArgs g) {
    __shared__ Aff sh[4];
    // the aggregates of tiles blockIdx.x + 1 .. tiles - 1 composed in order and applied to 0: thread j
    // takes a contiguous stretch of them (a stretch that reaches a restart, a = 0, needs no more)
    const int first = blockIdx.x + 1, cnt = g.tiles - first;
    const int per = (cnt + 255) / 256;
    Aff c{1.0, 0.0};
    for (int q = 0; q < per; ++q) {
        const int e = first + threadIdx.x * per + q;
        if (e >= g.tiles || c.a == 0.0) break;
        c = aff_comp(c, Aff{g.agg[2 * (size_t)e], g.agg[2 * (size_t)e + 1]});
    }
    Aff call;
    (void)aff_suffix_256(c, sh, call);
    const double carry = call.b;    // the advantage at the first row of the next tile (0 behind the last)

    const int64_t t0 = (int64_t)blockIdx.x * GAE_TILE + (int64_t)threadIdx.x * GAE_ROWS;
    Aff row[GAE_ROWS];
    float vs[GAE_ROWS], rw[GAE_ROWS];
    Aff m{1.0, 0.0};
#pragma unroll
    for (int i = GAE_ROWS - 1; i >= 0; --i) {
        const int64_t t = t0 + i;
        row[i] = Aff{1.0, 0.0};
        vs[i] = 0.f;
        rw[i] = 0.f;
        if (t < g.n) {
            row[i] = gae_row(g, t, vs[i], rw[i]);
            m = aff_comp(row[i], m);
        }
    }
    Aff total;
    const Aff behind = aff_suffix_256(m, sh, total);
    double y = behind.b + behind.a * carry;     // the advantage at the row behind this thread's last
#pragma unroll
    for (int i = GAE_ROWS - 1; i >= 0; --i) {
        const int64_t t = t0 + i;
        if (t < g.n) {
            y = row[i].b + row[i].a * y;
            const double rtg = y + (double)vs[i];               // buffer_utils.py:35-36
            g.adv[t] = (float)y;
            g.rtg[t] = (float)rtg;
            g.rtg_sp[t] = (float)((rtg - (double)rw[i]) / g.gamma);
        }
    }
}

// ==================================================================== launchers
void launch_vc_gather(const VcGatherArgs& a, hipStream_t s) {
    const dim3 grid((a.nc * a.mb + VC_GATHER_ROWS - 1) / VC_GATHER_ROWS, 1, vc_seeds_z(a.nseeds));
    if (a.nseeds > 1) hipLaunchKernelGGL(k_vc_gather<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_vc_gather<false>, grid, dim3(256), 0, s, a);
}
void launch_vc_head(const VcHeadArgs& a, hipStream_t s) {
    const dim3 grid((a.rows + 255) / 256, 1, vc_seeds_z(a.nseeds));
    if (a.nseeds > 1) hipLaunchKernelGGL(k_vc_head<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_vc_head<false>, grid, dim3(256), 0, s, a);
}
void launch_vc_final(const VcFinalArgs& a, hipStream_t s) {
    if (a.nseeds > 1) hipLaunchKernelGGL(k_vc_final<true>, dim3(1, 1, vc_seeds_z(a.nseeds)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_vc_final<false>, dim3(1), dim3(256), 0, s, a);
}
void launch_vc_adam(const VcAdamArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.n + 255) / 256), 1, vc_seeds_z(a.nseeds));
    if (a.nseeds > 1) hipLaunchKernelGGL(k_vc_adam<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_vc_adam<false>, grid, dim3(256), 0, s, a);
}
void launch_vc_rows(const VcRowsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_vc_rows, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
}
void launch_vc_reduce(const VcReduceArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_vc_reduce, dim3(1), dim3(VC_THREADS), 0, s, a);
}
void launch_gae(const GaeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_gae_tiles, dim3(a.tiles), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_gae_apply, dim3(a.tiles), dim3(256), 0, s, a);
}
void launch_vc_set(VcPar* dst, const VcPar& v, VcCtl* ctl, int32_t critic, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_vc_set, dim3(1), dim3(64), 0, s, dst, v, ctl, critic, n);
}

}  // namespace sacx
