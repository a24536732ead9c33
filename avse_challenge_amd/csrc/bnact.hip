// Fused BatchNorm -> [+ residual] -> activation (none / ReLU / PReLU) for gfx950: forward (training: batch
// statistics and the running-stat update; eval: running statistics) and backward.
//
// Replaces the MIOpen BatchNorm + separate PReLU / ReLU / residual-add passes of the avse1 lip stream
// (/root/reference/baseline/avse1/model.py:29-34 frontend3D BatchNorm3d -> PReLU; utils/resnet.py:40-67
// BasicBlock bn1 -> PReLU, bn2 + shortcut -> PReLU, downsample BatchNorm2d) and of the avse1 audio net
// (model.py:181-267 BatchNorm2d -> ReLU, channels-last).  In the round-2 avse1 step profile MIOpen's
// BatchNorm kernels and the PReLU passes took ~77 ms of kernel time per step (profiles/r02_avse1_*).
//
// One layout covers both memory formats: the activation is an (N, C, S) row-major view -- NCHW / NCDHW
// (S = H*W or T*H*W) and channels-last NHWC (N = batch*H*W, S = 1).  Every kernel maps a thread to a
// fixed column j of the (N, C*S) matrix (channel j / S) and walks rows, so all loads are coalesced
// row segments whatever S is (3x3 ResNet maps or 1-wide NHWC rows), and per-channel sums are per-column
// register partials, summed over the workgroup's row offsets in LDS, written as one (C*S)-wide row per
// row block and reduced per channel by a one-workgroup-per-channel kernel in fp64 (deterministic, no
// atomics).  The forward statistics are shifted by each channel's first element (x[0, c, 0]) so that
// E[x^2] - E[x]^2 does not cancel for large-mean inputs (raw 0..255 lip pixels through Conv3d).
//
// HBM traffic per element: forward 4 B (statistics) + 8 B (apply, +4 with a residual); backward 8 B
// (partials) + 12 B (apply); with a residual 12 + 4 (dres written) and 12.  Where dy comes from a split-fp16
// input-gradient convolution whose epilogue wrote the per-tile sums (bnact_cols.h, avse_bnact_bwd_rows) the backward's
// partials pass is not run: 12 B (apply) + 4 B (x, read in the producer's epilogue).  The lip front-ends' chain
// BatchNorm3d -> act -> MaxPool3d -> channels-last frames has kernels of its own (namespace pool below).
#include <algorithm>

#include "bnact_cols.h"
#include "common.h"
#include "split16.h"

namespace avse {
namespace bnact {

constexpr int THREADS = 256;

struct Geo {
    int64_t N, CS, S;
    int C, TW, RPI, tiles, nrb;
};

template <int V> struct vld;
template <> struct vld<1> {
    __device__ static inline void ld(const float* p, float* v) { v[0] = *p; }
    __device__ static inline void st(float* p, const float* v) { *p = v[0]; }
};
template <> struct vld<4> {
    __device__ static inline void ld(const float* p, float* v) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    __device__ static inline void st(float* p, const float* v) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};

// Sum NQ per-thread column partials over the workgroup's RPI row offsets (quantity MAXQ, if in range: their max);
// row offset 0 writes ws[(blockIdx.y * NQ + q) * CS + j].
template <int V, int NQ, int MAXQ = -1>
__device__ inline void block_partials(const Geo& g, float (&p)[NQ][V], bool valid, int64_t j0, float* ws) {
    __shared__ float part[NQ][THREADS * V];
    const int tx = threadIdx.x % g.TW, ty = threadIdx.x / g.TW;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int k = 0; k < V; ++k) part[q][threadIdx.x * V + k] = p[q][k];
    __syncthreads();
    if (ty == 0 && valid) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float s[V];
#pragma unroll
            for (int k = 0; k < V; ++k) s[k] = p[q][k];
            for (int t = 1; t < g.RPI; ++t)
#pragma unroll
                for (int k = 0; k < V; ++k)
                    s[k] = q == MAXQ ? fmaxf(s[k], part[q][(t * g.TW + tx) * V + k]) : s[k] + part[q][(t * g.TW + tx) * V + k];
            vld<V>::st(ws + ((int64_t)blockIdx.y * NQ + q) * g.CS + j0, s);
        }
    }
}

// max |out| of the workgroup -> one atomicMax on the float bits (split16.h) into omax: the producer-side max of the
// split operands (the convolution that consumes the output skips its absmax pass)
__device__ inline void block_max_out(float m, uint32_t* omax) {
    __shared__ uint32_t red[THREADS / 64];
    block_max_publish<THREADS / 64>(m, red, omax);
}

// ---- split output ("Q": the operand layout of dconv.hip / sconv.hip, round 5)
// With QOUT the apply passes write their channels-last output (S = 1, C % 64 == 0) directly as the fp16 hi / lo split the
// next convolution reads -- per pixel C / 16 chunks of 64 B = [hi of 16 channels][lo of 16 channels], the bytes of the
// fp32 tensor -- instead of fp32 values that a separate split pass (read 4 B + write 4 B per element) would convert.
// The split scale has to be known before the pass, so it comes from an upper bound of max |out| assembled from the
// per-channel statistics (a bound is enough: any power-of-two scale with no fp16 overflow keeps the 22-bit split; see
// stats_combine / bwd_combine), published as float bits where the exact max would be (y_max / dx_max).
// 4 channels c .. c + 3 (c % 4 == 0) of pixel r: hi at 64 (c / 16) + 2 (c % 16), lo 32 B further
__device__ inline void q_store4(uint16_t* q, int64_t r, int64_t C, int64_t c, const float* v, float sc) {
    uint32_t hi[2], lo[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) hi[k] = split_pair(v[2 * k], v[2 * k + 1], sc, lo[k]);
    uint16_t* base = q + r * 2 * C + 32 * (c >> 4) + (c & 15);
    *reinterpret_cast<uint2*>(base) = make_uint2(hi[0], hi[1]);
    *reinterpret_cast<uint2*>(base + 16) = make_uint2(lo[0], lo[1]);
}
// the bound's float bits, rounded up by 2^-10 (the apply pass's own fp32 rounding stays below it)
__device__ inline void q_bound_out(double bnd, uint32_t* omax) {
    const float f = (float)(bnd * (1.0 + 1.0 / 1024.0));
    if (f > 0.f) atomicMax(omax, __float_as_uint(f));
}

// ---- forward: statistics partials (shifted sums; MAXD: also max |x - shift| per column, for the split bound),
// finalize, apply
template <int V, bool MAXD>
__global__ __launch_bounds__(THREADS) void stats_kernel(Geo g, const float* __restrict__ x, float* __restrict__ ws) {
    constexpr int NQ = MAXD ? 3 : 2;
    const int tx = threadIdx.x % g.TW, ty = threadIdx.x / g.TW;
    const int64_t j0 = ((int64_t)blockIdx.x * g.TW + tx) * V;
    const bool valid = j0 < g.CS;
    float p[NQ][V], K[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) p[q][k] = 0.f;
        K[k] = valid ? x[((j0 + k) / g.S) * g.S] : 0.f;
    }
    if (valid) {
        for (int64_t r = (int64_t)blockIdx.y * g.RPI + ty; r < g.N; r += (int64_t)gridDim.y * g.RPI) {
            float v[V];
            vld<V>::ld(x + r * g.CS + j0, v);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float d = v[k] - K[k];
                p[0][k] += d;
                p[1][k] = fmaf(d, d, p[1][k]);
                if constexpr (MAXD) p[NQ - 1][k] = fmaxf(p[NQ - 1][k], fabsf(d));
            }
        }
    }
    block_partials<V, NQ, MAXD ? 2 : -1>(g, p, valid, j0, ws);
}

__device__ inline double block_sum_d(double v, double* red) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;
}

// Per-channel reduction of the column partials in two launches: chan_partial_kernel splits channel c's
// nrb * S partial entries over G workgroups (grid (C, G), fp64 sums, one value per workgroup and quantity),
// then a one-thread-per-channel combine.  (One workgroup per channel left most CUs idle: 64-512 workgroups
// looping over up to 172800 entries each took ~150 us per call at the avse1 shapes.)
constexpr int MAXG = 64;
inline int chan_groups(const Geo& g) {
    const int64_t cnt = (int64_t)g.nrb * g.S;
    return (int)std::max<int64_t>(1, std::min<int64_t>(MAXG, (cnt + 2047) / 2048));
}

__device__ inline double block_max_d(double v, double* red) {
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s = fmax(s, red[w]);
    return s;
}

// quantity MAXQ (if in range) is a column max, reduced by max; reset: the split bound's word, zeroed in stream order
// before the combine kernel's atomicMax
template <int NQ, int MAXQ = -1>
__global__ __launch_bounds__(THREADS) void chan_partial_kernel(Geo g, const float* __restrict__ ws,
                                                               double* __restrict__ fin, uint32_t* __restrict__ reset) {
    __shared__ double red[THREADS / 64];
    const int c = blockIdx.x, G = gridDim.y, gi = blockIdx.y;
    if (reset && c == 0 && gi == 0 && threadIdx.x == 0) *reset = 0u;
    const int S = (int)g.S, cnt = g.nrb * S;              // < 2^23: nrb * S <= 4096 * 1024 (make_geo)
    const int per = (cnt + G - 1) / G, i0 = gi * per, i1 = min(cnt, i0 + per);
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += THREADS) {
        const int y = i / S, sidx = i - y * S;
        const int64_t col = (int64_t)c * g.S + sidx;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const double v = ws[((int64_t)y * NQ + q) * g.CS + col];
            acc[q] = q == MAXQ ? fmax(acc[q], v) : acc[q] + v;
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const double v = q == MAXQ ? block_max_d(acc[q], red) : block_sum_d(acc[q], red);
        if (threadIdx.x == 0) fin[((int64_t)c * G + gi) * NQ + q] = v;
    }
}

// fin: sum (x - shift), sum (x - shift)^2, max |x - shift| per channel.  stats[4 c + 3] = a bound of max |x - mean| (the
// backward's split bound needs it); qb (split output): the channel's bound of |act(BN(x))| goes to omax (zeroed by
// chan_partial_kernel)
__global__ void stats_combine(Geo g, const float* __restrict__ x, const double* __restrict__ fin, int G, float eps,
                              float momentum, float* __restrict__ running_mean, float* __restrict__ running_var,
                              float* __restrict__ stats, uint32_t* __restrict__ omax, int qb,
                              const float* __restrict__ gamma, const float* __restrict__ beta,
                              const float* __restrict__ alpha, int alpha_n, int act) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (!qb && c == 0 && omax) *omax = 0u;               // the apply pass's max, reset in stream order before it
    if (c >= g.C) return;
    double s1 = 0.0, s2 = 0.0, dmax = 0.0;
    for (int gi = 0; gi < G; ++gi) {
        s1 += fin[((int64_t)c * G + gi) * 3];
        s2 += fin[((int64_t)c * G + gi) * 3 + 1];
        dmax = fmax(dmax, fin[((int64_t)c * G + gi) * 3 + 2]);
    }
    const double n = (double)g.N * (double)g.S;
    const double m1 = s1 / n;
    double var = s2 / n - m1 * m1;
    if (var < 0.0) var = 0.0;
    const double mean = (double)x[(int64_t)c * g.S] + m1;
    const float hi = (float)mean;
    stats[4 * c] = hi;
    stats[4 * c + 1] = (float)(mean - (double)hi);
    const double rstd = 1.0 / sqrt(var + (double)eps);
    stats[4 * c + 2] = (float)rstd;
    // |x - mean| <= max |x - shift| + |shift - mean|; |z| <= |gamma rstd| that + |beta|; ReLU / PReLU scale by <= max(1, |slope|)
    const double dev = dmax + fabs(m1);
    stats[4 * c + 3] = (float)(dev * (1.0 + 1.0 / 1024.0));
    if (qb) {
        const double ga = gamma ? fabs((double)gamma[c]) : 1.0;
        double bz = ga * rstd * dev + (beta ? fabs((double)beta[c]) : 0.0);
        if (act == ACT_PRELU) bz *= fmax(1.0, fabs((double)alpha[alpha_n > 1 ? c : 0]));
        q_bound_out(bz, omax);
    }
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mean);
    if (running_var) running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * var * n / (n - 1.0));
}

__global__ void eval_stats_kernel(int C, const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                  float* __restrict__ stats, uint32_t* __restrict__ omax) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && omax) *omax = 0u;
    if (c < C) {
        stats[4 * c] = rm[c];
        stats[4 * c + 1] = 0.f;
        stats[4 * c + 2] = (float)(1.0 / sqrt((double)rv[c] + (double)eps));
        stats[4 * c + 3] = 0.f;
    }
}

template <int V, int ACT, bool RES, bool QOUT = false>
__global__ __launch_bounds__(THREADS) void apply_kernel(Geo g, const float* __restrict__ x, const float* __restrict__ res,
                                                        const float* __restrict__ stats, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ alpha,
                                                        int alpha_n, float* __restrict__ y, uint32_t* __restrict__ ymax) {
    const int tx = threadIdx.x % g.TW, ty = threadIdx.x / g.TW;
    const int64_t j0 = ((int64_t)blockIdx.x * g.TW + tx) * V;
    float m = 0.f;
    if constexpr (QOUT) {                                 // S = 1, V = 4, no residual (host-checked)
        const float sc = split_scale(*ymax);
        if (j0 < g.CS) {
            ColConst<V, ACT> cc;
            cc.load(g, j0, stats, gamma, beta, alpha, alpha_n);
            for (int64_t r = (int64_t)blockIdx.y * g.RPI + ty; r < g.N; r += (int64_t)gridDim.y * g.RPI) {
                float v[V];
                vld<V>::ld(x + r * g.CS + j0, v);
#pragma unroll
                for (int k = 0; k < V; ++k) v[k] = act_fwd<ACT>(cc.preact(v[k], k), cc.al[k]);
                q_store4(reinterpret_cast<uint16_t*>(y), r, g.CS, j0, v, sc);
            }
        }
        return;
    }
    if (j0 < g.CS) {
        ColConst<V, ACT> cc;
        cc.load(g, j0, stats, gamma, beta, alpha, alpha_n);
        for (int64_t r = (int64_t)blockIdx.y * g.RPI + ty; r < g.N; r += (int64_t)gridDim.y * g.RPI) {
            const int64_t o = r * g.CS + j0;
            float v[V], rv[V];
            vld<V>::ld(x + o, v);
            if (RES) vld<V>::ld(res + o, rv);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float z = cc.preact(v[k], k);
                if (RES) z += rv[k];
                v[k] = act_fwd<ACT>(z, cc.al[k]);
                m = fmaxf(m, fabsf(v[k]));
            }
            vld<V>::st(y + o, v);
        }
    }
    if (ymax) block_max_out(m, ymax);                    // workgroup-uniform condition
}

// ---- backward: partials of sum dz, sum dz*xhat, PReLU slope; finalize; apply
template <int V, int ACT, bool RES, bool MAXDZ = false>
__global__ __launch_bounds__(THREADS) void bwd_partial_kernel(Geo g, const float* __restrict__ x,
                                                              const float* __restrict__ res, const float* __restrict__ dy,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ alpha, int alpha_n,
                                                              float* __restrict__ ws, float* __restrict__ dres) {
    constexpr int NQ = MAXDZ ? 4 : 3;
    const int tx = threadIdx.x % g.TW, ty = threadIdx.x / g.TW;
    const int64_t j0 = ((int64_t)blockIdx.x * g.TW + tx) * V;
    const bool valid = j0 < g.CS;
    float p[NQ][V];
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
        for (int q = 0; q < NQ; ++q) p[q][k] = 0.f;
    if (valid) {
        ColConst<V, ACT> cc;
        cc.load(g, j0, stats, gamma, beta, alpha, alpha_n);
        for (int64_t r = (int64_t)blockIdx.y * g.RPI + ty; r < g.N; r += (int64_t)gridDim.y * g.RPI) {
            const int64_t o = r * g.CS + j0;
            float v[V], gv[V], rv[V], dz[V];
            vld<V>::ld(x + o, v);
            vld<V>::ld(dy + o, gv);
            if (RES) vld<V>::ld(res + o, rv);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float z = cc.preact(v[k], k);
                if (RES) z += rv[k];
                dz[k] = act_bwd<ACT>(z, gv[k], cc.al[k]);
                const float xh = cc.xhat(v[k], k);
                p[0][k] += dz[k];
                p[1][k] = fmaf(dz[k], xh, p[1][k]);
                if (ACT == ACT_PRELU && !(z > 0.f)) p[2][k] = fmaf(gv[k], z, p[2][k]);
                if constexpr (MAXDZ) p[3][k] = fmaxf(p[3][k], fabsf(dz[k]));
            }
            if (RES) vld<V>::st(dres + o, dz);
        }
    }
    block_partials<V, NQ, MAXDZ ? 3 : -1>(g, p, valid, j0, ws);
}

// qb (split output): fin carries a fourth quantity, max |dz|; the channel's bound of |dx| goes to omax (zeroed by
// chan_partial_kernel): |dx| <= |gamma rstd| (max |dz| + |k1| + max |xhat| |k2|), max |xhat| from the forward's
// stats[4 c + 3] (training; eval: |gamma rstd| max |dz|)
__global__ void bwd_combine(Geo g, const double* __restrict__ fin, int G, int training, float* __restrict__ dgamma,
                            float* __restrict__ dbeta, float* __restrict__ dalpha_c, float* __restrict__ kbuf,
                            uint32_t* __restrict__ omax, int qb, const float* __restrict__ stats,
                            const float* __restrict__ gamma) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (!qb && c == 0 && omax) *omax = 0u;               // the apply pass's max, reset in stream order before it
    if (c >= g.C) return;
    const int NQ = qb ? 4 : 3;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, dzmax = 0.0;
    for (int gi = 0; gi < G; ++gi) {
        s0 += fin[((int64_t)c * G + gi) * NQ];
        s1 += fin[((int64_t)c * G + gi) * NQ + 1];
        s2 += fin[((int64_t)c * G + gi) * NQ + 2];
        if (qb) dzmax = fmax(dzmax, fin[((int64_t)c * G + gi) * NQ + 3]);
    }
    const double n = (double)g.N * (double)g.S;
    if (dbeta) dbeta[c] = (float)s0;
    if (dgamma) dgamma[c] = (float)s1;
    if (dalpha_c) dalpha_c[c] = (float)s2;
    kbuf[2 * c] = training ? (float)(s0 / n) : 0.f;
    kbuf[2 * c + 1] = training ? (float)(s1 / n) : 0.f;
    if (qb) {
        const double rstd = (double)stats[4 * c + 2];
        const double ga = (gamma ? fabs((double)gamma[c]) : 1.0) * rstd;
        const double b = training ? dzmax + fabs(s0 / n) + (double)stats[4 * c + 3] * rstd * fabs(s1 / n) : dzmax;
        q_bound_out(ga * b, omax);
    }
}

template <int V, int ACT, bool RES, bool QOUT = false>
__device__ inline void bwd_apply_cols(const Geo& g, int64_t j0, int ty, const float* __restrict__ x,
                                      const float* __restrict__ dy, const float* __restrict__ dres,
                                      const float* __restrict__ stats, const float* __restrict__ gamma,
                                      const float* __restrict__ beta, const float* __restrict__ alpha, int alpha_n,
                                      const float* __restrict__ kbuf, float* __restrict__ dx, float& m, float qsc = 1.f) {
    ColConst<V, ACT> cc;
    cc.load(g, j0, stats, gamma, beta, alpha, alpha_n);
    float k1[V], k2[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int c = (int)((j0 + k) / g.S);
        k1[k] = kbuf[2 * c];
        k2[k] = kbuf[2 * c + 1];
    }
    for (int64_t r = (int64_t)blockIdx.y * g.RPI + ty; r < g.N; r += (int64_t)gridDim.y * g.RPI) {
        const int64_t o = r * g.CS + j0;
        float v[V], dz[V];
        vld<V>::ld(x + o, v);
        if (RES) {
            vld<V>::ld(dres + o, dz);                  // dz of the pre-activation, written by the partial pass
        } else {
            float gv[V];
            vld<V>::ld(dy + o, gv);
#pragma unroll
            for (int k = 0; k < V; ++k) dz[k] = act_bwd<ACT>(cc.preact(v[k], k), gv[k], cc.al[k]);
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float xh = cc.xhat(v[k], k);
            v[k] = cc.a[k] * (dz[k] - k1[k] - xh * k2[k]);
            if constexpr (!QOUT) m = fmaxf(m, fabsf(v[k]));
        }
        if constexpr (QOUT) q_store4(reinterpret_cast<uint16_t*>(dx), r, g.CS, j0, v, qsc);
        else vld<V>::st(dx + o, v);
    }
}

template <int V, int ACT, bool RES, bool QOUT = false>
__global__ __launch_bounds__(THREADS) void bwd_apply_kernel(Geo g, const float* __restrict__ x,
                                                            const float* __restrict__ dy, const float* __restrict__ dres,
                                                            const float* __restrict__ stats,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ alpha, int alpha_n,
                                                            const float* __restrict__ kbuf, float* __restrict__ dx,
                                                            uint32_t* __restrict__ dxmax) {
    const int tx = threadIdx.x % g.TW, ty = threadIdx.x / g.TW;
    const int64_t j0 = ((int64_t)blockIdx.x * g.TW + tx) * V;
    float m = 0.f;
    if constexpr (QOUT) {                                 // S = 1, V = 4 (host-checked)
        const float sc = split_scale(*dxmax);
        if (j0 < g.CS)
            bwd_apply_cols<V, ACT, RES, true>(g, j0, ty, x, dy, dres, stats, gamma, beta, alpha, alpha_n, kbuf, dx, m, sc);
        return;
    }
    if (j0 < g.CS) bwd_apply_cols<V, ACT, RES>(g, j0, ty, x, dy, dres, stats, gamma, beta, alpha, alpha_n, kbuf, dx, m);
    if (dxmax) block_max_out(m, dxmax);                  // workgroup-uniform condition
}

// ---- the lip front-end chain BatchNorm3d -> ReLU / PReLU -> MaxPool3d((1, 3, 3), (1, 2, 2), (0, 1, 1)) -> frames as
// channels-last (avse1 VisualFeatNet.forward, avse4 VisualFrontend.forward), in one pass forward and two backward
// The unfused chain writes the activated (B, C, T, H, W) tensor only for the pool to read it back, the pooled planes
// only for the frame transpose to read them back, and the un-pooled gradient (three quarters of it zeros) only for the
// two BatchNorm backward passes to read it.  Here a workgroup owns (b, t, 64 channels, a band of RB pooled rows):
//   forward   reads x along each channel plane (the float4 + scalar pattern of maxpool.hip's fwd_k3s2p1_w4_kernel, the
//             rows between neighbouring windows and bands re-read from cache), forms z = act(ColConst::preact(x)) per
//             loaded element, pools it with that kernel's scan order and comparison, writes the argmax byte in
//             maxpool.hip's plane layout and transposes only the pooled tile through LDS: whole 256-B pixel rows of
//             the (B T, Ho, Wo, C) frames.
//   backward  stages the band's RB + 1 rows of the channels-last pooled gradient in LDS, forms each 2 x 4 input
//             block's un-pooled gradient from its 6 candidate windows in maxpool.hip's (ho, wo) order (the value the
//             unfused chain wrote to memory) and feeds it to the BatchNorm backward: the sums pass writes one row of
//             [3][C] per workgroup (chan_partial_kernel / bwd_combine finish them as for avse_bnact_bwd_rows:
//             deterministic, no atomics), the apply pass writes dx and publishes max |dx|.
// A thread group of GL = 8 lanes walks one channel's band, so the channel constants are per-thread registers and the
// 8 lanes read 128 contiguous bytes of a plane row.
namespace pool {

constexpr int CT = 64, RB = 4, LP = CT + 1, GL = 8, MAXW = 96;

struct PGeo {
    int B, C, T, H, W, Ho, Wo, bands, ctiles;
    uint32_t mq;                                          // j / (W / 4) = (j * mq) >> 16 for j < 128 (W / 4 <= 24)
};

struct Blk {
    int band, ct, b, t, r0, nr;
    int64_t bt;
    __device__ inline Blk(const PGeo& p) {
        band = (int)(blockIdx.x % p.bands);
        ct = (int)((blockIdx.x / p.bands) % p.ctiles);
        bt = blockIdx.x / (p.bands * p.ctiles);
        b = (int)(bt / p.T);
        t = (int)(bt - (int64_t)b * p.T);
        r0 = band * RB;
        nr = min(RB, p.Ho - r0);
    }
};

template <int ACT>
__global__ __launch_bounds__(THREADS) void fwd_kernel(PGeo p, const float* __restrict__ x,
                                                      const float* __restrict__ stats, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ alpha,
                                                      int alpha_n, float* __restrict__ y, uint8_t* __restrict__ idx) {
    extern __shared__ float tile[];                       // [nr * Wo pooled pixels][LP]
    const Blk k(p);
    const int Pb = p.W >> 2, items = k.nr * Pb;
    const int sub = threadIdx.x / GL, l8 = threadIdx.x % GL;
    for (int pass = 0; pass < CT * GL / THREADS; ++pass) {
        const int cl = pass * (THREADS / GL) + sub, c = k.ct * CT + cl;
        ColConst<1, ACT> cc;
        cc.load_channel(0, c, stats, gamma, beta, alpha, alpha_n);
        const int64_t pl = ((int64_t)k.b * p.C + c) * p.T + k.t;
        const float* xc = x + pl * p.H * p.W;
        uint8_t* ic = idx + pl * p.Ho * p.Wo;
        for (int j = l8; j < items; j += GL) {
            const int r = (int)(((uint32_t)j * p.mq) >> 16), wp = j - r * Pb, ho = k.r0 + r;
            const float* xp = xc + 4 * wp;
            float v[3][5];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int h = 2 * ho - 1 + kh;
                const bool ok = h >= 0 && h < p.H;
                const float4 q = ok ? *reinterpret_cast<const float4*>(xp + h * p.W) : make_float4(0.f, 0.f, 0.f, 0.f);
                v[kh][0] = (ok && wp > 0) ? xp[h * p.W - 1] : 0.f;
                v[kh][1] = q.x; v[kh][2] = q.y; v[kh][3] = q.z; v[kh][4] = q.w;
#pragma unroll
                for (int e = 0; e < 5; ++e) v[kh][e] = act_fwd<ACT>(cc.preact(v[kh][e], 0), cc.al[0]);
            }
            // the scan of maxpool.hip fwd_k3s2p1_w4_kernel: first maximum, strict '>', a NaN taken
            const int kh0 = ho == 0 ? 1 : 0;
            const int hmax = min(3, p.H - (2 * ho - 1));
            float best[2];
            int arg[2];
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const int kw0 = (wp == 0 && o == 0) ? 1 : 0;
                best[o] = -__builtin_inff();
                arg[o] = (kh0 << 4) | kw0;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    if (kh < kh0 || kh >= hmax) continue;
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        if (kw < kw0) continue;
                        const float e = v[kh][2 * o + kw];
                        if (e > best[o] || e != e) {
                            best[o] = e;
                            arg[o] = (kh << 4) | kw;
                        }
                    }
                }
            }
            tile[(r * p.Wo + 2 * wp) * LP + cl] = best[0];
            tile[(r * p.Wo + 2 * wp + 1) * LP + cl] = best[1];
            *reinterpret_cast<uint16_t*>(ic + ho * p.Wo + 2 * wp) = (uint16_t)(arg[0] | (arg[1] << 8));
        }
    }
    __syncthreads();
    float* yb = y + ((k.bt * p.Ho + k.r0) * p.Wo) * p.C + k.ct * CT;
    for (int q = threadIdx.x; q < k.nr * p.Wo * CT; q += THREADS) yb[(int64_t)(q / CT) * p.C + q % CT] = tile[(q / CT) * LP + q % CT];
}

template <int ACT, bool APPLY>
__global__ __launch_bounds__(THREADS) void bwd_kernel(PGeo p, const float* __restrict__ x, const float* __restrict__ g,
                                                      const uint8_t* __restrict__ idx, const float* __restrict__ stats,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ alpha, int alpha_n,
                                                      const float* __restrict__ kbuf, float* __restrict__ rows,
                                                      float* __restrict__ dx, uint32_t* __restrict__ dxmax) {
    extern __shared__ float tile[];                       // [ngr * Wo pooled pixels][LP]: pooled rows r0 .. r0 + ngr - 1
    const Blk k(p);
    const int ngr = min(RB + 1, p.Ho - k.r0);
    const float* gb = g + ((k.bt * p.Ho + k.r0) * p.Wo) * p.C + k.ct * CT;
    for (int q = threadIdx.x; q < ngr * p.Wo * CT; q += THREADS) tile[(q / CT) * LP + q % CT] = gb[(int64_t)(q / CT) * p.C + q % CT];
    __syncthreads();
    const int Nq = p.W >> 2, items = k.nr * Nq;
    const int sub = threadIdx.x / GL, l8 = threadIdx.x % GL;
    float mx = 0.f;
    for (int pass = 0; pass < CT * GL / THREADS; ++pass) {
        const int cl = pass * (THREADS / GL) + sub, c = k.ct * CT + cl;
        ColConst<1, ACT> cc;
        cc.load_channel(0, c, stats, gamma, beta, alpha, alpha_n);
        const float k1 = APPLY ? kbuf[2 * c] : 0.f, k2 = APPLY ? kbuf[2 * c + 1] : 0.f;
        const int64_t pl = ((int64_t)k.b * p.C + c) * p.T + k.t;
        const uint8_t* ic = idx + pl * p.Ho * p.Wo;
        float s[3] = {0.f, 0.f, 0.f};
        for (int j = l8; j < items; j += GL) {
            const int r = (int)(((uint32_t)j * p.mq) >> 16), nq = j - r * Nq, m = k.r0 + r;
            // input rows 2m, 2m + 1, columns 4nq .. 4nq + 3: windows ho = m, m + 1, wo = 2nq .. 2nq + 2; a window's
            // argmax lies at (2 dh - 1 + kh, 2 kk - 1 + kw) from (2m, 4nq)
            float gd[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int dh = 0; dh < 2; ++dh) {
                const int ho = m + dh;
                if (ho >= p.Ho) break;
                const uint8_t* ip = ic + ho * p.Wo + 2 * nq;
                const uint32_t a01 = *reinterpret_cast<const uint16_t*>(ip);
                const bool has2 = 2 * nq + 2 < p.Wo;
                const uint32_t a2 = has2 ? ip[2] : 0xffu;
                const float* tp = tile + ((r + dh) * p.Wo + 2 * nq) * LP + cl;
#pragma unroll
                for (int kk = 0; kk < 3; ++kk) {
                    if (kk == 2 && !has2) break;
                    const int a = kk == 0 ? (int)(a01 & 0xff) : (kk == 1 ? (int)(a01 >> 8) : (int)a2);
                    const float v = tp[kk * LP];
                    const int di = 2 * dh - 1 + (a >> 4), dj = 2 * kk - 1 + (a & 15);
#pragma unroll
                    for (int i = dh; i < 2; ++i)
#pragma unroll
                        for (int e = (kk == 0 ? 0 : 2 * kk - 1); e <= min(3, 2 * kk + 1); ++e)
                            if (di == i && dj == e) gd[i][e] += v;
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int64_t o = pl * p.H * p.W + (int64_t)(2 * m + i) * p.W + 4 * nq;
                float v[4];
                vld<4>::ld(x + o, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float z = cc.preact(v[e], 0);
                    const float dz = act_bwd<ACT>(z, gd[i][e], cc.al[0]);
                    const float xh = cc.xhat(v[e], 0);
                    if constexpr (APPLY) {
                        v[e] = cc.a[0] * (dz - k1 - xh * k2);
                        mx = fmaxf(mx, fabsf(v[e]));
                    } else {
                        s[0] += dz;
                        s[1] = fmaf(dz, xh, s[1]);
                        if (ACT == ACT_PRELU && !(z > 0.f)) s[2] = fmaf(gd[i][e], z, s[2]);
                    }
                }
                if constexpr (APPLY) vld<4>::st(dx + o, v);
            }
        }
        if constexpr (!APPLY) {
            const int64_t row = k.bt * p.bands + k.band;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                float v = s[q];
                for (int o = 1; o < GL; o <<= 1) v += __shfl_xor(v, o, 64);
                if (l8 == 0) rows[(row * 3 + q) * p.C + c] = v;
            }
        }
    }
    if constexpr (APPLY) {
        if (dxmax) block_max_out(mx, dxmax);            // workgroup-uniform condition
    }
}

}  // namespace pool

// ---- length-aware eval forward for zero-padded ragged batches (inference only): y = act(BN(x)) where the element's
// time index t lies in the sample's valid window toff <= t < toff + len[b], exact +0 elsewhere (a select: NaN or Inf in
// x's padding does not reach y or the max).  The valid elements go through apply_kernel's expressions, so they equal
// the dense eval forward bit for bit.  Where (b, t) comes from:
//   rows mode  row r of the (N, C S) matrix = ((b T + t) inner + i): channels-last (B, T, F, C) and (B, T, H, W, C)
//              with S = 1, the time-major TCN rows (inner = 1) and frame-major (B T, C, H, W) (inner = 1, S = H W);
//   cols mode  N = B and column j = (c, t, i) with S = T inner: contiguous (B, C, T, F) / (B, C, T, H, W).
// toff > 0 is the TCN's: BatchNorm runs on the conv's unchomped (T + pad) output, the valid window is the part the
// symmetric chomp keeps.  MODE 0 writes fp32 y and publishes max |y|; MODE 1 only publishes that max (over valid
// elements: the split scale of MODE 2 must be known before its pass); MODE 2 writes the split layout of apply_kernel's
// QOUT under *ymax.
struct LenGeo {
    int T, inner, toff, rows;
};

__device__ inline bool len_ok(const LenGeo& lg, const int32_t* __restrict__ lengths, int b, int t) {
    const int n = min(max(lengths[b], 0), lg.T - lg.toff);
    return t >= lg.toff && t - lg.toff < n;
}

template <int V, int ACT, int MODE>
__global__ __launch_bounds__(THREADS) void apply_len_kernel(Geo g, LenGeo lg, const float* __restrict__ x,
                                                            const int32_t* __restrict__ lengths,
                                                            const float* __restrict__ stats,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ alpha, int alpha_n,
                                                            float* __restrict__ y, uint32_t* __restrict__ ymax) {
    const int tx = threadIdx.x % g.TW, ty = threadIdx.x / g.TW;
    const int64_t j0 = ((int64_t)blockIdx.x * g.TW + tx) * V;
    float m = 0.f;
    float sc = 1.f;
    if constexpr (MODE == 2) sc = split_scale(*ymax);
    if (j0 < g.CS) {
        ColConst<V, ACT> cc;
        cc.load(g, j0, stats, gamma, beta, alpha, alpha_n);
        int tc[V];                                           // cols mode: the columns' time indices
#pragma unroll
        for (int k = 0; k < V; ++k) tc[k] = lg.rows ? 0 : (int)(((j0 + k) % g.S) / lg.inner);
        for (int64_t r = (int64_t)blockIdx.y * g.RPI + ty; r < g.N; r += (int64_t)gridDim.y * g.RPI) {
            const int64_t o = r * g.CS + j0;
            bool ok[V];
            bool any = false;
            if (lg.rows) {
                const int64_t q = r / lg.inner;
                const int b = (int)(q / lg.T), t = (int)(q - (int64_t)b * lg.T);
                any = len_ok(lg, lengths, b, t);
#pragma unroll
                for (int k = 0; k < V; ++k) ok[k] = any;
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    ok[k] = len_ok(lg, lengths, (int)r, tc[k]);
                    any |= ok[k];
                }
            }
            float v[V];
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = 0.f;
            if (any) {                                       // a wholly padded vector is not loaded
                vld<V>::ld(x + o, v);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float z = act_fwd<ACT>(cc.preact(v[k], k), cc.al[k]);
                    v[k] = ok[k] ? z : 0.f;
                    m = fmaxf(m, fabsf(v[k]));
                }
            }
            if constexpr (MODE == 0) vld<V>::st(y + o, v);
            if constexpr (MODE == 2 && V == 4) q_store4(reinterpret_cast<uint16_t*>(y), r, g.CS, j0, v, sc);
        }
    }
    if constexpr (MODE != 2) {
        if (ymax) block_max_out(m, ymax);                    // workgroup-uniform condition
    }
}

// ---- host side
inline int pow2ceil(int64_t v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

inline Geo make_geo(int64_t N, int64_t C, int64_t S, int V) {
    Geo g;
    g.N = N; g.S = S; g.C = (int)C; g.CS = C * S;
    const int64_t cw = (g.CS + V - 1) / V;
    g.TW = cw >= THREADS ? THREADS : pow2ceil(cw);
    g.RPI = THREADS / g.TW;
    g.tiles = (int)((cw + g.TW - 1) / g.TW);
    const int64_t want = (N + (int64_t)g.RPI * 8 - 1) / ((int64_t)g.RPI * 8);      // >= 8 rows per thread
    const int64_t cap = std::max<int64_t>(1, 4096 / g.tiles);
    g.nrb = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, cap), 65535));
    return g;
}

inline bool shape_ok(int64_t N, int64_t C, int64_t S) {
    return N > 0 && C > 0 && S > 0 && N * C * S < (1LL << 40) && C * S < (1LL << 31) && C < (1 << 20) &&
           (C * S + 3) / 4 <= (int64_t)THREADS * 0x7FFFFFFF;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// fp64 per-channel partials after the column partials and kbuf (the largest nrb of either vector width)
inline double* fin_ptr(float* workspace, const Geo& g) {
    const Geo g1 = make_geo(g.N, g.C, g.S, 1), g4 = make_geo(g.N, g.C, g.S, 4);
    const int64_t nrb = std::max(g1.nrb, g4.nrb);
    const uintptr_t p = (uintptr_t)(workspace + 4 * nrb * g.CS + 2 * (int64_t)g.C);
    return reinterpret_cast<double*>((p + 15) & ~(uintptr_t)15);
}

template <template <int, int, bool> class K>
struct dispatch {
    template <typename... A>
    static void run(int V, int act, bool res, dim3 grid, hipStream_t st, A... a) {
#define AVSE_BNACT_CASE(VV, AA, RR) \
    if (V == VV && act == AA && res == RR) { hipLaunchKernelGGL((K<VV, AA, RR>::fn), grid, dim3(THREADS), 0, st, a...); return; }
        AVSE_BNACT_CASE(4, ACT_NONE, false) AVSE_BNACT_CASE(4, ACT_RELU, false) AVSE_BNACT_CASE(4, ACT_PRELU, false)
        AVSE_BNACT_CASE(4, ACT_NONE, true) AVSE_BNACT_CASE(4, ACT_RELU, true) AVSE_BNACT_CASE(4, ACT_PRELU, true)
        AVSE_BNACT_CASE(1, ACT_NONE, false) AVSE_BNACT_CASE(1, ACT_RELU, false) AVSE_BNACT_CASE(1, ACT_PRELU, false)
        AVSE_BNACT_CASE(1, ACT_NONE, true) AVSE_BNACT_CASE(1, ACT_RELU, true) AVSE_BNACT_CASE(1, ACT_PRELU, true)
#undef AVSE_BNACT_CASE
    }
};
template <int V, int A, bool R> struct ApplyK { static constexpr auto fn = apply_kernel<V, A, R>; };
template <int V, int A, bool R> struct ApplyQK { static constexpr auto fn = apply_kernel<V, A, R, true>; };
template <int V, int A, bool R> struct BwdPartQK { static constexpr auto fn = bwd_partial_kernel<V, A, R, true>; };
template <int V, int A, bool R> struct BwdApplyQK { static constexpr auto fn = bwd_apply_kernel<V, A, R, true>; };
// the split-output kernels: V = 4, no residual
template <template <int, int, bool> class K>
struct dispatch_q {
    template <typename... A>
    static void run(int act, dim3 grid, hipStream_t st, A... a) {
        if (act == ACT_NONE) hipLaunchKernelGGL((K<4, ACT_NONE, false>::fn), grid, dim3(THREADS), 0, st, a...);
        else if (act == ACT_RELU) hipLaunchKernelGGL((K<4, ACT_RELU, false>::fn), grid, dim3(THREADS), 0, st, a...);
        else hipLaunchKernelGGL((K<4, ACT_PRELU, false>::fn), grid, dim3(THREADS), 0, st, a...);
    }
};
template <int V, int A, bool R> struct BwdPartK { static constexpr auto fn = bwd_partial_kernel<V, A, R>; };
template <int V, int A, bool R> struct BwdApplyK { static constexpr auto fn = bwd_apply_kernel<V, A, R>; };

template <int V, int MODE>
inline void launch_apply_len(int act, dim3 grid, hipStream_t st, const Geo& g, const LenGeo& lg, const float* x,
                             const int32_t* lengths, const float* stats, const float* gamma, const float* beta,
                             const float* alpha, int alpha_n, float* y, uint32_t* y_max) {
    if (act == ACT_NONE)
        hipLaunchKernelGGL((apply_len_kernel<V, ACT_NONE, MODE>), grid, dim3(THREADS), 0, st, g, lg, x, lengths, stats,
                           gamma, beta, alpha, alpha_n, y, y_max);
    else if (act == ACT_RELU)
        hipLaunchKernelGGL((apply_len_kernel<V, ACT_RELU, MODE>), grid, dim3(THREADS), 0, st, g, lg, x, lengths, stats,
                           gamma, beta, alpha, alpha_n, y, y_max);
    else
        hipLaunchKernelGGL((apply_len_kernel<V, ACT_PRELU, MODE>), grid, dim3(THREADS), 0, st, g, lg, x, lengths, stats,
                           gamma, beta, alpha, alpha_n, y, y_max);
}

}  // namespace bnact
}  // namespace avse

using namespace avse::bnact;

extern "C" {

int64_t avse_bnact_workspace_bytes(int64_t N, int64_t C, int64_t S) {
    if (!shape_ok(N, C, S)) return 0;
    const Geo g = make_geo(N, C, S, 1);                 // V = 1 has the most row blocks
    const Geo g4 = make_geo(N, C, S, 4);
    const int64_t nrb = std::max(g.nrb, g4.nrb);
    // column partials (up to 4 rows of C*S per row block), kbuf (2 C floats), then 8-aligned fp64 per-channel partials
    return 4 * (4 * nrb * C * S + 2 * C) + 16 + 8 * (int64_t)C * MAXG * 4;
}

// the forward's statistics: training: stats_kernel -> chan_partial_kernel -> stats_combine (batch statistics, the running
// update); eval: the running statistics.  y_max (may be null) is reset in stream order (qout: takes the split bound)
static int launch_stats(const Geo& g, int V, const float* x, const float* gamma, const float* beta, int32_t act,
                        const float* alpha, int32_t alpha_n, int32_t training, float eps, float momentum,
                        float* running_mean, float* running_var, float* stats, float* workspace, uint32_t* y_max,
                        bool qout, hipStream_t st) {
    const dim3 grid(g.tiles, g.nrb);
    const int64_t C = g.C;
    if (training) {
        if (V == 4) hipLaunchKernelGGL((stats_kernel<4, true>), grid, dim3(THREADS), 0, st, g, x, workspace);
        else hipLaunchKernelGGL((stats_kernel<1, true>), grid, dim3(THREADS), 0, st, g, x, workspace);
        AVSE_CHECK_LAUNCH();
        const int G = chan_groups(g);
        double* fin = fin_ptr(workspace, g);
        hipLaunchKernelGGL((chan_partial_kernel<3, 2>), dim3((unsigned)C, G), dim3(THREADS), 0, st, g,
                           (const float*)workspace, fin, qout ? y_max : (uint32_t*)nullptr);
        AVSE_CHECK_LAUNCH();
        hipLaunchKernelGGL(stats_combine, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, g, x, (const double*)fin,
                           G, eps, momentum, running_mean, running_var, stats, y_max, (int)qout, gamma, beta, alpha,
                           (int)alpha_n, (int)act);
    } else {
        hipLaunchKernelGGL(eval_stats_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, (int)C, running_mean,
                           running_var, eps, stats, y_max);
    }
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

static int bnact_fwd_impl(int64_t N, int64_t C, int64_t S, const float* x, const float* res, const float* gamma,
                          const float* beta, int32_t act, const float* alpha, int32_t alpha_n, int32_t training, float eps,
                          float momentum, float* running_mean, float* running_var, float* stats, float* y,
                          float* workspace, uint32_t* y_max, bool qout, hipStream_t st) {
    if (!x || !y || !stats || !workspace || (act == ACT_PRELU && !alpha)) return AVSE_EINVAL;
    if (!training && (!running_mean || !running_var)) return AVSE_EINVAL;
    if (!shape_ok(N, C, S) || act < ACT_NONE || act > ACT_PRELU) return AVSE_ESHAPE;
    if (act == ACT_PRELU && alpha_n != 1 && alpha_n != C) return AVSE_ESHAPE;
    if (training && N * S < 2) return AVSE_ESHAPE;       // as torch: more than one value per channel
    const int V = ((C * S) % 4 == 0 && al16(x) && al16(y) && (!res || al16(res)) && al16(workspace)) ? 4 : 1;
    if (qout && (!y_max || !training || res || S != 1 || C % 64 || V != 4)) return AVSE_ESHAPE;
    const Geo g = make_geo(N, C, S, V);
    const dim3 grid(g.tiles, g.nrb);
    const int rc = launch_stats(g, V, x, gamma, beta, act, alpha, alpha_n, training, eps, momentum, running_mean,
                                running_var, stats, workspace, y_max, qout, st);
    if (rc != AVSE_OK) return rc;
    if (qout)
        dispatch_q<ApplyQK>::run(act, grid, st, g, x, res, (const float*)stats, gamma, beta, alpha, (int)alpha_n, y, y_max);
    else
        dispatch<ApplyK>::run(V, act, res != nullptr, grid, st, g, x, res, (const float*)stats, gamma, beta, alpha,
                              (int)alpha_n, y, y_max);
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

int avse_bnact_fwd(int64_t N, int64_t C, int64_t S, const float* x, const float* res, const float* gamma,
                   const float* beta, int32_t act, const float* alpha, int32_t alpha_n, int32_t training, float eps,
                   float momentum, float* running_mean, float* running_var, float* stats, float* y, float* workspace,
                   uint32_t* y_max, avse_stream_t stream) {
    return bnact_fwd_impl(N, C, S, x, res, gamma, beta, act, alpha, alpha_n, training, eps, momentum, running_mean,
                          running_var, stats, y, workspace, y_max, false, (hipStream_t)stream);
}

int avse_bnact_fwd_q(int64_t N, int64_t C, int64_t S, const float* x, const float* gamma, const float* beta, int32_t act,
                     const float* alpha, int32_t alpha_n, float eps, float momentum, float* running_mean,
                     float* running_var, float* stats, void* yq, float* workspace, uint32_t* y_bound,
                     avse_stream_t stream) {
    return bnact_fwd_impl(N, C, S, x, nullptr, gamma, beta, act, alpha, alpha_n, 1, eps, momentum, running_mean,
                          running_var, stats, (float*)yq, workspace, y_bound, true, (hipStream_t)stream);
}

// the length-aware eval forward (apply_len_kernel): eval_stats_kernel (which resets *y_max), then for the split output
// the max pass and the split pass, else the one fp32 pass
static int bnact_fwd_len_impl(int64_t N, int64_t C, int64_t S, const float* x, const float* gamma, const float* beta,
                              int32_t act, const float* alpha, int32_t alpha_n, int32_t training, float eps,
                              const float* running_mean, const float* running_var, float* stats, float* y,
                              uint32_t* y_max, const int32_t* lengths, int64_t B, int64_t T, int64_t inner, int64_t t_off,
                              int32_t time_in_rows, bool qout, hipStream_t st) {
    if (!x || !y || !stats || !lengths || !running_mean || !running_var || (act == ACT_PRELU && !alpha)) return AVSE_EINVAL;
    if (training) return AVSE_EINVAL;                    // inference only: there is no length-aware statistics pass
    if (qout && !y_max) return AVSE_EINVAL;
    if (!shape_ok(N, C, S) || act < ACT_NONE || act > ACT_PRELU) return AVSE_ESHAPE;
    if (act == ACT_PRELU && alpha_n != 1 && alpha_n != C) return AVSE_ESHAPE;
    if (B <= 0 || T <= 0 || inner <= 0 || t_off < 0 || t_off >= T || B > 0x7FFFFFFF || T > 0x7FFFFFFF ||
        inner > 0x7FFFFFFF)
        return AVSE_ESHAPE;
    if (time_in_rows ? (N / T / inner != B || B * T * inner != N) : (N != B || S / inner != T || T * inner != S))
        return AVSE_ESHAPE;
    const int V = ((C * S) % 4 == 0 && al16(x) && al16(y)) ? 4 : 1;
    if (qout && (S != 1 || C % 64 || V != 4 || !time_in_rows)) return AVSE_ESHAPE;
    const Geo g = make_geo(N, C, S, V);
    const LenGeo lg{(int)T, (int)inner, (int)t_off, time_in_rows ? 1 : 0};
    const dim3 grid(g.tiles, g.nrb);
    hipLaunchKernelGGL(eval_stats_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, (int)C, running_mean,
                       running_var, eps, stats, y_max);
    AVSE_CHECK_LAUNCH();
    const float* cs = stats;
    if (qout) {
        launch_apply_len<4, 1>(act, grid, st, g, lg, x, lengths, cs, gamma, beta, alpha, (int)alpha_n, y, y_max);
        AVSE_CHECK_LAUNCH();
        launch_apply_len<4, 2>(act, grid, st, g, lg, x, lengths, cs, gamma, beta, alpha, (int)alpha_n, y, y_max);
    } else if (V == 4) {
        launch_apply_len<4, 0>(act, grid, st, g, lg, x, lengths, cs, gamma, beta, alpha, (int)alpha_n, y, y_max);
    } else {
        launch_apply_len<1, 0>(act, grid, st, g, lg, x, lengths, cs, gamma, beta, alpha, (int)alpha_n, y, y_max);
    }
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

int avse_bnact_fwd_len(int64_t N, int64_t C, int64_t S, const float* x, const float* gamma, const float* beta,
                       int32_t act, const float* alpha, int32_t alpha_n, int32_t training, float eps,
                       const float* running_mean, const float* running_var, float* stats, float* y, uint32_t* y_max,
                       const int32_t* lengths, int64_t B, int64_t T, int64_t inner, int64_t t_off, int32_t time_in_rows,
                       avse_stream_t stream) {
    return bnact_fwd_len_impl(N, C, S, x, gamma, beta, act, alpha, alpha_n, training, eps, running_mean, running_var,
                              stats, y, y_max, lengths, B, T, inner, t_off, time_in_rows, false, (hipStream_t)stream);
}

int avse_bnact_fwd_q_len(int64_t N, int64_t C, int64_t S, const float* x, const float* gamma, const float* beta,
                         int32_t act, const float* alpha, int32_t alpha_n, int32_t training, float eps,
                         const float* running_mean, const float* running_var, float* stats, void* yq, uint32_t* y_max,
                         const int32_t* lengths, int64_t B, int64_t T, int64_t inner, int64_t t_off, int32_t time_in_rows,
                         avse_stream_t stream) {
    return bnact_fwd_len_impl(N, C, S, x, gamma, beta, act, alpha, alpha_n, training, eps, running_mean, running_var,
                              stats, (float*)yq, y_max, lengths, B, T, inner, t_off, time_in_rows, true,
                              (hipStream_t)stream);
}

static int bnact_bwd_impl(int64_t N, int64_t C, int64_t S, const float* x, const float* res, const float* dy,
                          const float* stats, const float* gamma, const float* beta, int32_t act, const float* alpha,
                          int32_t alpha_n, int32_t training, float* dx, float* dres, float* dgamma, float* dbeta,
                          float* dalpha_c, float* workspace, uint32_t* dx_max, bool qout, hipStream_t st) {
    if (!x || !dy || !stats || !dx || !workspace || (act == ACT_PRELU && (!alpha || !dalpha_c)) || (res && !dres))
        return AVSE_EINVAL;
    if (!shape_ok(N, C, S) || act < ACT_NONE || act > ACT_PRELU) return AVSE_ESHAPE;
    if (act == ACT_PRELU && alpha_n != 1 && alpha_n != C) return AVSE_ESHAPE;
    const int V = ((C * S) % 4 == 0 && al16(x) && al16(dy) && al16(dx) && (!res || (al16(res) && al16(dres))) &&
                   al16(workspace)) ? 4 : 1;
    if (qout && (!dx_max || res || S != 1 || C % 64 || V != 4)) return AVSE_ESHAPE;
    const Geo g = make_geo(N, C, S, V);
    const dim3 grid(g.tiles, g.nrb);
    float* kbuf = workspace + 4 * (int64_t)g.nrb * g.CS;
    const int G = chan_groups(g);
    double* fin = fin_ptr(workspace, g);
    if (qout) {
        dispatch_q<BwdPartQK>::run(act, grid, st, g, x, res, dy, stats, gamma, beta, alpha, (int)alpha_n, workspace, dres);
        AVSE_CHECK_LAUNCH();
        hipLaunchKernelGGL((chan_partial_kernel<4, 3>), dim3((unsigned)C, G), dim3(THREADS), 0, st, g,
                           (const float*)workspace, fin, dx_max);
    } else {
        dispatch<BwdPartK>::run(V, act, res != nullptr, grid, st, g, x, res, dy, stats, gamma, beta, alpha, (int)alpha_n,
                                workspace, dres);
        AVSE_CHECK_LAUNCH();
        hipLaunchKernelGGL((chan_partial_kernel<3>), dim3((unsigned)C, G), dim3(THREADS), 0, st, g,
                           (const float*)workspace, fin, (uint32_t*)nullptr);
    }
    AVSE_CHECK_LAUNCH();
    hipLaunchKernelGGL(bwd_combine, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, g, (const double*)fin, G,
                       (int)training, dgamma, dbeta, dalpha_c, kbuf, dx_max, (int)qout, stats, gamma);
    AVSE_CHECK_LAUNCH();
    if (qout)
        dispatch_q<BwdApplyQK>::run(act, grid, st, g, x, dy, (const float*)dres, stats, gamma, beta, alpha, (int)alpha_n,
                                   (const float*)kbuf, dx, dx_max);
    else
        dispatch<BwdApplyK>::run(V, act, res != nullptr, grid, st, g, x, dy, (const float*)dres, stats, gamma, beta,
                                 alpha, (int)alpha_n, (const float*)kbuf, dx, dx_max);
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

int avse_bnact_bwd(int64_t N, int64_t C, int64_t S, const float* x, const float* res, const float* dy, const float* stats,
                   const float* gamma, const float* beta, int32_t act, const float* alpha, int32_t alpha_n,
                   int32_t training, float* dx, float* dres, float* dgamma, float* dbeta, float* dalpha_c,
                   float* workspace, uint32_t* dx_max, avse_stream_t stream) {
    return bnact_bwd_impl(N, C, S, x, res, dy, stats, gamma, beta, act, alpha, alpha_n, training, dx, dres, dgamma,
                          dbeta, dalpha_c, workspace, dx_max, false, (hipStream_t)stream);
}

int avse_bnact_bwd_q(int64_t N, int64_t C, int64_t S, const float* x, const float* dy, const float* stats,
                     const float* gamma, const float* beta, int32_t act, const float* alpha, int32_t alpha_n,
                     int32_t training, void* dxq, float* dgamma, float* dbeta, float* dalpha_c, float* workspace,
                     uint32_t* dx_bound, avse_stream_t stream) {
    return bnact_bwd_impl(N, C, S, x, nullptr, dy, stats, gamma, beta, act, alpha, alpha_n, training, (float*)dxq,
                          nullptr, dgamma, dbeta, dalpha_c, workspace, dx_bound, true, (hipStream_t)stream);
}

// ---- backward from producer-written rows (csrc/bnact_cols.h: the epilogue of the split-fp16 input-gradient
// convolution that wrote dy also wrote, per pixel tile, one row of the per-channel sums): chan_partial_kernel over
// `rows` rows in place of the row blocks of bwd_partial_kernel, then bwd_combine and bwd_apply_kernel as ever.
// workspace: [rows][NQ][C] floats (written by the producer), kbuf (2 C), 16-aligned fp64 per-channel partials.
static inline int64_t rows_floats(int64_t rows, int64_t C, int64_t nq) { return rows * nq * C; }

int64_t avse_bnact_rows_workspace_bytes(int64_t rows, int64_t C, int64_t nq) {
    if (rows <= 0 || rows >= (1 << 23) || C <= 0 || C >= (1 << 20) || (nq != 3 && nq != 4)) return 0;
    return 4 * (rows_floats(rows, C, nq) + 2 * C) + 16 + 8 * C * MAXG * 4;
}

int avse_bnact_bwd_rows(int64_t N, int64_t C, int64_t rows, const float* x, const float* dy, const float* stats,
                        const float* gamma, const float* beta, int32_t act, const float* alpha, int32_t alpha_n,
                        int32_t training, float* dx, float* dgamma, float* dbeta, float* dalpha_c, float* workspace,
                        uint32_t* dx_max, int32_t q_out, avse_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!x || !dy || !stats || !dx || !workspace || !dx_max || (act == ACT_PRELU && (!alpha || !dalpha_c)))
        return AVSE_EINVAL;
    if (!shape_ok(N, C, 1) || act < ACT_NONE || act > ACT_PRELU) return AVSE_ESHAPE;
    if (act == ACT_PRELU && alpha_n != 1 && alpha_n != C) return AVSE_ESHAPE;
    if (rows <= 0 || rows >= (1 << 23)) return AVSE_ESHAPE;                  // chan_partial_kernel: cnt < 2^23
    if (C % 4 || !al16(x) || !al16(dy) || !al16(dx) || !al16(workspace)) return AVSE_EALIGN;
    if (q_out && C % 64) return AVSE_ESHAPE;
    const int nq = q_out ? 4 : 3;
    const Geo g = make_geo(N, C, 1, 4);
    Geo gr = g;
    gr.nrb = (int)rows;
    float* kbuf = workspace + rows_floats(rows, C, nq);
    double* fin = reinterpret_cast<double*>(((uintptr_t)(kbuf + 2 * C) + 15) & ~(uintptr_t)15);
    const int G = chan_groups(gr);
    if (q_out)
        hipLaunchKernelGGL((chan_partial_kernel<4, 3>), dim3((unsigned)C, G), dim3(THREADS), 0, st, gr,
                           (const float*)workspace, fin, dx_max);
    else
        hipLaunchKernelGGL((chan_partial_kernel<3>), dim3((unsigned)C, G), dim3(THREADS), 0, st, gr,
                           (const float*)workspace, fin, (uint32_t*)nullptr);
    AVSE_CHECK_LAUNCH();
    hipLaunchKernelGGL(bwd_combine, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, g, (const double*)fin, G,
                       (int)training, dgamma, dbeta, dalpha_c, kbuf, dx_max, (int)(q_out != 0), stats, gamma);
    AVSE_CHECK_LAUNCH();
    const dim3 grid(g.tiles, g.nrb);
    if (q_out)
        dispatch_q<BwdApplyQK>::run(act, grid, st, g, x, dy, (const float*)nullptr, stats, gamma, beta, alpha,
                                   (int)alpha_n, (const float*)kbuf, dx, dx_max);
    else
        dispatch<BwdApplyK>::run(4, act, false, grid, st, g, x, dy, (const float*)nullptr, stats, gamma, beta, alpha,
                                 (int)alpha_n, (const float*)kbuf, dx, dx_max);
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

// ---- the fused lip front-end chain (namespace pool above)
static bool pool_geo(pool::PGeo& p, int64_t B, int64_t C, int64_t T, int64_t H, int64_t W) {
    if (B <= 0 || C <= 0 || T <= 0 || H < 2 || W < 4 || C % pool::CT || H % 2 || W % 4 || W > pool::MAXW) return false;
    if (H > (1 << 20) || !shape_ok(B, C, T * H * W)) return false;
    p.B = (int)B; p.C = (int)C; p.T = (int)T; p.H = (int)H; p.W = (int)W;
    p.Ho = (int)(H / 2); p.Wo = (int)(W / 2);
    p.bands = (p.Ho + pool::RB - 1) / pool::RB;
    p.ctiles = (int)(C / pool::CT);
    p.mq = 65536u / (uint32_t)(W / 4) + 1u;
    return B * T * p.ctiles * p.bands < (1LL << 31) && B * T * p.bands < (1 << 23);   // chan_partial_kernel: cnt < 2^23
}

int32_t avse_bnpool_supported(int64_t B, int64_t C, int64_t T, int64_t H, int64_t W) {
    pool::PGeo p;
    return pool_geo(p, B, C, T, H, W) ? 1 : 0;
}

int64_t avse_bnpool_rows(int64_t B, int64_t C, int64_t T, int64_t H, int64_t W) {
    pool::PGeo p;
    return pool_geo(p, B, C, T, H, W) ? B * T * p.bands : 0;
}

int avse_bnpool_fwd(int64_t B, int64_t C, int64_t T, int64_t H, int64_t W, const float* x, const float* gamma,
                    const float* beta, int32_t act, const float* alpha, int32_t alpha_n, int32_t training, float eps,
                    float momentum, float* running_mean, float* running_var, float* stats, float* y, uint8_t* idx,
                    float* workspace, avse_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!x || !y || !idx || !stats || !workspace || (act == ACT_PRELU && !alpha)) return AVSE_EINVAL;
    if (!training && (!running_mean || !running_var)) return AVSE_EINVAL;
    pool::PGeo p;
    if (!pool_geo(p, B, C, T, H, W) || act < ACT_NONE || act > ACT_PRELU) return AVSE_ESHAPE;
    if (act == ACT_PRELU && alpha_n != 1 && alpha_n != C) return AVSE_ESHAPE;
    if (!al16(x) || !al16(y) || !al16(workspace) || ((uintptr_t)idx & 1)) return AVSE_EALIGN;
    const Geo g = make_geo(B, C, T * H * W, 4);
    const int rc = launch_stats(g, 4, x, gamma, beta, act, alpha, alpha_n, training, eps, momentum, running_mean,
                                running_var, stats, workspace, nullptr, false, st);
    if (rc != AVSE_OK) return rc;
    const dim3 grid((unsigned)(B * T * p.ctiles * p.bands));
    const size_t lds = sizeof(float) * pool::RB * p.Wo * pool::LP;
#define AVSE_POOL_FWD(AA) \
    hipLaunchKernelGGL((pool::fwd_kernel<AA>), grid, dim3(THREADS), lds, st, p, x, (const float*)stats, gamma, beta, alpha, \
                       (int)alpha_n, y, idx)
    if (act == ACT_NONE) AVSE_POOL_FWD(ACT_NONE);
    else if (act == ACT_RELU) AVSE_POOL_FWD(ACT_RELU);
    else AVSE_POOL_FWD(ACT_PRELU);
#undef AVSE_POOL_FWD
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

int avse_bnpool_bwd(int64_t B, int64_t C, int64_t T, int64_t H, int64_t W, const float* x, const float* g,
                    const uint8_t* idx, const float* stats, const float* gamma, const float* beta, int32_t act,
                    const float* alpha, int32_t alpha_n, int32_t training, float* dx, float* dgamma, float* dbeta,
                    float* dalpha_c, float* workspace, uint32_t* dx_max, avse_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!x || !g || !idx || !stats || !dx || !workspace || (act == ACT_PRELU && (!alpha || !dalpha_c))) return AVSE_EINVAL;
    pool::PGeo p;
    if (!pool_geo(p, B, C, T, H, W) || act < ACT_NONE || act > ACT_PRELU) return AVSE_ESHAPE;
    if (act == ACT_PRELU && alpha_n != 1 && alpha_n != C) return AVSE_ESHAPE;
    if (!al16(x) || !al16(g) || !al16(dx) || !al16(workspace) || ((uintptr_t)idx & 1)) return AVSE_EALIGN;
    const int64_t rows = B * T * p.bands;
    // the per-channel reduction and the combine see the chain as a channels-last (B T H W, C) BatchNorm with `rows` rows
    Geo gc = make_geo(B * T * H * W, C, 1, 4);
    Geo gr = gc;
    gr.nrb = (int)rows;
    float* kbuf = workspace + rows_floats(rows, C, 3);
    double* fin = reinterpret_cast<double*>(((uintptr_t)(kbuf + 2 * C) + 15) & ~(uintptr_t)15);
    const int G = chan_groups(gr);
    const dim3 grid((unsigned)(B * T * p.ctiles * p.bands));
    const size_t lds = sizeof(float) * (pool::RB + 1) * p.Wo * pool::LP;
#define AVSE_POOL_BWD(AA, AP) \
    hipLaunchKernelGGL((pool::bwd_kernel<AA, AP>), grid, dim3(THREADS), lds, st, p, x, g, idx, stats, gamma, beta, alpha, \
                       (int)alpha_n, (const float*)kbuf, workspace, dx, dx_max)
    if (act == ACT_NONE) AVSE_POOL_BWD(ACT_NONE, false);
    else if (act == ACT_RELU) AVSE_POOL_BWD(ACT_RELU, false);
    else AVSE_POOL_BWD(ACT_PRELU, false);
    AVSE_CHECK_LAUNCH();
    hipLaunchKernelGGL((chan_partial_kernel<3>), dim3((unsigned)C, G), dim3(THREADS), 0, st, gr, (const float*)workspace,
                       fin, (uint32_t*)nullptr);
    AVSE_CHECK_LAUNCH();
    hipLaunchKernelGGL(bwd_combine, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, gc, (const double*)fin, G,
                       (int)training, dgamma, dbeta, dalpha_c, kbuf, dx_max, 0, stats, gamma);
    AVSE_CHECK_LAUNCH();
    if (act == ACT_NONE) AVSE_POOL_BWD(ACT_NONE, true);
    else if (act == ACT_RELU) AVSE_POOL_BWD(ACT_RELU, true);
    else AVSE_POOL_BWD(ACT_PRELU, true);
#undef AVSE_POOL_BWD
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

}  // extern "C"
