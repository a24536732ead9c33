// Channels-last GroupNorm(1, N) forward with a per-row valid extent, for gfx950: the dual-path norms of DPMamba
// (speechbrain Dual_Computation_Block intra_norm / inter_norm and Dual_Path_Model.norm, GroupNorm(1, N, eps 1e-8)) on a
// zero-padded ragged batch.  Inference only.
//
// x (B, R, C, N) fp32 contiguous; a "line" is the N contiguous channels of one (r, c).  Row b is valid for r < n_b
// (len_axis 0) or c < n_b (len_axis 1), n_b = lengths[b] clamped into the axis; mean and biased variance are taken over
// the row's valid elements alone, y = (x - mean) rstd gamma_n + beta_n (+ res) there and +0 everywhere else.  Invalid
// lines of x and res are never loaded.
//
// Three launches, no atomics, no wait on another workgroup:
//   1. line_stats_kernel   one wave per valid line: (sum d, sum d^2), d = x - x[b, 0, 0, 0], over the line's N elements
//                          in a lane order fixed by N alone -> ws[b][j], j = the line's rank among the row's valid
//                          lines in (r, c) order (so the cropped row alone fills the same slots with the same bits)
//   2. row_stats_kernel    one workgroup per row: its M valid line partials summed in double, in a tree fixed by M alone
//                          -> stats[b] = (mean, rstd)
//   3. apply_kernel        one wave per line of y: normalise and store (optionally as (B, C, R, N): the transpose that
//                          the inter norm's consumer wants), or store +0 for an invalid line
// so a row comes out bit for bit as the same entry point gives it on the row cropped and alone (B = 1, axis cut to n_b).
// HBM: x read twice (the second time from the Infinity Cache where the tensor fits), res read once, y written once.
#include "common.h"

namespace avse {
namespace gln_cl {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int LPW = 4, LPB = WAVES * LPW;        // lines per wave, per workgroup
constexpr int RED_THREADS = 1024;

__device__ inline int row_len(const int32_t* __restrict__ lengths, int b, int extent) {
    return min(max(lengths[b], 0), extent);
}

// A lane owns the quadruples n0 = 4 (lane + 64 i) of a line, whatever the access width, so that the vector form
// (N % 4 == 0 and 16-B aligned tensors) and the scalar form sum in the same order and give the same bits.
template <bool VEC>
__device__ inline float4 ld_quad(const float* __restrict__ line, int n0, int N) {
    if constexpr (VEC) {
        return *reinterpret_cast<const float4*>(line + n0);
    } else {
        float4 v;
        v.x = line[n0];                                   // n0 < N: the caller's loop bound
        v.y = n0 + 1 < N ? line[n0 + 1] : 0.f;
        v.z = n0 + 2 < N ? line[n0 + 2] : 0.f;
        v.w = n0 + 3 < N ? line[n0 + 3] : 0.f;
        return v;
    }
}
template <bool VEC>
__device__ inline void st_quad(float* __restrict__ line, int n0, int N, const float4& v) {
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(line + n0) = v;
    } else {
        line[n0] = v.x;
        if (n0 + 1 < N) line[n0 + 1] = v.y;
        if (n0 + 2 < N) line[n0 + 2] = v.z;
        if (n0 + 3 < N) line[n0 + 3] = v.w;
    }
}

struct Geo {
    int R, C, N, axis, bpr;                      // bpr: workgroups per row = ceil(R C / LPB)
};

template <bool VEC>
__global__ __launch_bounds__(THREADS) void line_stats_kernel(Geo g, const float* __restrict__ x,
                                                             const int32_t* __restrict__ lengths,
                                                             float2* __restrict__ ws) {
    const int b = (int)blockIdx.x / g.bpr, blk = (int)blockIdx.x % g.bpr;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int nb = row_len(lengths, b, g.axis == 0 ? g.R : g.C);
    if (nb == 0) return;
    const int lines = g.R * g.C;
    const float* xb = x + (int64_t)b * lines * g.N;
    const float shift = xb[0];                            // (b, 0, 0, 0) is valid whenever nb > 0
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        const int line = blk * LPB + wave * LPW + i;
        if (line >= lines) break;
        const int r = line / g.C, c = line % g.C;
        if (g.axis == 0 ? r >= nb : c >= nb) continue;
        const float* xl = xb + (int64_t)line * g.N;
        float s1 = 0.f, s2 = 0.f;
        for (int n0 = 4 * lane; n0 < g.N; n0 += 256) {
            const float4 v = ld_quad<VEC>(xl, n0, g.N);
            const float d0 = v.x - shift;
            const float d1 = (VEC || n0 + 1 < g.N) ? v.y - shift : 0.f;
            const float d2 = (VEC || n0 + 2 < g.N) ? v.z - shift : 0.f;
            const float d3 = (VEC || n0 + 3 < g.N) ? v.w - shift : 0.f;
            s1 += d0;
            s2 += d0 * d0;
            s1 += d1;
            s2 += d1 * d1;
            s1 += d2;
            s2 += d2 * d2;
            s1 += d3;
            s2 += d3 * d3;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            s1 += __shfl_xor(s1, m, 64);
            s2 += __shfl_xor(s2, m, 64);
        }
        if (lane == 0) ws[(int64_t)b * lines + (g.axis == 0 ? line : r * nb + c)] = make_float2(s1, s2);
    }
}

// stats[b] = (mean, rstd) from the row's M valid line partials, slots 0 .. M - 1 of its workspace part: thread t sums
// slots t, t + 1024, ... in double, then the wave, then the 16 waves in order -- a tree that M alone decides
__global__ __launch_bounds__(RED_THREADS) void row_stats_kernel(Geo g, const float* __restrict__ x,
                                                                const int32_t* __restrict__ lengths,
                                                                const float2* __restrict__ ws, float eps,
                                                                float2* __restrict__ stats) {
    __shared__ double red[2][RED_THREADS / 64];
    const int b = (int)blockIdx.x;
    const int nb = row_len(lengths, b, g.axis == 0 ? g.R : g.C);
    if (nb == 0) {
        if (threadIdx.x == 0) stats[b] = make_float2(0.f, 0.f);
        return;
    }
    const int lines = g.R * g.C;
    const int M = g.axis == 0 ? nb * g.C : g.R * nb;
    const float2* wb = ws + (int64_t)b * lines;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
    for (int j = (int)threadIdx.x; j < M; j += RED_THREADS) {
        const float2 v = wb[j];
        s1 += (double)v.x;
        s2 += (double)v.y;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        s1 += __shfl_xor(s1, m, 64);
        s2 += __shfl_xor(s2, m, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s1;
        red[1][threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < RED_THREADS / 64; ++w) {
            t1 += red[0][w];
            t2 += red[1][w];
        }
        const double n = (double)M * g.N;
        const double m1 = t1 / n, m2 = t2 / n;
        const double var = fmax(m2 - m1 * m1, 0.0);
        const float shift = x[(int64_t)b * lines * g.N];
        stats[b] = make_float2((float)(m1 + (double)shift), (float)(1.0 / sqrt(var + (double)eps)));
    }
}

// TR: y (and res) in the (B, C, R, N) layout.  The channel chunk is the outer loop, so a wave loads gamma / beta once
// for its LPW lines.
template <bool VEC, bool RES, bool TR>
__global__ __launch_bounds__(THREADS) void apply_kernel(Geo g, const float* __restrict__ x,
                                                        const int32_t* __restrict__ lengths,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float2* __restrict__ stats, const float* __restrict__ res,
                                                        float* __restrict__ y) {
    const int b = (int)blockIdx.x / g.bpr, blk = (int)blockIdx.x % g.bpr;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int nb = row_len(lengths, b, g.axis == 0 ? g.R : g.C);
    const int lines = g.R * g.C;
    const int line0 = blk * LPB + wave * LPW;
    const float2 st = stats[b];                            // written by row_stats_kernel for every b
    const int64_t row = (int64_t)b * lines;
    for (int n0 = 4 * lane; n0 < g.N; n0 += 256) {
        const float4 gm = ld_quad<VEC>(gamma, n0, g.N), bt = ld_quad<VEC>(beta, n0, g.N);
        const float4 gs = make_float4(gm.x * st.y, gm.y * st.y, gm.z * st.y, gm.w * st.y);
#pragma unroll
        for (int i = 0; i < LPW; ++i) {
            const int line = line0 + i;
            if (line >= lines) break;
            const int r = line / g.C, c = line % g.C;
            const bool valid = g.axis == 0 ? r < nb : c < nb;
            const int64_t oline = row + (TR ? c * g.R + r : line);
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid) {
                const float4 v = ld_quad<VEC>(x + (row + line) * g.N, n0, g.N);
                o.x = (v.x - st.x) * gs.x + bt.x;
                o.y = (v.y - st.x) * gs.y + bt.y;
                o.z = (v.z - st.x) * gs.z + bt.z;
                o.w = (v.w - st.x) * gs.w + bt.w;
                if constexpr (RES) {
                    const float4 q = ld_quad<VEC>(res + oline * g.N, n0, g.N);
                    o.x += q.x;
                    o.y += q.y;
                    o.z += q.z;
                    o.w += q.w;
                }
            }
            st_quad<VEC>(y + oline * g.N, n0, g.N, o);
        }
    }
}

}  // namespace gln_cl
}  // namespace avse

using namespace avse::gln_cl;

extern "C" {

int64_t avse_gln_cl_workspace_bytes(int64_t B, int64_t R, int64_t C) { return B * R * C * (int64_t)sizeof(float2); }

int avse_gln_cl_fwd_len(int64_t B, int64_t R, int64_t C, int64_t N, const float* x, const int32_t* lengths,
                        int len_axis, const float* gamma, const float* beta, float eps, const float* res,
                        int transpose_out, float* y, float* stats, float* workspace, avse_stream_t stream) {
    if (!x || !lengths || !gamma || !beta || !y || !stats || !workspace) return AVSE_EINVAL;
    if (B <= 0 || R <= 0 || C <= 0 || N <= 0 || (len_axis != 0 && len_axis != 1)) return AVSE_ESHAPE;
    const int64_t lim = (1LL << 31) - 1;
    if (R > lim || C > lim || N > lim - 256 || R * C > lim - LPB || B > lim) return AVSE_ESHAPE;
    const int64_t bpr = (R * C + LPB - 1) / LPB;
    if (B * bpr > lim) return AVSE_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const Geo g{(int)R, (int)C, (int)N, len_axis, (int)bpr};
    const bool vec = N % 4 == 0 &&
                     (((uintptr_t)x | (uintptr_t)y | (uintptr_t)res | (uintptr_t)gamma | (uintptr_t)beta) % 16) == 0;
    float2* ws = (float2*)workspace;
    const dim3 grid((unsigned)(B * bpr)), block(THREADS);
    if (vec) hipLaunchKernelGGL(line_stats_kernel<true>, grid, block, 0, st, g, x, lengths, ws);
    else hipLaunchKernelGGL(line_stats_kernel<false>, grid, block, 0, st, g, x, lengths, ws);
    AVSE_CHECK_LAUNCH();
    hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)B), dim3(RED_THREADS), 0, st, g, x, lengths, (const float2*)ws,
                       eps, (float2*)stats);
    AVSE_CHECK_LAUNCH();
#define A_(V, RS, T) hipLaunchKernelGGL((apply_kernel<V, RS, T>), grid, block, 0, st, g, x, lengths, gamma, beta, \
                                        (const float2*)stats, res, y)
#define A_T(V, RS) do { if (transpose_out) A_(V, RS, true); else A_(V, RS, false); } while (0)
    if (vec) {
        if (res) A_T(true, true); else A_T(true, false);
    } else {
        if (res) A_T(false, true); else A_T(false, false);
    }
#undef A_T
#undef A_
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

}  // extern "C"
