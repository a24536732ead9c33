// Per-utterance linear upsampling of the visual stream for ragged avse4 batches (gfx950).
//
// Replaces, per sample, F.interpolate(v, scale_factor=32, mode="linear") followed by the pad / crop to the audio
// frame count of baseline/avse4/model.py:166-176 (TemporalConvNet.forward): with n_in = vlen[b] video
// frames and n_out = klen[b] audio frames,
//   out[b, c, j] = (1 - lam) v[b, c, i0] + lam v[b, c, min(i0 + 1, n_in - 1)],   j < min(up n_in, n_out)
// with the align_corners=False source coordinate (j + 0.5) / up - 0.5 clamped at 0, i0 its floor, lam its fraction;
// 0 for every other j < K.  The coordinate is formed in integers (2 up src = 2 j + 1 - up), so lam is the exact
// multiple of 1 / (2 up) for every up.  v and out carry batch and channel strides: out may be a channel slice of the
// tensor the next 1x1 conv reads (the torch.cat of model.py:177 without a copy).  One workgroup per (b, c) row.
#include "common.h"

namespace avse {
namespace ups {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void linear_len_kernel(int C, int n_in_max, int K, int up,
                                                             const float* __restrict__ v, int64_t v_bs, int64_t v_cs,
                                                             const int32_t* __restrict__ vlen,
                                                             const int32_t* __restrict__ klen, float* __restrict__ out,
                                                             int64_t o_bs, int64_t o_cs) {
    const int row = blockIdx.x, b = row / C, c = row % C;
    const int n_in = min(max(vlen[b], 0), n_in_max), n_out = min(max(klen[b], 0), K);
    const int n = (int)min((int64_t)up * n_in, (int64_t)n_out);      // interpolated columns; 0 when n_in == 0
    const float* vr = v + b * v_bs + c * v_cs;
    float* orow = out + b * o_bs + c * o_cs;
    const float inv = 1.f / (float)(2 * up);
    for (int j = threadIdx.x; j < K; j += THREADS) {
        float r = 0.f;
        if (j < n) {
            const int num = max(2 * j + 1 - up, 0);                  // 2 up src
            const int i0 = num / (2 * up), i1 = min(i0 + 1, n_in - 1);
            const float lam = (float)(num - i0 * 2 * up) * inv;
            r = (1.f - lam) * vr[i0] + lam * vr[i1];
        }
        orow[j] = r;
    }
}

// Per-utterance nearest-neighbour gather of the avse1 lip features onto the audio frames (time-major rows): replaces,
// per sample, F.interpolate(vis, size=(T_b, C), mode="nearest") of baseline/avse1/model.py:124-126, i.e.
//   out[b, t, :C] = vis[b, (t n_in) / n_out, :C]  (integer division: torch.div(..., rounding_mode="floor"))  for t < n_out,
// 0 for n_out <= t < T, with n_in = vlen[b], n_out = tlen[b].  out rows carry a row stride >= C: the left C columns of
// the cat((vis, audio), -1) tensor the LSTM's input GEMM reads.  One workgroup per GROWS output rows, a wave per row.
constexpr int GROWS = THREADS / 64;

template <int V>
__global__ __launch_bounds__(THREADS) void nearest_len_kernel(int C, int n_in_max, int T, const float* __restrict__ v,
                                                              int64_t v_bs, int64_t v_ts,
                                                              const int32_t* __restrict__ vlen,
                                                              const int32_t* __restrict__ tlen, float* __restrict__ out,
                                                              int64_t o_bs, int64_t o_ts, int64_t rows) {
    const int64_t row = (int64_t)blockIdx.x * GROWS + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
    const int n_in = min(max(vlen[b], 0), n_in_max), n_out = min(max(tlen[b], 0), T);
    float* orow = out + b * o_bs + t * o_ts;
    const bool ok = t < n_out && n_in > 0;
    const int src = ok ? (int)(((int64_t)t * n_in) / n_out) : 0;          // < n_in since t < n_out
    const float* vr = v + b * v_bs + src * v_ts;
    for (int c = lane * V; c < C; c += 64 * V) {
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(orow + c) =
                ok ? *reinterpret_cast<const float4*>(vr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            orow[c] = ok ? vr[c] : 0.f;
        }
    }
}

}  // namespace ups
}  // namespace avse

using namespace avse::ups;

extern "C" {

int avse_upsample_linear_len(int64_t B, int64_t C, int64_t n_in_max, int64_t K, int64_t up, const float* v, int64_t v_bs,
                             int64_t v_cs, const int32_t* vlen, const int32_t* klen, float* out, int64_t out_bs,
                             int64_t out_cs, avse_stream_t stream) {
    if (!v || !vlen || !klen || !out) return AVSE_EINVAL;
    if (B <= 0 || C <= 0 || n_in_max <= 0 || K <= 0 || up <= 0 || up > 4096 || K > (1LL << 29) ||
        n_in_max > (1LL << 29) || B * C > (1LL << 31) - 1)
        return AVSE_ESHAPE;
    // rows must not overlap: a row's elements lie inside its channel stride, a sample's rows inside its batch stride
    if (v_cs < n_in_max || v_bs < C * v_cs || out_cs < K || out_bs < C * out_cs) return AVSE_ESHAPE;
    hipLaunchKernelGGL(linear_len_kernel, dim3((unsigned)(B * C)), dim3(THREADS), 0, (hipStream_t)stream, (int)C,
                       (int)n_in_max, (int)K, (int)up, v, v_bs, v_cs, vlen, klen, out, out_bs, out_cs);
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

int avse_gather_nearest_len(int64_t B, int64_t C, int64_t n_in_max, int64_t T, const float* v, int64_t v_bs, int64_t v_ts,
                            const int32_t* vlen, const int32_t* tlen, float* out, int64_t out_bs, int64_t out_ts,
                            avse_stream_t stream) {
    if (!v || !vlen || !tlen || !out) return AVSE_EINVAL;
    if (B <= 0 || C <= 0 || n_in_max <= 0 || T <= 0 || T > (1LL << 29) || n_in_max > (1LL << 29) || C > (1LL << 29) ||
        B * T > (1LL << 31) - 1)
        return AVSE_ESHAPE;
    // rows must not overlap: a row's C elements inside its time stride, a sample's rows inside its batch stride
    if (v_ts < C || v_bs < n_in_max * v_ts || out_ts < C || out_bs < T * out_ts) return AVSE_ESHAPE;
    const int64_t rows = B * T;
    const dim3 grid((unsigned)((rows + GROWS - 1) / GROWS));
    const bool vec = C % 4 == 0 && v_bs % 4 == 0 && v_ts % 4 == 0 && out_bs % 4 == 0 && out_ts % 4 == 0 &&
                     ((uintptr_t)v & 15) == 0 && ((uintptr_t)out & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(nearest_len_kernel<4>, grid, dim3(THREADS), 0, (hipStream_t)stream, (int)C, (int)n_in_max,
                           (int)T, v, v_bs, v_ts, vlen, tlen, out, out_bs, out_ts, rows);
    else
        hipLaunchKernelGGL(nearest_len_kernel<1>, grid, dim3(THREADS), 0, (hipStream_t)stream, (int)C, (int)n_in_max,
                           (int)T, v, v_bs, v_ts, vlen, tlen, out, out_bs, out_ts, rows);
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

}  // extern "C"
