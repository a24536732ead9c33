// Per-column maths of the fused BatchNorm -> activation passes (csrc/bnact.hip), shared with the convolution kernels
// whose input-gradient epilogues take the BatchNorm backward's per-channel sums (csrc/dconv.hip, csrc/sconv.hip): the
// pre-activation z, the activation and its mask have ONE definition, so a mask formed in an epilogue is bit-identical
// to the one the forward apply pass and the backward apply pass form.
#pragma once

#include "common.h"

namespace avse {
namespace bnact {

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_PRELU = 2 };

// per-column constants of the thread's V columns: z = (x - mean) a + b (+ res) -- centred first, as torch does,
// so large-mean inputs do not lose the low bits of z to a cancelling a x + (beta - mean a) -- act slope, rstd
// The mean is carried as a float pair (hi + lo): x - hi is exact for x near the mean (Sterbenz), so the
// centred value keeps its low bits even when |mean| >> std (a ReLU/PReLU mask computed from z would
// otherwise flip for |z| below a * ulp(mean); torch's CPU kernels centre in double).
template <int V, int ACT>
struct ColConst {
    float a[V], b[V], al[V], mean[V], mlo[V], rstd[V], gam[V];
    __device__ inline float centred(float v, int k) const { return (v - mean[k]) - mlo[k]; }
    // the pre-activation (without a residual) and the normalised value of column k
    __device__ inline float preact(float v, int k) const { return fmaf(centred(v, k), a[k], b[k]); }
    __device__ inline float xhat(float v, int k) const { return centred(v, k) * rstd[k]; }
    __device__ inline void load_channel(int k, int c, const float* stats, const float* gamma, const float* beta,
                                        const float* alpha, int alpha_n) {
        mean[k] = stats[4 * c];
        mlo[k] = stats[4 * c + 1];
        rstd[k] = stats[4 * c + 2];
        gam[k] = gamma ? gamma[c] : 1.f;
        a[k] = gam[k] * rstd[k];
        b[k] = beta ? beta[c] : 0.f;
        al[k] = ACT == ACT_PRELU ? alpha[alpha_n > 1 ? c : 0] : 0.f;
    }
    template <class G>
    __device__ inline void load(const G& g, int64_t j0, const float* stats, const float* gamma, const float* beta,
                                const float* alpha, int alpha_n) {
#pragma unroll
        for (int k = 0; k < V; ++k) load_channel(k, (int)((j0 + k) / g.S), stats, gamma, beta, alpha, alpha_n);
    }
};

template <int ACT>
__device__ inline float act_fwd(float z, float al) {
    if constexpr (ACT == ACT_RELU) return z > 0.f ? z : 0.f;
    else if constexpr (ACT == ACT_PRELU) return z > 0.f ? z : al * z;
    else return z;
}
template <int ACT>
__device__ inline float act_bwd(float z, float g, float al) {
    if constexpr (ACT == ACT_RELU) return z > 0.f ? g : 0.f;
    else if constexpr (ACT == ACT_PRELU) return z > 0.f ? g : al * g;
    else return g;
}

// ---- BatchNorm-backward partials in the epilogue of a split-fp16 input-gradient convolution
// The convolution's output dy is the gradient of y = act(BN(x)); the workgroup that holds a (pixels x channels) tile of
// dy in its MFMA accumulators also forms the backward's per-channel sums over that tile -- sum dz, sum dz xhat, the
// PReLU slope sum dy z over !(z > 0) and (MAXDZ) max |dz| -- so that bnact's reduction pass over x and dy (8 B per
// element) is not run: x is read here, at the addresses dy was just stored to.
struct BnEpi {
    const float* x;            // the BatchNorm's input, NHWC, the shape of the convolution's output
    const float* stats;        // (C, 4) of the forward
    const float* gamma;
    const float* beta;
    const float* alpha;
    int alpha_n;
    float* rows;               // [tile row][NQ][C] floats, the layout chan_partial_kernel reads
};

// The accumulator layout of the dcf / scv forward kernels: a wave holds 64 pixels x 64 channels as acc[i][j] (i: pixel
// block of 32, j: channel block of 32), register 4 g + e = pixel 32 i + 8 g + 4 (lane >> 5) + e, channel 32 j +
// (lane & 31); a lane owns 2 channels x 32 pixels.  dyv(i, j, r) returns the value stored for register r; store(j)
// stores channel block j of dy; pix0 the wave's first pixel, npix the pixel count of the tensor (pixels at or past it
// contribute nothing); ch0 the wave's first channel, C the tensor's channels.  part: NQ x 64 floats of this wave.
// Per channel block the lane's 32 x values are requested first, unconditionally, so that they are all in flight
// together and under the block's dy stores (loads behind a per-pixel branch went out one round trip at a time): buffer
// loads off one wave-uniform descriptor that starts at the wave's first pixel and ends with the tensor, so a load
// costs one offset register, not an address pair (32 of those spilled), and a pixel past the end reads 0 with its
// gradient zeroed.  Order of the sums: per lane e, g, i ascending; then lane + 32 added to lane.
template <int ACT, bool MAXDZ, class F, class ST>
__device__ inline void bn_epi_wave(const BnEpi& b, F dyv, ST store, int64_t pix0, int64_t npix, int ch0, int C,
                                   int lane, float* part) {
    constexpr int NQ = MAXDZ ? 4 : 3;
    // x from the wave's (pixel pix0, channel ch0) to the end of the tensor; the range check covers the whole offset
    // (all of it is in the offset register and the instruction's immediate)
    const uint64_t xa = (uint64_t)(b.x + pix0 * C + ch0);
    const int64_t left = ((npix - pix0) * C - ch0) * 4;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xa >> 32)) << 32) |
                (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xa)),
        0, __builtin_amdgcn_readfirstlane((int)(left < 0 ? 0 : (left > 0x7FFFFFF0LL ? 0x7FFFFFF0LL : left))), 0x00020000);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int o = ch0 + 32 * j + (lane & 31);
        ColConst<1, ACT> cc;
        cc.load_channel(0, o, b.stats, b.gamma, b.beta, b.alpha, b.alpha_n);
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        float xv[2][4][4];
        const int voff = (4 * (lane >> 5) * C + 32 * j + (lane & 31)) * 4;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    xv[i][g][e] = __builtin_bit_cast(
                        float, __builtin_amdgcn_raw_buffer_load_b32(rx, voff + (32 * i + 8 * g + e) * C * 4, 0, 0));
        store(j);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool in = pix0 + 32 * i + 8 * g + 4 * (lane >> 5) + e < npix;
                    const float gv = in ? dyv(i, j, 4 * g + e) : 0.f;       // a zero gradient adds exact zeros
                    const float z = cc.preact(xv[i][g][e], 0);
                    const float dz = act_bwd<ACT>(z, gv, cc.al[0]);
                    s[0] += dz;
                    s[1] = fmaf(dz, cc.xhat(xv[i][g][e], 0), s[1]);
                    if constexpr (ACT == ACT_PRELU) s[2] = fmaf(z > 0.f ? 0.f : gv, z, s[2]);
                    if constexpr (MAXDZ) s[3] = fmaxf(s[3], fabsf(dz));
                }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float t = __shfl_xor(s[q], 32, 64);
            const float v = (MAXDZ && q == 3) ? fmaxf(s[q], t) : s[q] + t;
            if (lane < 32) part[q * 64 + 32 * j + lane] = v;
        }
    }
}

// part[wave][NQ][64] of the workgroup's waves -> one row: channel slice ch0 .. ch0 + 64 nwn of row `row`; waves that
// share a channel slice (wave = wm * nwn + wn, wm = 0 .. nwm - 1) are summed in wm order.  Call after a barrier.
template <bool MAXDZ>
__device__ inline void bn_epi_row(const BnEpi& b, const float* part, int nwm, int nwn, int64_t row, int ch0, int C) {
    constexpr int NQ = MAXDZ ? 4 : 3;
    for (int t = threadIdx.x; t < NQ * 64 * nwn; t += blockDim.x) {
        const int c = t % (64 * nwn), q = t / (64 * nwn), wn = c >> 6, cl = c & 63;
        float v = part[(wn * NQ + q) * 64 + cl];
        for (int wm = 1; wm < nwm; ++wm) {
            const float u = part[((wm * nwn + wn) * NQ + q) * 64 + cl];
            v = (MAXDZ && q == 3) ? fmaxf(v, u) : v + u;
        }
        b.rows[(row * NQ + q) * C + ch0 + c] = v;
    }
}

}  // namespace bnact
}  // namespace avse
