// The numerical contract of the "split fp16" operands, in one place: the scale exponent of a max word,
// the hi / lo split of a value, and the workgroup reduction that produces a max word.  Every producer and consumer of
// a max word or of a pair of planes goes through these functions, so they compute the same e and the same bytes.
//
// A max word holds the float bits of max |x| (or of an upper bound of it).  The reductions run on the bits, not on the
// floats: non-negative floats order like their bits, and a NaN (exponent all ones, mantissa non-zero) orders above
// every finite value and +inf, so a NaN input wins and reaches the word instead of being dropped as fmaxf drops it.
// A workgroup publishes with ONE atomicMax: the atomics on one word serialise at the memory side (~17 ns each), so one
// per wave of a large grid costs more than the pass that feeds it.
#pragma once
#include "common.h"

namespace avse {

// power-of-two scale exponent e of a tensor whose max |x| has the float bits maxbits: max |x| 2^e in [2^14, 2^15),
// clamped to +-100 (subnormal and inf / NaN maxima), 0 for an all-zero tensor
__host__ __device__ constexpr inline int split_exp(uint32_t maxbits) {
    if (maxbits == 0) return 0;
    const int ef = (int)((maxbits >> 23) & 0xff);
    const int e = 14 - (ef == 0 ? -127 : ef - 127);
    const int lo = e < -100 ? -100 : e;
    return lo > 100 ? 100 : lo;
}
static_assert(split_exp(0u) == 0, "an all-zero tensor is not scaled");
static_assert(split_exp(0x3f800000u) == 14, "1.0f -> 2^14");
static_assert(split_exp(0x46ffffffu) == 0, "the largest float below 2^15 stays");
static_assert(split_exp(0x00000001u) == 100, "the smallest subnormal: clamped");
static_assert(split_exp(0x7f800000u) == -100, "+inf: clamped");

// 2^e of a max word, and alpha 2^-(e0 + e1) for the epilogue of a product of two split operands (dconv.hip writes the
// latter out: through this function its MFMA kernels' instruction schedules came out different)
__device__ inline float split_scale(uint32_t maxbits) { return __builtin_ldexpf(1.f, split_exp(maxbits)); }
__device__ inline float split_unscale(float alpha, uint32_t maxbits0, uint32_t maxbits1) {
    return __builtin_ldexpf(alpha, -(split_exp(maxbits0) + split_exp(maxbits1)));
}

// hi = fp16(sv), lo = fp16(sv - hi) of an already scaled value sv = x 2^e: as fp16 values (typed LDS images) ...
__device__ inline void split16(float sv, _Float16& hi, _Float16& lo) {
    const _Float16 h = (_Float16)sv;
    hi = h;
    lo = (_Float16)(sv - (float)h);
}
// ... or as their bits
__device__ inline void split16(float sv, uint16_t& hi, uint16_t& lo) {
    _Float16 h, l;
    split16(sv, h, l);
    hi = __builtin_bit_cast(uint16_t, h);
    lo = __builtin_bit_cast(uint16_t, l);
}
// two scaled values -> the packed hi word (returned) and lo word, element 0 in the low half
__device__ inline uint32_t split_pair(float s0, float s1, uint32_t& lo) {
    uint16_t h0, h1, l0, l1;
    split16(s0, h0, l0);
    split16(s1, h1, l1);
    lo = (uint32_t)l0 | ((uint32_t)l1 << 16);
    return (uint32_t)h0 | ((uint32_t)h1 << 16);
}
__device__ inline uint32_t split_pair(float x0, float x1, float sc, uint32_t& lo) {
    return split_pair(x0 * sc, x1 * sc, lo);
}

// ---------------------------------------------------------------- max of float bits
__device__ inline uint32_t wave_max_bits(uint32_t b) {
    for (int o = 32; o >= 1; o >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, o, 64));
    return b;
}
template <int N>
__device__ inline uint32_t max_of_words(const uint32_t* r) {
    if constexpr (N == 1) return r[0];
    else return max(max_of_words<N / 2>(r), max_of_words<N - N / 2>(r + N / 2));
}
// Workgroup maximum of m >= 0 as float bits, for a workgroup of NW waves; called by every thread.  red: NW LDS words
// of the caller's.  First step of both forms below: every wave's maximum into red, then a barrier.
__device__ inline void block_wave_maxima(float m, uint32_t* red) {
    const uint32_t b = wave_max_bits(__float_as_uint(m));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
}
// The maximum, returned to thread 0 only (ALL = false: the other threads get 0) or to every thread (ALL = true).  What
// becomes of a zero maximum is the caller's business.
template <int NW, bool ALL = false>
__device__ inline uint32_t block_max_bits(float m, uint32_t* red) {
    block_wave_maxima(m, red);
    return (ALL || threadIdx.x == 0) ? max_of_words<NW>(red) : 0u;
}
// One atomicMax of the maximum into *out by thread 0.  A zero maximum is not sent (a word reset to 0 stays untouched by
// all-zero data) unless ZERO_TOO.
template <int NW, bool ZERO_TOO = false>
__device__ inline void block_max_publish(float m, uint32_t* red, uint32_t* out) {
    block_wave_maxima(m, red);
    if (threadIdx.x == 0) {
        const uint32_t b = max_of_words<NW>(red);
        if (ZERO_TOO || b) atomicMax(out, b);
    }
}

}  // namespace avse
