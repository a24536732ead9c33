// Forward and input gradient of the avse1 AudioFeatNet dilated convolutions for gfx950, as an implicit GEMM on the
// fp16 MFMA with fp32-accurate split operands ("fp16x3").
//
// Replaces the forward and the data-gradient halves of nn.Conv2d(64, 64, 5, padding=2d, dilation=d), d = 2, 4, 8, 16 —
// conv2..conv5 of /root/reference/baseline/avse1/model.py:199-215 (AudioFeatNet, built in the loop at :202-209).  MIOpen
// ran them at 0.6-0.8 of the fp32 MFMA peak (29 + 27 ms of the 145 ms avse1 C2 step, profiles/r04p_*).
//
//   Y[n][h][w][o] = sum_{i,kh,kw} X[n][h + d (kh - 2)][w + d (kw - 2)][i] * W[o][i][kh][kw]      (0 outside the image)
//   input gradient: the same with X = dY and W'[o = ci][i = co][kh][kw] = W[co][ci][4 - kh][4 - kw]
//
// Precision: the fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the f16 rate.  Each fp32 operand is split into
// two fp16 values after a power-of-two scale 2^e that puts the tensor's max |x| in [2^14, 2^15):
//   hi = fp16(x 2^e), lo = fp16(x 2^e - hi)        (22 significant bits; hi <= 2^15 cannot overflow)
// and each product is formed as hi*hi + hi*lo + lo*hi: three v_mfma_f32_32x32x16_f16 (exact 22-bit products, fp32
// accumulation), dropping lo*lo (2^-22 of the product).  The representation error (2^-22 relative per operand) is below
// the fp32 accumulation error of a K = 1600 dot product, so the result has fp32 accuracy at 16/3 = 5.3x the fp32 MFMA
// rate.  Elements far below the tensor's max keep an absolute error of 2^-25 of the scaled unit (fp16 subnormals).
//
// Operands: X (and dY) are split once into the "Q4" layout: per pixel 4 channel quarters of 64 B = [hi 16 ci][lo 16 ci]
// (avse_split16: absmax pass, then the split; the same 256 B per pixel as fp32).  W is split into
// [stage = kh * 4 + quarter][kw][o][hi 16 | lo 16] (avse_dconv_wprep), 20 KB per stage.
//
// Work decomposition: workgroup = 256 consecutive output pixels of one image in raster order (they span one row or
// the end of one and the start of the next, W = 257 > 256) x all 64 output channels; 4 waves, wave w = pixels
// 64 w .. 64 w + 63 (2 MFMA blocks) x 64 channels (2 blocks): 64 accumulators per lane.  The reduction runs in 20
// stages (kernel row kh x channel quarter q); per stage the input segment is staged once for all 5 kw taps: the tile's
// pixels of row h, shifted by d (kh - 2), with the 2d halo on both sides, at LDS positions 0 .. nA + 4d, and for a
// two-row tile the next row's pixels behind a 4d gap, so that output pixel j reads position pos(j) + d kw for tap kw
// (pos(j) = j, or j + 4d in the second row) and the halo columns outside the image stage as zeros.  Per stage and
// wave: 5 taps x 2 x 2 blocks x 3 products = 60 MFMAs on 8 fragment reads per tap.  Stages are staged HBM/L2 -> LDS
// by LDS-DMA (buffer_load_dwordx4 ... lds, out-of-image pixels read past the buffer range and land as 0) into a ring
// of 3 buffers, issued 2 stages ahead; one barrier per stage.  LDS rows are 64 B with the 16-B chunk c of row r at
// c ^ ((r >> 2) & 3), so the 16 lanes of a ds_read_b128 group read 16 distinct bank slots.
#include <algorithm>

#include "bnact_cols.h"
#include "common.h"
#include "split16.h"

namespace avse {
namespace dcf {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int C = 64, KS = 5, NQ = 4, TP = 256, THREADS = 256, WAVES = THREADS / 64;
constexpr int ROWB = 64;                       // LDS bytes per staged row (position or W row): hi 16 | lo 16 channels
constexpr int WIMG = KS * C * ROWB;            // one stage's W image: 5 taps x 64 output channels (20 KB)
constexpr int NSTG = KS * NQ;                  // stages per tile
constexpr int MAXD = 16;
constexpr int XIMG_MAX = (TP + 8 * MAXD) * ROWB;
constexpr int STAGE = XIMG_MAX + WIMG;         // ring slot (44 KB)
constexpr int NBUF = 3;
constexpr int MAXP = (XIMG_MAX + WIMG) / 1024 / WAVES + 1;   // LDS-DMA pieces per wave and stage (<= 11)
static_assert(NBUF * STAGE <= 160 * 1024, "LDS");

__device__ inline int swz(int r) { return (r >> 2) & 3; }

// s_waitcnt vmcnt(n) for a wave-uniform n in 0 .. 12 (the immediate must be a constant)
__device__ inline void wait_all_but(int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    }
}

__device__ inline half8 frag(const uint8_t* img, int row, int c) {
    return *reinterpret_cast<const half8*>(img + row * ROWB + 16 * (c ^ swz(row)));
}

struct Args {
    const void* xq;              // Q4 split input (n_pix x 256 B)
    const void* wq;              // prepped weights (NSTG x WIMG)
    const uint32_t* maxbits;     // [0] = max |x| bits, [1] = max |w| bits
    const float* bias;           // (64) or NULL
    float* y;                    // NHWC fp32
    int N, H, W, tiles;          // tiles per image
    bnact::BnEpi bn;             // EPI launches only (input gradient of a conv whose input is ReLU(BN(bn.x)))
};

// NW waves, tile = TP = 64 NW raster pixels spanning up to NSEG rows (W >= 256): row segment k of the tile sits at LDS
// positions S_k .. S_k + n_k + 4 D (its n_k pixels with the 2 D halo each side), S_k = n_0 + .. + n_{k-1} + 4 D k, so
// output pixel j of segment k reads position j + 4 D k + D kw for tap kw.
// WGS workgroups per CU: 2 (NW = 4) takes 2 LDS buffers, so that two workgroups fit; 1: 3 buffers where they fit.
// EPI (input-gradient launches; 0: none, the forward's code): the tile's BatchNorm-backward partials of
// y = ReLU(BN(a.bn.x)) with dy = this kernel's output (bnact_cols.h), one row a.bn.rows[workgroup] per tile, NQ = 3
// (EPI = 1) or 4 (EPI = 2: with max |dz|) quantities.
template <int D, int NW, int WGS = 1, int EPI = 0>
__global__ __launch_bounds__(64 * NW, WGS) void fwd_kernel(Args a) {
    constexpr int TPX = 64 * NW, NSEG = NW == 4 ? 2 : 3;
    constexpr int NP = (TPX + 4 * D * NSEG + 15) / 16 * 16;   // staged positions (whole 1-KB DMA pieces)
    constexpr int XIMG = NP * ROWB;
    constexpr int STG = XIMG + WIMG;
    constexpr int NB = WGS == 2 ? 2 : ((3 * STG <= 160 * 1024) ? 3 : 2);
    constexpr int PX = XIMG / 1024, PT = PX + WIMG / 1024;      // X pieces, all pieces of a stage
    constexpr int MP = PT / NW + 1;
    __shared__ __attribute__((aligned(1024))) uint8_t lds[NB * STG];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int n = bid / a.tiles, t = bid % a.tiles;
    const int HW = a.H * a.W;
    const int p0 = t * TPX;
    const int r0 = p0 / a.W, w0 = p0 - r0 * a.W;
    // pixels of the tile in its first, second and third row, and the segments' first positions
    const int n0 = min(TPX, a.W - w0), n1 = min(TPX - n0, a.W), n2 = TPX - n0 - n1;
    const int S1 = n0 + 4 * D, S2 = n0 + n1 + 8 * D;
    const i4_t rx = dma_rsrc(a.xq, (int64_t)a.N * HW * 256);
    const i4_t rw = dma_rsrc(a.wq, (int64_t)NSTG * WIMG);
    const uint32_t lds0 = lds_u32(lds);

    // this wave's LDS-DMA pieces of a stage: k = wave + NW m; X pieces (k < PX) carry the lane's position column (or -1
    // outside the image / the segments) and row; W pieces the lane's byte offset in the stage's W image
    int pcol[MP], prow[MP];
    uint32_t pchunk[MP];
    const int npieces = (PT - wave + NW - 1) / NW;
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        const int k = wave + NW * m;
        if (k < PX) {
            const int r = 16 * k + (lane >> 2), c = (lane & 3) ^ swz(r);
            int col, row;
            if (r < S1) {
                col = w0 - 2 * D + r;
                row = r0;
            } else if (r < S2 || NSEG == 2) {
                col = -2 * D + (r - S1);
                row = (n1 > 0 && r < S1 + n1 + 4 * D) ? r0 + 1 : -1000000;
            } else {
                col = -2 * D + (r - S2);
                row = (n2 > 0 && r < S2 + n2 + 4 * D) ? r0 + 2 : -1000000;
            }
            pcol[m] = (col >= 0 && col < a.W) ? col : -1;
            prow[m] = row;
            pchunk[m] = 16u * c;
        } else {
            const int r = 16 * (k - PX) + (lane >> 2), c = (lane & 3) ^ swz(r);
            pcol[m] = 0;
            prow[m] = 0;
            pchunk[m] = (uint32_t)(r * ROWB + 16 * c);
        }
    }
    auto issue = [&](int s) {
        const int kh = s / NQ, q = s % NQ;
        const uint32_t img = lds0 + (s % NB) * STG;
#pragma unroll
        for (int m = 0; m < MP; ++m) {
            if (m >= npieces) break;
            const int k = wave + NW * m;
            if (k < PX) {
                const int row = prow[m] + D * (kh - 2);
                const bool ok = pcol[m] >= 0 && row >= 0 && row < a.H;
                const uint32_t pix = ((uint32_t)n * (uint32_t)a.H + (uint32_t)row) * (uint32_t)a.W + (uint32_t)pcol[m];
                const uint32_t off = ok ? pix * 256u + (uint32_t)(q * 64) + pchunk[m] : 0x7FFFFFF0u;
                dma16(rx, img + k * 1024, off);
            } else {
                dma16(rw, img + XIMG + (k - PX) * 1024, (uint32_t)(s * WIMG) + pchunk[m]);
            }
        }
    };

    // the lane's fragment rows: output pixel j = 64 wave + 32 i + (lane & 31) reads position pos(j) + D kw
    int posA[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = 64 * wave + 32 * i + (lane & 31);
        posA[i] = j + 4 * D * ((j >= n0) + (j >= n0 + n1));
    }
    const int hc = lane >> 5;                   // fragment chunk: hi = hc, lo = 2 + hc

    floatx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    issue(0);
    if (NB == 3) issue(1);
    for (int s = 0; s < NSTG; ++s) {
        // this wave's stage-s pieces have landed (with 3 buffers stage s + 1 may still fly); the barrier makes that
        // hold for every wave and releases the buffer of stage s - 1 (3 buffers) or s - 1 = s + 1 (2 buffers)
        if (NB == 3 && s + 1 < NSTG) wait_all_but(npieces);
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (s + NB - 1 < NSTG) issue(s + NB - 1);
        const uint8_t* ximg = lds + (s % NB) * STG;
        const uint8_t* wimg = ximg + XIMG;
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
            half8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = posA[i] + D * kw;
                ah[i] = frag(ximg, r, hc);
                al[i] = frag(ximg, r, 2 + hc);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int r = kw * C + 32 * j + (lane & 31);
                bh[j] = frag(wimg, r, hc);
                bl[j] = frag(wimg, r, 2 + hc);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
        if (NB == 2) {                                 // the next issue refills this buffer: every wave must be done
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }

    // epilogue: acc[i][j] register 4 g + e = pixel 64 wave + 32 i + 8 g + 4 (lane >> 5) + e, channel 32 j + (lane & 31)
    const float scale = __builtin_ldexpf(1.f, -(split_exp(a.maxbits[0]) + split_exp(a.maxbits[1])));
    auto store = [&](int j) {
        const int o = 32 * j + (lane & 31);
        const float bv = a.bias ? a.bias[o] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int p = p0 + 64 * wave + 32 * i + 8 * g + 4 * (lane >> 5) + e;
                    const float v = acc[i][j][4 * g + e] * scale + bv;
                    if constexpr (EPI != 0) acc[i][j][4 * g + e] = v;      // the stored value, kept for the partials
                    if (p < HW) a.y[((int64_t)n * HW + p) * C + o] = v;
                }
    };
    if constexpr (EPI == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) store(j);
    } else {
        constexpr int ENQ = EPI == 2 ? 4 : 3;
        float* part = reinterpret_cast<float*>(lds);      // every wave is past its last fragment read (lgkmcnt(0) or
        __syncthreads();                                  // the MFMAs' operands) before the staging ring is reused
        bnact::bn_epi_wave<bnact::ACT_RELU, EPI == 2>(
            a.bn, [&](int i, int j, int r) { return acc[i][j][r]; }, store, (int64_t)n * HW + p0 + 64 * wave,
            (int64_t)(n + 1) * HW, 0, C, lane, part + wave * ENQ * 64);
        __syncthreads();
        bnact::bn_epi_row<EPI == 2>(a.bn, part, NW, 1, (int64_t)bid, 0, C);
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// dW[o][i][kh][kw] = sum_{n,h,w} dY[n][h][w][o] X[n][h + d (kh - 2)][w + d (kw - 2)][i] from the two Q4-split operands
// (X split in the forward, dY for the input gradient), scaled back by 2^-(e_dy + e_x).  Per-tap GEMM with M = o, N = i
// and the reduction over pixels.  Both operands are contiguous along the GEMM's M / N (channels), so the fragments are
// read with ds_read_b64_tr_b16 (4 pixels x 16 channels per 16-lane group, delivered transposed) from swizzled pixel
// rows.  One more MFMA pair per k-step against a ones fragment gives the bias gradient db[o] = sum dY[.][o].  Partial
// slabs per workgroup pair, summed in a fixed order by a second kernel (deterministic).
constexpr int WG_CHUNK = 64;                     // pixels per column chunk (4 k-steps of 16); the narrowest row
constexpr int PIXB = 256;                        // LDS / Q4 bytes per pixel

typedef short s4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s4_t lds_s4_t;

// 16-B chunk c of staged pixel row r sits at physical chunk tswz(r, c).  A transposed fragment read (LaneOff) takes, per
// 32-lane half, 4 consecutive rows x 4 chunks whose logical indices differ in bits 0 and 2; the rows' XOR masks must
// then differ in bits 1 and 3 for the 16 (row, chunk) pairs to land on 16 distinct 4-bank groups (every row starts on
// bank 0: 256-B rows).  Round 5's mask ((r & 3) << 2) moved bits 2-3 only: 2-way conflicts on every read
// (SQ_LDS_BANK_CONFLICT = 0.5 x SQ_LDS_IDX_ACTIVE, gpurun_out/r06f_pmc_dconv); this one is conflict-free.
__device__ inline int tswz(int r, int c) { return c ^ (((r & 1) << 1) | ((r & 2) << 2)); }

// dW[o][i][kh][kw] = sum over slabs of part[slab][kh][kw][o][i]; db[o] = sum over slabs of dbpart[slab][o] (summed
// in order: deterministic)
__global__ void wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ dbpart, int slabs,
                                    float* __restrict__ dw, float* __restrict__ db) {
    constexpr int TOTAL = KS * KS * C * C;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= TOTAL) {
        if (db != nullptr && idx < TOTAL + C) {
            float v = 0.f;
            for (int g = 0; g < slabs; ++g) v += dbpart[(int64_t)g * C + idx - TOTAL];
            db[idx - TOTAL] = v;
        }
        return;
    }
    float v = 0.f;
    for (int g = 0; g < slabs; ++g) v += part[(int64_t)g * TOTAL + idx];
    const int i = idx % C, o = (idx / C) % C, kw = (idx / (C * C)) % KS, kh = idx / (KS * C * C);
    dw[((o * C + i) * KS + kh) * KS + kw] = v;
}


// ------------------------------------------------------------------- weight gradient, rows walked in steps of d
// The same sums from a walk in which every input segment and every dY segment is staged once for all 25 taps.  Output
// rows rho, rho + d, rho + 2 d, ... of one residue class rho = h mod d need input rows of that class only, and each
// needs exactly one row its predecessor did not: row h + 2 d.
//   unit  = (image n, residue class rho, column chunk, input-channel half ib); a column chunk is 64 columns, the last
//           one the rest of the row, or 64 + the rest where the rest is <= 16 columns (W = 257: 64, 64, 64, 65), so a
//           chunk has 1 .. 5 k-steps of 16 pixels;
//   step  = output row h = rho + t d of the unit: the chunk's dY pixels (256 B each, one of 2 buffers) against the five
//           input segments of rows h - 2 d .. h + 2 d, columns w0 - 2 d .. w0 + 16 ks + 2 d, the ib half only (128 B
//           per position), which sit in a ring of 6 slots: row index tau = t + kh - 2 of the class in slot (tau + 2)
//           mod 6.  Output pixel j reads position j + d kw of the slot of its kernel row.  While step t computes, the
//           one new segment of step t + 1 (row index t + 3, into the slot step t - 1 read last) and the next dY
//           segment are staged; their LDS-DMA pieces are issued between the MFMAs of the wave's first k-step.
// Rows and columns outside the image, and dY pixels beyond the chunk's width (the dead pixels of a partial k-step),
// are staged through the out-of-range offset and land as zeros: every byte a fragment reads was written by the DMA of
// the step or unit that reads it, nothing is assumed of the LDS contents, and a unit restarts the ring (5 segments).
// Workgroups are persistent: workgroup b (after xcd_remap) takes units b, b + G, b + 2 G, ... of the list ordered
// (n, rho, chunk, ib), ib fastest, so that at any time 8 neighbouring workgroups of one XCD share one (n, rho)'s rows
// and dY in its L2.  G is even, so a workgroup keeps its ib.  4 waves, one per SIMD: wave = (o block of 32, tap set)
// owns 32 o x 32 i x 13 taps (0 .. 12: set 0) or 12 taps (13 .. 24: set 1, which also carries the bias gradient's ones
// fragment in the ib = 0 workgroups) over every k-step of the chunk: 156 / 152 MFMAs per wave behind each barrier at 64
// columns.  (One wave with all 25 taps over half the k-steps, 400 accumulators, does not build: with one wave per
// SIMD hipcc places MFMA accumulators in the 256 AGPRs only and copies the rest in and out around every MFMA; 13
// tiles + the bias tile are 224.)  The workgroup writes the ib columns of slab b / 2; wgrad_reduce_kernel sums the
// G / 2 slabs in order: no atomics.
namespace rows {

constexpr int RTHREADS = 256;
constexpr int XPIXB = 128;                       // ring bytes per input position (one input-channel half)
constexpr int CWMAX = 80;                        // widest column chunk: 5 k-steps
constexpr int NSLOT = 6;
constexpr int YBUF = CWMAX * PIXB;               // one dY buffer (20 KB)
constexpr int TAPS0 = 13;                        // taps of set 0; set 1 takes the other 12
constexpr int MAXWG = 256;                       // one workgroup per CU

constexpr int slot_bytes(int D) { return (CWMAX + 4 * D) * XPIXB; }
constexpr int lds_bytes(int D) { return NSLOT * slot_bytes(D) + 2 * YBUF; }
static_assert(lds_bytes(MAXD) <= 160 * 1024, "LDS");
static_assert(slot_bytes(2) % 1024 == 0, "whole DMA pieces");

// column chunks of a row of W >= 64 columns; chunk c starts at 64 c, the last one ends the row
inline __host__ __device__ int chunks_of(int W) { return W / 64 + (W % 64 > 16 ? 1 : 0); }

struct Plan {
    int nck, nwg, slabs, lds;
    int64_t units, steps, pieces;
};

// The static plan of a launch.  pieces = 1-KB LDS-DMA wave-instructions: a unit of T > 0 steps stages 5 input
// segments and T - 1 more (npx = (16 ks + 4 D) / 8 pieces each) and T dY segments (4 ks pieces); empty units stage
// nothing.
inline Plan make_plan(int64_t N, int64_t H, int64_t W, int D) {
    Plan p;
    p.nck = chunks_of((int)W);
    p.units = N * p.nck * D * 2;
    p.nwg = (int)std::min<int64_t>(MAXWG, p.units);
    p.slabs = p.nwg / 2;
    p.lds = lds_bytes(D);
    p.steps = 0;
    p.pieces = 0;
    for (int c = 0; c < p.nck; ++c) {
        const int cw = c == p.nck - 1 ? (int)W - 64 * c : 64, ks = (cw + 15) / 16, npx = (16 * ks + 4 * D) / 8;
        for (int rho = 0; rho < D; ++rho) {
            const int64_t T = rho < H ? (H - rho + D - 1) / D : 0;
            if (T == 0) continue;
            p.steps += 2 * N * T;
            p.pieces += 2 * N * ((T + 4) * npx + T * 4 * ks);
        }
    }
    return p;
}

struct RArgs {
    const void* xq;
    const void* dyq;
    const uint32_t* xmax;
    const uint32_t* dymax;
    float* part;                 // [slabs][kh][kw][o][i]
    float* dbpart;               // [slabs][o] or NULL
    int N, H, W, nck, units;
};

// The lane's addresses of the MFMA operand fragments (32 channels x 16 pixels), as LDS byte offsets: a k-step adds one
// wave-uniform base per kernel row and the tap's columns ride in the instruction's offset field.  Lane l (g = l >> 4,
// i = l & 15)
// reads pixel p_u = 8 (g >> 1) + (i >> 2) + 4 u of the k-step, u = 0, 1, channels 16 (g & 1) + 4 (i & 3) .. + 3 of its
// 32-channel block, plane pl (0 hi, 1 lo):
//   y[u][pl]: dY buffer, 256-B pixels, tswz (the block is ob); + 4096 s for k-step s (16 pixels: p & 3 unchanged);
//   x[u][pl]: ring slot, 128-B positions (quarters 0, 1 of the unit's ib half) whose 16-B chunk c sits at c ^ (r & 2);
//             + 128 (16 s + d kw) for k-step s and tap column kw.  d kw is even: where it has bit 1 set (d = 2, kw odd)
//             the position's mask flips, which is the other plane's address: chunk c = 4 (g & 1) + 2 pl + (i & 3) / 2.
// A 32-lane half reads 4 consecutive positions x 4 chunks that differ in bits 0 and 2; even and odd positions lie in
// opposite halves of the 256-B bank row and the mask separates the two of each parity: conflict-free, as tswz is.
struct LaneOff {
    uint32_t x[2][2], y[2][2];
    __device__ void init(int lane, int ob) {
        const int g = lane >> 4, i = lane & 15;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const int p = 8 * (g >> 1) + (i >> 2) + 4 * u;
                const int bx = (g & 1) * 64 + pl * 32 + 8 * (i & 3);
                x[u][pl] = (uint32_t)(p * XPIXB + 16 * ((bx >> 4) ^ (p & 2)) + (bx & 15));
                const int by = (2 * ob + (g & 1)) * 64 + pl * 32 + 8 * (i & 3);
                y[u][pl] = (uint32_t)(p * PIXB + 16 * tswz(p, by >> 4) + (by & 15));
            }
    }
};

template <int OFF>
__device__ __forceinline__ half8 frag2(uint32_t a0, uint32_t a1) {
    const s4_t w0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(uintptr_t)(a0 + OFF));
    const s4_t w1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(uintptr_t)(a1 + OFF));
    const short __attribute__((ext_vector_type(8))) w = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
    return __builtin_bit_cast(half8, w);
}

// the fragments a k-step starts from: its dY (A) pair and the input (B) pair of its first tap
struct Frags {
    half8 ah, al, bh, bl;
};

__device__ __forceinline__ void load_a(const LaneOff& lo, uint32_t ybase, half8& ah, half8& al) {
    ah = frag2<0>(ybase + lo.y[0][0], ybase + lo.y[1][0]);
    al = frag2<0>(ybase + lo.y[0][1], ybase + lo.y[1][1]);
}

// tap TAP's input pair: xb = the k-step's first position in the slot of the tap's kernel row.  The tap's column offset
// is a constant of the instruction; (d kw) & 2 swaps the planes' addresses (LaneOff)
template <int D, int TAP>
__device__ __forceinline__ void load_b(const LaneOff& lo, const uint32_t (&xbase)[KS], half8& bh, half8& bl) {
    constexpr int KH = TAP / KS, KW = TAP % KS, F_ = ((D * KW) >> 1) & 1, O_ = D * KW * XPIXB;
    const uint32_t xb = xbase[KH];
    bh = frag2<O_>(xb + lo.x[0][F_], xb + lo.x[1][F_]);
    bl = frag2<O_>(xb + lo.x[0][1 - F_], xb + lo.x[1][1 - F_]);
}

// One k-step, taps T0 .. T1 - 1 (accumulators acc[tap - T0]): ybase / xbase[kh] = LDS addresses of the k-step's first
// dY pixel and of its first position in kernel row kh's slot.  One wave per SIMD has nobody to hide its LDS latency, so
// the fragments run one tap ahead: f holds the k-step's first fragments on entry; every tap reads the next tap's input
// pair before its own three MFMAs, and the last tap reads the next k-step's first fragments into f (has_next).
// piece(k), k = 0 .. 9, issues the wave's k-th staging piece of the next step behind tap T0 + k (ISSUE only).
template <int D, int T0, int T1, bool ISSUE, typename F>
__device__ __forceinline__ void kstep(floatx16 (&acc)[TAPS0], floatx16& accb, const LaneOff& lo, uint32_t ybase,
                                      const uint32_t (&xbase)[KS], bool want_db, F&& piece, Frags& f, bool has_next) {
    const half8 ah = f.ah, al = f.al;
    half8 bh = f.bh, bl = f.bl;
#pragma unroll
    for (int tap = T0; tap < T1; ++tap) {
        half8 nh = bh, nl = bl;
        if (tap + 1 < T1) {
            // (the unrolled loop's tap is a constant; the switch names it for the template argument)
#define AVSE_ROWS_NEXT(K) case T0 + K: load_b<D, (T0 + K + 1 < KS * KS ? T0 + K + 1 : 0)>(lo, xbase, nh, nl); break;
            switch (tap) {
                AVSE_ROWS_NEXT(0) AVSE_ROWS_NEXT(1) AVSE_ROWS_NEXT(2) AVSE_ROWS_NEXT(3) AVSE_ROWS_NEXT(4)
                AVSE_ROWS_NEXT(5) AVSE_ROWS_NEXT(6) AVSE_ROWS_NEXT(7) AVSE_ROWS_NEXT(8) AVSE_ROWS_NEXT(9)
                AVSE_ROWS_NEXT(10) AVSE_ROWS_NEXT(11)
                default: break;
            }
#undef AVSE_ROWS_NEXT
        } else if (has_next) {
            uint32_t xn[KS];
#pragma unroll
            for (int kh = 0; kh < KS; ++kh) xn[kh] = xbase[kh] + 16 * XPIXB;
            load_a(lo, ybase + 16 * PIXB, f.ah, f.al);
            load_b<D, T0>(lo, xn, f.bh, f.bl);
        }
        __builtin_amdgcn_sched_barrier(0);
        acc[tap - T0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[tap - T0], 0, 0, 0);
        acc[tap - T0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[tap - T0], 0, 0, 0);
        acc[tap - T0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[tap - T0], 0, 0, 0);
        if constexpr (ISSUE) {
            if (tap - T0 < 10) piece(tap - T0);
        }
        bh = nh;
        bl = nl;
    }
    if (want_db) {
        half8 ones;
#pragma unroll
        for (int e = 0; e < 8; ++e) ones[e] = (_Float16)1.0f;
        accb = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ones, accb, 0, 0, 0);
        accb = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, ones, accb, 0, 0, 0);
    }
}

// a wave's whole launch, TS = its tap set (a template parameter: the two sets' code shares no accumulator registers)
template <int D, int TS>
__device__ __forceinline__ void wave_body(const RArgs& a, uint8_t* lds, int wave, int lane) {
    constexpr int SLOTB = slot_bytes(D), RING = NSLOT * SLOTB;
    constexpr int T0 = TS == 0 ? 0 : TAPS0, T1 = TS == 0 ? TAPS0 : KS * KS, ts = TS;
    const int nwg = gridDim.x;                                    // even
    const int bid = xcd_remap(blockIdx.x, nwg);
    const int ib = bid & 1, ob = wave & 1;                       // input-channel half, o block
    const int HW = a.H * a.W;
    const i4_t rx = dma_rsrc(a.xq, (int64_t)a.N * HW * PIXB);
    const i4_t ry = dma_rsrc(a.dyq, (int64_t)a.N * HW * PIXB);
    const uint32_t lds0 = lds_u32(lds);
    // the lane's share of a staging piece.  dY piece 4 m + wave: pixel 16 m + ypx0 (4 pixels x 16 chunks per piece);
    // input piece 4 m + wave: position 32 m + xpos0 (8 positions x 8 chunks); the swizzles do not depend on m
    const int ypx0 = 4 * wave + (lane >> 4), xpos0 = 8 * wave + (lane >> 3);
    const uint32_t ysw = 16u * tswz(lane >> 4, lane & 15);
    const uint32_t xsw = (uint32_t)(ib * XPIXB) + 16u * ((lane & 7) ^ ((lane >> 3) & 2));
    const bool want_db = TS == 1 && a.dbpart != nullptr && ib == 0;
    LaneOff lo;
    lo.init(lane, ob);

    floatx16 acc[TAPS0], accb;
#pragma unroll
    for (int k = 0; k < TAPS0; ++k)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[k][e] = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) accb[e] = 0.f;

    for (int u = bid; u < a.units; u += nwg) {
        int rest = u >> 1;
        const int cc = rest % a.nck;
        rest /= a.nck;
        const int rho = rest % D, n = rest / D;
        const int T = rho < a.H ? (a.H - rho + D - 1) / D : 0;
        if (T == 0) continue;
        const int w0 = 64 * cc, cw = cc == a.nck - 1 ? a.W - w0 : 64;
        const int ks = (cw + 15) >> 4, npx = (16 * ks + 4 * D) >> 3;
        const int nH = n * a.H;
        // dY piece m of row index t into buffer t & 1; input piece m of row index tau into its slot
        auto dma_y = [&](int m, int t) {
            const int px = ypx0 + 16 * m;
            const int pix = (nH + rho + t * D) * a.W + w0 + px;
            dma16(ry, lds0 + RING + (t & 1) * YBUF + (wave + 4 * m) * 1024,
                  px < cw ? (uint32_t)pix * PIXB + ysw : 0x7FFFFFF0u);
        };
        auto dma_x = [&](int m, int tau, int slot) {
            const int row = rho + tau * D, col = w0 - 2 * D + xpos0 + 32 * m;
            const bool ok = tau >= 0 && row < a.H && (unsigned)col < (unsigned)a.W;
            const int pix = (nH + row) * a.W + col;
            dma16(rx, lds0 + slot * SLOTB + (wave + 4 * m) * 1024, ok ? (uint32_t)pix * PIXB + xsw : 0x7FFFFFF0u);
        };
        // restart the ring: every wave is past the previous unit's last fragment read, nothing is in flight
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#pragma unroll 1
        for (int tau = -2; tau <= 2; ++tau)
            for (int m = 0; wave + 4 * m < npx; ++m) dma_x(m, tau, tau + 2);
        for (int m = 0; m < ks; ++m) dma_y(m, 0);
        int s0 = 0;                                              // slot of row index t - 2
#pragma unroll 1
        for (int t = 0; t < T; ++t) {
            // everything staged for this step has landed (this wave's pieces; the barrier: every wave's), and every
            // wave is past step t - 1, whose slot and dY buffer the pieces issued below overwrite
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            int sb[KS];
#pragma unroll
            for (int kh = 0; kh < KS; ++kh) sb[kh] = (s0 + kh >= NSLOT ? s0 + kh - NSLOT : s0 + kh) * SLOTB;
            const int snew = s0 + 5 >= NSLOT ? s0 + 5 - NSLOT : s0 + 5;
            const bool more = t + 1 < T;
            auto piece = [&](int k) {
                if (!more) return;
                const int m = k >> 1;
                if (k & 1) {
                    if (wave + 4 * m < npx) dma_x(m, t + 3, snew);
                } else {
                    if (m < ks) dma_y(m, t + 1);
                }
            };
            const uint32_t ybuf = lds0 + RING + (t & 1) * YBUF;
            // k-step s: dY pixels 16 s .. 16 s + 15 and, in every slot, the positions from 16 s on; the next step's
            // pieces go out behind the taps of k-step 0
            uint32_t xb[KS];
#pragma unroll
            for (int kh = 0; kh < KS; ++kh) xb[kh] = lds0 + sb[kh];
            Frags f;
            load_a(lo, ybuf, f.ah, f.al);
            load_b<D, T0>(lo, xb, f.bh, f.bl);
            kstep<D, T0, T1, true>(acc, accb, lo, ybuf, xb, want_db, piece, f, ks > 1);
#pragma unroll 1
            for (int s = 1; s < ks; ++s) {
#pragma unroll
                for (int kh = 0; kh < KS; ++kh) xb[kh] += 16 * XPIXB;
                kstep<D, T0, T1, false>(acc, accb, lo, ybuf + s * 16 * PIXB, xb, want_db, piece, f, s + 1 < ks);
            }
            s0 = s0 + 1 >= NSLOT ? 0 : s0 + 1;
        }
    }

    // acc[k] = tap 13 ts + k; register 4 q + e = row o = 32 ob + 8 q + 4 (lane >> 5) + e, column i = 32 ib +
    // (lane & 31)
    const float sc = __builtin_ldexpf(1.f, -(split_exp(*a.xmax) + split_exp(*a.dymax)));
    float* pp = a.part + ((int64_t)(bid >> 1) * KS * KS + TAPS0 * ts) * C * C;
#pragma unroll
    for (int k = 0; k < TAPS0; ++k) {
        if (k < T1 - T0) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int o = 32 * ob + 8 * q + 4 * (lane >> 5) + e, i = 32 * ib + (lane & 31);
                    pp[((int64_t)k * C + o) * C + i] = acc[k][4 * q + e] * sc;
                }
        }
    }
    if (want_db && (lane & 31) == 0) {
        const float sd = __builtin_ldexpf(1.f, -split_exp(*a.dymax));
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                a.dbpart[(int64_t)(bid >> 1) * C + 32 * ob + 8 * q + 4 * (lane >> 5) + e] = accb[4 * q + e] * sd;
    }
}

template <int D>
__global__ __launch_bounds__(RTHREADS, 1) void wgrad_rows_kernel(RArgs a) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds[lds_bytes(D)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave < 2) wave_body<D, 0>(a, lds, wave, lane);
    else wave_body<D, 1>(a, lds, wave, lane);
}

}  // namespace rows

// ------------------------------------------------------------------------------------------------ operand preparation
// max |x| over n floats -> atomicMax on the float bits (split16.h), one per 1024-thread workgroup of a 256-workgroup
// grid: one per wave of a 2048 x 256 grid cost ~140 us of a 165 us pass (profiles/r05v3_avse1_timed_window_stats.csv)
constexpr int AMAX_NT = 1024, AMAX_GRID = 256;
__global__ __launch_bounds__(AMAX_NT) void absmax_kernel(const float4* x, int64_t n4, uint32_t* out) {
    __shared__ uint32_t red[AMAX_NT / 64];
    float m = 0.f;
    const int64_t stride = (int64_t)gridDim.x * AMAX_NT;
    for (int64_t i0 = blockIdx.x * (int64_t)AMAX_NT + threadIdx.x; i0 < n4; i0 += 4 * stride) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i0 + u * stride < n4 ? x[i0 + u * stride] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) m = fmaxf(m, fmaxf(fmaxf(fabsf(v[u].x), fabsf(v[u].y)), fmaxf(fabsf(v[u].z), fabsf(v[u].w))));
    }
    block_max_publish<AMAX_NT / 64>(m, red, out);
}

// NHWC fp32 (n_pix x 64) -> Q4 (n_pix x 4 quarters x [hi 16 | lo 16] fp16); thread = one (pixel, quarter)
__global__ void split_kernel(const float* x, int64_t nq, const uint32_t* maxbits, uint4* xq) {
    const float sc = split_scale(maxbits[0]);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
        const float4* s = reinterpret_cast<const float4*>(x + i * 16);
        uint32_t hi[8], lo[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = s[k];
            hi[2 * k] = split_pair(v.x, v.y, sc, lo[2 * k]);
            hi[2 * k + 1] = split_pair(v.z, v.w, sc, lo[2 * k + 1]);
        }
        uint4* d = xq + i * 4;
        d[0] = uint4{hi[0], hi[1], hi[2], hi[3]};
        d[1] = uint4{hi[4], hi[5], hi[6], hi[7]};
        d[2] = uint4{lo[0], lo[1], lo[2], lo[3]};
        d[3] = uint4{lo[4], lo[5], lo[6], lo[7]};
    }
}

// W (64 o, 64 i, 5, 5) fp32 -> [kh * 4 + q][kw][o][hi 16 | lo 16]; transposed = the input gradient's W'[o][i][kh][kw] =
// W[i][o][4 - kh][4 - kw].  One workgroup: max |w| first, then the split with that scale.
__global__ __launch_bounds__(1024) void wprep_kernel(const float* w, int transposed, uint32_t* maxbits, uint16_t* wq) {
    __shared__ uint32_t red[16];
    constexpr int TOT = C * C * KS * KS;
    float m = 0.f;
    for (int i = threadIdx.x; i < TOT; i += blockDim.x) m = fmaxf(m, fabsf(w[i]));
    const uint32_t b = block_max_bits<16, true>(m, red);        // the launch is 1024 threads
    if (threadIdx.x == 0) maxbits[1] = b;                       // a plain store: a zero maximum is published too
    const float sc = split_scale(b);
    // destination element e: stage s = kh * 4 + q, kw, o, plane, c (16)
    for (int e = threadIdx.x; e < TOT; e += blockDim.x) {
        const int c = e % 16, o = (e / 16) % C, kw = (e / (16 * C)) % KS, s = e / (16 * C * KS);
        const int kh = s / NQ, q = s % NQ, i = q * 16 + c;
        const float v = transposed ? w[((i * C + o) * KS + (KS - 1 - kh)) * KS + (KS - 1 - kw)]
                                   : w[((o * C + i) * KS + kh) * KS + kw];
        const int64_t row = ((int64_t)s * KS + kw) * C + o;
        split16(v * sc, wq[row * 32 + c], wq[row * 32 + 16 + c]);
    }
}

// The same images from one launch of NSTG workgroups per orientation (blockIdx.x = orientation * NSTG + stage): every
// workgroup recomputes max |w| from the 400-KB tensor (L2-resident after the first) and writes its own stage's 20 KB;
// orientation 1 is the transposed image under the same max.  The max is a maximum of the same values and the split
// the same expression, so the bytes equal wprep_kernel's.  Workgroup 0 publishes the max bits (mb0[1], mb1[1]).
__global__ __launch_bounds__(1024) void wprep2_kernel(const float* w, uint32_t* mb0, uint32_t* mb1, uint16_t* wq0,
                                                      uint16_t* wq1) {
    __shared__ uint32_t red[16];
    constexpr int TOT = C * C * KS * KS, PER = KS * C * 16;       // elements per stage
    float m = 0.f;
    for (int i = threadIdx.x; i < TOT; i += 1024) m = fmaxf(m, fabsf(w[i]));
    const uint32_t b = block_max_bits<16, true>(m, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) {                  // plain stores: a zero maximum is published too
        mb0[1] = b;
        if (mb1) mb1[1] = b;
    }
    const float sc = split_scale(b);
    const int transposed = blockIdx.x / NSTG, s = blockIdx.x % NSTG;
    uint16_t* wq = transposed ? wq1 : wq0;
    const int kh = s / NQ, q = s % NQ;
    for (int e = threadIdx.x; e < PER; e += 1024) {
        const int c = e % 16, o = (e / 16) % C, kw = e / (16 * C);
        const int i = q * 16 + c;
        const float v = transposed ? w[((i * C + o) * KS + (KS - 1 - kh)) * KS + (KS - 1 - kw)]
                                   : w[((o * C + i) * KS + kh) * KS + kw];
        const int64_t row = ((int64_t)s * KS + kw) * C + o;
        split16(v * sc, wq[row * 32 + c], wq[row * 32 + 16 + c]);
    }
}

}  // namespace dcf
}  // namespace avse

using namespace avse::dcf;

extern "C" {

int64_t avse_dconv_wprep_bytes(void) { return (int64_t)NSTG * WIMG; }

int avse_split16(int64_t n_pix, const float* x, void* xq, uint32_t* maxbits, avse_stream_t stream) {
    if (!x || !xq || !maxbits) return AVSE_EINVAL;
    if (n_pix <= 0) return AVSE_ESHAPE;
    if (((uintptr_t)x & 15) || ((uintptr_t)xq & 15)) return AVSE_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(maxbits, 0, 4, st) != hipSuccess) return AVSE_ELAUNCH;
    const int64_t n4 = n_pix * C / 4;
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(AMAX_GRID, (n4 + AMAX_NT - 1) / AMAX_NT))),
                       dim3(AMAX_NT), 0, st, reinterpret_cast<const float4*>(x), n4, maxbits);
    AVSE_CHECK_LAUNCH();
    const int64_t nq = n_pix * NQ;
    const int blocks = (int)std::min<int64_t>((nq + 255) / 256, 8192);
    hipLaunchKernelGGL(split_kernel, dim3(blocks), dim3(256), 0, st, x, nq, maxbits, reinterpret_cast<uint4*>(xq));
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

int avse_split16_known(int64_t n_pix, const float* x, void* xq, const uint32_t* maxbits, avse_stream_t stream) {
    if (!x || !xq || !maxbits) return AVSE_EINVAL;
    if (n_pix <= 0) return AVSE_ESHAPE;
    if (((uintptr_t)x & 15) || ((uintptr_t)xq & 15)) return AVSE_EALIGN;
    const int64_t nq = n_pix * NQ;
    const int blocks = (int)std::min<int64_t>((nq + 255) / 256, 8192);
    hipLaunchKernelGGL(split_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, nq, maxbits,
                       reinterpret_cast<uint4*>(xq));
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

int avse_dconv_wprep(const float* w, int32_t transposed, void* wq, uint32_t* maxbits, avse_stream_t stream) {
    if (!w || !wq || !maxbits) return AVSE_EINVAL;
    hipLaunchKernelGGL(wprep_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, w, transposed, maxbits,
                       reinterpret_cast<uint16_t*>(wq));
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

int avse_dconv_wprep2(const float* w, void* wq, void* wq_t, uint32_t* maxbits, uint32_t* maxbits_t,
                      avse_stream_t stream) {
    if (!w || !wq || !maxbits || (wq_t == nullptr) != (maxbits_t == nullptr)) return AVSE_EINVAL;
    hipLaunchKernelGGL(wprep2_kernel, dim3(wq_t ? 2 * NSTG : NSTG), dim3(1024), 0, (hipStream_t)stream, w, maxbits,
                       maxbits_t, reinterpret_cast<uint16_t*>(wq), reinterpret_cast<uint16_t*>(wq_t));
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

static bool wgrad16_shape_ok(int64_t N, int64_t H, int64_t W, int64_t dil) {
    if (N <= 0 || H <= 0 || W < WG_CHUNK || (dil != 2 && dil != 4 && dil != 8 && dil != 16)) return false;
    return N * H * W * 256 < (1LL << 31) - 1024;                // 32-bit byte offsets into the split operands
}

// the slab count does not fall with the dilation (more units), so dilation 16's covers every launch of the shape
int64_t avse_dconv_wgrad16_workspace_bytes(int64_t N, int64_t H, int64_t W) {
    if (!wgrad16_shape_ok(N, H, W, MAXD)) return 0;
    return 4 * (int64_t)rows::make_plan(N, H, W, MAXD).slabs * (KS * KS * C * C + C);
}

int avse_dconv_wgrad16_plan(int64_t N, int64_t H, int64_t W, int64_t dil, int64_t out[6]) {
    if (!out) return AVSE_EINVAL;
    if (!wgrad16_shape_ok(N, H, W, dil)) return AVSE_ESHAPE;
    const rows::Plan p = rows::make_plan(N, H, W, (int)dil);
    out[0] = p.units;
    out[1] = p.steps;
    out[2] = p.pieces;
    out[3] = p.slabs;
    out[4] = p.lds;
    out[5] = p.nwg;
    return AVSE_OK;
}

int avse_dconv_wgrad16(int64_t N, int64_t H, int64_t W, int64_t dil, const void* xq, const uint32_t* xmax,
                       const void* dyq, const uint32_t* dymax, float* dw, float* db, float* workspace,
                       avse_stream_t stream) {
    if (!xq || !xmax || !dyq || !dymax || !dw || !workspace) return AVSE_EINVAL;
    if (!wgrad16_shape_ok(N, H, W, dil)) return AVSE_ESHAPE;
    const rows::Plan p = rows::make_plan(N, H, W, (int)dil);
    rows::RArgs a;
    a.xq = xq;
    a.dyq = dyq;
    a.xmax = xmax;
    a.dymax = dymax;
    a.N = (int)N;
    a.H = (int)H;
    a.W = (int)W;
    a.nck = p.nck;
    a.units = (int)p.units;
    a.part = workspace;
    a.dbpart = db ? workspace + (int64_t)p.slabs * KS * KS * C * C : nullptr;
    const dim3 grid((unsigned)p.nwg), block(rows::RTHREADS);
    hipStream_t st = (hipStream_t)stream;
    switch (dil) {
        case 2: hipLaunchKernelGGL(rows::wgrad_rows_kernel<2>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(rows::wgrad_rows_kernel<4>, grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL(rows::wgrad_rows_kernel<8>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(rows::wgrad_rows_kernel<16>, grid, block, 0, st, a); break;
    }
    AVSE_CHECK_LAUNCH();
    constexpr int TOTAL = KS * KS * C * C;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((TOTAL + C + 255) / 256), dim3(256), 0, st, a.part, a.dbpart, p.slabs,
                       dw, db);
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

static inline int dcf_nw(int64_t dil) { return dil <= 8 ? 4 : 8; }

int64_t avse_dconv_bn_rows(int64_t N, int64_t H, int64_t W, int64_t dil) {
    if (N <= 0 || H <= 0 || W < 256) return 0;
    return N * ((H * W + 64 * dcf_nw(dil) - 1) / (64 * dcf_nw(dil)));
}

static int dconv_launch(int64_t N, int64_t H, int64_t W, int64_t dil, const void* xq, const void* wq,
                        const uint32_t* maxbits, const float* bias, float* y, const avse::bnact::BnEpi* bn, int epi,
                        avse_stream_t stream);

int avse_dconv_fwd(int64_t N, int64_t H, int64_t W, int64_t dil, const void* xq, const void* wq,
                   const uint32_t* maxbits, const float* bias, float* y, avse_stream_t stream) {
    return dconv_launch(N, H, W, dil, xq, wq, maxbits, bias, y, nullptr, 0, stream);
}

int avse_dconv_dgrad_bn(int64_t N, int64_t H, int64_t W, int64_t dil, const void* dyq, const void* wq_t,
                        const uint32_t* maxbits, float* dx, const float* bn_x, const float* bn_stats,
                        const float* gamma, const float* beta, int32_t act, int32_t want_max, float* rows,
                        avse_stream_t stream) {
    if (!bn_x || !bn_stats || !rows) return AVSE_EINVAL;
    if (act != avse::bnact::ACT_RELU) return AVSE_ESHAPE;
    avse::bnact::BnEpi bn;
    bn.x = bn_x;
    bn.stats = bn_stats;
    bn.gamma = gamma;
    bn.beta = beta;
    bn.alpha = nullptr;
    bn.alpha_n = 0;
    bn.rows = rows;
    return dconv_launch(N, H, W, dil, dyq, wq_t, maxbits, nullptr, dx, &bn, want_max ? 2 : 1, stream);
}

static int dconv_launch(int64_t N, int64_t H, int64_t W, int64_t dil, const void* xq, const void* wq,
                        const uint32_t* maxbits, const float* bias, float* y, const avse::bnact::BnEpi* bn, int epi,
                        avse_stream_t stream) {
    if (!xq || !wq || !maxbits || !y) return AVSE_EINVAL;
    if (N <= 0 || H <= 0 || W < 256 || (dil != 2 && dil != 4 && dil != 8 && dil != 16)) return AVSE_ESHAPE;
    if (N * H * W * 256 >= (1LL << 31) - 1024) return AVSE_ESHAPE;       // 32-bit byte offsets into the split input
    Args a;
    a.xq = xq;
    a.wq = wq;
    a.maxbits = maxbits;
    a.bias = bias;
    a.y = y;
    a.N = (int)N;
    a.H = (int)H;
    a.W = (int)W;
    // d <= 8: tile = 256 raster pixels on 4 waves, two workgroups per CU (2 LDS buffers of <= 40 KB each): the two
    // workgroups' barriers and DMA phases interleave, 1.61 vs 1.69 ms per launch at C2 against one 8-wave 512-pixel
    // workgroup per CU (profiles/r06g_dconv_fwd_ab.jsonl; one 4-wave workgroup per CU with 3 buffers measured slower in
    // round 5).  d = 16: the 4-wave tile's 4d halos need 89 KB per workgroup, so it keeps the 8-wave form.
    const int nw = dcf_nw(dil);
    if (bn) a.bn = *bn;
    else a.bn = avse::bnact::BnEpi{nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr};
    a.tiles = (int)((H * W + 64 * nw - 1) / (64 * nw));
    const dim3 grid((unsigned)(N * a.tiles)), block(64 * nw);
    hipStream_t st = (hipStream_t)stream;
#define AVSE_DCF_CASES(E)                                                                           \
    switch (dil) {                                                                                  \
        case 2: hipLaunchKernelGGL((fwd_kernel<2, 4, 2, E>), grid, block, 0, st, a); break;         \
        case 4: hipLaunchKernelGGL((fwd_kernel<4, 4, 2, E>), grid, block, 0, st, a); break;         \
        case 8: hipLaunchKernelGGL((fwd_kernel<8, 4, 2, E>), grid, block, 0, st, a); break;         \
        default: hipLaunchKernelGGL((fwd_kernel<16, 8, 1, E>), grid, block, 0, st, a); break;       \
    }
    if (epi == 0) { AVSE_DCF_CASES(0) }
    else if (epi == 1) { AVSE_DCF_CASES(1) }
    else { AVSE_DCF_CASES(2) }
#undef AVSE_DCF_CASES
    AVSE_CHECK_LAUNCH();
    return AVSE_OK;
}

}  // extern "C"
