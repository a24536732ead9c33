/*
 * avse_hip.h — C ABI of the MI355X (gfx950) hot-path kernels of avse_challenge_amd.
 *
 * Plain pointers + sizes + strides; no torch types.  Every entry point:
 *   - enqueues on the given hipStream_t only (NULL = default stream), never synchronises,
 *     never allocates: outputs and workspaces are caller-owned (graph-capture safe);
 *   - returns AVSE_OK (0) or a negative error code (see avse_strerror) after validating
 *     shapes / strides / alignment on the host, BEFORE any launch;
 *   - is stateless and thread-safe.
 * Element strides are in ELEMENTS of the tensor's dtype; the innermost (seqlen / time)
 * dimension must be contiguous (stride 1), as the reference kernels require
 * (Mamba-TasNet/modules/mamba/selective_scan_interface.py:23-35, :171-173).
 *
 * Which reference interface each entry replaces is cited per function; the reference-side
 * binding a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef AVSE_HIP_H
#define AVSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* avse_stream_t; /* a hipStream_t */

enum { AVSE_OK = 0, AVSE_EINVAL = -1, AVSE_ESHAPE = -2, AVSE_EDTYPE = -3, AVSE_ELAUNCH = -4, AVSE_EALIGN = -5,
       AVSE_ENORESIDENT = -6 };
enum { AVSE_F32 = 0, AVSE_BF16 = 1, AVSE_U8 = 2 };

const char* avse_strerror(int code);
int avse_abi_version(void);

/* ---------------------------------------------------------------- selective scan ------
 * Replaces selective_scan_cuda.fwd / .bwd of mamba-ssm 1.1.3.post1 as called at
 * Mamba-TasNet/modules/mamba/selective_scan_interface.py:42,67 (SelectiveScanFn) and
 * :218,252 (MambaInnerFnNoOutProj).  Semantics: selective_scan_ref (:91-157), real A,
 * B/C "variable" with n_groups == 1 (B, C: (b, 1, n, l)).  dstate n must be 16.
 *
 * x (scan intermediates) layout: (b, d, n_chunks, 2*n) fp32 with n_chunks =
 * avse_scan_n_chunks(l) = ceil(l / 32); row k holds two 16-step checkpoints of the state:
 * x[..., k, 2i] = state i after step min(32k + 15, l - 1), x[..., k, 2i+1] = state i after step
 * min(32k + 31, l - 1) (so x[..., -1, 1::2] is the last state, as SelectiveScanFn reads at :45).
 * The backward restarts every 16-step sub-chunk from these checkpoints.
 */
typedef struct {
    int64_t batch, dim, seqlen, dstate;
    int32_t in_dtype;          /* AVSE_F32 or AVSE_BF16: dtype of u, delta, z, B, C, out, out_z */
    int32_t delta_softplus;    /* 0: delta used as given (+ delta_bias); 1: softplus(delta + delta_bias) per element, as
                                  selective_scan_cuda; 2: delta already holds softplus(delta_raw + bias) (avse_dtproj's
                                  epilogue; delta_bias must be NULL) -- the backward then returns ddelta and
                                  ddelta_bias w.r.t. delta_raw and the bias (x sigmoid = 1 - exp(-delta)) */
    int32_t reverse;           /* 1: scan over time backwards, i.e. flip(scan(flip(.))) without copies
                                  (the BiMamba v2 backward direction, bimamba.py:236-253) */
    const void* u;      int64_t u_bs, u_ds;          /* batch / dim strides */
    const void* delta;  int64_t delta_bs, delta_ds;
    const float* A;                                  /* (d, n) contiguous */
    const void* B;      int64_t B_bs, B_ns;          /* (b, 1, n, l): batch / state strides */
    const void* C;      int64_t C_bs, C_ns;
    const float* D;                                  /* (d) or NULL */
    const void* z;      int64_t z_bs, z_ds;          /* NULL = no gating */
    const float* delta_bias;                         /* (d) or NULL */
    void* out;          int64_t out_bs, out_ds;      /* y + D*u (before gating); may be NULL when z is given (bwd recomputes it) */
    float* x;                                        /* (b, d, n_chunks, 2n) contiguous */
    void* out_z;        int64_t out_z_bs, out_z_ds;  /* out * silu(z); ignored when z == NULL */
    int32_t out_z_accumulate;  /* 1: out_z += out * silu(z) (round 6: the BiMamba v2 direction sum of bimamba.py:253,
                                  0.5 f + 0.5 b up to the out_proj's 0.5, added by the second direction's flush) */
    uint32_t* out_z_max;       /* NULL, or a word (zeroed by the caller) that receives max |out_z| as float bits by
                                  atomic max: the producer-side max for the split GEMM that consumes out_z */
} avse_scan_fwd_args;

typedef struct {
    int64_t batch, dim, seqlen, dstate;
    int32_t in_dtype, delta_softplus;
    int32_t recompute_out_z;
    int32_t reverse;
    const void* u;      int64_t u_bs, u_ds;
    const void* delta;  int64_t delta_bs, delta_ds;
    const float* A;
    const void* B;      int64_t B_bs, B_ns;
    const void* C;      int64_t C_bs, C_ns;
    const float* D;
    const void* z;      int64_t z_bs, z_ds;
    const float* delta_bias;
    const void* dout;   int64_t dout_bs, dout_ds;
    const float* x;                                  /* forward checkpoints */
    /* outputs */
    void* du;           int64_t du_bs, du_ds;
    void* ddelta;       int64_t ddelta_bs, ddelta_ds;
    float* dA;                                       /* (d, n) */
    float* dB;          int64_t dB_bs, dB_ns;        /* (b, 1, n, l) fp32 (as mamba-ssm) */
    float* dC;          int64_t dC_bs, dC_ns;
    float* dD;                                       /* (d) or NULL when D == NULL */
    float* ddelta_bias;                              /* (d) or NULL when delta_bias == NULL */
    void* dz;           int64_t dz_bs, dz_ds;        /* written when z != NULL */
    void* out_z;        int64_t out_z_bs, out_z_ds;  /* written when recompute_out_z */
    float* workspace;                                /* avse_scan_bwd_workspace_bytes() */
    int32_t dz_accumulate;     /* 1: dz += (round 6: the serial BiMamba v2 directions sum their xz gradients in place) */
    uint32_t* dz_max;          /* NULL, or a zeroed word that receives max |dz| as float bits by atomic max */
} avse_scan_bwd_args;

int64_t avse_scan_n_chunks(int64_t seqlen);
int64_t avse_scan_bwd_workspace_bytes(int64_t batch, int64_t dim, int64_t seqlen, int64_t dstate);
int avse_scan_fwd(const avse_scan_fwd_args* a, avse_stream_t stream);
int avse_scan_bwd(const avse_scan_bwd_args* a, avse_stream_t stream);

/* Forward scan with carried state (causal streaming inference; no backward).  Replaces
 * selective_scan_fn(..., return_last_state=True) continued from a cached ssm_state (bimamba.py:299-313,
 * selective_scan_interface.py:83-88).  s: the fields of avse_scan_fwd with these differences: s.x may be NULL (no
 * checkpoints are written: an inference call has no backward to restart), and s.reverse, s.out_z_accumulate and
 * s.out_z_max must be 0 / NULL (AVSE_EINVAL).  h0: the state before the first step, (b, d, 16) fp32 with the given
 * batch / channel strides (the reference's ssm_state layout), or NULL for zeros.  h_last: receives the state after
 * the last step (or NULL); it may alias h0 (in-place update: each lane reads the states it later writes).  Both
 * 16-B aligned with strides that are multiples of 4 (AVSE_EALIGN). */
typedef struct {
    avse_scan_fwd_args s;
    const float* h0;    int64_t h0_bs, h0_ds;
    float* h_last;      int64_t h_last_bs, h_last_ds;
} avse_scan_fwd_state_args;
int avse_scan_fwd_state(const avse_scan_fwd_state_args* a, avse_stream_t stream);

/* Forward scan of a zero-padded batch of rows of different lengths (inference; no backward).  a: the fields of
 * avse_scan_fwd; lengths: a->batch int32 values on the device.  With n_b = clamp(lengths[b], 0, seqlen), clamped in
 * the kernel, row b is processed exactly as avse_scan_fwd processes the row cropped to n_b columns (the same arithmetic
 * in the same order per element):
 *   - with a->reverse, logical step t lives at memory position n_b - 1 - t, not at seqlen - 1 - t;
 *   - what u, delta, B, C, z hold at columns >= n_b is never used (selects, so NaN or Inf there do not propagate);
 *   - out, out_z are written as +0 at columns n_b .. seqlen - 1; with a->out_z_accumulate those columns of out_z are
 *     left as they are (the first direction already wrote its zeros there);
 *   - a->out_z_max covers the valid columns only; n_b = 0 gives an all-zero row;
 *   - a->x (the checkpoints) may be NULL and is not written;
 *   - chunks that lie wholly past n_b are neither loaded nor stepped: a short row's workgroup ends early.
 * A NULL lengths or required pointer returns AVSE_EINVAL, bad shapes AVSE_ESHAPE, before any launch. */
int avse_scan_fwd_len(const avse_scan_fwd_args* a, const int32_t* lengths, avse_stream_t stream);

/* One recurrence step on a cached state: the selective_state_update(state, x, dt, A, B, C, D, z, dt_bias,
 * dt_softplus) contract of mamba-ssm 1.1.3 as called at bimamba.py:360-362, semantics bimamba.py:352-358:
 *   dt' = softplus(dt + dt_bias) (dt_softplus != 0; else dt + dt_bias); state = state exp(dt' A) + dt' x B;
 *   out = (sum_n state C + D x) silu(z).
 * state (b, d, 16) fp32, updated in place (16-B aligned, strides multiples of 4); x, dt, z, out (b, d) of dtype
 * (AVSE_F32 / AVSE_BF16) with d contiguous and the given batch strides; B, C (b, 16) of dtype; A (d, 16) fp32
 * contiguous, 16-B aligned; D, dt_bias (d) fp32 or NULL; z NULL = no gate.  batch <= 65535. */
typedef struct {
    int64_t batch, dim, dstate;
    int32_t dtype, dt_softplus;
    float* state;       int64_t state_bs, state_ds;
    const void* x;      int64_t x_bs;
    const void* dt;     int64_t dt_bs;
    const float* A;
    const void* B;      int64_t B_bs;
    const void* C;      int64_t C_bs;
    const float* D;
    const void* z;      int64_t z_bs;
    const float* dt_bias;
    void* out;          int64_t out_bs;
} avse_ssm_step_args;
int avse_ssm_step(const avse_ssm_step_args* a, avse_stream_t stream);

/* dt_proj with the scan's softplus in the epilogue.  Replaces
 *   delta = delta_proj_weight @ x_dbl[:, :delta_rank].t()      selective_scan_interface.py:187
 * followed by selective_scan_cuda's per-element softplus(delta + delta_bias) (selective_scan_ref :110-112):
 *   delta[b][d][t] = softplus(sum_r W[d][r] x[b][r][t] + bias[d])   (softplus = 0: the affine value only).
 * x (b, rank, l) with t contiguous (rows x_rs apart, batches x_bs apart; the first rank rows of x_proj's
 * transposed output), W (dim, rank) rows w_ds apart, bias (dim) fp32 or NULL, delta (b, dim, l) rows delta_ds
 * apart.  dtype AVSE_F32 or AVSE_BF16 for x, W and delta; fp32 accumulation; rank <= 64.  Feeds avse_scan_* with
 * delta_softplus = 2. */
int avse_dtproj(int64_t batch, int64_t dim, int64_t rank, int64_t seqlen, int32_t dtype,
                const void* w, int64_t w_ds, const void* x, int64_t x_bs, int64_t x_rs,
                const float* bias, int32_t softplus, void* delta, int64_t delta_bs, int64_t delta_ds,
                avse_stream_t stream);

/* ---------------------------------------------------------------- causal conv1d -------
 * Replaces causal_conv1d_cuda.causal_conv1d_fwd / causal_conv1d_bwd (causal-conv1d
 * 1.1.3.post1) as called at selective_scan_interface.py:182,244 and :286.  Depthwise,
 * width w <= 4, left zero-padding w-1, optional SiLU; x: (b, d, l) with l contiguous.
 * Semantics pinned by bimamba.py:278-279 (act(conv1d(x)[..., :seqlen])).  reverse = 1 computes
 * flip(conv(flip(x))) (anti-causal) in place of the xz.flip(-1) copy of bimamba.py:236.
 */
int64_t avse_cconv_bwd_workspace_bytes(int64_t batch, int64_t dim, int64_t width);
int avse_cconv_fwd(int64_t batch, int64_t dim, int64_t seqlen, int64_t width,
                   const float* x, int64_t x_bs, int64_t x_ds,
                   const float* weight /* (d, w) */, const float* bias /* (d) or NULL */,
                   float* out, int64_t out_bs, int64_t out_ds, int32_t silu, int32_t reverse,
                   avse_stream_t stream);
int avse_cconv_bwd(int64_t batch, int64_t dim, int64_t seqlen, int64_t width,
                   const float* x, int64_t x_bs, int64_t x_ds,
                   const float* weight, const float* bias,
                   const float* dout, int64_t dout_bs, int64_t dout_ds,
                   float* dx, int64_t dx_bs, int64_t dx_ds,
                   float* dweight /* (d, w) */, float* dbias /* (d) or NULL */,
                   int32_t silu, int32_t reverse, float* workspace,
                   int32_t dx_accumulate /* 1: dx += (the BiMamba v2 direction sum, round 6) */,
                   uint32_t* dx_max /* NULL, or a zeroed word: max |dx| as float bits by atomic max */,
                   avse_stream_t stream);
/* bf16 activations (x, out, dout, dx as raw bf16 bit patterns; weights, bias and their gradients fp32;
 * fp32 arithmetic): the dtype causal_conv1d_cuda sees under bf16 autocast (selective_scan_interface.py:182). */
int avse_cconv_fwd_bf16(int64_t batch, int64_t dim, int64_t seqlen, int64_t width,
                        const uint16_t* x, int64_t x_bs, int64_t x_ds,
                        const float* weight, const float* bias,
                        uint16_t* out, int64_t out_bs, int64_t out_ds, int32_t silu, int32_t reverse,
                        avse_stream_t stream);
/* The forward for a zero-padded batch of rows of different lengths (inference; no backward): the arguments of
 * avse_cconv_fwd / avse_cconv_fwd_bf16 plus lengths, batch int32 values on the device.  With n_b = clamp(lengths[b],
 * 0, seqlen), clamped in the kernel, row b is processed exactly as the dense entry point processes the row cropped to
 * n_b columns (bias + sum_k w[k] x, k ascending): with reverse, logical step t lives at memory position n_b - 1 - t;
 * what x holds at columns >= n_b is never used (a select: NaN or Inf there do not propagate); out is written as +0 at
 * columns n_b .. seqlen - 1, so n_b = 0 gives an all-zero row.  A NULL lengths, x, weight or out returns AVSE_EINVAL,
 * bad shapes AVSE_ESHAPE, before any launch. */
int avse_cconv_fwd_len(int64_t batch, int64_t dim, int64_t seqlen, int64_t width,
                       const float* x, int64_t x_bs, int64_t x_ds, const int32_t* lengths,
                       const float* weight, const float* bias,
                       float* out, int64_t out_bs, int64_t out_ds, int32_t silu, int32_t reverse,
                       avse_stream_t stream);
int avse_cconv_fwd_len_bf16(int64_t batch, int64_t dim, int64_t seqlen, int64_t width,
                            const uint16_t* x, int64_t x_bs, int64_t x_ds, const int32_t* lengths,
                            const float* weight, const float* bias,
                            uint16_t* out, int64_t out_bs, int64_t out_ds, int32_t silu, int32_t reverse,
                            avse_stream_t stream);
int avse_cconv_bwd_bf16(int64_t batch, int64_t dim, int64_t seqlen, int64_t width,
                        const uint16_t* x, int64_t x_bs, int64_t x_ds,
                        const float* weight, const float* bias,
                        const uint16_t* dout, int64_t dout_bs, int64_t dout_ds,
                        uint16_t* dx, int64_t dx_bs, int64_t dx_ds,
                        float* dweight, float* dbias,
                        int32_t silu, int32_t reverse, float* workspace, int32_t dx_accumulate, uint32_t* dx_max,
                        avse_stream_t stream);
/* Causal conv with carried left context (streaming inference).  conv_state: (b, d, w) in the activation dtype, the
 * last w inputs of the row, oldest first (the reference's conv_state, bimamba.py:277,328-329), w contiguous, batch /
 * channel strides st_bs / st_ds shared by state_in and state_out.  The conv reads x[t < 0] from state_in (NULL =
 * zeros) and state_out (or NULL) receives the last w of concat(state_in, x), also for l < w.  state_out may alias
 * state_in: the thread that reads a row's old state is the one that writes its new state.  reverse is not taken. */
int avse_cconv_fwd_state(int64_t batch, int64_t dim, int64_t seqlen, int64_t width,
                         const float* x, int64_t x_bs, int64_t x_ds,
                         const float* weight, const float* bias,
                         float* out, int64_t out_bs, int64_t out_ds, int32_t silu,
                         const float* state_in, float* state_out, int64_t st_bs, int64_t st_ds,
                         avse_stream_t stream);
int avse_cconv_fwd_state_bf16(int64_t batch, int64_t dim, int64_t seqlen, int64_t width,
                              const uint16_t* x, int64_t x_bs, int64_t x_ds,
                              const float* weight, const float* bias,
                              uint16_t* out, int64_t out_bs, int64_t out_ds, int32_t silu,
                              const uint16_t* state_in, uint16_t* state_out, int64_t st_bs, int64_t st_ds,
                              avse_stream_t stream);
/* One conv step on a cached state: the causal_conv1d_update(x, conv_state, weight, bias, activation) contract of
 * causal-conv1d 1.1.3 as called at bimamba.py:335-341, semantics bimamba.py:328-333: conv_state (b, d, w) is rolled
 * left by one, x (b, d) becomes its last column, out[b, d] = act(bias[d] + sum_k w[d, k] conv_state[b, d, k]).
 * x / out: d contiguous, batch strides x_bs / out_bs.  dtype AVSE_F32 or AVSE_BF16 (x, conv_state, out). */
int avse_cconv_update(int64_t batch, int64_t dim, int64_t width, int32_t dtype,
                      const void* x, int64_t x_bs, void* conv_state, int64_t st_bs, int64_t st_ds,
                      const float* weight, const float* bias, void* out, int64_t out_bs, int32_t silu,
                      avse_stream_t stream);

/* ---------------------------------------------------------------- add + RMSNorm -------
 * Replaces the Block pre-norm of Mamba-TasNet/modules/mamba/bimamba.py:447-451
 * (residual = h + residual; RMSNorm(residual), mamba-ssm Triton RMSNorm, eps 1e-5) and
 * MambaBlocksSequential's final norm_f (mamba_blocks.py:195-197).  Rows of width n.  y_max / dx_max (or NULL): set to the
 * bits of max |y| / |dx| (zeroed by the call in stream order), the producer-side max the split-fp16 projection GEMMs
 * take instead of an absmax pass (avse_split16_planes_known).
 */
int avse_add_rmsnorm_fwd(int64_t rows, int64_t n, const float* h, const float* res_in /* or NULL */,
                         const float* weight, float eps, float* y, float* res_out, float* rstd, uint32_t* y_max,
                         avse_stream_t stream);
int64_t avse_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t n);
int avse_rmsnorm_bwd(int64_t rows, int64_t n, const float* dy, const float* dres_out /* or NULL */,
                     const float* res_out, const float* weight, const float* rstd,
                     float* dx, float* dweight, float* workspace, uint32_t* dx_max, avse_stream_t stream);
/* The same with the row dtypes named (round 6): h / y (forward) and dy (backward) AVSE_F32 or AVSE_BF16 (bf16 rows 8-B
 * aligned; y rounded to nearest even; the statistics, res_in / res_out and dx stay fp32): the autocast Block of C5, whose
 * mixer output enters and whose norm output leaves in bf16, as mamba-ssm's fused add_norm returns its input's dtype. */
int avse_add_rmsnorm_fwd2(int64_t rows, int64_t n, const void* h, int32_t h_dtype, const float* res_in /* or NULL */,
                          const float* weight, float eps, void* y, int32_t y_dtype, float* res_out, float* rstd,
                          uint32_t* y_max, avse_stream_t stream);
int avse_rmsnorm_bwd2(int64_t rows, int64_t n, const void* dy, int32_t dy_dtype, const float* dres_out /* or NULL */,
                      const float* res_out, const float* weight, const float* rstd, float* dx, float* dweight,
                      float* workspace, uint32_t* dx_max, avse_stream_t stream);

/* ---------------------------------------------------------------- STFT / iSTFT --------
 * Replaces the CPU librosa 0.8.1 calls of baseline/avse1/dataset.py:112-118 (stft, n_fft
 * 512, hop 128, periodic Hann, center=True reflect padding, |.|, transposed to
 * (frames, 257)) and baseline/avse1/test.py:85-88 (istft with the noisy phase, length).
 * wave: (b, T) fp32 contiguous.  mag: (b, frames, 257).  spec (optional): interleaved
 * complex (b, frames, 257, 2).  frames = 1 + T / 128 (T >= 257 for reflect padding).
 */
int64_t avse_stft_frames(int64_t T);
int avse_stft_fwd(int64_t batch, int64_t T, const float* wave, float* mag, float* spec_or_null,
                  avse_stream_t stream);
/* iSTFT of mag * exp(i*angle(phase_spec)); frames_buf: workspace (b, frames, 512) fp32 */
int avse_istft(int64_t batch, int64_t frames, int64_t length, const float* mag, const float* phase_spec,
               float* frames_buf, float* wave_out, avse_stream_t stream);

/* Forward of the lip front-end nn.Conv3d(CIN, 64, (5, 7, 7), stride (1, 2, 2), padding (2, 3, 3), bias=False)
 * (baseline/avse1/model.py:29-34, frontend3D[0]; baseline/avse4/utils.py:97-118) as a split-fp16 MFMA implicit GEMM
 * that reads the lips in their stored dtype (fp32-accurate: the weights split into hi + lo fp16, fp32 frames too).
 * x: (B, CIN, T, H, W) contiguous, x_dtype AVSE_U8 (the raw uint8 frames) or AVSE_F32; w: (64, CIN, 5, 7, 7) fp32;
 * y: (B, 64, T, HO, WO) fp32 with HO = (H - 1) / 2 + 1.  Compiled shapes: CIN 3, 96 x 96 and CIN 1, 112 x 112
 * (workspace_bytes returns 0 for any other; the call then returns AVSE_ESHAPE).  workspace: the split weights
 * (2 * CIN * 5 * 8192 bytes), then max |W| and max |x| as float bits (uint32 words 0 and 1), then scratch.
 * xmax_offset: the byte offset of the max |x| word inside the workspace (what an fp32 forward leaves there is the
 * xmax of avse_conv3d_wgrad_split); <= 0 for a shape that is not compiled in. */
int64_t avse_conv3d_fwd_workspace_bytes(int64_t CIN, int64_t H, int64_t W);
int64_t avse_conv3d_fwd_xmax_offset(int64_t CIN, int64_t H, int64_t W);
int avse_conv3d_fwd(int64_t B, int64_t CIN, int64_t T, int64_t H, int64_t W, int32_t x_dtype, const void* x,
                    const float* w, float* y, float* workspace, avse_stream_t stream);

/* ---------------------------------------------------------------- lip front-end Conv3d dW
 * Weight gradient of nn.Conv3d(CIN, 64, (KT,KH,KW), stride (1,2,2), pad (PT,PH,PW), bias=False)
 * — baseline/avse1/model.py:29-34 (CIN 3, (5,7,7), pad (2,3,3)); baseline/avse4/utils.py:100-106
 * (CIN 1).  x: (B, CIN, T, H, W), dy: (B, 64, TO, HO, WO) contiguous fp32; dw: (64, CIN, KT, KH, KW).
 * accumulate != 0 adds into dw.  avse_conv3d_wgrad / _u8: the exact-fp32 MFMA implicit GEMM; WO <= 64.
 */
int64_t avse_conv3d_wgrad_workspace_bytes(int64_t B, int64_t TO, int64_t HO, int64_t N);
int avse_conv3d_wgrad(int64_t B, int64_t CIN, int64_t T, int64_t H, int64_t W, int64_t KT, int64_t KH, int64_t KW,
                      int64_t PT, int64_t PH, int64_t PW, const float* x, const float* dy, float* dw,
                      int32_t accumulate, float* workspace, avse_stream_t stream);
/* the same with x the uint8 lip frames (values 0..255 read as floats: the cast of baseline/avse1/model.py:122) */
/* avse_conv3d_wgrad_u8 on the f16 MFMA: uint8 frames (exact in fp16) against dy split into hi + lo fp16 under the
 * power-of-two scale of max |dy| (float bits in *dymax, e.g. avse_bnact_bwd's dx_max): fp32-accurate. */
int avse_conv3d_wgrad_u8_split(int64_t B, int64_t CIN, int64_t T, int64_t H, int64_t W, int64_t KT, int64_t KH,
                               int64_t KW, int64_t PT, int64_t PH, int64_t PW, const uint8_t* x, const float* dy,
                               const uint32_t* dymax, float* dw, int32_t accumulate, float* workspace,
                               avse_stream_t stream);
/* fp32 frames on the f16 MFMA (round 6): x split under max |x| (*xmax, e.g. the bits avse_conv3d_fwd leaves in its
 * workspace) and dy under max |dy|, 3 MFMAs per product (hi hi, lo hi, hi lo): fp32-accurate. */
int avse_conv3d_wgrad_split(int64_t B, int64_t CIN, int64_t T, int64_t H, int64_t W, int64_t KT, int64_t KH,
                            int64_t KW, int64_t PT, int64_t PH, int64_t PW, const float* x, const uint32_t* xmax,
                            const float* dy, const uint32_t* dymax, float* dw, int32_t accumulate, float* workspace,
                            avse_stream_t stream);
int avse_conv3d_wgrad_u8(int64_t B, int64_t CIN, int64_t T, int64_t H, int64_t W, int64_t KT, int64_t KH, int64_t KW,
                         int64_t PT, int64_t PH, int64_t PW, const uint8_t* x, const float* dy, float* dw,
                         int32_t accumulate, float* workspace, avse_stream_t stream);

/* ---------------------------------------------------------------- dilated Conv2d dW --------
 * Weight gradient of nn.Conv2d(64, 64, 5, padding=2*dil, dilation=dil) — conv2..conv5 of the avse1 AudioFeatNet
 * (baseline/avse1/model.py:199-215, dil 2, 4, 8, 16).  x, dy: (N, H, W, 64) channels-last fp32 (x the conv input, dy
 * the output gradient); dw: (64, 64, 5, 5) (Cout, Cin, KH, KW) contiguous, overwritten.  Exact-fp32 MFMA implicit GEMM;
 * dil <= 16, N*H*W*64 < 2^29.  db (nullable): the bias gradient, dy's channel sum (64), from the same pass.
 */
int64_t avse_dconv_wgrad_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t dil);
int avse_dconv_wgrad(int64_t N, int64_t H, int64_t W, int64_t dil, const float* x, const float* dy, float* dw,
                     float* db, float* workspace, avse_stream_t stream);

/* ---------------------------------------------------------------- PReLU -----------------
 * nn.PReLU(num_parameters in {1, C}) on an (N, C, S) contiguous view — avse1 lip stream
 * (model.py:32, utils/resnet.py:45-46, utils/tcn.py) and avse4 TCN (model.py:260,282).
 * Pointers 16-byte aligned.  bwd writes dx and the slope gradient da (num_params).
 */
int avse_prelu_fwd(int64_t N, int64_t C, int64_t S, int32_t num_params, const float* x, const float* a, float* y,
                   avse_stream_t stream);
int64_t avse_prelu_bwd_workspace_bytes(int64_t N, int64_t C);
int avse_prelu_bwd(int64_t N, int64_t C, int64_t S, int32_t num_params, const float* x, const float* a,
                   const float* dy, float* dx, float* da, float* workspace, avse_stream_t stream);
/* The same on a channels-last (R, C) row-major view (NHWC activations: R = N*H*W; the avse1 lip ResNet,
 * utils/resnet.py:45-46, in the layout MIOpen's NHWC convolutions use).  C % 4 == 0 and (C / 4) divides 256;
 * x, y, dy, dx, workspace (and a when num_params == C) 16-byte aligned. */
int avse_prelu_nhwc_fwd(int64_t R, int64_t C, int32_t num_params, const float* x, const float* a, float* y,
                        avse_stream_t stream);
int64_t avse_prelu_nhwc_bwd_workspace_bytes(int64_t R, int64_t C);
int avse_prelu_nhwc_bwd(int64_t R, int64_t C, int32_t num_params, const float* x, const float* a, const float* dy,
                        float* dx, float* da, float* workspace, avse_stream_t stream);

/* ---------------------------------------------------------------- BatchNorm -> [+ res] -> act ---
 * y = act(BN(x) [+ res]) with BN over the (N, S) axes of an (N, C, S) row-major view: NCHW / NCDHW
 * (S = H*W, T*H*W) or channels-last NHWC (N = batch*H*W, S = 1).  act: 0 none, 1 ReLU, 2 PReLU (alpha_n 1 or C).
 * training != 0: batch statistics (biased variance for the normalisation), running_mean / running_var (may be
 * null) updated with momentum and the unbiased variance, as nn.BatchNorm{1,2,3}d in train mode; training == 0:
 * the running statistics.  stats (C, 4) = (mean as a float pair hi + lo, rstd, bound of max |x - mean| in training /
 * 0 in eval) written by fwd, read by bwd.  gamma / beta may be null
 * (affine=False).  bwd writes dx, dgamma, dbeta (C, may be null), the per-channel PReLU slope gradient
 * dalpha_c (C; sum it for a single slope) and, with res, dres (= the gradient of the pre-activation).
 * Replaces nn.BatchNorm3d/2d + nn.PReLU / F.relu (+ the residual add) of the avse1 lip front-end and ResNet
 * BasicBlock (/root/reference/baseline/avse1/model.py:29-34, utils/resnet.py:40-67) and of the avse1 audio net
 * (model.py:181-267).  workspace: avse_bnact_workspace_bytes.  y_max / dx_max (may be null): max |y| / |dx| as float
 * bits, the producer-side max of a split operand (avse_split16_known then skips its absmax pass).
 */
int64_t avse_bnact_workspace_bytes(int64_t N, int64_t C, int64_t S);
int avse_bnact_fwd(int64_t N, int64_t C, int64_t S, const float* x, const float* res, const float* gamma,
                   const float* beta, int32_t act, const float* alpha, int32_t alpha_n, int32_t training, float eps,
                   float momentum, float* running_mean, float* running_var, float* stats, float* y, float* workspace,
                   uint32_t* y_max, avse_stream_t stream);
int avse_bnact_bwd(int64_t N, int64_t C, int64_t S, const float* x, const float* res, const float* dy, const float* stats,
                   const float* gamma, const float* beta, int32_t act, const float* alpha, int32_t alpha_n,
                   int32_t training, float* dx, float* dres, float* dgamma, float* dbeta, float* dalpha_c,
                   float* workspace, uint32_t* dx_max, avse_stream_t stream);
/* The same passes with the output written as the fp16 hi / lo split the split-fp16 convolutions read (avse_split16's
 * Q layout: per pixel C / 16 chunks of 64 B = [hi of 16 channels][lo of 16 channels], the size of the fp32 tensor), in
 * place of fp32 y / dx + a separate split pass.  The scale comes from an upper bound of max |y| / |dx| assembled from
 * the per-channel statistics, written as float bits to y_bound / dx_bound (which the consumer passes on as the split's
 * max).  Channels-last only (S = 1, C % 64 == 0, 16-B aligned pointers), no residual; the forward in training mode;
 * the backward with the stats of a training-mode forward (or eval).  Returns AVSE_ESHAPE otherwise. */
int avse_bnact_fwd_q(int64_t N, int64_t C, int64_t S, const float* x, const float* gamma, const float* beta, int32_t act,
                     const float* alpha, int32_t alpha_n, float eps, float momentum, float* running_mean,
                     float* running_var, float* stats, void* yq, float* workspace, uint32_t* y_bound,
                     avse_stream_t stream);
int avse_bnact_bwd_q(int64_t N, int64_t C, int64_t S, const float* x, const float* dy, const float* stats,
                     const float* gamma, const float* beta, int32_t act, const float* alpha, int32_t alpha_n,
                     int32_t training, void* dxq, float* dgamma, float* dbeta, float* dalpha_c, float* workspace,
                     uint32_t* dx_bound, avse_stream_t stream);
/* The backward of a BatchNorm -> ReLU / PReLU whose output feeds ONE split-fp16 convolution (AudioFeatNet bn1..bn4 ->
 * conv2..conv5, baseline/avse1/model.py:199-215; BasicBlock bn1 -> conv2, baseline/avse1/utils/resnet.py:40-67), from
 * per-channel sums that the convolution's input-gradient launch formed in its epilogue (avse_dconv_dgrad_bn,
 * avse_sconv_dgrad1_bn): `rows` rows of [nq][C] floats at the start of `workspace` (nq = 4 with q_out, else 3: sum
 * dz, sum dz xhat, PReLU slope sum, max |dz|), reduced per channel in fp64, then the apply pass.  No pass over x and
 * dy for the sums.  Channels-last (S = 1), C % 4 == 0 (q_out: C % 64 == 0), 16-B aligned pointers, rows < 2^23;
 * workspace of avse_bnact_rows_workspace_bytes(rows, C, nq) (0: not supported).  dx_max as avse_bnact_bwd's (q_out:
 * the bound, as avse_bnact_bwd_q's dx_bound, dx the split planes). */
int64_t avse_bnact_rows_workspace_bytes(int64_t rows, int64_t C, int64_t nq);
int avse_bnact_bwd_rows(int64_t N, int64_t C, int64_t rows, const float* x, const float* dy, const float* stats,
                        const float* gamma, const float* beta, int32_t act, const float* alpha, int32_t alpha_n,
                        int32_t training, float* dx, float* dgamma, float* dbeta, float* dalpha_c, float* workspace,
                        uint32_t* dx_max, int32_t q_out, avse_stream_t stream);
/* The lip front-end chain BatchNorm3d -> none / ReLU / PReLU -> MaxPool3d((1, 3, 3), (1, 2, 2), (0, 1, 1)) -> frames in
 * channels-last memory (baseline/avse1/model.py:29-34 and :46-50, avse4 VisualFrontend) as one pass forward and two
 * backward, in place of avse_bnact_fwd -> avse_maxpool2d_fwd -> avse_transpose_cp and their backwards: neither the
 * activated tensor nor the un-pooled gradient is written.  x, dx: (B, C, T, H, W) contiguous; y, g (the gradient of
 * y): (B T, H / 2, W / 2, C) contiguous; idx: one argmax byte per pooled element, (B, C, T, H / 2, W / 2) with
 * avse_maxpool2d_fwd's encoding; stats, the running statistics, act, alpha, training as avse_bnact_fwd / _bwd.  The
 * forward's statistics launches are avse_bnact_fwd's, y and idx are bit-identical to the three calls; dx, dgamma,
 * dbeta, dalpha_c agree with theirs to the rounding of a re-ordered fp32 sum (deterministic, no atomics); dx_max (may
 * be null): max |dx| as avse_bnact_bwd's.  Needs C % 64 == 0, H even, W % 4 == 0, W <= 96, 16-B aligned pointers
 * (avse_bnpool_supported: 1 / 0; other shapes return AVSE_ESHAPE).  workspace: forward
 * avse_bnact_workspace_bytes(B, C, T H W), backward avse_bnact_rows_workspace_bytes(avse_bnpool_rows(...), C, 3). */
int32_t avse_bnpool_supported(int64_t B, int64_t C, int64_t T, int64_t H, int64_t W);
int64_t avse_bnpool_rows(int64_t B, int64_t C, int64_t T, int64_t H, int64_t W);
int avse_bnpool_fwd(int64_t B, int64_t C, int64_t T, int64_t H, int64_t W, const float* x, const float* gamma,
                    const float* beta, int32_t act, const float* alpha, int32_t alpha_n, int32_t training, float eps,
                    float momentum, float* running_mean, float* running_var, float* stats, float* y, uint8_t* idx,
                    float* workspace, avse_stream_t stream);
int avse_bnpool_bwd(int64_t B, int64_t C, int64_t T, int64_t H, int64_t W, const float* x, const float* g,
                    const uint8_t* idx, const float* stats, const float* gamma, const float* beta, int32_t act,
                    const float* alpha, int32_t alpha_n, int32_t training, float* dx, float* dgamma, float* dbeta,
                    float* dalpha_c, float* workspace, uint32_t* dx_max, avse_stream_t stream);

/* ---------------------------------------------------------------- max pooling over planes -------
 * nn.MaxPool3d((1, KH, KW), (1, SH, SW), (0, PH, PW)) of the lip front-ends (avse1 model.py:29-34, avse4
 * VisualFrontend) on `planes` = B*C*T contiguous H x W planes; y: planes x Ho x Wo, idx: the argmax's position
 * in its window (kh << 4 | kw, one byte), read by bwd.  torch semantics: first maximum, NaN taken; bwd gathers
 * (deterministic).  KH, KW <= 15, pad <= kernel / 2.
 */
int64_t avse_maxpool2d_out_size(int64_t H, int64_t K, int64_t S, int64_t P);
int avse_maxpool2d_fwd(int64_t planes, int64_t H, int64_t W, int64_t KH, int64_t KW, int64_t SH, int64_t SW, int64_t PH,
                       int64_t PW, const float* x, float* y, uint8_t* idx, avse_stream_t stream);
int avse_maxpool2d_bwd(int64_t planes, int64_t H, int64_t W, int64_t KH, int64_t KW, int64_t SH, int64_t SW, int64_t PH,
                       int64_t PW, const float* dy, const uint8_t* idx, float* dx, avse_stream_t stream);

/* ---------------------------------------------------------------- batched transpose ------------
 * y[n][p][c] = x[n][c][p], fp32, x and y (N, C, P) / (N, P, C) contiguous, y must not alias x.  The avse1 lip front-end
 * output (B, C, T, H, W) -> (B*T, H, W, C) for the channels-last ResNet trunk and its gradient back (the reference
 * folds frames into the batch at baseline/avse1/model.py:46-50).  64 x 64 LDS tiles.
 */
int avse_transpose_cp(int64_t N, int64_t C, int64_t P, const float* x, float* y, avse_stream_t stream);

/* ---------------------------------------------------------------- PReLU -> gLN (avse4) ----
 * y = gLN(PReLU(x)) of baseline/avse4/model.py:259-266,284-292 (PReLU with one slope; gLN
 * :225-252, EPS inside the sqrt).  x, y: (B, C, K) contiguous; gamma, beta: (C); stats: (B, 2)
 * = (mean, rstd) written by fwd and read by bwd.  workspace: avse_prelu_gln_workspace_bytes.
 */
int64_t avse_prelu_gln_workspace_bytes(int64_t B, int64_t C);
int avse_prelu_gln_fwd(int64_t B, int64_t C, int64_t K, const float* x, const float* alpha, const float* gamma,
                       const float* beta, float eps, float* y, float* stats, float* workspace, avse_stream_t stream);
int avse_prelu_gln_bwd(int64_t B, int64_t C, int64_t K, const float* x, const float* alpha, const float* gamma,
                       const float* stats, const float* dy, float* dx, float* dalpha, float* dgamma, float* dbeta,
                       float* workspace, avse_stream_t stream);
/* the same with dx written only as the split-fp16 planes of the 1x1 Conv1d GEMM whose output x is (TemporalBlock's
 * first conv, model.py:259-266): dx_hi / dx_lo rows of kp elements (kp >= K, kp % 8 == 0, pads written as 0, 16-B
 * aligned planes), scaled by *dx_maxbits = an upper bound of max |dx| from the reduction pass's row maxima
 * (|dx| <= max(1, |a|) rstd (|gamma_c| max|dy| + |mean_g| + max|xhat| |mean_gxh|); bits of a float). */
int avse_prelu_gln_bwd_q(int64_t B, int64_t C, int64_t K, const float* x, const float* alpha, const float* gamma,
                         const float* stats, const float* dy, void* dx_hi, void* dx_lo, int64_t kp, uint32_t* dx_maxbits,
                         float* dalpha, float* dgamma, float* dbeta, float* workspace, avse_stream_t stream);

/* ---------------------------------------------------------------- depthwise dilated conv1d --
 * nn.Conv1d(C, C, P, padding=(P-1)/2*dil, dilation=dil, groups=C, bias=False) — avse4
 * model.py:278-285 (TCN, dil 2^x) and :191-198 (VisualConv1D).  P in {1,3,5,7}, halo <= 512.
 */
int64_t avse_dwconv_bwd_workspace_bytes(int64_t B, int64_t C);
int avse_dwconv_fwd(int64_t B, int64_t C, int64_t K, int64_t P, int64_t dil, const float* x, const float* w, float* y,
                    avse_stream_t stream);
int avse_dwconv_bwd(int64_t B, int64_t C, int64_t K, int64_t P, int64_t dil, const float* x, const float* w,
                    const float* dy, float* dx, float* dw, float* workspace, avse_stream_t stream);

/* ---------------------------------------------------------------- fused dwconv <-> PReLU -> gLN (avse4 TCN) ----
 * DepthwiseSeparableConv.net[:3] of baseline/avse4/model.py:278-292: y1 = depthwise dilated "same" conv1d(x)
 * (w (C, P), no bias, as avse_dwconv_fwd), y = gLN(PReLU(y1)) (as avse_prelu_gln_fwd).  The forward computes the
 * gLN statistics inside the conv pass (x read once, y1 written once, y1 read once by the apply pass); the
 * backward turns (y1, dy) into the conv's output gradient inside the conv-backward pass.  y1 and stats (B, 2) are
 * saved by the caller for the backward.  Workspace: avse_dwconv_gln_workspace_bytes(B, C). */
int64_t avse_dwconv_gln_workspace_bytes(int64_t B, int64_t C);
int avse_dwconv_gln_fwd(int64_t B, int64_t C, int64_t K, int64_t P, int64_t dil, const float* x, const float* w,
                        const float* alpha, const float* gamma, const float* beta, float eps, float* y1, float* y,
                        float* stats, float* workspace, avse_stream_t stream);
/* the same with y written as the split-fp16 planes of the 1x1 Conv1d that consumes it (DepthwiseSeparableConv's
 * pointwise conv, model.py:284-292, on avse_gemm_f32s): y_hi / y_lo rows of kp elements (kp >= K, kp % 8 == 0, 16-B
 * aligned planes) holding fp16(y 2^e) and fp16(y 2^e - hi), e from *y_maxbits = an upper bound of max |y| (set by the
 * call from the rows' PReLU extremes before the apply pass; bits of a float) — no fp32 y, no absmax or split pass. */
int avse_dwconv_gln_fwd_q(int64_t B, int64_t C, int64_t K, int64_t P, int64_t dil, const float* x, const float* w,
                          const float* alpha, const float* gamma, const float* beta, float eps, float* y1, void* y_hi,
                          void* y_lo, int64_t kp, uint32_t* y_maxbits, float* stats, float* workspace,
                          avse_stream_t stream);
int avse_dwconv_gln_bwd(int64_t B, int64_t C, int64_t K, int64_t P, int64_t dil, const float* x, const float* w,
                        const float* y1, const float* alpha, const float* gamma, const float* stats, const float* dy,
                        float* dx, float* dw, float* dalpha, float* dgamma, float* dbeta, float* workspace,
                        avse_stream_t stream);

/* ---------------------------------------------------------------- ragged inference batches (avse4) ----
 * Forwards for a zero-padded batch of utterances of different lengths: lengths (device, B x int32) is each sample's
 * extent along K.  Row (b, c) runs the dense forward's loops with len[b] (clamped into [0, K]) in place of K at row
 * stride K, so the valid part of y and stats[b] equal the dense call on the contiguous slice x[b:b+1, :, :len[b]] bit
 * for bit; what x holds at columns >= len[b] is never used (it reads as 0: NaN / Inf there do not propagate), and
 * y (or the planes, up to kp) is written as +0 there.  y1's columns past len[b] are not written.  len[b] == 0 gives
 * an all-zero sample with stats (0, 0).  Inference only: there is no backward.  Workspaces as the dense calls. */
int avse_prelu_gln_fwd_len(int64_t B, int64_t C, int64_t K, const float* x, const int32_t* lengths, const float* alpha,
                           const float* gamma, const float* beta, float eps, float* y, float* stats, float* workspace,
                           avse_stream_t stream);
int avse_dwconv_gln_fwd_len(int64_t B, int64_t C, int64_t K, int64_t P, int64_t dil, const float* x,
                            const int32_t* lengths, const float* w, const float* alpha, const float* gamma,
                            const float* beta, float eps, float* y1, float* y, float* stats, float* workspace,
                            avse_stream_t stream);
/* y as the split-fp16 planes (as avse_dwconv_gln_fwd_q); *y_maxbits bounds max |y| over the valid parts of all samples */
int avse_dwconv_gln_fwd_q_len(int64_t B, int64_t C, int64_t K, int64_t P, int64_t dil, const float* x,
                              const int32_t* lengths, const float* w, const float* alpha, const float* gamma,
                              const float* beta, float eps, float* y1, void* y_hi, void* y_lo, int64_t kp,
                              uint32_t* y_maxbits, float* stats, float* workspace, avse_stream_t stream);
/* avse_dwconv_fwd with the same length semantics (VisualConv1D over video frames, model.py:191-198) */
int avse_dwconv_fwd_len(int64_t B, int64_t C, int64_t K, int64_t P, int64_t dil, const float* x, const int32_t* lengths,
                        const float* w, float* y, avse_stream_t stream);
/* Per sample linear upsampling by `up` of v (B, C, n_in_max), valid frames vlen[b], to klen[b] columns of out
 * (B, C, K): F.interpolate(v[b, :, :vlen[b]], scale_factor=up, mode="linear") padded with 0 / cropped to klen[b]
 * (model.py:166-176), 0 from there to K.  v / out: element strides of the batch and channel axes (unit stride along
 * time), so out may be a channel slice of a wider tensor. */
int avse_upsample_linear_len(int64_t B, int64_t C, int64_t n_in_max, int64_t K, int64_t up, const float* v, int64_t v_bs,
                             int64_t v_cs, const int32_t* vlen, const int32_t* klen, float* out, int64_t out_bs,
                             int64_t out_cs, avse_stream_t stream);

/* ---------------------------------------------------------------- ragged inference batches (avse1) ----
 * The avse1 front-end, BatchNorm passes and lip-to-audio gather for a zero-padded batch of utterances of different
 * lengths (baseline/avse1/test.py:58-89 walks the set one scene at a time).  lengths: device int32, one per sample,
 * clamped in the kernels so that no value moves an access out of a row.  Inference only: no backward exists.
 *
 * avse_stft_fwd_len: avse_stft_fwd on rows of T_b = lengths[b] samples at row stride T.  Row b has F_b = 1 + T_b / 128
 * frames (0 when T_b <= 256), reflect-padded at its own end: frames f < F_b equal avse_stft_fwd on the row cropped to
 * T_b bit for bit, mag / spec are +0 for F_b <= f < 1 + T / 128, and wave[b, T_b:] is never read.
 * avse_istft_len: avse_istft with the row's own F_b (at most `frames`) and T_b = lengths[b] <= length: the overlap-add
 * and the window-sum normalisation of the row cropped to (F_b, T_b), bit for bit, +0 from T_b to length; frames
 * f >= F_b of mag / phase_spec are never read. */
int avse_stft_fwd_len(int64_t batch, int64_t T, const float* wave, const int32_t* lengths, float* mag,
                      float* spec_or_null, avse_stream_t stream);
int avse_istft_len(int64_t batch, int64_t frames, int64_t length, const float* mag, const float* phase_spec,
                   const int32_t* lengths, float* frames_buf, float* wave_out, avse_stream_t stream);
/* Eval-mode avse_bnact_fwd (no residual) whose output is exact +0 outside each sample's valid window of the time axis:
 * y = act(BN(x)) where t_off <= t < t_off + lengths[b] (lengths clamped into [0, T - t_off]), +0 elsewhere by a select
 * (NaN / Inf in x there reach neither y nor y_max).  The valid elements equal avse_bnact_fwd's bit for bit; y_max (may be
 * null) is max |y| over them.  (b, t) of an element of the (N, C, S) view:
 *   time_in_rows != 0: N = B T inner, row r = (b T + t) inner + i -- channels-last (B, T, F, C) and (B, T, H, W, C)
 *                      (S = 1, inner = F or H W), time-major (B T, C) rows (inner = 1), frames (B T, C, H, W);
 *   time_in_rows == 0: N = B, S = T inner, column (c, t, i) -- contiguous (B, C, T, F) and (B, C, T, H, W).
 * t_off > 0 serves a BatchNorm over a padded convolution output of which a later chomp keeps [t_off, t_off + T').
 * training != 0 is refused (AVSE_EINVAL): there is no length-aware statistics pass.  stats as avse_bnact_fwd's (eval).
 * avse_bnact_fwd_q_len writes the split layout of avse_bnact_fwd_q (channels-last: S = 1, C % 64 == 0, time_in_rows,
 * 16-B aligned) under the exact max over the valid elements, found by a pass of its own and left in *y_max: the bytes
 * avse_split16_known makes of avse_bnact_fwd_len's output under that word. */
int avse_bnact_fwd_len(int64_t N, int64_t C, int64_t S, const float* x, const float* gamma, const float* beta,
                       int32_t act, const float* alpha, int32_t alpha_n, int32_t training, float eps,
                       const float* running_mean, const float* running_var, float* stats, float* y, uint32_t* y_max,
                       const int32_t* lengths, int64_t B, int64_t T, int64_t inner, int64_t t_off, int32_t time_in_rows,
                       avse_stream_t stream);
int avse_bnact_fwd_q_len(int64_t N, int64_t C, int64_t S, const float* x, const float* gamma, const float* beta,
                         int32_t act, const float* alpha, int32_t alpha_n, int32_t training, float eps,
                         const float* running_mean, const float* running_var, float* stats, void* yq, uint32_t* y_max,
                         const int32_t* lengths, int64_t B, int64_t T, int64_t inner, int64_t t_off, int32_t time_in_rows,
                         avse_stream_t stream);
/* Nearest-neighbour gather of the lip features onto the audio frames (baseline/avse1/model.py:124-126,
 * F.interpolate(mode="nearest") over time): out[b, t, :C] = v[b, (t vlen[b]) / tlen[b], :C] (integer division) for
 * t < tlen[b], +0 for tlen[b] <= t < T.  v (B, n_in_max, C), out (B, T, >= C): element strides of the batch and time
 * axes (unit stride along C), so out may be the left C columns of a wider tensor. */
int avse_gather_nearest_len(int64_t B, int64_t C, int64_t n_in_max, int64_t T, const float* v, int64_t v_bs, int64_t v_ts,
                            const int32_t* vlen, const int32_t* tlen, float* out, int64_t out_bs, int64_t out_ts,
                            avse_stream_t stream);

/* ---------------------------------------------------------------- ragged inference batches (DPMamba) ----
 * Channels-last GroupNorm(1, N) (speechbrain Dual_Computation_Block intra_norm / inter_norm, Dual_Path_Model.norm:
 * biased variance, eps inside the rsqrt) with a per-row valid extent.  x (B, R, C, N) fp32 contiguous; lengths (device,
 * B x int32, clamped into the axis): row b is valid for r < n_b with len_axis 0 and for c < n_b with len_axis 1.  The
 * statistics run over the row's valid elements alone; y = (x - mean) rstd gamma_n + beta_n (+ res, may be null) there
 * and +0 at every other position; x and res are never loaded at an invalid position.  transpose_out != 0: y and res
 * are (B, C, R, N).  stats (B, 2) = (mean, rstd), (0, 0) for n_b == 0.  Row b comes out bit for bit (y and stats) as
 * the call on the row cropped and alone: B = 1, the axis cut to n_b, contiguous.  No atomics; every element of y and
 * stats is written.  N % 4 == 0 with 16-B aligned tensors takes 16-B accesses, any other N dword ones (same bits).
 * workspace: avse_gln_cl_workspace_bytes, need not be initialised.  Inference only: there is no backward. */
int64_t avse_gln_cl_workspace_bytes(int64_t B, int64_t R, int64_t C);
int avse_gln_cl_fwd_len(int64_t B, int64_t R, int64_t C, int64_t N, const float* x, const int32_t* lengths,
                        int32_t len_axis, const float* gamma, const float* beta, float eps, const float* res,
                        int32_t transpose_out, float* y, float* stats, float* workspace, avse_stream_t stream);

/* ---------------------------------------------------------------- LSTM recurrence ----------
 * Replaces the per-step cuDNN/MIOpen LSTM behind nn.LSTM at baseline/avse1/model.py:88 (FusionNet:
 * LSTM(1540 -> 257), batch_first) and baseline/avse2/model.py:101-102 (DPRNN, bidirectional: one call per
 * direction, reverse = 1 for the backward one).  PyTorch semantics: gate order i, f, g, o; h0 = c0 = 0.
 * Forward: gx (B, T, 4H) = X W_ih^T + b_ih + b_hh precomputed by the caller (one GEMM); whhT = W_hh^T (H, 4H)
 * contiguous; writes h (strided: hout[b*hout_bs + t*hout_ts + j]), c (B, T, H) and the gate activations
 * (B, T, 4H) the backward needs.  Backward: dh_out strided like hout; whh_pad = W_hh (4H, H) zero-padded to
 * (4H, avse_lstm_padded_hidden(H)); writes dgates (B, T, 4H) = dL/d(pre-activation gates).  H <= 512.
 * One workgroup per sequence, the whole recurrence in one launch; no workspace. */
int64_t avse_lstm_padded_hidden(int64_t H);
int avse_lstm_fwd(int64_t B, int64_t T, int64_t H, int32_t reverse, const float* gx, const float* whhT, float* hout,
                  int64_t hout_bs, int64_t hout_ts, float* c_all, float* gates, avse_stream_t stream);
int avse_lstm_bwd(int64_t B, int64_t T, int64_t H, int32_t reverse, const float* dh_out, int64_t dh_bs, int64_t dh_ts,
                  const float* gates, const float* c_all, const float* whh_pad, float* dgates, avse_stream_t stream);
/* The same recurrences with each sequence spread over G = avse_lstm_group_size(B, H) workgroups (0: not available
 * for this shape: B * G > 256 or H > 384), W_hh resident in their LDS, h / dh exchanged through data-tagged
 * granules in `workspace` (avse_lstm_group_workspace_bytes; zeroed by the call).  A sequence's G workgroups must be
 * co-resident: the call returns AVSE_ENORESIDENT without enqueueing anything when B * G exceeds
 * avse_lstm_group_capacity(H, backward) (that kernel's workgroups the current device holds at once; the caller then
 * runs avse_lstm_fwd / avse_lstm_bwd).  Every inter-workgroup wait is bounded: a wait that times out (e.g. CUs held
 * by another process's persistent kernels) writes 0x71000000 + step into *error_flag (device memory, never cleared
 * by the call; the outputs of that launch are invalid) — the caller checks it after the step and raises.
 * whh = W_hh (4H, H) contiguous for both directions; other arguments and outputs as avse_lstm_fwd / avse_lstm_bwd. */
int64_t avse_lstm_group_size(int64_t B, int64_t H);
int64_t avse_lstm_group_workspace_bytes(int64_t B, int64_t H);
int64_t avse_lstm_group_capacity(int64_t H, int32_t backward);
int avse_lstm_fwd_group(int64_t B, int64_t T, int64_t H, int32_t reverse, const float* gx, const float* whh,
                        float* hout, int64_t hout_bs, int64_t hout_ts, float* c_all, float* gates, void* workspace,
                        uint32_t* error_flag, avse_stream_t stream);
int avse_lstm_bwd_group(int64_t B, int64_t T, int64_t H, int32_t reverse, const float* dh_out, int64_t dh_bs,
                        int64_t dh_ts, const float* gates, const float* c_all, const float* whh, float* dgates,
                        void* workspace, uint32_t* error_flag, avse_stream_t stream);

/* ---------------------------------------------------------------- bf16 projection GEMM ------
 * The bf16 GEMMs BiMamba v2 runs under autocast (BASELINE configs[4]): in_proj (Mamba-TasNet/modules/mamba/
 * bimamba.py:190-196, xz = W_in h^T), out_proj (:250-253), their input gradients and weight gradients —
 * torch.matmul / F.linear on bf16 operands in the reference.  Batched, fp32 accumulation:
 *     c[g][q][p] = alpha * sum_{b in group g} sum_k P(b, p, k) * Q(b, q, k),
 *     P(b, p, k) = p_ptr[b*p_bs + p*p_sx + k*p_sk]  (Q alike),  groups of `fold` consecutive batches (0 or 1: none)
 * c_dtype AVSE_BF16 (round to nearest even; c 8-byte aligned) or AVSE_F32 (c 16-byte aligned); c has p contiguous,
 * c_sq % 4 == 0, batch stride c_bs per group.  Exactly one of p_sx / p_sk is 1 (and one of q_sx / q_sk): the operand
 * is K-contiguous or contiguous along p (q); the other stride a multiple of 8, p / q 16-byte aligned.  A batch stride
 * of 0 shares the operand (a weight).  Any k >= 1 (elements past it are never summed, whatever lies there).
 * p_extent / q_extent: elements readable from p / q (reads past them return 0).  Per batch, every offset an operand
 * tile reaches must stay below 2^31 bytes. */
typedef struct {
    int64_t batch, mp, mq, k, fold;
    const void* p;  int64_t p_bs, p_sx, p_sk, p_extent;
    const void* q;  int64_t q_bs, q_sx, q_sk, q_extent;
    void* c;        int64_t c_bs, c_sq;
    float alpha;
    int32_t c_dtype;                 /* AVSE_BF16 */
} avse_gemm_bf16_args;
int avse_gemm_bf16(const avse_gemm_bf16_args* a, avse_stream_t stream);

/* fp32 GEMMs of the fp32 models (Mamba-TasNet C3 projections) on the same kernel, fp32-accurate: each fp32 operand is
 * given as two fp16 planes with the operand's strides, hi = fp16(x 2^e) and lo = fp16(x 2^e - hi), e from the operand's
 * max |x| (bits in *p_max / *q_max, avse_split16_planes), and c = alpha 2^-(e_p + e_q) (P_hi Q_hi + P_hi Q_lo + P_lo Q_hi)
 * on the f16 MFMA with fp32 accumulation: three MFMAs per product at 16/3 of the fp32 MFMA rate, 22-bit operands (the
 * dropped lo*lo term is 2^-22 of a product).  Layout rules as avse_gemm_bf16; c fp32. */
typedef struct {
    int64_t batch, mp, mq, k, fold;
    const void* p_hi; const void* p_lo;  int64_t p_bs, p_sx, p_sk, p_extent;  const uint32_t* p_max;
    const void* q_hi; const void* q_lo;  int64_t q_bs, q_sx, q_sk, q_extent;  const uint32_t* q_max;
    float* c;       int64_t c_bs, c_sq;
    float alpha;
    /* nsub > 1: batch b of P / Q sits at (b / nsub) p_bs + (b % nsub) p_bs2 (a reduction split into nsub chunks of k
     * per batch: the avse4 1x1-conv weight gradient over time chunks, folded and summed as batches); 0 or 1: b p_bs */
    int64_t nsub, p_bs2, q_bs2;
} avse_gemm_f32s_args;
int avse_gemm_f32s(const avse_gemm_f32s_args* a, avse_stream_t stream);
/* x (b, r, c) fp32 with c contiguous (rows x_rs, batches x_bs apart) -> hi / lo fp16 planes at the same element
 * offsets (their padding untouched) and *maxbits = bits of max |x|. */
int avse_split16_planes(int64_t b, int64_t r, int64_t c, const float* x, int64_t x_bs, int64_t x_rs, void* hi, void* lo,
                        uint32_t* maxbits, avse_stream_t stream);
/* y = a + b over the padded (rows, lp) storage of two (b, c, l) fp32 operands (16-B aligned, lp % 4 == 0; the pad
 * columns hold don't-care values) and *maxbits = bits of max |y| over the logical columns < l (the BiMamba v2
 * direction sum bimamba.py:253 that the C3 out_proj splits next) */
int avse_add_max(int64_t rows, int64_t lp, int64_t l, const float* a, const float* b, float* y, uint32_t* maxbits,
                 avse_stream_t stream);
/* the same with *maxbits already max |x| (e.g. avse_add_rmsnorm_fwd's y_max): the split pass only */
int avse_split16_planes_known(int64_t b, int64_t r, int64_t c, const float* x, int64_t x_bs, int64_t x_rs, void* hi,
                              void* lo, const uint32_t* maxbits, avse_stream_t stream);
/* the same into planes with their own strides (rows h_rs, batches h_bs apart: e.g. rows padded to a multiple of 8
 * elements, so that an (b, c, K) activation with K % 8 != 0 can be a GEMM operand read along K or along c — the avse4
 * 1x1 Conv1d, baseline/avse4/model.py:255-293), the padding columns c .. h_rs - 1 written as 0 (h_rs % 4 == 0, 8-B
 * aligned planes); known != 0: *maxbits is already max |x| (no absmax pass).  avse_gemm_f32s
 * with fold == 1 takes an output row stride c_sq that is not a multiple of 4 (those rows are stored per element). */
int avse_split16_planes_to(int64_t b, int64_t r, int64_t c, const float* x, int64_t x_bs, int64_t x_rs, void* hi,
                           void* lo, int64_t h_bs, int64_t h_rs, uint32_t* maxbits, int32_t known, avse_stream_t stream);

/* ---------------------------------------------------------------- dilated Conv2d fwd / input gradient ----
 * Replaces the forward and the data gradient of nn.Conv2d(64, 64, 5, padding=2d, dilation=d), d = 2, 4, 8, 16
 * (AudioFeatNet conv2..conv5, baseline/avse1/model.py:199-215), channels-last activations, as an implicit GEMM on the
 * fp16 MFMA with fp32-accurate split operands: every operand x is scaled by 2^e (the tensor's max |x| into
 * [2^14, 2^15)) and split into hi = fp16(x 2^e) and lo = fp16(x 2^e - hi); each product is hi*hi + hi*lo + lo*hi with
 * fp32 accumulation.
 *   avse_split16: x NHWC fp32 (n_pix, 64) -> xq (n_pix, 256 B): 4 channel quarters of [hi 16][lo 16] fp16, and
 *                 maxbits[0] = bits of max |x| (maxbits is a 2-entry device buffer: [0] input, [1] weight).
 *   avse_dconv_wprep: W (64, 64, 5, 5) fp32 -> wq (avse_dconv_wprep_bytes()), maxbits[1]; transposed = 1 prepares
 *                 the input gradient's W'[o][i][kh][kw] = W[i][o][4 - kh][4 - kw].
 *   avse_dconv_fwd: y[n][h][w][o] = sum x[n][h + d (kh - 2)][w + d (kw - 2)][i] W[o][i][kh][kw] (+ bias[o]); with
 *                 x = dY and a transposed wq it is the input gradient.  W >= 256 (tiles of 256 raster pixels span at
 *                 most two rows), n_pix * 256 < 2^31. */
int64_t avse_dconv_wprep_bytes(void);
int avse_split16(int64_t n_pix, const float* x, void* xq, uint32_t* maxbits, avse_stream_t stream);
/* avse_split16 with max |x| already in maxbits[0] (e.g. avse_bnact_fwd's y_max): the split pass only */
int avse_split16_known(int64_t n_pix, const float* x, void* xq, const uint32_t* maxbits, avse_stream_t stream);
int avse_dconv_wprep(const float* w, int32_t transposed, void* wq, uint32_t* maxbits, avse_stream_t stream);
/* Both images from one launch (one workgroup per stage and orientation): wq as transposed = 0 and, when wq_t is given,
 * wq_t as transposed = 1, the same bytes as avse_dconv_wprep's; max |w| bits to maxbits[1] and maxbits_t[1] (the
 * input gradient's pair).  wq_t and maxbits_t are both null or both set. */
int avse_dconv_wprep2(const float* w, void* wq, void* wq_t, uint32_t* maxbits, uint32_t* maxbits_t,
                      avse_stream_t stream);

/* 3x3 convolutions of the lip-encoder ResNet trunks (csrc/sconv.hip), replacing
 * nn.Conv2d(ci, co, 3, stride, padding=1, bias=False) of baseline/avse1/utils/resnet.py:9-10 (BasicBlock :26-67)
 * and baseline/avse4/utils.py:40-84 (ResNetLayer); ci, co multiples of 64, stride 1 or 2, NHWC fp32 activations.
 * Split-fp16 MFMA implicit GEMMs (fp32-accurate, as avse_dconv_fwd).  Operands in the Q layout of avse_split16 (a
 * (pixels, C) tensor split as (pixels C / 64, 64)); max |x| bits from avse_split16, max |w| bits from avse_sconv_wprep.
 *   avse_sconv_wprep: W (co, ci, 3, 3) fp32 -> wq (avse_sconv_wprep_bytes(co, ci)); transposed = 1 prepares the
 *     stride-1 input gradient's W'[ci][co][kh][kw] = W[co][ci][2 - kh][2 - kw] (then call avse_sconv_fwd with ci, co
 *     swapped); transposed = 2 the stride-2 input gradient's phase images (avse_sconv_dgrad2);
 *   avse_sconv_fwd: y (N, Ho, Wo, co) fp32, Ho = (Hi - 1) / stride + 1;
 *   avse_sconv_wgrad: dW (co, ci, 3, 3) from the split input (N, Hi, Wi, ci) and output gradient (N, Ho, Wo, co);
 *     workspace of avse_sconv_wgrad_workspace_bytes (< 0: shape not supported): the kernel's partial slabs, summed in
 *     a fixed order (no atomics).  Stride 1 with rows of up to 28 pixels (30 .. 34 too): one workgroup covers all 9
 *     taps of its (o, i) block; stride 2 and wider rows: one workgroup per kernel row;
 *   avse_sconv_dgrad2: the stride-2 input gradient dX (N, Hi, Wi, ci) fp32 NHWC (every pixel written) from the split
 *     output gradient (N, Ho, Wo, co) and wq = avse_sconv_wprep(co, ci, W, transposed = 2) (the 4 parity phases'
 *     taps, same byte count); replaces the stride-2 blocks' input gradient of resnet.py:26-67 (conv1 of layer2..4)
 *     that torch's conv2d backward computes; avse_sconv_dgrad2_supported(...) = 1 when the kernel takes the shape. */
/* AudioFeatNet.conv1 = nn.Conv2d(1, 64, 5, padding=2) (baseline/avse1/model.py:199-215) on x (N, 1, H, W) fp32
 * (csrc/conv1.hip): y (N, H, W, 64) NHWC fp32 = conv(x, w (64, 1, 5, 5)) + b (b may be null); dx (N, 1, H, W) from
 * dy (N, H, W, 64); dW (64, 1, 5, 5) and db (64, may be null) from x and dy (workspace:
 * avse_conv1_wgrad_workspace_bytes).  W >= 128 for the forward. */
int avse_conv1_fwd(int64_t N, int64_t H, int64_t W, const float* x, const float* w, const float* b, float* y,
                   avse_stream_t stream);
int avse_conv1_dgrad(int64_t N, int64_t H, int64_t W, const float* dy, const float* w, float* dx, avse_stream_t stream);
int64_t avse_conv1_wgrad_workspace_bytes(int64_t N, int64_t H, int64_t W);
int avse_conv1_wgrad(int64_t N, int64_t H, int64_t W, const float* x, const float* dy, float* dw, float* db,
                     float* workspace, avse_stream_t stream);
/* AudioFeatNet.convf = nn.Conv2d(64, 4, 1) (baseline/avse1/model.py:211-213, called at :246-249) on npix NHWC pixels
 * (csrc/convf.hip): y (npix, 4) = x (npix, 64) W^T (4, 64) + b (b may be null); dx (npix, 64) = dy (npix, 4) W; dW (4, 64)
 * and db (4, may be null) = sums over the pixels (workspace: avse_convf_wgrad_workspace_bytes).  x, dy, dx, W 16-B
 * aligned. */
int avse_convf_fwd(int64_t npix, const float* x, const float* w, const float* b, float* y, avse_stream_t stream);
int avse_convf_dgrad(int64_t npix, const float* dy, const float* w, float* dx, avse_stream_t stream);
int64_t avse_convf_wgrad_workspace_bytes(int64_t npix);
int avse_convf_wgrad(int64_t npix, const float* x, const float* dy, float* dw, float* db, float* workspace,
                     avse_stream_t stream);

int64_t avse_sconv_wprep_bytes(int64_t co, int64_t ci);
int avse_sconv_wprep(int64_t co, int64_t ci, const float* w, int32_t transposed, void* wq, uint32_t* wmax,
                     avse_stream_t stream);
int avse_sconv_fwd(int64_t N, int64_t Hi, int64_t Wi, int64_t ci, int64_t co, int64_t stride, const void* xq,
                   const uint32_t* xmax, const void* wq, const uint32_t* wmax, float* y, avse_stream_t stream);
int64_t avse_sconv_wgrad_workspace_bytes(int64_t N, int64_t Hi, int64_t Wi, int64_t ci, int64_t co, int64_t stride);
int avse_sconv_dgrad2_supported(int64_t N, int64_t Hi, int64_t Wi, int64_t ci, int64_t co);
int avse_sconv_dgrad2(int64_t N, int64_t Hi, int64_t Wi, int64_t ci, int64_t co, const void* dyq,
                      const uint32_t* dymax, const void* wq, const uint32_t* wmax, float* dx, avse_stream_t stream);
int avse_sconv_wgrad(int64_t N, int64_t Hi, int64_t Wi, int64_t ci, int64_t co, int64_t stride, const void* xq,
                     const uint32_t* xmax, const void* dyq, const uint32_t* dymax, float* dw, float* workspace,
                     avse_stream_t stream);
int avse_dconv_fwd(int64_t N, int64_t H, int64_t W, int64_t dil, const void* xq, const void* wq,
                   const uint32_t* maxbits, const float* bias, float* y, avse_stream_t stream);
/* The input gradient dx of conv_{i+1}(ReLU(BN_i(bn_x))) (model.py:199-215) = avse_dconv_fwd on the split dY and the
 * transposed weight image, bit for bit, whose workgroups also write the BatchNorm backward's per-channel partial sums
 * over their pixel tile (dz = dx masked by the forward's z > 0, recomputed from bn_x and bn_stats): one row of
 * [nq][64] floats per workgroup, avse_dconv_bn_rows(N, H, W, dil) rows, nq = 4 with want_max (max |dz| too), else 3;
 * avse_bnact_bwd_rows finishes the backward from them.  act: 1 (ReLU) only.  No atomics: deterministic. */
int64_t avse_dconv_bn_rows(int64_t N, int64_t H, int64_t W, int64_t dil);
int avse_dconv_dgrad_bn(int64_t N, int64_t H, int64_t W, int64_t dil, const void* dyq, const void* wq_t,
                        const uint32_t* maxbits, float* dx, const float* bn_x, const float* bn_stats,
                        const float* gamma, const float* beta, int32_t act, int32_t want_max, float* rows,
                        avse_stream_t stream);
/* The same for the stride-1 trunk convolution conv2(PReLU(bn1(bn_x))) of a BasicBlock (resnet.py:40-67): dx (N, H, W,
 * co) = avse_sconv_fwd(N, H, W, ci, co, 1, dyq, ...) on the transposed = 1 weight image, bit for bit, plus one row of
 * [nq][co] floats per pixel tile (avse_sconv_bn_rows rows).  act: 2 (PReLU) only, alpha_n 1 or co. */
int64_t avse_sconv_bn_rows(int64_t N, int64_t H, int64_t W, int64_t co);
int avse_sconv_dgrad1_bn(int64_t N, int64_t H, int64_t W, int64_t ci, int64_t co, const void* dyq,
                         const uint32_t* dymax, const void* wq_t, const uint32_t* wmax, float* dx, const float* bn_x,
                         const float* bn_stats, const float* gamma, const float* beta, int32_t act, const float* alpha,
                         int32_t alpha_n, int32_t want_max, float* rows, avse_stream_t stream);
/* Weight (and bias) gradient of the same convolution from the split input xq (max bits *xmax) and the split output
 * gradient dyq (*dymax): dw (64, 64, 5, 5), db (64) or NULL; workspace avse_dconv_wgrad16_workspace_bytes() (partial
 * slabs, every one written by every launch).  N, H >= 1, W >= 64, dil in {2, 4, 8, 16}.  Persistent workgroups walk the
 * rows of one residue class h mod dil in steps of dil, so that each input-row segment and each dy segment is staged
 * once for all 25 taps; slabs are summed in a fixed order: no atomics, two calls give the same bits. */
int64_t avse_dconv_wgrad16_workspace_bytes(int64_t N, int64_t H, int64_t W);
int avse_dconv_wgrad16(int64_t N, int64_t H, int64_t W, int64_t dil, const void* xq, const uint32_t* xmax,
                       const void* dyq, const uint32_t* dymax, float* dw, float* db, float* workspace,
                       avse_stream_t stream);
/* The static plan avse_dconv_wgrad16 launches with (host only, no GPU work): out = { units, steps, 1-KB LDS-DMA pieces
 * per launch, partial slabs, LDS bytes per workgroup, workgroups }. */
int avse_dconv_wgrad16_plan(int64_t N, int64_t H, int64_t W, int64_t dil, int64_t out[6]);

/* ---------------------------------------------------------------- MBSTOI scoring (fp64) ------
 * The binaural intelligibility metric the AVSE-4 challenge ranks by (evaluation/avse4/objective_evaluation.py:60-69,
 * mbstoi/mbstoi.py:31-334 with its defaults: 10 kHz, frame 256, hop 128, FFT 512, 15 third-octave bands from 150 Hz,
 * segments of 30 frames, 40 dB dynamic range), after the resampling of mbstoi.py:107-124, which the caller does.
 * sig: (batch, 4, max_len) fp64, rows clean left, clean right, processed left, processed right; len[b] <= max_len
 * is utterance b's own sample count (device int32).  F = avse_mbstoi_frames(max_len) = len(range(0, max_len - 256,
 * 128)) frame slots per utterance (exclusive end: 256 + 128 k samples give k frames).  window: the 256 doubles
 * hanning(258)[1:-1].  Everything stays on the device; no entry point synchronises.  No float atomics: the same bits
 * from run to run, and for an utterance alone as inside a batch. */
int64_t avse_mbstoi_frames(int64_t len);
/* bytes of avse_mbstoi_gate's workspace (the frame energies) */
int64_t avse_mbstoi_workspace_bytes(int64_t batch, int64_t max_len);
/* Silent-frame gate (mbstoi_utils.py:392-484): frame energies 20 log10(|windowed frame| + eps) of the two clean ears, a
 * frame is kept if max - 40 - e < 0 for either ear.  kept (batch, F) int32: the kept frame indices in ascending order,
 * then -1; count (batch) int32: K[b], how many. */
int avse_mbstoi_gate(int64_t batch, int64_t max_len, const double* sig, const int32_t* len, const double* window,
                     double* workspace, int32_t* kept, int32_t* count, avse_stream_t stream);
/* STFT of the re-stitched signals (mbstoi_utils.py:361-389 on the overlap-add of :471-482; K kept frames give K - 1 STFT
 * frames) reduced to the third-octave bands of thirdoct (:487-540): bq (batch, F - 1, 15, 8) fp64 = PL, PR, Re rho,
 * Im rho of the clean pair, then of the processed pair, with PL = sum |X_L|^2, PR = sum |X_R|^2, rho = sum conj(X_R)
 * X_L over the band's bins (the quantities of :126-143); frames from K[b] - 1 on are written as zeros.  F >= 2. */
int avse_mbstoi_bands(int64_t batch, int64_t max_len, const double* sig, const double* window, const int32_t* kept,
                      const int32_t* count, double* bq, avse_stream_t stream);
/* Equalisation-cancellation grid search (mbstoi_utils.py:17-224) and better-ear selection (mbstoi.py:279-329) per cell
 * (utterance, band, segment j of frames j .. j + 29).  bq (batch, frame_slots, 15, 8); utterance b has
 * frames[b] - frames_offset STFT frames (frames_offset 1: frames = the gate's count K; 0: a frame count).
 * tau_table (15, n_taus, 6): cos(w tau), -sin(w tau), cos(2 w tau), -sin(2 w tau), deltexp, exp(-w^2 sigma_delta^2 / 2);
 * gamma_table (n_gammas, 6): 10^g, 10^-g, 10^2g, 10^-2g, epsexp, exp(ln(10)^2 sigma_eps^2 / 2) (mbstoi.py:200-212,
 * mbstoi_utils.py:78-95), n_gammas <= 64.  d (batch, 15, frame_slots - 29): the intermediate correlation after the
 * better-ear selection, 0 outside the utterance's own frames[b] - frames_offset - 29 segments.  Optional, same
 * shape: d_ec (before the selection), p_ec (p_ec_max), winner (int32, tau index * n_gammas + gamma index of the first
 * maximum in the reference's order; -1 where the `-1` rule of :208 fired or outside the utterance). */
int avse_mbstoi_ec(int64_t batch, int64_t frame_slots, const int32_t* frames, int32_t frames_offset, int64_t n_taus,
                   int64_t n_gammas, const double* bq, const double* tau_table, const double* gamma_table, double* d,
                   double* d_ec_or_null, double* p_ec_or_null, int32_t* winner_or_null, avse_stream_t stream);
/* score (batch) fp64: the mean of d over the utterance's own 15 x segments cells (mbstoi.py:330), NaN with none, summed
 * in an order that depends on the utterance's segment count alone. */
int avse_mbstoi_score(int64_t batch, int64_t frame_slots, const int32_t* frames, int32_t frames_offset, const double* d,
                      double* score, avse_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AVSE_HIP_H */
