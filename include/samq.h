/*
 * libsamq_hip.so -- C ABI of the MI355X (gfx950) quantized SAM image-encoder hot path.
 *
 * Drop-in boundary for the reference's Python/Triton path (zhanglei1172/sam-quantization):
 * every entry point below names the reference interface it replaces (file:line, relative to
 * the reference repository).  Conventions:
 *   - all tensor arguments are DEVICE pointers on the current HIP device, caller-owned and
 *     caller-allocated (no globals: the reference's shared `workspace`,
 *     gptq_triton/quant_linear.py:13, is gone, so calls are reentrant);
 *   - every launch is enqueued on the explicit `stream` (0 = legacy default stream);
 *     nothing synchronises the host, so a caller may capture any sequence into a hipGraph;
 *   - return 0 on success, a negative SAMQ_ERR_* on failure; samq_last_error() returns a
 *     thread-local message.  The Python layer maps SAMQ_ERR_INVALID -> AssertionError
 *     (the reference's shape asserts, quant_linear.py:378-399), SAMQ_ERR_UNSUPPORTED ->
 *     NotImplementedError (quant_linear.py:72-73, fused_attention.py:134-135) and
 *     SAMQ_ERR_HIP -> RuntimeError;
 *   - an empty batch (zero rows / tokens / images: M, rows, n or B == 0) returns 0 before any
 *     pointer is checked or dereferenced (an empty tensor's data pointer may be null).
 * Data types: "f16" = IEEE binary16, "f32" = binary32; int4 weights use the reference's
 * GPTQ packing (qweight int32 (K/8,N), qzeros int32 (G,N/8), scales f16 (G,N),
 * gptq4sam.py:434-497) -- repacked once per layer by samq_w4_repack.
 */
#ifndef SAMQ_H
#define SAMQ_H

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAMQ_OK 0
#define SAMQ_ERR_INVALID (-1)
#define SAMQ_ERR_UNSUPPORTED (-2)
#define SAMQ_ERR_HIP (-3)

/* GEMM epilogues (y = acc * scale[n] + bias[n]) */
#define SAMQ_EPI_BIAS 0        /* C f16  = y                        (QuantLinear.forward)     */
#define SAMQ_EPI_BIAS_GELU 1   /* C f16  = GELU_erf(y)              (MLPBlock lin1 + act)     */
#define SAMQ_EPI_RESADD_F32 2  /* C f32 += y (in place)             (Block residual adds)     */
#define SAMQ_EPI_F32 3         /* C f32  = y                                                  */
/* int8-activation GEMMs only (samq_w8a8_gemm / samq_w4a8_gemm); C = int8 codes, q(v, s) =
 * clamp(round_half_even(v / s), -128, 127) (fq_vit quantizer/uniform.py:23-45) */
#define SAMQ_EPI_Q8 4          /* C i8 = q(y, out_scale)                  (Linear -> QAct)        */
#define SAMQ_EPI_Q8_GELU 5     /* C i8 = q(GELU(y), out_scale)            (lin1 -> GELU -> QAct)  */
#define SAMQ_EPI_Q8_RES 6      /* C i8 = q(R*res_scale + q(y,mid)*mid, out_scale)  (residual)   */

/* Thread-local description of the last failure on this thread ("" if none). */
const char* samq_last_error(void);
/* ABI version of this library (major*100 + minor). */
int samq_version(void);

/* ---------------------------------------------------------------- W4A16 (GPTQ int4) */

/* Number of int32 words of the repacked weight of a K x N layer (= K*N/8). */
size_t samq_w4_packed_words(int K, int N);

/* Repack a reference `QuantLinear.qweight` (int32 (K/8, N), gptq_triton/quant_linear.py:81-85)
 * into the kernel's MFMA-fragment order.  K % 64 == 0, N % 32 == 0.  Called once per layer
 * by load_quant (replaces the reference's per-call B-tile addressing, quant_linear.py:292-294). */
int samq_w4_repack(const int32_t* qweight, int32_t* packed, int K, int N, hipStream_t stream);

/* Same with an explicit fragment layout: 1 = the W4A16 layout (32x32x16 MFMA order, what
 * samq_w4_repack produces and every samq_w4a16_gemm_cfg config of this library consumes),
 * 3 = the W4A8 layout (samq_w4a8_gemm / samq_i8_gemm_cfg).  Any other value returns
 * SAMQ_ERR_INVALID. */
int samq_w4_repack_layout(const int32_t* qweight, int32_t* packed, int K, int N, int layout,
                          hipStream_t stream);

/* C = epilogue(A[M,K] (f16, row stride lda) x W4[K,N]).  Replaces triton_matmul4 +
 * matmul4_kernel (gptq_triton/quant_linear.py:355-437, 231-352) and the separate `c + bias`
 * (:434-435).  wpacked from samq_w4_repack; scales f16 (G,N); qzeros int32 (G,N/8);
 * bias f16 (N) or NULL; groupsize -1 (== K) or a multiple of 64.  C is f16 for
 * SAMQ_EPI_BIAS / SAMQ_EPI_BIAS_GELU and f32 (row stride ldc) for the F32 epilogues.
 * Shapes: K % 64 == 0, N % 32 == 0 (a superset of the reference's K%128/N%256). */
int samq_w4a16_gemm(const void* A, int64_t lda, const int32_t* wpacked, const void* scales,
                    const int32_t* qzeros, const void* bias, void* C, int64_t ldc, int M, int N,
                    int K, int groupsize, int epilogue, hipStream_t stream);

/* Same with an explicit tile configuration (0 = automatic); for tests and in-graph A/B runs.
 * All accept layout-1 weights and compute the same result (up to fp32 summation order).  N must
 * be a multiple of the tile's BN (BM x BN below).
 *   v1, register-staged B; any C alignment; per-channel and grouped weights:
 *     1 256x256  2 256x128  3 128x128  4 64x64  5 64x32  6 128x256 (1 wave row)
 *     7 256x256 (8 waves in N)  9 128x256
 *   v3, LDS-DMA ring; C 16-byte aligned, ldc % 8 == 0; per-channel and grouped weights:
 *     21 256x256  22 128x256  23 128x128  24 256x128  25 128x256 (1 wave row)  26 64x64
 *     29 128x320  30 256x320  31 128x320 (1 wave row)
 *   v6 ping-pong, all 256x256; C 16-byte aligned, ldc % 8 == 0:
 *     55  3 ring slots, lookahead 2          56  4 slots, lookahead 2
 *     57  4 slots, lookahead 3 (the default for wide N)
 *     58  56 with one phase per K tile       62  4x2 waves of 64x128 instead of 2x4 of 128x64
 *     64  57 on 16x16x32 MFMA (the default for N < 2048)      65  56 on 16x16x32 MFMA
 *     100 / 101  57 / 64 with the LDS-DMA issue spread through the MFMA burst
 *     104  57 with transposed accumulators and an f16-staged epilogue: SAMQ_EPI_BIAS /
 *          SAMQ_EPI_BIAS_GELU only (SAMQ_ERR_UNSUPPORTED for the f32 outputs)
 *     107 / 108  57 / 64 persistent (one workgroup per CU loops over the tiles)
 *     109 / 110  57 / 64 with the epilogue's scale / bias loaded before the main loop
 *     111  57 with f16 outputs staged transposed (f32 outputs run 57 itself)
 *     112 / 113  for grouped weights 57 / 64 with the group rows prefetched into registers;
 *          for per-channel weights 57 / 64 themselves
 *     114  57 (the grouped form of 57 under its own id)
 *   Of the ping-pong configs 57, 64, 112, 113 and 114 take grouped weights (groupsize < K); the
 *   others return SAMQ_ERR_INVALID for them.
 * Any other id (the tuning build's timing-only configs among them) returns SAMQ_ERR_INVALID
 * with "unknown tile config". */
int samq_w4a16_gemm_cfg(const void* A, int64_t lda, const int32_t* wpacked, const void* scales,
                        const int32_t* qzeros, const void* bias, void* C, int64_t ldc, int M,
                        int N, int K, int groupsize, int epilogue, int cfg, hipStream_t stream);

/* LayerNorm folded into the projection GEMMs around it (the W4A16 encoder block's norm2 between
 * proj and lin1, and the next block's norm1 between lin2 and qkv; image_encoder.py:194-207):
 * the HBM round trip of a standalone LayerNorm (read the f32 residual, write the f16 normalised
 * rows) is replaced by exact algebra,  LN(x).W = rstd*((x - mu_p)*gamma).W - rstd*delta*(gamma.W)
 * + beta.W,  with mu_p the row mean of the PREVIOUS LayerNorm of the same row (so the f16 operand
 * (x - mu_p)*gamma carries no large mean) and delta = mean(x) - mu_p from per-row partial sums:
 *   SAMQ_EPI_RESADD_LNF (producer, C f32 [M,N] residual x += y in place), then
 *     aout f16 [M,N] = f16((x_new - mu[r]) * gamma[n]) and, per 64-column block b,
 *     stats[(r*(N/64) + b)*2 + {0,1}] = sum over the block of (x_new - mu[r]), (x_new - mu[r])^2;
 *   SAMQ_EPI_BIAS_LNF / SAMQ_EPI_GELU_LNF (consumer, A = the producer's aout, K = its N):
 *     delta = S1/K, rstd = 1/sqrt(S2/K - delta^2 + eps) from stats[r, 0..K/64),
 *     C f16 = y = rstd*(acc*scale[n] - delta*gw[n]) + bw[n] + bias[n]  (GELU_erf(y) for GELU_LNF),
 *     gw = gamma.W, bw = beta.W (f32 [N], the next LayerNorm's weights times this layer's dequantised
 *     weight); the tiles of column block 0 set mu[r] += delta (the next producer's mu_p). */
#define SAMQ_EPI_RESADD_LNF 7
#define SAMQ_EPI_BIAS_LNF 8
#define SAMQ_EPI_GELU_LNF 9
#define SAMQ_EPI_SILU_MUL 10   /* internal: the samq_w4a16_gated_mlp epilogue */
/* samq_w4a16_gemm_cfg with the LayerNorm-fold epilogues above (ping-pong configs 57 / 64 / 0 =
 * automatic at M >= 8192 only, else SAMQ_ERR_UNSUPPORTED): gamma f32 [N] (producer), gw / bw f32
 * [N] (consumer), stats f32, mu f32 [M], aout f16 [M,N] (producer), eps of the folded LayerNorm.
 * The consumer stages its 256 rows' partial sums in LDS: K <= 3008 (cfg 57) / 3968 (cfg 64) for
 * per-channel weights, K <= 1728 / 2688 for grouped ones (3-slot rings), else SAMQ_ERR_UNSUPPORTED. */
int samq_w4a16_gemm_lnf(const void* A, int64_t lda, const int32_t* wpacked, const void* scales,
                        const int32_t* qzeros, const void* bias, void* C, int64_t ldc, int M, int N, int K,
                        int groupsize, int epilogue, int cfg, const float* gamma, const float* gw,
                        const float* bw, float* stats, float* mu, void* aout, float eps, hipStream_t stream);

/* ---------------------------------------------------------------- int8 activations */

/* fq_vit int8 weights: W int8 [N][K] row-major (QLinear / flattened QConv2d weight codes,
 * fq_vit/models/ptq/layers.py:160-200, 11-74) -> int8 MFMA fragment order (K*N bytes).
 * K % 128 == 0, N % 32 == 0, 16-byte aligned pointers. */
int samq_w8_repack(const int8_t* w, int8_t* packed, int K, int N, hipStream_t stream);

/* W8A8 GEMM (fq_vit QLinear in quant mode, layers.py:190-200, fed by the int8 codes of the
 * preceding QAct, layers.py:203-242):  y[m,n] = float(sum_k A[m,k] W[n,k]) * a_scale *
 * wscale[n] + bias[n] (int32 exact sum), then the epilogue (SAMQ_EPI_*; Q8_RES reads the int8
 * residual codes R (row stride ldr; may alias C) with res_scale and quantises y with mid_scale
 * first when mid_scale > 0).  A int8 [M,K] (16-byte aligned, lda % 16 == 0); wpacked from
 * samq_w8_repack; wscale/bias f32 [N] (bias may be NULL); K % 128 == 0, N % 64 == 0. */
int samq_w8a8_gemm(const int8_t* A, int64_t lda, const int8_t* wpacked, const float* wscale,
                   const float* bias, void* C, int64_t ldc, const int8_t* R, int64_t ldr, int M,
                   int N, int K, int epilogue, float a_scale, float mid_scale, float res_scale,
                   float out_scale, hipStream_t stream);

/* W4A8 GEMM: GPTQ int4 weights (QuantLinear buffers, gptq_triton/quant_linear.py:81-85, repacked
 * with samq_w4_repack_layout(..., layout 3, ...)) x int8 activation codes (fq_vit QAct on the
 * QuantLinear input, SURVEY.md §8c "Oracle W4A8"): y = float(sum_k A (q - zp)) * a_scale *
 * wscale[n] + bias[n]; wscale = the QuantLinear scales as f32 [G, N] (G = 1 per-channel);
 * epilogues BIAS/BIAS_GELU (f16 out), RESADD_F32/F32, Q8/Q8_GELU.  groupsize -1 (== K), or a
 * multiple of 128 (grouped weights, quant_linear.py:324-335: per group g = k / groupsize the
 * exact int32 sum over the group times wscale[g, n], summed in f32; qzeros [G, N/8]); other
 * groupsizes SAMQ_ERR_UNSUPPORTED. */
int samq_w4a8_gemm(const int8_t* A, int64_t lda, const int32_t* wpacked, const float* wscale,
                   const int32_t* qzeros, const float* bias, void* C, int64_t ldc, int M, int N,
                   int K, int groupsize, int epilogue, float a_scale, float out_scale,
                   hipStream_t stream);
/* The same with an explicit tile config (0 = automatic; per-channel: as samq_i8_gemm_cfg; grouped:
 * 83 128x128, 84 64x64, 87 128x64, 88 64x128, the other ids of samq_i8_gemm_cfg return
 * SAMQ_ERR_INVALID for grouped weights).  Any id samq_i8_gemm_cfg does not list returns
 * SAMQ_ERR_INVALID with "unknown tile config". */
int samq_w4a8_gemm_cfg(const int8_t* A, int64_t lda, const int32_t* wpacked, const float* wscale,
                       const int32_t* qzeros, const float* bias, void* C, int64_t ldc, int M, int N,
                       int K, int groupsize, int epilogue, float a_scale, float out_scale, int cfg,
                       hipStream_t stream);

/* samq_w8a8_gemm with the Q8 epilogue (the fq_vit qkv QLinear + attn.qact1) that also stores the
 * codes of output columns [v_col0, N) as fp16 values into v16 [M, ldv] (column c at c - v_col0): the V
 * third of qkv for samq_rel_attention_q8_rows' v16.  v_col0 % 64 == 0.  cfg: 0 = automatic or a
 * tile config of samq_i8_gemm_cfg that takes W8 weights. */
int samq_w8a8_gemm_v16(const int8_t* A, int64_t lda, const int8_t* wpacked, const float* wscale,
                       const float* bias, int8_t* C, int64_t ldc, int M, int N, int K, float a_scale,
                       float out_scale, void* v16, int v_col0, int64_t ldv, int cfg, hipStream_t stream);

/* Per-channel W4A8 GEMM with the zero point's row sums moved to the producers:
 * rowsum_in (optional, int32 [M]) = S[m] = sum_k A[m, k] of the int8 input rows -- the ping-pong
 * kernel (cfg 86) then subtracts zp[n] * S[m] without re-summing A per column tile; the other tile
 * configs ignore it.  cfg as for samq_i8_gemm_cfg with W4 weights.  rowsum_out (optional, int32 [M], ZEROED by the caller;
 * epilogue Q8 / Q8_GELU only) accumulates the row sums of the int8 output codes with atomics, the
 * next GEMM's rowsum_in (replaces the per-tile row sums of quant_linear.py:299-343's zero-point
 * subtraction; fq_vit uniform.py:23-45 codes).  Outputs are bit-identical to samq_w4a8_gemm_cfg. */
int samq_w4a8_gemm_rs(const int8_t* A, int64_t lda, const int32_t* wpacked, const float* wscale,
                      const int32_t* qzeros, const float* bias, void* C, int64_t ldc, int M, int N, int K,
                      int epilogue, float a_scale, float out_scale, const int32_t* rowsum_in,
                      int32_t* rowsum_out, int cfg, hipStream_t stream);

/* Both int8 GEMMs with an explicit weight format (0 = W8 packed, 1 = W4 layout 3) and tile
 * config; for tuning and tests.  cfg (N must be a multiple of the tile width, else
 * SAMQ_ERR_INVALID):
 *     0  automatic
 *     3-slot LDS ring (W4: 3 slots, W8: 2 for 81): 81 256x256, 82 128x256, 83 128x128, 84 64x64,
 *          87 128x64, 88 64x128
 *     2-slot ring: 89 64x64, 90 64x128, 91 32x64, 92 64x32, 180 128x128, 181 128x64,
 *          182 128x128 on 8 waves
 *     85 / 86  W4 only (SAMQ_ERR_INVALID for W8): the 256x256 ping-pong kernel; 86 with the zero
 *          point through the row sums of A (K < 65536, else SAMQ_ERR_UNSUPPORTED)
 * Any other id (the tuning build's timing-only configs among them) returns SAMQ_ERR_INVALID
 * with "unknown tile config". */
int samq_i8_gemm_cfg(const int8_t* A, int64_t lda, int bfmt, const void* wpacked, const float* wscale,
                     const int32_t* qzeros, const float* bias, void* C, int64_t ldc, const int8_t* R,
                     int64_t ldr, int M, int N, int K, int epilogue, float a_scale, float mid_scale,
                     float res_scale, float out_scale, int cfg, hipStream_t stream);

/* W8A8 convolution as an implicit GEMM (fq_vit QConv2d on int8 codes, layers.py:11-74): the A
 * operand is gathered from the code map by the LDS-DMA loader, no im2col copy.
 *   mode 1 (PatchEmbed, fq_vit image_encoder.py PatchEmbed): x int8 [B, Cin, side, side] NCHW,
 *     16x16 patches stride 16; weight codes flattened (n, c, kh, kw) (K = Cin*256);
 *   mode 2 (neck 3x3, padding 1, image_encoder.py:88-104): x int8 [B, side, side, Cin] NHWC,
 *     Cin % 128 == 0; weight codes permuted to (n, ky, kx, c) (K = 9*Cin).
 * Weights from samq_w8_repack; output C int8 [B*G*G, N] codes (row stride N) with epilogue Q8 or
 * Q8_RES as samq_w8a8_gemm; Q8_RES reads residual codes R [rmod, N] at row (r % rmod) when
 * rmod > 0 (the pos_embed codes shared by every image), else R [B*G*G, N]. */
int samq_w8a8_conv_gemm(const int8_t* x, int mode, int B, int Cin, int side, const int8_t* wpacked,
                        const float* wscale, const float* bias, void* C, const int8_t* R, int rmod,
                        int N, int epilogue, float a_scale, float mid_scale, float res_scale,
                        float out_scale, hipStream_t stream);

/* Elementwise activation quantiser (fq_vit QAct in quant mode, layers.py:232-242 ->
 * UniformQuantizer.forward, quantizer/base.py:43-49, uniform.py:23-45, zero point 0):
 * codes[i] = q(x[i], scale); x f32 (or f16 with SAMQ_Q_IN_F16); with SAMQ_Q_OUT_FQ the output is
 * the f32 fake-quant value codes*scale instead of int8 codes. */
#define SAMQ_Q_IN_F16 1
#define SAMQ_Q_OUT_FQ 2
int samq_quantize(const void* x, void* y, int64_t n, float scale, int flags, hipStream_t stream);

/* ---- int8 activations with zero points (fq_vit asymmetric QActs: the omse observer, uint8
 * BIT_TYPE_A).  A quantiser is (scale, zp), zp an integer in [-128, 127] (else SAMQ_ERR_INVALID):
 *   code = clamp(rint(fl(fl(x / s) + zp)), -128, 127),  value = (code - zp) * s
 * -- the zero point is added to the correctly rounded fp32 quotient BEFORE the round-half-even
 * (quantizer/uniform.py:31-33).  With every zero point 0 (and col_offset NULL) each entry below is
 * bit-identical to the entry it extends. */

/* samq_quantize with an output zero point; SAMQ_Q_OUT_FQ gives (code - zp) * scale. */
int samq_quantize_zp(const void* x, void* y, int64_t n, float scale, int zp, int flags, hipStream_t stream);

/* samq_layernorm_q with zero points: SAMQ_LN_IN_I8 reads x = (code - zp_in) * in_scale (the
 * subtraction in integers); SAMQ_LN_OUT_I8 writes the codes of (out_scale, zp_out), with
 * SAMQ_LN_OUT_F32 as well the f32 fake-quant value (code - zp_out) * out_scale. */
int samq_layernorm_q_zp(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C,
                        float eps, int flags, float in_scale, float out_scale, int zp_in, int zp_out,
                        hipStream_t stream);

/* samq_i8_gemm_cfg for W8 weights on activations with zero points; epilogues SAMQ_EPI_Q8 / Q8_GELU /
 * Q8_RES (any other: SAMQ_ERR_UNSUPPORTED), cfg 0 or a tile config that takes W8 weights:
 *   y[m,n] = float(sum_k A[m,k] W[n,k] + col_offset[n]) * a_scale * wscale[n] + bias[n]
 * col_offset int32 [N] or NULL (= 0): the input's zero point as -zp_a * sum_k W[n,k], precomputed per
 * layer and added in int32 (exact; it nearly cancels against the sum, so it must not be folded into
 * the float bias).  Q8_RES: residual (R - res_zp) * res_scale, read at row m % rmod when rmod > 0;
 * mid quantiser (mid_scale > 0) (clamp(rint(y / mid_scale + mid_zp)) - mid_zp) * mid_scale; every
 * output quantiser (out_scale, out_zp). */
int samq_i8_gemm_zp(const int8_t* A, int64_t lda, const int8_t* wpacked, const float* wscale, const float* bias,
                    void* C, int64_t ldc, const int8_t* R, int64_t ldr, int M, int N, int K, int epilogue,
                    float a_scale, float mid_scale, float res_scale, float out_scale, int cfg,
                    const int32_t* col_offset, int mid_zp, int res_zp, int out_zp, int rmod, hipStream_t stream);

/* samq_w8a8_conv_gemm on activations with zero points (arguments as samq_i8_gemm_zp).  pad16 (mode 2,
 * required there; 16-byte aligned): 16 device bytes, each the code of the input's zero point -- the
 * 3x3 gather reads them outside the map (a padded value of 0.0 is the code zp, not the code 0), so
 * col_offset holds for border pixels as well. */
int samq_w8a8_conv_gemm_zp(const int8_t* x, int mode, int B, int Cin, int side, const int8_t* wpacked,
                           const float* wscale, const float* bias, void* C, const int8_t* R, int rmod, int N,
                           int epilogue, float a_scale, float mid_scale, float res_scale, float out_scale,
                           const int32_t* col_offset, int mid_zp, int res_zp, int out_zp, const int8_t* pad16,
                           hipStream_t stream);

/* ---- Power-of-Two Factor activations (fq_vit observer/ptf.py; the QActs that feed a LayerNorm under
 * Config(ptf=True)).  A PTF quantiser is (s0, zp, exp[C]): channel c has the scale s0 * 2^exp[c] with
 * exp[c] in 0..3 and the layer's one zero point.  exp arrays are device uint8, 16-byte aligned.
 * Powers of two keep everything exact: fl(x / (s0 2^e)) = fl(x / s0) 2^-e, and
 * (code - zp) (s0 2^e) = ((code - zp) << e) s0.
 *
 * samq_layernorm_q_ptf: samq_layernorm_q_zp (SAMQ_LN_IN_I8 required) on an input under (in_scale,
 * zp_in, in_exp[C]); in_exp must not be NULL.  Outputs as _zp (int8 codes or f32).
 *
 * samq_i8_gemm_ptf: samq_i8_gemm_zp with
 *   out_exp [N]  (NULL = 0) the output quantiser's exponents: column n is quantised under
 *                (out_scale * 2^out_exp[n], out_zp);
 *   res_exp [N]  (NULL = 0, Q8_RES only) the residual's: ((R - res_zp) << res_exp[n]) * res_scale;
 *   k_tiles_a, k_shift0..2  an INPUT with per-k exponents (Q8 only): A has k_tiles_a * 128 columns and K
 *                is P * k_tiles_a * 128, P <= 4 -- wpacked is the repack of P masked copies of W stacked
 *                along K, copy p holding W[n, k] where in_exp[k] == e_p (e_0 > e_1 > ... > e_{P-1} = 0)
 *                and 0 elsewhere; the int32 sums are shifted left by k_shift[p] = e_p - e_{p+1} (1..3)
 *                after pass p < P - 1, unused shifts are 0.  The result is sum_k a_k 2^in_exp[k] W[n, k];
 *                col_offset[n] = -zp_a sum_k 2^in_exp[k] W[n, k].  P = 1: k_tiles_a = K / 128.
 * Built for the tile configs the automatic pick returns for W8 weights (cfg 0, 82, 83, 84, 88, 89, 90);
 * any other is SAMQ_ERR_UNSUPPORTED.  P = 1 with both arrays NULL equals samq_i8_gemm_zp bit for bit.
 *
 * samq_w8a8_conv_gemm_ptf: samq_w8a8_conv_gemm_zp with out_exp. */
int samq_layernorm_q_ptf(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C,
                         float eps, int flags, float in_scale, float out_scale, int zp_in, int zp_out,
                         const uint8_t* in_exp, hipStream_t stream);
int samq_i8_gemm_ptf(const int8_t* A, int64_t lda, const int8_t* wpacked, const float* wscale, const float* bias,
                     void* C, int64_t ldc, const int8_t* R, int64_t ldr, int M, int N, int K, int epilogue,
                     float a_scale, float mid_scale, float res_scale, float out_scale, int cfg,
                     const int32_t* col_offset, int mid_zp, int res_zp, int out_zp, int rmod, const uint8_t* out_exp,
                     const uint8_t* res_exp, int k_tiles_a, int k_shift0, int k_shift1, int k_shift2,
                     hipStream_t stream);
int samq_w8a8_conv_gemm_ptf(const int8_t* x, int mode, int B, int Cin, int side, const int8_t* wpacked,
                            const float* wscale, const float* bias, void* C, const int8_t* R, int rmod, int N,
                            int epilogue, float a_scale, float mid_scale, float res_scale, float out_scale,
                            const int32_t* col_offset, int mid_zp, int res_zp, int out_zp, const int8_t* pad16,
                            const uint8_t* out_exp, hipStream_t stream);

/* The PTF observer's scores (observer/ptf.py:53-72) in one read of a row-major (rows, C) tensor (f32, or
 * f16 with in_f16): sums[c][k] = sum_r (x - (clamp(rint(x / s_k + zp), qmin, qmax) - zp) s_k)^2 with
 * s_k = scale1 * 2^k, k = 0..3; every f32 step as in samq_omse_scores, float64 sums in a fixed order.
 * sums: double [C][4].  The workspace (samq_ptf_scores_workspace(rows, C) bytes, 8-byte aligned) is
 * the caller's. */
size_t samq_ptf_scores_workspace(int64_t rows, int C);
int samq_ptf_scores(const void* x, int64_t rows, int C, int in_f16, float scale1, float zero_point, float qmin,
                    float qmax, double* sums, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* samq_rel_attention_q8_rows on codes with zero points: qkv codes (s_qkv, zp_qkv), the two score
 * quantisers (s_a1, zp_a1) / (s_a2, zp_a2), output codes (s_out, zp_out).  q.k is
 * sum_d (q - zp_qkv)(k - zp_qkv), exact in int32; the rel-pos terms take (q - zp_qkv) s_qkv; the
 * output is softmax . ((v - zp_qkv) s_qkv).  Pad tokens of a window: the codes of qkv_bias under
 * (s_qkv, zp_qkv), or the code zp_qkv (the value 0.0) when qkv_bias is NULL.  v16 must be NULL
 * (SAMQ_ERR_UNSUPPORTED otherwise): the 64 x 64 kernel runs its int8-V form. */
int samq_rel_attention_q8_zp(const int8_t* qkv, const float* qkv_bias, const float* rel_pos_h,
                             const float* rel_pos_w, int8_t* out, int B, int H, int W, int heads, int hd,
                             int window, float sm_scale, float s_qkv, float s_a1, float s_a2, float s_out,
                             int row0, int rows, const void* v16, int zp_qkv, int zp_a1, int zp_a2, int zp_out,
                             hipStream_t stream);

/* Running min / max of a calibration tensor viewed as (rows, C) row-major -- fq_vit
 * MinmaxObserver.update (observer/minmax.py:14-29, reshape_tensor observer/base.py:16-29):
 *   SAMQ_MM_PER_ROW: one value per row     (conv / linear weights, v.reshape(out, -1));
 *   SAMQ_MM_PER_COL: one value per column  (channel-last activations, channel_wise);
 *   SAMQ_MM_ALL:     one scalar            (layer_wise).
 * x f32 (f16 with in_f16); max_io / min_io f32 (rows, C or 1 values): overwritten when init != 0,
 * else merged with max(old, new) / min(old, new).  NaN propagates as in torch.max / torch.min.
 * PER_COL and ALL need a float workspace of samq_minmax_workspace(rows, C, axis) elements. */
#define SAMQ_MM_PER_ROW 0
#define SAMQ_MM_PER_COL 1
#define SAMQ_MM_ALL 2
size_t samq_minmax_workspace(int64_t rows, int C, int axis);
int samq_minmax(const void* x, int64_t rows, int C, int in_f16, int axis, float* max_io, float* min_io,
                int init, float* workspace, size_t workspace_floats, hipStream_t stream);

/* Exact order statistics of a flat tensor -- what fq_vit PercentileObserver.update takes from
 * torch.quantile / np.percentile (observer/percentile.py:27-39).  x: n values, f32 (f16 with
 * in_f16, converted exactly); ranks: HOST array of nranks (1..4) zero-based ranks in [0, n);
 * out (device, f32[nranks]) receives the value at each rank of the sorted tensor; nan_flag
 * (device int) is set to 1 if any input is NaN (out is then unspecified), else 0.  +-0 compare
 * equal, either may be returned.  Radix select on the order-preserving uint32 image of the
 * floats: three histogram passes (11 / 11 / 10 bits) that serve every rank, the bin selection
 * in between on the device; nothing is read back.  1 <= n < 2^40.  The workspace
 * (samq_order_stats_workspace(n, nranks) bytes, 8-byte aligned) is the caller's. */
size_t samq_order_stats_workspace(int64_t n, int nranks);
int samq_order_stats(const void* x, int64_t n, int in_f16, const int64_t* ranks, int nranks, float* out,
                     int* nan_flag, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* The fq_vit OmseObserver candidate scores in one read of the tensor (observer/omse.py:45-49,
 * lp_loss observer/utils.py:9).  cand: device f32 [ncand][2] = (scale, zero_point), ncand 1..96.
 * sums (device f64[ncand]): sums[c] = sum_i e_ci with, in f32 and rounded step by step as torch's
 * separate ops do (IEEE division, no fused multiply-add),
 *   q = clamp(rint(x_i / s_c + zp_c), qmin, qmax);  xq = (q - zp_c) * s_c;  d = x_i - xq;  e = d * d,
 * accumulated in float64 in a fixed order (lane, wave, workgroup, then a second-pass fold): the
 * same sums on every run.  x f32 (f16 with in_f16).  The workspace
 * (samq_omse_scores_workspace(n, ncand) bytes, 8-byte aligned) is the caller's. */
size_t samq_omse_scores_workspace(int64_t n, int ncand);
int samq_omse_scores(const void* x, int64_t n, int in_f16, const float* cand, int ncand, float qmin, float qmax,
                     double* sums, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* Fused gated MLP in ONE launch: C f16 [M, N] = silu(A . Wg) * (A . Wu) with both int4 weight
 * sets in one packed matrix of 2N columns whose 32-column blocks alternate gate block j, up
 * block j (the samq_w4_repack layout-1 blocks interleaved; scales / qzeros interleaved the same
 * way, N2 = 2N, N2 % 256 == 0): each wave's 64-column tile holds a gate block and its up block,
 * the epilogue multiplies them in registers.  fp32 accumulate, exact integer weights (G1).
 * Replaces llama_mlp_fused_4_kernel / triton_llama_mlp_4 (gptq_triton/fused_mlp.py:230-388,
 * 391-477); biases are ignored as there. */
int samq_w4a16_gated_mlp(const void* A, int64_t lda, const int32_t* wpacked, const void* scales,
                         const int32_t* qzeros, void* C, int64_t ldc, int M, int N2, int K, int groupsize,
                         hipStream_t stream);

/* Gated-MLP activation: out f16[i] = silu(gate[i]) * up[i] (f32 inputs).  With two
 * samq_w4a16_gemm(..., SAMQ_EPI_F32) calls it replaces triton_llama_mlp_4 /
 * llama_mlp_fused_4_kernel (gptq_triton/fused_mlp.py:391-477, 230-388). */
int samq_silu_mul(const float* gate, const float* up, void* out, int64_t n, hipStream_t stream);

/* ---------------------------------------------------------------- normalisation */

/* y[r,:] = LayerNorm(x[r,:]) * gamma + beta over C channels (row stride C), f32 statistics.
 * flags: SAMQ_LN_IN_F16 -> x is f16 (else f32); SAMQ_LN_OUT_F32 -> y is f32 (else f16).
 * gamma/beta f32.  Replaces nn.LayerNorm(eps=1e-6) of Block.norm1/norm2
 * (segment_anything/modeling/image_encoder.py:184,187,194,205; build_sam.py:72) and the
 * channel LayerNorm2d of the neck on NHWC tokens (segment_anything/modeling/common.py:31-43). */
#define SAMQ_LN_IN_F16 1
#define SAMQ_LN_OUT_F32 2
/* tuning: rows per wave (1, 2 or 4; 0 = the library default) in bits 16-18 of flags */
#define SAMQ_LN_RPW(n) ((n) << 16)
int samq_layernorm(const void* x, void* y, const float* gamma, const float* beta, int64_t rows,
                   int C, float eps, int flags, hipStream_t stream);
/* samq_layernorm that also writes the row means (f32 [rows]) -- the mu_p of the first folded
 * LayerNorm (SAMQ_EPI_RESADD_LNF) downstream. */
int samq_layernorm_mean(const void* x, void* y, const float* gamma, const float* beta, int64_t rows,
                        int C, float eps, int flags, float* mean_out, hipStream_t stream);

/* LayerNorm with int8 activation codes on either side (fq_vit QIntLayerNorm = nn.LayerNorm
 * between two QActs, layers.py:245-258, fq_vit/models/sam/image_encoder.py:310-331; neck
 * QIntLayerNorm2D eps 1e-5, fq_vit/models/sam/common.py:93-108):
 *   SAMQ_LN_IN_I8:  x = int8 codes * in_scale (else f32 / f16 per SAMQ_LN_IN_F16);
 *   SAMQ_LN_OUT_I8: y = q(LN(x), out_scale) int8 codes; with SAMQ_LN_OUT_F32 as well, y is the
 *   f32 fake-quant value q(..)*out_scale (else f16 / f32 per SAMQ_LN_OUT_F32). */
#define SAMQ_LN_IN_I8 4
#define SAMQ_LN_OUT_I8 8
int samq_layernorm_q(const void* x, void* y, const float* gamma, const float* beta, int64_t rows,
                     int C, float eps, int flags, float in_scale, float out_scale,
                     hipStream_t stream);
/* samq_layernorm_q with int8-code output (SAMQ_LN_OUT_I8) plus rowsum[r] = sum_c y[r, c] (int32
 * [rows], the W4A8 GEMM's rowsum_in) and, when zero_rows is not null, zero_rows[r] = 0 (the
 * accumulator of the next int8-code GEMM's rowsum_out). */
int samq_layernorm_q_rs(const void* x, void* y, const float* gamma, const float* beta, int64_t rows,
                        int C, float eps, int flags, float in_scale, float out_scale, int32_t* rowsum,
                        int32_t* zero_rows, hipStream_t stream);

/* Residual add + LayerNorm (Block.forward's x = x + attn(...) / x = x + mlp(...) followed by the
 * next norm, image_encoder.py:199-207): x f32 [rows, C] += delta (f16 with SAMQ_LN_DELTA_F16,
 * else f32 -- the preceding GEMM's plain-stored output), written back in place, then
 * y = LayerNorm(x) (f16, or int8 codes q(LN(x), out_scale) with SAMQ_LN_OUT_I8).  C <= 1280. */
#define SAMQ_LN_DELTA_F16 16
int samq_add_layernorm(void* x, const void* delta, void* y, const float* gamma, const float* beta,
                       int64_t rows, int C, float eps, int flags, float out_scale, hipStream_t stream);

/* ---------------------------------------------------------------- attention */

/* Multi-head attention with in-kernel decomposed relative-position bias over an image token
 * grid, windowed or global, reading Q/K/V straight from the qkv projection output.
 * Replaces QuantAttention.forward's attention part -- add_decomposed_rel_pos + the Triton
 * `_fwd_kernel1` + `forward` (gptq_triton/fused_attention.py:46-80, 107-149, 159-358) -- AND
 * the window_partition / window_unpartition copies around it
 * (segment_anything/modeling/image_encoder.py:195-202, 282-333):
 *   qkv  f16 [B, H, W, 3, heads, hd]  (the qkv Linear output, natural token order)
 *   out  f16 [B, H, W, heads*hd]      (natural token order; window padding cropped)
 *   window = 0: global attention over the H x W grid (requires H == W, H % 16 == 0);
 *   window = S > 0: attention inside S x S windows of the grid zero-padded to a multiple of S;
 *     padded tokens are keys/values whose q/k/v equal the qkv bias (the reference projects the
 *     zero-padded LayerNorm output), given by qkv_bias (f16 [3*heads*hd]) or zeros if NULL;
 *   rel_pos_h / rel_pos_w f16 [2*side-1, hd] with side = window or H; the width term uses the
 *     query ROW as the table index (reference quirk, image_encoder.py:402 /
 *     fused_attention.py:78).  hd in {64, 80}; side <= 64 and (window == 0 => side % 16 == 0).
 *   sm_scale multiplies q.k (the reference passes head_dim**-0.5). */
int samq_rel_attention(const void* qkv, const void* qkv_bias, const void* rel_pos_h,
                       const void* rel_pos_w, void* out, int B, int H, int W, int heads, int hd,
                       int window, float sm_scale, hipStream_t stream);

/* samq_rel_attention with the W4A8 proj input quantiser folded into its store: out int8
 * [B, H, W, heads*hd] = clamp(rne(fp16(o) / out_scale), -128, 127) -- the fq_vit QAct on the
 * QuantLinear input (fq_vit/models/ptq/layers.py:203-242, quantizer/uniform.py:31-36) applied to
 * the fp16 attention output, bit-identical to samq_rel_attention + samq_quantize.  out_scale > 0. */
int samq_rel_attention_q(const void* qkv, const void* qkv_bias, const void* rel_pos_h,
                         const void* rel_pos_w, int8_t* out, int B, int H, int W, int heads, int hd,
                         int window, float sm_scale, float out_scale, hipStream_t stream);

/* Reference functional API `fused_attention.forward(inp, pos_emb1, pos_emb2, head_num,
 * hidden_dim, sm_scale)` (gptq_triton/fused_attention.py:312-358): attention over each of B
 * independent S x S grids with PRECOMPUTED bias terms rel_h, rel_w f16 [B*heads, S, S, S]
 * (bias[m, n] = rel_h[m, n // S] + rel_w[m, n % S]).  inp f16 [B, S, S, 3*heads*hd],
 * out f16 [B, S, S, heads*hd]. */
int samq_attention_relbias(const void* inp, const void* rel_h, const void* rel_w, void* out, int B,
                           int S, int heads, int hd, float sm_scale, hipStream_t stream);

/* W8A8 attention (fq_vit quant-mode Attention.forward, fq_vit/models/sam/image_encoder.py:437-478,
 * with window_partition / window_unpartition :282-333 folded in) on int8 codes:
 *   qkv  int8 [B, H, W, 3, heads, hd] codes of attn.qact1 (scale s_qkv), natural token order;
 *   scores = q8((q*s_qkv*sm_scale).(k*s_qkv), s_a1) * s_a1            (qact_attn1)
 *   scores = q8(scores + rel_h + rel_w, s_a2) * s_a2                   (use_rel_pos_qact; rel_w
 *            indexed by the query ROW, quirk 1; rel tables f32 [2*side-1, hd])
 *   out  int8 [B, H, W, heads*hd] = q8(softmax(scores) . (v*s_qkv), s_out)     (qact2)
 * window > 0: S x S windows over the grid padded to a multiple of S (pad tokens' q/k/v =
 * q8(qkv_bias f32 [3*heads*hd], s_qkv), or 0 if qkv_bias is NULL), window <= 16;
 * window == 0: global over an H == W <= 64 grid.  hd 64 or 80 (else SAMQ_ERR_UNSUPPORTED). */
int samq_rel_attention_q8(const int8_t* qkv, const float* qkv_bias, const float* rel_pos_h,
                          const float* rel_pos_w, int8_t* out, int B, int H, int W, int heads,
                          int hd, int window, float sm_scale, float s_qkv, float s_a1, float s_a2,
                          float s_out, hipStream_t stream);
/* samq_rel_attention_q8 over a range of the grid's rows (round 6: the W8A8 engine's opt-in row lanes
 * run one image as two concurrent kernel chains): global (window == 0, H == W == 64) -- the queries of
 * grid rows [row0, row0 + rows) against all keys; windows -- the windows of rows [row0, row0 + rows),
 * row0 a multiple of window and rows too unless the range ends at H.  rows < 0: the whole grid.
 * v16 (optional, 16-byte aligned): the V codes as fp16 [B, H, W, heads*hd] (samq_w8a8_gemm_v16) --
 * the 64 x 64 global kernel then stages V without converting it; same output codes. */
int samq_rel_attention_q8_rows(const int8_t* qkv, const float* qkv_bias, const float* rel_pos_h,
                               const float* rel_pos_w, int8_t* out, int B, int H, int W, int heads, int hd,
                               int window, float sm_scale, float s_qkv, float s_a1, float s_a2, float s_out,
                               int row0, int rows, const void* v16, hipStream_t stream);

/* W8A8 attention of the mask decoder's two-way transformer (fq_vit quant-mode Attention.forward
 * between the input projections and out_proj, fq_vit/models/sam/transformer.py:520-537) on int8
 * codes; q [B, Nq, heads*hd] (qact1_1, s_q), k / v [B, Nk, heads*hd] (qact1_2 / qact1_3, s_k / s_v):
 *   a   = q8(float(sum_d q k) * (s_q s_k / sqrt(hd)), s_a1)                 (qact_attn1; exact int32 sum)
 *   out int8 [B, Nq, heads*hd] = q8(softmax(a * s_a1) . (v * s_v), s_out)   (qact2; fp32 softmax)
 * hd 16 or 32 and heads*hd <= 256 (else SAMQ_ERR_UNSUPPORTED); any Nq >= 0, Nk >= 1 (Nq == 0 or
 * B == 0: SAMQ_OK, nothing read).  One launch: Nq <= 16 with Nk > 64 splits the keys over the lanes
 * and waves of a workgroup (exact integer-max / sum combine), everything else runs one lane per
 * query.  16-byte aligned pointers. */
int samq_attention_q8_plain(const int8_t* q, const int8_t* k, const int8_t* v, int8_t* out, int B, int Nq,
                            int Nk, int heads, int hd, float s_q, float s_k, float s_v, float s_a1,
                            float s_out, hipStream_t stream);

/* The adds between two QActs of the mask decoder (transformer.py:141-142, 339, 347-348, 363-364;
 * mask_decoder.py:245) on int8 codes: out[i] = q8(fl(a[i] s_a) + fl(b[i % bmod] s_b), s_out) -- two
 * rounded products and a rounded sum, bit-identical to torch's `x + y` of the two fake-quant f32
 * tensors followed by UniformQuantizer (quantizer/uniform.py:23-45).  b NULL: out = q8(a s_a, s_out)
 * (a QAct on a QAct's output, transformer.py:339 qact_pos).  bmod = b's period in elements (the
 * positional encoding shared over the batch; n when b is not broadcast).  flags: SAMQ_Q_OUT_FQ ->
 * out is the f32 fake-quant value code * s_out, else int8 codes.  16-byte aligned pointers. */
int samq_add_q8(const int8_t* a, float s_a, const int8_t* b, float s_b, int64_t bmod, void* out, int64_t n,
                float s_out, int flags, hipStream_t stream);

/* x = max(x, 0) in place on int8 codes: the ReLU of the decoder's MLPBlock (common.py:65-71 with
 * act = nn.ReLU, transformer.py:317) after samq_w8a8_gemm's SAMQ_EPI_Q8 -- q8(relu(y), s) ==
 * max(q8(y, s), 0) exactly.  x 4-byte aligned. */
int samq_relu_q8(int8_t* x, int64_t n, hipStream_t stream);

/* ---- the mask decoder's tail (mask_decoder.py:251-279) on int8 codes: three launches.
 * ConvTranspose2d(k2 s2) weights stay float (QConvTranspose2d is outside the Sam switches): the
 * fp32 weight [Cin, Cout, 2, 2] is passed as W[n][k] = weight[k][co][kh][kw], n = (2 kh + kw) Cout + co,
 * split w = hi + lo 2^-11 (hi = fp16(w), lo = fp16((w - hi) 2^11)) into two fp16 planes, each in MFMA
 * fragment order: [4 Cout / 32][Cin / 16][64 lanes][8], lane = 32 khalf + nn holds
 * W[32 tile + nn][16 kstep + 8 khalf + 0..7] (ops.convt_split_weight builds them).  All QActs
 * layer-wise, zero point 0.  Empty shapes: SAMQ_OK, nothing read.  16-byte aligned pointers. */

/* output_upscaling[0..2] + qacts[0..2]: x int8 [B*h*w, Cin] token rows (the transformer's keys, s_in)
 *   c0 = q8(s_in * sum_k x w + bias, s0)                       (qacts[0]; fp32-level sum)
 *   c1 = q8(LayerNorm2D over the 64 channels of (c0 s0), s1)    (two-pass fp32 statistics, eps)
 *   out int8 [B, 2h, 2w, 64] (NHWC) = q8(gelu_erf(c1 s1), s2)   (qacts[2])
 * dbg_q0 / dbg_q1 (optional, NULL to skip): the codes c0 / c1 in out's layout.  Cout == 64,
 * Cin % 16 == 0 (else SAMQ_ERR_UNSUPPORTED); any B, h, w >= 0. */
int samq_upscale0_q8(const int8_t* x, const void* w_hi, const void* w_lo, const float* bias, const float* gamma,
                     const float* beta, int8_t* out, int8_t* dbg_q0, int8_t* dbg_q1, int B, int h, int w, int Cin,
                     int Cout, float eps, float s_in, float s0, float s1, float s2, hipStream_t stream);

/* The hypernetwork MLPs and the IoU head (mask_decoder.py:284-362, bare QLinears: one weight scale
 * each) in one launch: MLP j < n_hyper on token 1 + j of q int8 [B, Nt, C] (the transformer's qact4,
 * s_in), MLP n_hyper (the IoU head) on token 0.  w1 [n_hyper + 1][C/4][Hd][4], w2 [..][Hd/4][Hd][4],
 * w3 [..][Hd/4][NO][4] int8 weight codes (4 consecutive k of an output column together; NO =
 * max(no_hyper, no_iou), unused columns zero), b1 / b2 [..][Hd], b3 [..][NO] f32, scales [..][8] f32 =
 * s_w1, s_w2, s_w3, qacts1[0], qacts2[0], qacts1[1], qacts2[1], qact3.  Hidden layer, both quantisers:
 *   c1 = q8(float(sum x w) (s_x s_w) + bias, s1); r = max(c1, 0); c2 = q8(r s1, s2)  (r when s1 == s2)
 * -- bit-identical to samq_w8a8_gemm(SAMQ_EPI_Q8) -> samq_relu_q8 -> samq_add_q8; last layer
 * q8(.., qact3).  hyper int8 [B, n_hyper, no_hyper] codes; iou f32 [B, no_iou] = code * s3.  dbg
 * (optional) int8 [B, n_hyper + 1, 4, Hd]: c1, c2 of both hidden layers.  C % 4 == 0, C <= 1024,
 * Hd % 4 == 0, Hd <= 256, outputs <= 256 (else SAMQ_ERR_UNSUPPORTED); Nt >= 1 + n_hyper. */
int samq_decoder_mlps_q8(const int8_t* q, const void* w1, const void* w2, const void* w3, const float* b1,
                         const float* b2, const float* b3, const float* scales, int8_t* hyper, float* iou,
                         int8_t* dbg, int B, int Nt, int C, int Hd, int n_hyper, int no_hyper, int no_iou,
                         float s_in, hipStream_t stream);

/* output_upscaling[3..4] + qacts[3..4], the mask product and the decoder's qact1: x int8
 * [B, H, W, Cin] (NHWC: samq_upscale0_q8's out, s_in), hyper int8 [B, n_masks, 32] with scales
 * s_hyper f32 [n_masks] (device memory):
 *   c3 = q8(s_in * sum_k x w + bias, s3);  c4 = q8(gelu_erf(c3 s3), s4)       [B, 2H, 2W, 32]
 *   masks f32 [B, n_masks, 2H, 2W] = q8(float(sum_c hyper c4) (s_hyper[m] s4), s_q1) * s_q1
 * (the sum an exact int32 dot).  dbg_q3 / x4 (optional): the codes c3 / c4, NHWC.  Cout == 32,
 * Cin % 16 == 0 (else SAMQ_ERR_UNSUPPORTED). */
int samq_upscale1_masks_q8(const int8_t* x, const void* w_hi, const void* w_lo, const float* bias,
                           const int8_t* hyper, const float* s_hyper, float* masks, int8_t* dbg_q3, int8_t* x4,
                           int B, int H, int W, int Cin, int Cout, int n_masks, float s_in, float s3, float s4,
                           float s_q1, hipStream_t stream);

/* ---------------------------------------------------------------- patch embedding / neck */

/* PatchEmbed (segment_anything/modeling/image_encoder.py:411-442) + pos_embed add (:108-110)
 * as one implicit GEMM: img f16 [B, Cin, S, S] (NCHW, S = img_size), weight f16 [N, Cin*p*p]
 * (the Conv2d weight flattened (c, kh, kw)), bias f32 [N] or NULL, pos f32 [(S/p)^2, N] or NULL
 * -> out f32 [B, S/p, S/p, N] (the residual stream; fp32 accumulate, no fp16 rounding).
 * patch % 8 == 0, Cin*p*p % 32 == 0, N % 128 == 0. */
int samq_patch_embed(const void* img, const void* weight, const float* bias, const float* pos, float* out,
                     int B, int Cin, int img_size, int patch, int N, hipStream_t stream);

/* The same in fp32 end to end (img f32, weight f32, fp32 MFMA): the W4A8 encoder's patch
 * embedding, whose int8 quantiser follows directly (fq_vit image_encoder.py PatchEmbed + QAct).
 * patch % 4 == 0, Cin*p*p % 16 == 0, N % 128 == 0. */
int samq_patch_embed_f32(const float* img, const float* weight, const float* bias, const float* pos,
                         float* out, int B, int Cin, int img_size, int patch, int N, hipStream_t stream);

/* PatchEmbed straight from RAW pixels (SamPredictor.set_image -> set_torch_image,
 * segment_anything/predictor.py:34-90): img uint8 [B, Cin, h, w] (NCHW, h, w <= img_size) is
 * normalised in the A-operand gather exactly as Sam.preprocess does (modeling/sam.py:164-174):
 * (pixel - pixel_mean[c]) / pixel_std[c] (f32 [Cin] each), zero-padded to img_size x img_size;
 * then as samq_patch_embed (weight f16) or, with weight_f32, as samq_patch_embed_f32. */
int samq_patch_embed_u8(const uint8_t* img, int h, int w, const float* pixel_mean, const float* pixel_std,
                        const void* weight, int weight_f32, const float* bias, const float* pos, float* out,
                        int B, int Cin, int img_size, int patch, int N, hipStream_t stream);

/* Neck 1x1 conv, no bias (image_encoder.py:88-104 neck[0]) on the fp32 token rows:
 * x f32 [M, K] (converted to f16 on load, as the reference's fp16 neck), weight f16 [N, K]
 * -> out f16 [M, N].  K % 32 == 0, N % 128 == 0. */
int samq_conv1x1_f32(const float* x, const void* weight, void* out, int64_t M, int N, int K,
                     hipStream_t stream);

/* Neck 3x3 conv, padding 1, no bias (neck[2]) on an NHWC f16 map: x f16 [B, G, G, Cin],
 * weight f16 [N, 3, 3, Cin] (the Conv2d weight permuted (n, ky, kx, c)) -> out f16 [B, G, G, N].
 * Cin % 32 == 0, N % 128 == 0. */
int samq_conv3x3_nhwc(const void* x, const void* weight, void* out, int B, int G, int Cin, int N,
                      hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SAMQ_H */
