// The tail of the fq_vit W8A8 mask decoder (fq_vit/models/sam/mask_decoder.py:251-279) on int8
// codes, three launches behind the two-way transformer:
//  * upscale0: ConvTranspose2d(C -> 64, k2 s2) + qacts[0] + LayerNorm2D + qacts[1] + GELU + qacts[2];
//  * decoder_mlps: the hypernetwork MLPs and the IoU head (3 bare QLinears each, ReLU between);
//  * upscale1_masks: ConvTranspose2d(64 -> 32, k2 s2) + qacts[3] + GELU + qacts[4], the product with
//    the hypernetwork rows and the decoder's qact1 -> the low-res masks.
// A k2 s2 transposed convolution is one GEMM row per input pixel, [pixels, Cin] x [Cin, 4 Cout] with
// column (kh, kw, co): output pixel (2y + kh, 2x + kw) has no other contributor.  The convolutions
// keep the reference's FLOAT weights (QConvTranspose2d is outside the Sam switches' type list): the
// fp32 weight is split w = hi + lo 2^-11 (two fp16, conv_gemm.hip's split8), the int8 activation
// codes are exact in fp16, so two v_mfma_f32_32x32x16_f16 per fragment give the fp32-level sum
// acc_hi + acc_lo 2^-11.  64 input pixels per workgroup, wave w of 4 owns sub-pixel (kh, kw) = w:
// every channel of an output pixel lies in one wave's accumulators, and a per-wave LDS tile turns
// them into one output pixel per lane for the channel statistics / the mask dot products.
// Both operands are read as MFMA fragments straight from global memory (the weights pre-ordered by
// fragment at engine build, 1 KiB contiguous per fragment; the 16 KiB of codes of a tile from L1):
// K is 256 / 64, too short for an LDS pipeline to pay.
// GELU between two quantisers is a map from 256 codes to codes: each workgroup builds it once with
// the exact erf form (one erff per thread) and the per-element work is a table look-up.
#include "common.h"

namespace samq {

// B fragment (ntile, kstep) of a [N][K] fp16 matrix in fragment order: 64 lanes x 8 halves, lane =
// 32 * khalf + n: W[ntile * 32 + n][kstep * 16 + 8 * khalf + 0..7]
__device__ __forceinline__ half8_t tail_bfrag(const _Float16* w, int ntile, int ksteps, int ks, int lane) {
  return *(const half8_t*)(w + (((int64_t)ntile * ksteps + ks) * 64 + lane) * 8);
}

// 8 consecutive int8 codes -> fp16 (exact)
__device__ __forceinline__ half8_t tail_afrag(const int8_t* p) {
  const uint2 v = *(const uint2*)p;
  half8_t r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[j] = (_Float16)(int)(int8_t)((v.x >> (8 * j)) & 0xFFu);
    r[4 + j] = (_Float16)(int)(int8_t)((v.y >> (8 * j)) & 0xFFu);
  }
  return r;
}

// lut[c + 128] = q8(gelu(c s_in), s_out): GELU between two layer-wise quantisers, on the codes
__device__ __forceinline__ void tail_gelu_lut(int8_t* lut, int tid, float s_in, float s_out) {
  if (tid < 256) lut[tid] = (int8_t)(int)q8_exact(gelu_erf((float)(tid - 128) * s_in), s_out, 1.0f / s_out);
}

struct Up0Args {
  const int8_t* x;       // [B * h * w, Cin] codes (token rows)
  const _Float16* wh;    // fragment-ordered hi / lo planes of the [4 * 64][Cin] weight
  const _Float16* wl;
  const float* bias;     // [64]
  const float* gamma;    // [64]
  const float* beta;
  int8_t* out;           // [B, 2h, 2w, 64] codes of qacts[2]
  int8_t* dbg0;          // optional: codes of qacts[0], same layout
  int8_t* dbg1;          // optional: codes of qacts[1]
  int B, h, w, Cin;
  float s_in, s0, s1, s2, eps;
};

__global__ __launch_bounds__(256) void upscale0_kernel(Up0Args a) {
  constexpr int CO = 64, PITCH = CO / 4 + 1;   // dwords per row of codes; odd: a lane per row reads conflict-free
  __shared__ uint32_t tile[4][64 * PITCH];
  __shared__ int8_t lut[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hsel = lane >> 5;
  const int hw = a.h * a.w;
  const int M = a.B * hw;
  const int m0 = blockIdx.x * 64;
  const int ksteps = a.Cin / 16;
  tail_gelu_lut(lut, tid, a.s1, a.s2);

  float16_t acc[2][2], accx[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][t][r] = accx[i][t][r] = 0.f;
  const int8_t* xa[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int row = m0 + i * 32 + (lane & 31);
    row = row < M ? row : M - 1;   // rows past the end: read the last row, never stored
    xa[i] = a.x + (int64_t)row * a.Cin + 8 * hsel;
  }
  // the next K step's fragments are in flight over this one's MFMAs
  half8_t af[2], bh[2], bl[2];
  auto load = [&](int ks) {
#pragma unroll
    for (int i = 0; i < 2; ++i) af[i] = tail_afrag(xa[i] + ks * 16);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      bh[t] = tail_bfrag(a.wh, wave * 2 + t, ksteps, ks, lane);
      bl[t] = tail_bfrag(a.wl, wave * 2 + t, ksteps, ks, lane);
    }
  };
  load(0);
  for (int ks = 0; ks < ksteps; ++ks) {
    half8_t ca[2], ch[2], cl[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ca[i] = af[i];
      ch[i] = bh[i];
      cl[i] = bl[i];
    }
    if (ks + 1 < ksteps) load(ks + 1);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ca[i], ch[t], acc[i][t], 0, 0, 0);
        accx[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ca[i], cl[t], accx[i][t], 0, 0, 0);
      }
  }

  // qacts[0] on conv + bias, the codes as bytes into this wave's tile
  int8_t* tw = (int8_t*)tile[wave];
  const float inv0 = 1.0f / a.s0;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int co = t * 32 + (lane & 31);
    const float bc = a.bias[co];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
        const float v = __builtin_fmaf(accx[i][t][r], 1.0f / 2048.0f, acc[i][t][r]);
        tw[rl * PITCH * 4 + co] = (int8_t)(int)q8_exact(__builtin_fmaf(v, a.s_in, bc), a.s0, inv0);
      }
  }
  __syncthreads();

  // one output pixel per lane: LayerNorm over its 64 channels (two-pass, fp32), qacts[1], GELU, qacts[2]
  const int row = m0 + lane;
  if (row >= M) return;
  const int b = row / hw, p = row - b * hw, y = p / a.w, x = p - y * a.w;
  const int64_t pix = ((int64_t)b * 2 * a.h + 2 * y + (wave >> 1)) * (2 * a.w) + 2 * x + (wave & 1);
  float v[CO];
  int si = 0;
#pragma unroll
  for (int j = 0; j < CO / 4; ++j) {
    const uint32_t wq = tile[wave][lane * PITCH + j];
    if (a.dbg0) ((uint32_t*)(a.dbg0 + pix * CO))[j] = wq;
    si = __builtin_amdgcn_sdot4((int)wq, 0x01010101, si, false);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * j + e] = (float)(int8_t)((wq >> (8 * e)) & 0xFFu);
  }
  const float mean = (float)si * a.s0 / (float)CO;   // the codes' sum is exact
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < CO; ++c) {
    v[c] = v[c] * a.s0 - mean;
    q += v[c] * v[c];
  }
  const float rstd = rsqrtf(q / (float)CO + a.eps);
  const float inv1 = 1.0f / a.s1;
#pragma unroll
  for (int c = 0; c < CO; c += 4) {
    float c1[4];
    int c2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c1[e] = q8_exact(v[c + e] * rstd * a.gamma[c + e] + a.beta[c + e], a.s1, inv1);
      c2[e] = lut[(int)c1[e] + 128];
    }
    if (a.dbg1) ((uint32_t*)(a.dbg1 + pix * CO))[c / 4] = q8_pack4(c1[0], c1[1], c1[2], c1[3]);
    ((uint32_t*)(a.out + pix * CO))[c / 4] = (uint32_t)(c2[0] & 0xFF) | ((uint32_t)(c2[1] & 0xFF) << 8) |
                                              ((uint32_t)(c2[2] & 0xFF) << 16) | ((uint32_t)(c2[3] & 0xFF) << 24);
  }
}

struct Up1Args {
  const int8_t* x;       // [B, H, W, Cin] codes (NHWC; H = 2h, W = 2w)
  const _Float16* wh;    // fragment-ordered hi / lo planes of the [4 * 32][Cin] weight
  const _Float16* wl;
  const float* bias;     // [32]
  const int8_t* hyper;   // [B, nm, 32] codes of the hypernetwork MLPs' qact3
  const float* s_hyper;  // [nm] their scales
  float* masks;          // [B, nm, 2H, 2W] fake-quant f32 of the decoder's qact1
  int8_t* dbg3;          // optional: [B, 2H, 2W, 32] codes of qacts[3]
  int8_t* x4;            // optional: codes of qacts[4]
  int B, H, W, Cin, nm;
  float s_in, s3, s4, s_q1;
};

__global__ __launch_bounds__(256) void upscale1_masks_kernel(Up1Args a) {
  constexpr int CO = 32, PITCH = CO / 4 + 1;   // dwords per row of codes, odd
  __shared__ uint32_t t3[4][64 * PITCH], t4[4][64 * PITCH];
  __shared__ int8_t lut[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hsel = lane >> 5;
  const int hw = a.H * a.W;
  const int M = a.B * hw;
  const int m0 = blockIdx.x * 64;
  const int ksteps = a.Cin / 16;
  tail_gelu_lut(lut, tid, a.s3, a.s4);

  float16_t acc[2], accx[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = accx[i][r] = 0.f;
  const int8_t* xa[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int row = m0 + i * 32 + (lane & 31);
    row = row < M ? row : M - 1;
    xa[i] = a.x + (int64_t)row * a.Cin + 8 * hsel;
  }
  half8_t af[2], bh, bl;
  auto load = [&](int ks) {
#pragma unroll
    for (int i = 0; i < 2; ++i) af[i] = tail_afrag(xa[i] + ks * 16);
    bh = tail_bfrag(a.wh, wave, ksteps, ks, lane);
    bl = tail_bfrag(a.wl, wave, ksteps, ks, lane);
  };
  load(0);
  for (int ks = 0; ks < ksteps; ++ks) {
    const half8_t ca[2] = {af[0], af[1]}, ch = bh, cl = bl;
    if (ks + 1 < ksteps) load(ks + 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ca[i], ch, acc[i], 0, 0, 0);
      accx[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ca[i], cl, accx[i], 0, 0, 0);
    }
  }
  __syncthreads();   // the table is complete

  // qacts[3], GELU + qacts[4] (table): the codes as bytes into this wave's tiles
  int8_t* b3 = (int8_t*)t3[wave];
  int8_t* b4 = (int8_t*)t4[wave];
  const int co = lane & 31;
  const float bc = a.bias[co], inv3 = 1.0f / a.s3;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
      const float v = __builtin_fmaf(accx[i][r], 1.0f / 2048.0f, acc[i][r]);
      const int c3 = (int)q8_exact(__builtin_fmaf(v, a.s_in, bc), a.s3, inv3);
      b3[rl * PITCH * 4 + co] = (int8_t)c3;
      b4[rl * PITCH * 4 + co] = lut[c3 + 128];
    }
  __syncthreads();

  // one output pixel per lane: nm exact int32 dot products with the hypernetwork rows, qact1
  const int row = m0 + lane;
  if (row >= M) return;
  const int b = row / hw, p = row - b * hw, y = p / a.W, x = p - y * a.W;
  const int Y = 2 * y + (wave >> 1), X = 2 * x + (wave & 1);
  const int64_t pix = ((int64_t)b * 2 * a.H + Y) * (2 * a.W) + X;
  uint32_t xc[CO / 4];
#pragma unroll
  for (int j = 0; j < CO / 4; ++j) xc[j] = t4[wave][lane * PITCH + j];
  if (a.x4) {
#pragma unroll
    for (int j = 0; j < CO / 4; ++j) ((uint32_t*)(a.x4 + pix * CO))[j] = xc[j];
  }
  if (a.dbg3) {
#pragma unroll
    for (int j = 0; j < CO / 4; ++j) ((uint32_t*)(a.dbg3 + pix * CO))[j] = t3[wave][lane * PITCH + j];
  }
  const float invq = 1.0f / a.s_q1;
  for (int m = 0; m < a.nm; ++m) {
    const uint32_t* hy = (const uint32_t*)(a.hyper + ((int64_t)b * a.nm + m) * CO);
    int d = 0;
#pragma unroll
    for (int j = 0; j < CO / 4; ++j) d = __builtin_amdgcn_sdot4((int)hy[j], (int)xc[j], d, false);
    const float c = q8_exact((float)d * (a.s_hyper[m] * a.s4), a.s_q1, invq);
    a.masks[(((int64_t)b * a.nm + m) * 2 * a.H + Y) * (2 * a.W) + X] = c * a.s_q1;
  }
}

// The hypernetwork MLPs (MLP j < nh on token 1 + j) and the IoU head (MLP nh on token 0): workgroup
// (b, j) carries its row through the three layers, thread n = output column n, v_dot4_i32_i8 over
// weight dwords laid out [K / 4][N] (4 consecutive k of column n per dword: coalesced over n).
// M = 1 latency work, as samq_attention_q8_plain's token side.
struct MlpArgs {
  const int8_t* q;        // [B, Nt, C] codes of the transformer's qact4
  const uint32_t* w1;     // [nmlp][C / 4][H]
  const uint32_t* w2;     // [nmlp][H / 4][H]
  const uint32_t* w3;     // [nmlp][H / 4][NO]   (NO = max(no_h, no_i), zero-padded columns)
  const float* b1;        // [nmlp][H]
  const float* b2;
  const float* b3;        // [nmlp][NO]
  const float* sc;        // [nmlp][8]: s_w1, s_w2, s_w3, qacts1[0], qacts2[0], qacts1[1], qacts2[1], qact3
  int8_t* hyper;          // [B, nh, no_h] codes
  float* iou;             // [B, no_i] fake-quant f32
  int8_t* dbg;            // optional: [B, nmlp, 4, H] codes of qacts1[0], qacts2[0], qacts1[1], qacts2[1]
  int B, Nt, C, H, nh, no_h, no_i, NO;
  float s_in;
};

__device__ __forceinline__ int mlp_dot(const uint32_t* __restrict__ w, const uint32_t* x, int k4n, int N, int n) {
  int acc = 0;
#pragma unroll 8
  for (int k4 = 0; k4 < k4n; ++k4) acc = __builtin_amdgcn_sdot4((int)w[(int64_t)k4 * N + n], (int)x[k4], acc, false);
  return acc;
}

// hidden layer: c1 = q8(acc (s_in s_w) + bias, s1); r = max(c1, 0); c2 = q8(r s1, s2) (r when s1 == s2)
__device__ __forceinline__ float mlp_hidden(int acc, float s_in, float s_w, float bias, float s1, float s2, float& c1) {
  c1 = q8_exact(__builtin_fmaf((float)acc, s_in * s_w, bias), s1, 1.0f / s1);
  const float r = fmaxf(c1, 0.f);
  return s1 == s2 ? r : q8_exact(r * s1, s2, 1.0f / s2);
}

__global__ __launch_bounds__(256) void decoder_mlps_kernel(MlpArgs a) {
  __shared__ uint32_t xs[256], h1[64], h2[64];
  const int tid = threadIdx.x, b = blockIdx.x, j = blockIdx.y;
  const int tok = j < a.nh ? 1 + j : 0;
  const int nmlp = a.nh + 1;
  if (tid < a.C / 4) xs[tid] = ((const uint32_t*)(a.q + ((int64_t)b * a.Nt + tok) * a.C))[tid];
  const float* sc = a.sc + 8 * j;
  const float sw1 = sc[0], sw2 = sc[1], sw3 = sc[2], s10 = sc[3], s20 = sc[4], s11 = sc[5], s21 = sc[6], s3 = sc[7];
  int8_t* dbg = a.dbg ? a.dbg + ((int64_t)b * nmlp + j) * 4 * a.H : nullptr;
  __syncthreads();
  if (tid < a.H) {
    const int acc = mlp_dot(a.w1 + (int64_t)j * (a.C / 4) * a.H, xs, a.C / 4, a.H, tid);
    float c1;
    const float c2 = mlp_hidden(acc, a.s_in, sw1, a.b1[j * a.H + tid], s10, s20, c1);
    ((int8_t*)h1)[tid] = (int8_t)(int)c2;
    if (dbg) {
      dbg[tid] = (int8_t)(int)c1;
      dbg[a.H + tid] = (int8_t)(int)c2;
    }
  }
  __syncthreads();
  if (tid < a.H) {
    const int acc = mlp_dot(a.w2 + (int64_t)j * (a.H / 4) * a.H, h1, a.H / 4, a.H, tid);
    float c1;
    const float c2 = mlp_hidden(acc, s20, sw2, a.b2[j * a.H + tid], s11, s21, c1);
    ((int8_t*)h2)[tid] = (int8_t)(int)c2;
    if (dbg) {
      dbg[2 * a.H + tid] = (int8_t)(int)c1;
      dbg[3 * a.H + tid] = (int8_t)(int)c2;
    }
  }
  __syncthreads();
  const int no = j < a.nh ? a.no_h : a.no_i;
  if (tid < no) {
    const int acc = mlp_dot(a.w3 + (int64_t)j * (a.H / 4) * a.NO, h2, a.H / 4, a.NO, tid);
    const float c3 = q8_exact(__builtin_fmaf((float)acc, s21 * sw3, a.b3[j * a.NO + tid]), s3, 1.0f / s3);
    if (j < a.nh) a.hyper[((int64_t)b * a.nh + j) * a.no_h + tid] = (int8_t)(int)c3;
    else a.iou[(int64_t)b * a.no_i + tid] = c3 * s3;
  }
}

}  // namespace samq

using namespace samq;

static bool tail_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int samq_upscale0_q8(const int8_t* x, const void* w_hi, const void* w_lo, const float* bias,
                                const float* gamma, const float* beta, int8_t* out, int8_t* dbg_q0, int8_t* dbg_q1,
                                int B, int h, int w, int Cin, int Cout, float eps, float s_in, float s0, float s1,
                                float s2, hipStream_t stream) {
  SAMQ_REQUIRE(B >= 0 && h >= 0 && w >= 0, SAMQ_ERR_INVALID, "upscale0_q8: negative size");
  if (B == 0 || h == 0 || w == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(x && w_hi && w_lo && bias && gamma && beta && out, SAMQ_ERR_INVALID, "upscale0_q8: null pointer");
  SAMQ_REQUIRE(Cout == 64, SAMQ_ERR_UNSUPPORTED, "upscale0_q8: 64 output channels (one wave per sub-pixel)");
  SAMQ_REQUIRE(Cin > 0 && Cin % 16 == 0, SAMQ_ERR_UNSUPPORTED, "upscale0_q8: Cin must be a multiple of 16");
  SAMQ_REQUIRE((int64_t)B * h * w * 4 < ((int64_t)1 << 31) / 64, SAMQ_ERR_INVALID, "upscale0_q8: too many pixels");
  SAMQ_REQUIRE(s_in > 0.f && s0 > 0.f && s1 > 0.f && s2 > 0.f, SAMQ_ERR_INVALID, "upscale0_q8: scales must be > 0");
  SAMQ_REQUIRE(tail_aligned16(x) && tail_aligned16(w_hi) && tail_aligned16(w_lo) && tail_aligned16(out) &&
                   tail_aligned16(dbg_q0) && tail_aligned16(dbg_q1),
               SAMQ_ERR_INVALID, "upscale0_q8: pointers must be 16-byte aligned");
  Up0Args a{x, (const _Float16*)w_hi, (const _Float16*)w_lo, bias, gamma, beta, out, dbg_q0, dbg_q1,
            B, h, w, Cin, s_in, s0, s1, s2, eps};
  hipLaunchKernelGGL(upscale0_kernel, dim3((unsigned)((B * h * w + 63) / 64)), dim3(256), 0, stream, a);
  SAMQ_LAUNCH_CHECK("upscale0_q8 launch");
  return SAMQ_OK;
}

extern "C" int samq_upscale1_masks_q8(const int8_t* x, const void* w_hi, const void* w_lo, const float* bias,
                                      const int8_t* hyper, const float* s_hyper, float* masks, int8_t* dbg_q3,
                                      int8_t* x4, int B, int H, int W, int Cin, int Cout, int n_masks, float s_in,
                                      float s3, float s4, float s_q1, hipStream_t stream) {
  SAMQ_REQUIRE(B >= 0 && H >= 0 && W >= 0 && n_masks >= 0, SAMQ_ERR_INVALID, "upscale1_masks_q8: negative size");
  if (B == 0 || H == 0 || W == 0) return SAMQ_OK;
  SAMQ_REQUIRE(x && w_hi && w_lo && bias && masks && (n_masks == 0 || (hyper && s_hyper)), SAMQ_ERR_INVALID,
               "upscale1_masks_q8: null pointer");
  SAMQ_REQUIRE(Cout == 32, SAMQ_ERR_UNSUPPORTED, "upscale1_masks_q8: 32 output channels (one wave per sub-pixel)");
  SAMQ_REQUIRE(Cin > 0 && Cin % 16 == 0, SAMQ_ERR_UNSUPPORTED, "upscale1_masks_q8: Cin must be a multiple of 16");
  SAMQ_REQUIRE((int64_t)B * H * W * 4 < ((int64_t)1 << 31) / 64 && n_masks <= 64, SAMQ_ERR_INVALID,
               "upscale1_masks_q8: too many pixels or masks");
  SAMQ_REQUIRE(s_in > 0.f && s3 > 0.f && s4 > 0.f && s_q1 > 0.f, SAMQ_ERR_INVALID,
               "upscale1_masks_q8: scales must be > 0");
  SAMQ_REQUIRE(tail_aligned16(x) && tail_aligned16(w_hi) && tail_aligned16(w_lo) && tail_aligned16(hyper) &&
                   tail_aligned16(masks) && tail_aligned16(dbg_q3) && tail_aligned16(x4),
               SAMQ_ERR_INVALID, "upscale1_masks_q8: pointers must be 16-byte aligned");
  Up1Args a{x, (const _Float16*)w_hi, (const _Float16*)w_lo, bias, hyper, s_hyper, masks, dbg_q3, x4,
            B, H, W, Cin, n_masks, s_in, s3, s4, s_q1};
  hipLaunchKernelGGL(upscale1_masks_kernel, dim3((unsigned)((B * H * W + 63) / 64)), dim3(256), 0, stream, a);
  SAMQ_LAUNCH_CHECK("upscale1_masks_q8 launch");
  return SAMQ_OK;
}

extern "C" int samq_decoder_mlps_q8(const int8_t* q, const void* w1, const void* w2, const void* w3, const float* b1,
                                    const float* b2, const float* b3, const float* scales, int8_t* hyper, float* iou,
                                    int8_t* dbg, int B, int Nt, int C, int Hd, int n_hyper, int no_hyper, int no_iou,
                                    float s_in, hipStream_t stream) {
  SAMQ_REQUIRE(B >= 0, SAMQ_ERR_INVALID, "decoder_mlps_q8: negative batch");
  if (B == 0) return SAMQ_OK;
  SAMQ_REQUIRE(q && w1 && w2 && w3 && b1 && b2 && b3 && scales && hyper && iou, SAMQ_ERR_INVALID,
               "decoder_mlps_q8: null pointer");
  SAMQ_REQUIRE(n_hyper >= 1 && Nt >= 1 + n_hyper, SAMQ_ERR_INVALID,
               "decoder_mlps_q8: the row needs the IoU token and one token per hypernetwork MLP");
  SAMQ_REQUIRE(C > 0 && C % 4 == 0 && C <= 1024 && Hd > 0 && Hd % 4 == 0 && Hd <= 256, SAMQ_ERR_UNSUPPORTED,
               "decoder_mlps_q8: input dim a multiple of 4 up to 1024, hidden dim a multiple of 4 up to 256");
  SAMQ_REQUIRE(no_hyper >= 1 && no_iou >= 1 && no_hyper <= 256 && no_iou <= 256, SAMQ_ERR_UNSUPPORTED,
               "decoder_mlps_q8: 1 to 256 outputs per MLP");
  SAMQ_REQUIRE(B <= 65535 && n_hyper < 65535, SAMQ_ERR_INVALID, "decoder_mlps_q8: grid too large");
  SAMQ_REQUIRE(s_in > 0.f, SAMQ_ERR_INVALID, "decoder_mlps_q8: s_in must be > 0");
  SAMQ_REQUIRE(tail_aligned16(q) && tail_aligned16(w1) && tail_aligned16(w2) && tail_aligned16(w3), SAMQ_ERR_INVALID,
               "decoder_mlps_q8: pointers must be 16-byte aligned");
  MlpArgs a{q, (const uint32_t*)w1, (const uint32_t*)w2, (const uint32_t*)w3, b1, b2, b3, scales, hyper, iou, dbg,
            B, Nt, C, Hd, n_hyper, no_hyper, no_iou, no_hyper > no_iou ? no_hyper : no_iou, s_in};
  hipLaunchKernelGGL(decoder_mlps_kernel, dim3((unsigned)B, (unsigned)(n_hyper + 1)), dim3(256), 0, stream, a);
  SAMQ_LAUNCH_CHECK("decoder_mlps_q8 launch");
  return SAMQ_OK;
}
