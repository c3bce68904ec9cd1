// The tail of the FLOAT mask decoder (samq/sam_decoder.py MaskDecoder.predict_masks, everything behind the
// two-way transformer) in two launches on fp32 activations:
//  * decoder_mlps_f32: the four hypernetwork MLPs and the IoU head (3 Linears each, ReLU between);
//  * upscale_masks_f32: ConvTranspose2d(256 -> 64, k2 s2) + LayerNorm2d + GELU + ConvTranspose2d(64 -> 32,
//    k2 s2) + GELU + the product with the hypernetwork rows -> the low-res masks.
// A k2 s2 transposed convolution has one contributor per output pixel and LayerNorm2d is per pixel, so one
// input pixel's 256 channels decide its 2 x 2 mid pixels, their 4 x 4 output pixels and those pixels' mask
// values: the chain runs per tile of 64 input pixels and neither the [B, 64, 2h, 2w] mid map nor the
// [B, 32, 4h, 4w] upscaled map exists in memory.  Wave w of 4 owns the first convolution's sub-pixel
// (kh, kw) = w: 64 mid pixels x 64 channels in its accumulators, then in its private 17 KB LDS tile, where
// a lane takes one mid pixel for the channel statistics and the GELU.  The result is the second GEMM's A
// operand: the wave lifts it into registers as MFMA fragments (64 VGPRs), which frees the LDS tile to turn
// the second convolution's accumulators (one sub-pixel (kh2, kw2) = 32 columns at a time) into one output
// pixel per lane for the four 32-term mask dot products.
// Both GEMMs run on v_mfma_f32_32x32x2_f32: fp32 operands, fp32 accumulation, no range or splitting
// hazard at any input scale (DESIGN.md "Float mask decoder tail" has the count against split fp16).  A lane
// supplies one k per instruction, so the K order is ours to choose: lane (row, khalf) reads the float4 at
// k = 8 j + 4 khalf + 0..3 and feeds MFMA s of group j with element s; the weights are pre-ordered to match
// (ops.convt_frag_weight_f32), 1 KiB contiguous per (column tile, j).  Every operand load is 16 bytes.
// No atomics, fixed summation orders: results are bit-identical from run to run.
#include "common.h"

namespace samq {

constexpr int TF_C = 256;      // transformer width
constexpr int TF_C4 = 64;      // mid channels
constexpr int TF_C8 = 32;      // upscaled channels
constexpr int TF_NM = 4;       // mask tokens
constexpr int TF_P1 = 68;      // floats per row of the mid tile: 16-byte rows, ds_read_b128 by a lane per row conflict-free
constexpr int TF_P2 = 36;      // floats per row of the output tile, the same

struct UpF32Args {
  const float* keys;    // [B * h * w, 256] token rows
  const float* w1;      // [8][32][64][4] fragment order of the [4 * 64][256] matrix
  const float* b1;      // [64]
  const float* gamma;   // [64]
  const float* beta;
  const float* w2;      // [4][8][64][4] fragment order of the [4 * 32][64] matrix
  const float* b2;      // [32]
  const float* hyper;   // [B, 4, 32]
  float* masks;         // [B, 4, 4h, 4w]
  int B, h, w;
  float eps;
};

__global__ __launch_bounds__(256) void upscale_masks_f32_kernel(UpF32Args a) {
  __shared__ __attribute__((aligned(16))) float tile[4][64 * TF_P1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hsel = lane >> 5, l32 = lane & 31;
  const int hw = a.h * a.w;
  const int64_t M = (int64_t)a.B * hw;
  const int64_t m0 = (int64_t)blockIdx.x * 64;
  float* tw = tile[wave];

  // ---- GEMM 1: [64 px, 256] x [256, 64 columns of sub-pixel `wave`]
  float16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][t][r] = 0.f;
  const float* xa[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int64_t row = m0 + i * 32 + l32;
    row = row < M ? row : M - 1;   // rows past the end: read the last row, never stored
    xa[i] = a.keys + row * TF_C + 4 * hsel;
  }
  const float* wb = a.w1 + ((int64_t)wave * 2 * (TF_C / 8) * 64 + lane) * 4;
  // the next group's fragments are in flight over this one's 16 MFMAs
  float4_t af[2], bf[2];
  auto load = [&](int j) {
#pragma unroll
    for (int i = 0; i < 2; ++i) af[i] = *(const float4_t*)(xa[i] + 8 * j);
#pragma unroll
    for (int t = 0; t < 2; ++t) bf[t] = *(const float4_t*)(wb + ((int64_t)t * (TF_C / 8) + j) * 256);
  };
  load(0);
  for (int j = 0; j < TF_C / 8; ++j) {
    const float4_t ca[2] = {af[0], af[1]}, cb[2] = {bf[0], bf[1]};
    if (j + 1 < TF_C / 8) load(j + 1);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[i][s], cb[t][s], acc[i][t], 0, 0, 0);
  }

  // conv + bias into this wave's tile, [mid pixel = input pixel of the tile][channel]
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int co = t * 32 + l32;
    const float bc = a.b1[co];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
        tw[rl * TF_P1 + co] = acc[i][t][r] + bc;
      }
  }
  __syncthreads();

  // one mid pixel per lane: LayerNorm2d over its 64 channels (two passes, fp32), exact-erf GELU, in place
  {
    float v[TF_C4];
#pragma unroll
    for (int c = 0; c < TF_C4; c += 4) {
      const float4_t q = *(const float4_t*)(tw + lane * TF_P1 + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[c + e] = q[e];
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < TF_C4; ++c) s += v[c];
    const float mean = s * (1.0f / TF_C4);
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < TF_C4; ++c) {
      v[c] -= mean;
      q = __builtin_fmaf(v[c], v[c], q);
    }
    const float rstd = 1.0f / sqrtf(q * (1.0f / TF_C4) + a.eps);
#pragma unroll
    for (int c = 0; c < TF_C4; c += 4) {
      float4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = gelu_erf(__builtin_fmaf(v[c + e] * rstd, a.gamma[c + e], a.beta[c + e]));
      *(float4_t*)(tw + lane * TF_P1 + c) = o;
    }
  }
  __syncthreads();

  // the second GEMM's A operand, [64 mid px, 64] of this wave, as fragments in registers; the tile is free after
  float4_t a2[2][TF_C4 / 8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TF_C4 / 8; ++j) a2[i][j] = *(const float4_t*)(tw + (i * 32 + l32) * TF_P1 + 8 * j + 4 * hsel);
  __syncthreads();

  // this lane's input pixel and its prompt's hypernetwork rows
  const int64_t row = m0 + lane;
  const bool valid = row < M;
  const int64_t rc = valid ? row : M - 1;
  const int b = (int)(rc / hw), p = (int)(rc - (int64_t)b * hw), y = p / a.w, x = p - y * a.w;
  const float* hy = a.hyper + (int64_t)b * TF_NM * TF_C8;
  const int H4 = 4 * a.h, W4 = 4 * a.w;

  // ---- GEMM 2 per output sub-pixel (kh2, kw2): [64 mid px, 64] x [64, 32], GELU, the four mask dots
#pragma unroll 1
  for (int kh2 = 0; kh2 < 2; ++kh2) {
    float mk[2][TF_NM];
#pragma unroll
    for (int kw2 = 0; kw2 < 2; ++kw2) {
      const float* w2 = a.w2 + ((int64_t)(2 * kh2 + kw2) * (TF_C4 / 8) * 64 + lane) * 4;
      float4_t b2f[TF_C4 / 8];
#pragma unroll
      for (int j = 0; j < TF_C4 / 8; ++j) b2f[j] = *(const float4_t*)(w2 + j * 256);
      float16_t c2[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) c2[i][r] = 0.f;
#pragma unroll
      for (int j = 0; j < TF_C4 / 8; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            c2[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[i][j][s], b2f[j][s], c2[i], 0, 0, 0);
      const float bc = a.b2[l32];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
          tw[rl * TF_P2 + l32] = gelu_erf(c2[i][r] + bc);
        }
      __syncthreads();
      // one output pixel per lane: its 32 channels against the four rows of hyper[b], channel order
      float u[TF_C8];
#pragma unroll
      for (int c = 0; c < TF_C8; c += 4) {
        const float4_t q = *(const float4_t*)(tw + lane * TF_P2 + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) u[c + e] = q[e];
      }
#pragma unroll
      for (int m = 0; m < TF_NM; ++m) {
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < TF_C8; c += 4) {
          const float4_t hv = *(const float4_t*)(hy + m * TF_C8 + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) d = __builtin_fmaf(hv[e], u[c + e], d);
        }
        mk[kw2][m] = d;
      }
      __syncthreads();   // the tile is rewritten by the next sub-pixel
    }
    if (valid) {
      const int Y = 4 * y + 2 * (wave >> 1) + kh2, X = 4 * x + 2 * (wave & 1);
#pragma unroll
      for (int m = 0; m < TF_NM; ++m)
        *(float2_t*)(a.masks + (((int64_t)b * TF_NM + m) * H4 + Y) * W4 + X) = float2_t{mk[0][m], mk[1][m]};
    }
  }
}

// The hypernetwork MLPs (MLP j < 4 on token 1 + j) and the IoU head (MLP 4 on token 0): workgroup (b, j)
// carries its 256-wide row through the three layers in LDS, thread n = output column n, one fp32 FMA chain
// over k in index order; the weights are transposed to [K][N] so a wave's loads are one row segment.
struct MlpF32Args {
  const float* hs;    // [B, Nt, 256]
  const float* w1;    // [5][256][256]  (k, n)
  const float* w2;    // [5][256][256]
  const float* w3;    // [5][256][32]   (the IoU head's columns 4..31 zero)
  const float* b1;    // [5][256]
  const float* b2;
  const float* b3;    // [5][32]
  float* hyper;       // [B, 4, 32]
  float* iou;         // [B, 4]
  int B, Nt;
};

template <int N>
__device__ __forceinline__ float mlp_f32_dot(const float* __restrict__ w, const float* x, int n, float bias) {
  float acc = 0.f;
#pragma unroll 16
  for (int k = 0; k < TF_C; ++k) acc = __builtin_fmaf(x[k], w[(int64_t)k * N + n], acc);
  return acc + bias;
}

__global__ __launch_bounds__(256) void decoder_mlps_f32_kernel(MlpF32Args a) {
  __shared__ float xs[TF_C], h1[TF_C], h2[TF_C];
  const int tid = threadIdx.x, b = blockIdx.x, j = blockIdx.y;
  const int tok = j < TF_NM ? 1 + j : 0;
  xs[tid] = a.hs[((int64_t)b * a.Nt + tok) * TF_C + tid];
  __syncthreads();
  h1[tid] = fmaxf(mlp_f32_dot<TF_C>(a.w1 + (int64_t)j * TF_C * TF_C, xs, tid, a.b1[j * TF_C + tid]), 0.f);
  __syncthreads();
  h2[tid] = fmaxf(mlp_f32_dot<TF_C>(a.w2 + (int64_t)j * TF_C * TF_C, h1, tid, a.b2[j * TF_C + tid]), 0.f);
  __syncthreads();
  const int no = j < TF_NM ? TF_C8 : TF_NM;
  if (tid < no) {
    const float v = mlp_f32_dot<TF_C8>(a.w3 + (int64_t)j * TF_C * TF_C8, h2, tid, a.b3[j * TF_C8 + tid]);
    if (j < TF_NM) a.hyper[((int64_t)b * TF_NM + j) * TF_C8 + tid] = v;
    else a.iou[(int64_t)b * TF_NM + tid] = v;
  }
}

}  // namespace samq

using namespace samq;

static bool tail_f32_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int samq_decoder_mlps_f32(const float* hs, const float* w1, const float* w2, const float* w3,
                                     const float* b1, const float* b2, const float* b3, float* hyper, float* iou,
                                     int B, int n_tokens, int C, hipStream_t stream) {
  SAMQ_REQUIRE(B >= 0 && n_tokens >= 0 && C >= 0, SAMQ_ERR_INVALID, "decoder_mlps_f32: negative size");
  if (B == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(hs && w1 && w2 && w3 && b1 && b2 && b3 && hyper && iou, SAMQ_ERR_INVALID,
               "decoder_mlps_f32: null pointer");
  SAMQ_REQUIRE(C == TF_C, SAMQ_ERR_UNSUPPORTED, "decoder_mlps_f32: the transformer width must be 256");
  SAMQ_REQUIRE(n_tokens >= 1 + TF_NM, SAMQ_ERR_INVALID,
               "decoder_mlps_f32: the row needs the IoU token and four mask tokens");
  SAMQ_REQUIRE(tail_f32_aligned16(hs) && tail_f32_aligned16(w1) && tail_f32_aligned16(w2) && tail_f32_aligned16(w3) &&
                   tail_f32_aligned16(b1) && tail_f32_aligned16(b2) && tail_f32_aligned16(b3) &&
                   tail_f32_aligned16(hyper) && tail_f32_aligned16(iou),
               SAMQ_ERR_INVALID, "decoder_mlps_f32: pointers must be 16-byte aligned");
  MlpF32Args a{hs, w1, w2, w3, b1, b2, b3, hyper, iou, B, n_tokens};
  hipLaunchKernelGGL(decoder_mlps_f32_kernel, dim3((unsigned)B, TF_NM + 1), dim3(256), 0, stream, a);
  SAMQ_LAUNCH_CHECK("decoder_mlps_f32 launch");
  return SAMQ_OK;
}

extern "C" int samq_upscale_masks_f32(const float* keys, const float* w1, const float* b1, const float* gamma,
                                      const float* beta, const float* w2, const float* b2, const float* hyper,
                                      float* masks, int B, int h, int w, int C, float eps, hipStream_t stream) {
  SAMQ_REQUIRE(B >= 0 && h >= 0 && w >= 0 && C >= 0, SAMQ_ERR_INVALID, "upscale_masks_f32: negative size");
  if (B == 0 || h == 0 || w == 0) return SAMQ_OK;
  SAMQ_REQUIRE(keys && w1 && b1 && gamma && beta && w2 && b2 && hyper && masks, SAMQ_ERR_INVALID,
               "upscale_masks_f32: null pointer");
  SAMQ_REQUIRE(C == TF_C, SAMQ_ERR_UNSUPPORTED, "upscale_masks_f32: the transformer width must be 256");
  SAMQ_REQUIRE((int64_t)B * h * w <= ((int64_t)1 << 31) / 64 && (int64_t)4 * h * 4 * w < ((int64_t)1 << 31),
               SAMQ_ERR_INVALID, "upscale_masks_f32: too many pixels");
  SAMQ_REQUIRE(tail_f32_aligned16(keys) && tail_f32_aligned16(w1) && tail_f32_aligned16(b1) &&
                   tail_f32_aligned16(gamma) && tail_f32_aligned16(beta) && tail_f32_aligned16(w2) &&
                   tail_f32_aligned16(b2) && tail_f32_aligned16(hyper) && tail_f32_aligned16(masks),
               SAMQ_ERR_INVALID, "upscale_masks_f32: pointers must be 16-byte aligned");
  UpF32Args a{keys, w1, b1, gamma, beta, w2, b2, hyper, masks, B, h, w, eps};
  hipLaunchKernelGGL(upscale_masks_f32_kernel, dim3((unsigned)(((int64_t)B * h * w + 63) / 64)), dim3(256), 0,
                     stream, a);
  SAMQ_LAUNCH_CHECK("upscale_masks_f32 launch");
  return SAMQ_OK;
}
