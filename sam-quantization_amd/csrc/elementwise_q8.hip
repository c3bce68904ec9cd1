// Elementwise kernels on int8 activation codes for the fq_vit mask decoder (gfx950): the residual /
// positional-encoding adds between two QActs and the MLP's ReLU.
#include "common.h"

namespace samq {

// out = q8(fl(a s_a) + fl(b s_b), s_out): two rounded products and a rounded sum (torch's
// `x + y` on two materialised fake-quant tensors -- no FMA contraction), then the exact quantiser.
// b (optional) is read at i % bmod (rows shared over the batch).  FQ: f32 code * s_out out.
template <bool FQ>
__global__ __launch_bounds__(256) void add_q8_kernel(const int8_t* __restrict__ a, const int8_t* __restrict__ b,
                                                     void* __restrict__ out, int64_t n, int64_t bmod, float s_a,
                                                     float s_b, float s_out, int vec) {
#pragma clang fp contract(off)   // a s_a + b s_b as two rounded products and a rounded sum, never an FMA
  const float inv = 1.0f / s_out, lim = 130.0f * s_out;
  const int64_t n4 = vec ? n / 4 : 0;
  const int64_t work = n4 + (n - 4 * n4);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < work; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n4) {
      const uint32_t wa = ((const uint32_t*)a)[i];
      const uint32_t wb = b ? ((const uint32_t*)b)[(4 * i) % bmod / 4] : 0u;
      float x[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float fa = (float)(int8_t)((wa >> (8 * e)) & 0xFFu) * s_a;
        const float fb = (float)(int8_t)((wb >> (8 * e)) & 0xFFu) * s_b;
        x[e] = b ? fa + fb : fa;
      }
      const float2_t c0 = q8_exact2(float2_t{x[0], x[1]}, s_out, inv, lim);
      const float2_t c1 = q8_exact2(float2_t{x[2], x[3]}, s_out, inv, lim);
      if (FQ) ((float4_t*)out)[i] = float4_t{c0.x * s_out, c0.y * s_out, c1.x * s_out, c1.y * s_out};
      else ((uint32_t*)out)[i] = q8_pack4(c0.x, c0.y, c1.x, c1.y);
    } else {
      const int64_t e = 4 * n4 + (i - n4);
      const float fa = (float)a[e] * s_a;
      const float x = b ? fa + (float)b[e % bmod] * s_b : fa;
      const float c = q8_exact(x, s_out, inv);
      if (FQ) ((float*)out)[e] = c * s_out;
      else ((int8_t*)out)[e] = (int8_t)(int)c;
    }
  }
}

// codes = max(codes, 0) in place: q8(relu(y), s) == max(q8(y, s), 0) (round to nearest is monotone
// and q8(0) = 0), so the ReLU of lin1 -> ReLU -> QAct runs on the Q8 epilogue's codes
__global__ __launch_bounds__(256) void relu_q8_kernel(int8_t* __restrict__ x, int64_t n) {
  const int64_t n4 = n / 4, work = n4 + (n & 3);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < work; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n4) {
      const uint32_t w = ((const uint32_t*)x)[i];
      const uint32_t neg = (w & 0x80808080u) >> 7;   // 1 in the low bit of every negative byte
      ((uint32_t*)x)[i] = w & ~(neg * 0xFFu);
    } else {
      const int64_t e = 4 * n4 + (i - n4);
      x[e] = x[e] < 0 ? (int8_t)0 : x[e];
    }
  }
}

}  // namespace samq

using namespace samq;

extern "C" int samq_add_q8(const int8_t* a, float s_a, const int8_t* b, float s_b, int64_t bmod, void* out, int64_t n,
                           float s_out, int flags, hipStream_t stream) {
  SAMQ_REQUIRE(n >= 0, SAMQ_ERR_INVALID, "add_q8: negative size");
  if (n == 0) return SAMQ_OK;
  SAMQ_REQUIRE(a && out, SAMQ_ERR_INVALID, "add_q8: null pointer");
  SAMQ_REQUIRE(s_a > 0.f && s_out > 0.f && (!b || s_b > 0.f), SAMQ_ERR_INVALID, "add_q8: scales must be > 0");
  SAMQ_REQUIRE(!b || (bmod > 0 && bmod <= n), SAMQ_ERR_INVALID, "add_q8: b's period must be in [1, n]");
  SAMQ_REQUIRE((flags & ~SAMQ_Q_OUT_FQ) == 0, SAMQ_ERR_INVALID, "add_q8: unknown flag");
  SAMQ_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0, SAMQ_ERR_INVALID,
               "add_q8: pointers must be 16-byte aligned");
  const int vec = !b || bmod % 4 == 0;   // a dword of b never wraps around its period
  const int64_t work = vec ? n / 4 + (n & 3) : n;
  const int blocks = (int)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
  if (flags & SAMQ_Q_OUT_FQ)
    hipLaunchKernelGGL((add_q8_kernel<true>), dim3(blocks), dim3(256), 0, stream, a, b, out, n, b ? bmod : n, s_a, s_b,
                       s_out, vec);
  else
    hipLaunchKernelGGL((add_q8_kernel<false>), dim3(blocks), dim3(256), 0, stream, a, b, out, n, b ? bmod : n, s_a, s_b,
                       s_out, vec);
  SAMQ_LAUNCH_CHECK("add_q8 launch");
  return SAMQ_OK;
}

extern "C" int samq_relu_q8(int8_t* x, int64_t n, hipStream_t stream) {
  SAMQ_REQUIRE(n >= 0, SAMQ_ERR_INVALID, "relu_q8: negative size");
  if (n == 0) return SAMQ_OK;
  SAMQ_REQUIRE(x && ((uintptr_t)x & 3) == 0, SAMQ_ERR_INVALID, "relu_q8: x must be a 4-byte aligned pointer");
  const int64_t work = n / 4 + (n & 3);
  const int blocks = (int)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
  hipLaunchKernelGGL(relu_q8_kernel, dim3(blocks), dim3(256), 0, stream, x, n);
  SAMQ_LAUNCH_CHECK("relu_q8 launch");
  return SAMQ_OK;
}
