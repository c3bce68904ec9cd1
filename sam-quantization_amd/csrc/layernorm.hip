// Row LayerNorm (f32 statistics, f16 output) for the ViT blocks' norm1 / norm2.
// Reference: nn.LayerNorm(eps=1e-6) (segment_anything/build_sam.py:72) applied in
// Block.forward (segment_anything/modeling/image_encoder.py:194, 205).  HBM-bound: one wave
// per row, 16-byte vector loads, the row held in registers (two-pass mean / variance).
#include "common.h"

namespace samq {

// IN: 0 f32, 1 f16, 2 int8 codes (x = code * in_scale)
// OUT: 0 f16, 1 f32, 2 int8 codes q(y, out_scale), 3 f32 fake-quant q(y, out_scale) * out_scale
enum { LN_F32 = 0, LN_F16 = 1, LN_I8 = 2, LN_FQ32 = 3 };

__device__ __forceinline__ float ln_q8(float v, float s) {   // fq_vit uniform.py:31-36
  return q8_exact(v, s, 1.0f / s);   // the reciprocal is loop-invariant (hoisted)
}

// ADD (f32 input only): the residual add of the GEMM before the LayerNorm runs here instead of in
// that GEMM's epilogue -- x += delta (delta f16 when ADD == 1, f32 when ADD == 2; the GEMM wrote
// y = acc * s + b with a plain store), x written back in place, then the LayerNorm of the new x.
// f32 delta: the same fp32 add as the GEMM's read-modify-write epilogue (bit-identical x).  The ADD
// variants read AND write the residual through ``xres`` (plain, non-const: the buffer is updated in
// place); ``xin`` (const restrict) is the input of the ADD == 0 variants only.
// ZP (samq_layernorm_q_zp): int8 input (code - zp_in) * in_scale, the subtraction in integers; the
// output quantiser (out_scale, zp_out) with the fake-quant value (code - zp_out) * out_scale.
// PTF (samq_layernorm_q_ptf; ZP, int8 input): the input quantiser's scale is in_scale * 2^exp[c], exp a
// uint8 [C] array in 0..3: x = ((code - zp_in) << exp[c]) * in_scale.  A lane's 4 channels take one
// dword of exponents.  The array travels in ``delta``, which only the ADD variants read.
template <int IN, int OUT, int VPT, int RPW, int ADD = 0, bool ZP = false, bool PTF = false>
__global__ __launch_bounds__(256) void layernorm_kernel(const void* __restrict__ xin, void* __restrict__ y,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int64_t rows, int C,
                                                        float eps, float in_scale, float out_scale,
                                                        float* __restrict__ mean_out,
                                                        const void* __restrict__ delta = nullptr,
                                                        float* xres = nullptr, int* __restrict__ rs_out = nullptr,
                                                        int* __restrict__ rs_zero = nullptr, int zp_in = 0,
                                                        float zp_out = 0.f) {
  static_assert(ADD == 0 || IN == LN_F32, "residual add: f32 rows");
  static_assert(!PTF || (ZP && IN == LN_I8 && ADD == 0), "power-of-two factors: int8 input with a zero point");
  const int lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
  if (row0 >= rows) return;
  const int nvec = C / 4;
  // all RPW rows' loads are issued before the first reduction: RPW x VPT 16-byte loads in flight
  float4_t v[RPW][VPT];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int64_t row = row0 + r < rows ? row0 + r : rows - 1;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int j = lane + 64 * i;
      if (j < nvec) {
        if (IN == LN_F16) {
          const half4_t h = ((const half4_t*)xin)[row * nvec + j];
          v[r][i] = float4_t{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        } else if (IN == LN_I8) {
          const uint32_t w = ((const uint32_t*)xin)[row * nvec + j];
          uint32_t ew = 0;
          if constexpr (PTF) ew = ((const uint32_t*)delta)[j];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if constexpr (PTF)   // (code - zp) << exp: |.| <= 255 * 8, exact
              v[r][i][e] = (float)(((int)(int8_t)((w >> (8 * e)) & 0xFFu) - zp_in) * (1 << ((ew >> (8 * e)) & 3u))) * in_scale;
            else if constexpr (ZP) v[r][i][e] = (float)((int)(int8_t)((w >> (8 * e)) & 0xFFu) - zp_in) * in_scale;
            else v[r][i][e] = (float)(int8_t)((w >> (8 * e)) & 0xFFu) * in_scale;
          }
        } else {
          v[r][i] = ADD != 0 ? ((const float4_t*)xres)[row * nvec + j] : ((const float4_t*)xin)[row * nvec + j];
          if constexpr (ADD == 1) {
            const half4_t h = ((const half4_t*)delta)[row * nvec + j];
            v[r][i] += float4_t{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
          } else if constexpr (ADD == 2) {
            v[r][i] += ((const float4_t*)delta)[row * nvec + j];
          }
        }
      } else {
        v[r][i] = float4_t{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  if constexpr (ADD != 0) {   // the new residual rows back in place
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int64_t row = row0 + r;
      if (row < rows) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
          const int j = lane + 64 * i;
          if (j < nvec) ((float4_t*)xres)[row * nvec + j] = v[r][i];
        }
      }
    }
  }
  // int8-code output (the W4A8 LN-q): gamma / beta loaded beside the rows, not behind the
  // reductions (measured: LN-q 26.1 -> 21.3 us at 16384 rows, W4A8 step +0.6 %; the f16-output
  // LayerNorm of W4A16 runs inside the other lane's GEMMs and lost 0.5 % with it: late loads there)
  constexpr bool EARLY_GB = OUT == LN_I8;
  float4_t gv[EARLY_GB ? VPT : 1], bv[EARLY_GB ? VPT : 1];
  if constexpr (EARLY_GB) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int j = lane + 64 * i;
      gv[i] = j < nvec ? ((const float4_t*)gamma)[j] : float4_t{0.f, 0.f, 0.f, 0.f};
      bv[i] = j < nvec ? ((const float4_t*)beta)[j] : float4_t{0.f, 0.f, 0.f, 0.f};
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int64_t row = row0 + r;
    if (row >= rows) break;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) s += v[r][i][0] + v[r][i][1] + v[r][i][2] + v[r][i][3];
    const float mean = wave_sum_valu(s) / (float)C;
    if (mean_out && lane == 0) mean_out[row] = mean;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int j = lane + 64 * i;
      if (j < nvec) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = v[r][i][e] - mean;
          q += d * d;
        }
      }
    }
    const float rstd = rsqrtf(wave_sum_valu(q) / (float)C + eps);
    int rsi = 0;   // LN_I8 with rs_out: the row's codes summed (the W4A8 GEMM's zero-point row sum)
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int j = lane + 64 * i;
      if (j < nvec) {
        const float4_t g = EARLY_GB ? gv[EARLY_GB ? i : 0] : ((const float4_t*)gamma)[j];
        const float4_t b = EARLY_GB ? bv[EARLY_GB ? i : 0] : ((const float4_t*)beta)[j];
        float4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (v[r][i][e] - mean) * rstd * g[e] + b[e];
        if (OUT == LN_F32) {
          ((float4_t*)y)[row * nvec + j] = o;
        } else if (OUT == LN_FQ32) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if constexpr (ZP) o[e] = (q8_exact_zp(o[e], out_scale, 1.0f / out_scale, zp_out) - zp_out) * out_scale;
            else o[e] = ln_q8(o[e], out_scale) * out_scale;
          }
          ((float4_t*)y)[row * nvec + j] = o;
        } else if (OUT == LN_I8) {
          const float inv = 1.0f / out_scale, lim = (ZP ? 260.0f : 130.0f) * out_scale;   // (loop-invariant: hoisted)
          float2_t c01, c23;
          if constexpr (ZP) {
            c01 = q8_exact2_zp(float2_t{o[0], o[1]}, out_scale, inv, lim, zp_out);
            c23 = q8_exact2_zp(float2_t{o[2], o[3]}, out_scale, inv, lim, zp_out);
          } else {
            c01 = q8_exact2(float2_t{o[0], o[1]}, out_scale, inv, lim);
            c23 = q8_exact2(float2_t{o[2], o[3]}, out_scale, inv, lim);
          }
          const uint32_t wq = q8_pack4(c01.x, c01.y, c23.x, c23.y);
          ((uint32_t*)y)[row * nvec + j] = wq;
          if (rs_out) rsi = __builtin_amdgcn_sdot4((int)wq, 0x01010101, rsi, false);
        } else {
          ((half4_t*)y)[row * nvec + j] = half4_t{(_Float16)o[0], (_Float16)o[1], (_Float16)o[2], (_Float16)o[3]};
        }
      }
    }
    if (OUT == LN_I8 && rs_out) {   // |sum| <= 128 C < 2^24: the f32 wave sum is exact
      const float t = wave_sum_valu((float)rsi);
      if (lane == 0) rs_out[row] = (int)t;
    }
    if (rs_zero && lane == 0) rs_zero[row] = 0;   // the next GEMM's rs_out accumulator
  }
}

}  // namespace samq

using namespace samq;

// rows per wave: SAMQ_LN_RPW(n) in flags (0 = default; rows wider than 1280 channels use 1)
#define SAMQ_LN_DEFAULT_RPW 2   // measured: ViT-H rows 33.0 -> 27.3 us uncached (tools/bench_ln.py)
static int ln_rpw(int flags) {
  const int r = (flags >> 16) & 7;
  return r == 0 ? SAMQ_LN_DEFAULT_RPW : r;
}

static int ln_launch(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C, float eps,
                     int in, int out, float in_scale, float out_scale, int rpw, hipStream_t stream,
                     float* mean_out = nullptr, int* rs_out = nullptr, int* rs_zero = nullptr, bool zp = false,
                     int zp_in = 0, int zp_out = 0) {
  if (rows == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(x && y && gamma && beta, SAMQ_ERR_INVALID, "layernorm: null pointer");
  SAMQ_REQUIRE(C > 0 && C % 4 == 0 && C <= 4096, SAMQ_ERR_INVALID, "layernorm: C must be a multiple of 4, <= 4096");
  if (rows <= 0) return SAMQ_OK;
  SAMQ_REQUIRE(rpw == 1 || rpw == 2 || rpw == 4, SAMQ_ERR_INVALID, "layernorm: rows per wave must be 1, 2 or 4");
  const int vpt = (C / 4 + 63) / 64;
  if (vpt > 5) rpw = 1;
  const dim3 grid((unsigned)((rows + 4 * rpw - 1) / (4 * rpw)));
  // zero points (samq_layernorm_q_zp): the ZP kernels; int8 on at least one side
#define LN_Z(I, O, V, R) hipLaunchKernelGGL((layernorm_kernel<I, O, V, R, 0, true>), grid, dim3(256), 0, stream, x, y, gamma, beta, rows, C, eps, in_scale, out_scale, mean_out, nullptr, nullptr, rs_out, rs_zero, zp_in, (float)zp_out)
#define LN_R(I, O, V) \
  do { \
    if (zp) { if (rpw == 1) LN_Z(I, O, V, 1); else if (rpw == 2) LN_Z(I, O, V, 2); else LN_Z(I, O, V, 4); break; } \
    if (rpw == 1) hipLaunchKernelGGL((layernorm_kernel<I, O, V, 1>), grid, dim3(256), 0, stream, x, y, gamma, beta, rows, C, eps, in_scale, out_scale, mean_out, nullptr, nullptr, rs_out, rs_zero); \
    else if (rpw == 2) hipLaunchKernelGGL((layernorm_kernel<I, O, V, 2>), grid, dim3(256), 0, stream, x, y, gamma, beta, rows, C, eps, in_scale, out_scale, mean_out, nullptr, nullptr, rs_out, rs_zero); \
    else hipLaunchKernelGGL((layernorm_kernel<I, O, V, 4>), grid, dim3(256), 0, stream, x, y, gamma, beta, rows, C, eps, in_scale, out_scale, mean_out, nullptr, nullptr, rs_out, rs_zero); \
  } while (0)
#define LN_V(I, O) \
  do { \
    if (vpt <= 1) LN_R(I, O, 1); \
    else if (vpt <= 3) LN_R(I, O, 3); \
    else if (vpt <= 4) LN_R(I, O, 4); \
    else if (vpt <= 5) LN_R(I, O, 5); \
    else LN_R(I, O, 16); \
  } while (0)
#define LN_O(I) \
  do { \
    switch (out) { case LN_F16: LN_V(I, LN_F16); break; case LN_F32: LN_V(I, LN_F32); break; \
                   case LN_I8: LN_V(I, LN_I8); break; default: LN_V(I, LN_FQ32); break; } \
  } while (0)
  switch (in) { case LN_F16: LN_O(LN_F16); break; case LN_I8: LN_O(LN_I8); break; default: LN_O(LN_F32); break; }
#undef LN_O
#undef LN_V
#undef LN_R
#undef LN_Z
  SAMQ_LAUNCH_CHECK("layernorm launch");
  return SAMQ_OK;
}

extern "C" int samq_layernorm(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C,
                              float eps, int flags, hipStream_t stream) {
  return ln_launch(x, y, gamma, beta, rows, C, eps, (flags & SAMQ_LN_IN_F16) ? LN_F16 : LN_F32,
                   (flags & SAMQ_LN_OUT_F32) ? LN_F32 : LN_F16, 1.f, 1.f, ln_rpw(flags), stream);
}

extern "C" int samq_layernorm_mean(const void* x, void* y, const float* gamma, const float* beta, int64_t rows,
                                   int C, float eps, int flags, float* mean_out, hipStream_t stream) {
  SAMQ_REQUIRE(mean_out, SAMQ_ERR_INVALID, "layernorm_mean: null mean_out");
  return ln_launch(x, y, gamma, beta, rows, C, eps, (flags & SAMQ_LN_IN_F16) ? LN_F16 : LN_F32,
                   (flags & SAMQ_LN_OUT_F32) ? LN_F32 : LN_F16, 1.f, 1.f, ln_rpw(flags), stream, mean_out);
}

// x += delta (f16 [rows, C] with SAMQ_LN_DELTA_F16, else f32), in place, then y = LN(x) (f16, or
// int8 codes q(LN(x), out_scale) with SAMQ_LN_OUT_I8): the residual add of the preceding GEMM
// moved out of its epilogue.  Rows of C <= 1280 (the ViT-H / vit_b widths).
extern "C" int samq_add_layernorm(void* x, const void* delta, void* y, const float* gamma, const float* beta,
                                  int64_t rows, int C, float eps, int flags, float out_scale, hipStream_t stream) {
  if (rows == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(x && delta && y && gamma && beta, SAMQ_ERR_INVALID, "add_layernorm: null pointer");
  SAMQ_REQUIRE(C > 0 && C % 4 == 0 && C <= 1280, SAMQ_ERR_INVALID, "add_layernorm: C must be a multiple of 4, <= 1280");
  SAMQ_REQUIRE(!(flags & SAMQ_LN_OUT_I8) || out_scale > 0.f, SAMQ_ERR_INVALID, "add_layernorm: out_scale must be > 0");
  if (rows <= 0) return SAMQ_OK;
  const int rpw = ln_rpw(flags);
  SAMQ_REQUIRE(rpw == 1 || rpw == 2 || rpw == 4, SAMQ_ERR_INVALID, "add_layernorm: rows per wave must be 1, 2 or 4");
  const dim3 grid((unsigned)((rows + 4 * rpw - 1) / (4 * rpw)));
  const bool i8 = (flags & SAMQ_LN_OUT_I8) != 0, d16 = (flags & SAMQ_LN_DELTA_F16) != 0;
  const int vpt = (C / 4 + 63) / 64;
#define ALN(O, V, R, A) hipLaunchKernelGGL((layernorm_kernel<LN_F32, O, V, R, A>), grid, dim3(256), 0, stream, \
                                           (const void*)nullptr, y, gamma, beta, rows, C, eps, 1.f, out_scale, nullptr, \
                                           delta, (float*)x)
#define ALN_R(O, V, A) do { if (rpw == 1) ALN(O, V, 1, A); else if (rpw == 2) ALN(O, V, 2, A); else ALN(O, V, 4, A); } while (0)
#define ALN_V(O, A) do { if (vpt <= 3) ALN_R(O, 3, A); else if (vpt <= 4) ALN_R(O, 4, A); else ALN_R(O, 5, A); } while (0)
  if (i8) { if (d16) ALN_V(LN_I8, 1); else ALN_V(LN_I8, 2); }
  else { if (d16) ALN_V(LN_F16, 1); else ALN_V(LN_F16, 2); }
#undef ALN_V
#undef ALN_R
#undef ALN
  SAMQ_LAUNCH_CHECK("add_layernorm launch");
  return SAMQ_OK;
}

extern "C" int samq_layernorm_q(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C,
                                float eps, int flags, float in_scale, float out_scale, hipStream_t stream) {
  SAMQ_REQUIRE(!(flags & SAMQ_LN_IN_I8) || in_scale > 0.f, SAMQ_ERR_INVALID, "layernorm_q: in_scale must be > 0");
  SAMQ_REQUIRE(!(flags & SAMQ_LN_OUT_I8) || out_scale > 0.f, SAMQ_ERR_INVALID, "layernorm_q: out_scale must be > 0");
  const int in = (flags & SAMQ_LN_IN_I8) ? LN_I8 : ((flags & SAMQ_LN_IN_F16) ? LN_F16 : LN_F32);
  const int out = (flags & SAMQ_LN_OUT_I8) ? ((flags & SAMQ_LN_OUT_F32) ? LN_FQ32 : LN_I8)
                                           : ((flags & SAMQ_LN_OUT_F32) ? LN_F32 : LN_F16);
  return ln_launch(x, y, gamma, beta, rows, C, eps, in, out, in_scale, out_scale, ln_rpw(flags), stream);
}

extern "C" int samq_layernorm_q_zp(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C,
                                   float eps, int flags, float in_scale, float out_scale, int zp_in, int zp_out,
                                   hipStream_t stream) {
  SAMQ_REQUIRE(!(flags & SAMQ_LN_IN_I8) || in_scale > 0.f, SAMQ_ERR_INVALID, "layernorm_q_zp: in_scale must be > 0");
  SAMQ_REQUIRE(!(flags & SAMQ_LN_OUT_I8) || out_scale > 0.f, SAMQ_ERR_INVALID, "layernorm_q_zp: out_scale must be > 0");
  SAMQ_REQUIRE(zp_in >= -128 && zp_in <= 127 && zp_out >= -128 && zp_out <= 127, SAMQ_ERR_INVALID,
               "layernorm_q_zp: zero points must be in [-128, 127]");
  const int in = (flags & SAMQ_LN_IN_I8) ? LN_I8 : ((flags & SAMQ_LN_IN_F16) ? LN_F16 : LN_F32);
  const int out = (flags & SAMQ_LN_OUT_I8) ? ((flags & SAMQ_LN_OUT_F32) ? LN_FQ32 : LN_I8)
                                           : ((flags & SAMQ_LN_OUT_F32) ? LN_F32 : LN_F16);
  return ln_launch(x, y, gamma, beta, rows, C, eps, in, out, in_scale, out_scale, ln_rpw(flags), stream, nullptr,
                   nullptr, nullptr, true, zp_in, zp_out);
}

// samq_layernorm_q_zp on an int8 input under a Power-of-Two Factor quantiser (fq_vit observer/ptf.py):
// x = ((code - zp_in) << in_exp[c]) * in_scale, in_exp uint8 [C] in 0..3.  Outputs as _zp: int8 codes,
// f32 fake-quant or plain f32.
template <int O, int V, int R>
static void ln_ptf_launch(dim3 grid, hipStream_t stream, const void* x, void* y, const float* gamma, const float* beta,
                          int64_t rows, int C, float eps, float in_scale, float out_scale, int zp_in, int zp_out,
                          const uint8_t* in_exp) {
  hipLaunchKernelGGL((layernorm_kernel<LN_I8, O, V, R, 0, true, true>), grid, dim3(256), 0, stream, x, y, gamma, beta,
                     rows, C, eps, in_scale, out_scale, nullptr, (const void*)in_exp, nullptr, nullptr, nullptr, zp_in,
                     (float)zp_out);
}

extern "C" int samq_layernorm_q_ptf(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C,
                                    float eps, int flags, float in_scale, float out_scale, int zp_in, int zp_out,
                                    const uint8_t* in_exp, hipStream_t stream) {
  SAMQ_REQUIRE((flags & SAMQ_LN_IN_I8) != 0, SAMQ_ERR_INVALID, "layernorm_q_ptf: int8 input only (SAMQ_LN_IN_I8)");
  SAMQ_REQUIRE(in_exp && ((uintptr_t)in_exp & 15) == 0, SAMQ_ERR_INVALID,
               "layernorm_q_ptf: in_exp must be a 16-byte aligned array of C bytes");
  SAMQ_REQUIRE(in_scale > 0.f, SAMQ_ERR_INVALID, "layernorm_q_ptf: in_scale must be > 0");
  SAMQ_REQUIRE(!(flags & SAMQ_LN_OUT_I8) || out_scale > 0.f, SAMQ_ERR_INVALID, "layernorm_q_ptf: out_scale must be > 0");
  SAMQ_REQUIRE((flags & (SAMQ_LN_OUT_I8 | SAMQ_LN_OUT_F32)) != 0, SAMQ_ERR_UNSUPPORTED,
               "layernorm_q_ptf: int8-code or f32 output");
  SAMQ_REQUIRE(zp_in >= -128 && zp_in <= 127 && zp_out >= -128 && zp_out <= 127, SAMQ_ERR_INVALID,
               "layernorm_q_ptf: zero points must be in [-128, 127]");
  if (rows == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(x && y && gamma && beta, SAMQ_ERR_INVALID, "layernorm_q_ptf: null pointer");
  SAMQ_REQUIRE(C > 0 && C % 4 == 0 && C <= 4096, SAMQ_ERR_INVALID, "layernorm_q_ptf: C must be a multiple of 4, <= 4096");
  if (rows <= 0) return SAMQ_OK;
  int rpw = ln_rpw(flags);
  SAMQ_REQUIRE(rpw == 1 || rpw == 2 || rpw == 4, SAMQ_ERR_INVALID, "layernorm_q_ptf: rows per wave must be 1, 2 or 4");
  const int vpt = (C / 4 + 63) / 64;
  if (vpt > 5) rpw = 1;
  const dim3 grid((unsigned)((rows + 4 * rpw - 1) / (4 * rpw)));
  const int out = (flags & SAMQ_LN_OUT_I8) ? ((flags & SAMQ_LN_OUT_F32) ? LN_FQ32 : LN_I8) : LN_F32;
#define LNP(O, V, R) ln_ptf_launch<O, V, R>(grid, stream, x, y, gamma, beta, rows, C, eps, in_scale, out_scale, zp_in, zp_out, in_exp)
#define LNP_R(O, V) do { if (rpw == 1) LNP(O, V, 1); else if (rpw == 2) LNP(O, V, 2); else LNP(O, V, 4); } while (0)
#define LNP_V(O) \
  do { \
    if (vpt <= 1) LNP_R(O, 1); else if (vpt <= 3) LNP_R(O, 3); else if (vpt <= 4) LNP_R(O, 4); \
    else if (vpt <= 5) LNP_R(O, 5); else LNP(O, 16, 1); \
  } while (0)
  if (out == LN_I8) LNP_V(LN_I8); else if (out == LN_FQ32) LNP_V(LN_FQ32); else LNP_V(LN_F32);
#undef LNP_V
#undef LNP_R
#undef LNP
  SAMQ_LAUNCH_CHECK("layernorm_q_ptf launch");
  return SAMQ_OK;
}

// LN-q with the output rows' code sums (round 6): rowsum[r] = sum_c y[r, c] (int8 codes, SAMQ_LN_OUT_I8
// required) for the W4A8 zero-point GEMM that reads y; zero_rows (optional) [rows] int32 set to 0 --
// the accumulator the next int8-code GEMM epilogue adds its output row sums into
extern "C" int samq_layernorm_q_rs(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C,
                                   float eps, int flags, float in_scale, float out_scale, int32_t* rowsum,
                                   int32_t* zero_rows, hipStream_t stream) {
  SAMQ_REQUIRE((flags & SAMQ_LN_OUT_I8) && !(flags & SAMQ_LN_OUT_F32), SAMQ_ERR_INVALID,
               "layernorm_q_rs: row sums of int8-code outputs only (SAMQ_LN_OUT_I8)");
  SAMQ_REQUIRE(rows == 0 || rowsum, SAMQ_ERR_INVALID, "layernorm_q_rs: null rowsum");
  SAMQ_REQUIRE(!(flags & SAMQ_LN_IN_I8) || in_scale > 0.f, SAMQ_ERR_INVALID, "layernorm_q_rs: in_scale must be > 0");
  SAMQ_REQUIRE(out_scale > 0.f, SAMQ_ERR_INVALID, "layernorm_q_rs: out_scale must be > 0");
  const int in = (flags & SAMQ_LN_IN_I8) ? LN_I8 : ((flags & SAMQ_LN_IN_F16) ? LN_F16 : LN_F32);
  return ln_launch(x, y, gamma, beta, rows, C, eps, in, LN_I8, in_scale, out_scale, ln_rpw(flags), stream, nullptr,
                   rowsum, zero_rows);
}
