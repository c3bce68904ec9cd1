// GPTQ producer: the blocked column loop of GPTQ.fasterquant (reference gptq.py:97-146) in one launch.
//
// Every output row of W runs the same column recurrence against one shared upper Cholesky factor U
// ("Hinv") and never reads another row, so a workgroup of four waves owns a slab of 16 rows and walks
// all K / 128 column blocks for them; workgroups never synchronise with each other.  Per block:
//
//   stage      the 128 x 128 diagonal block of U goes to LDS as its upper triangle only, packed by column
//              PAIRS: entry (p, l >= p) is the float4 U[2p][2l], U[2p][2l+1], U[2p+1][2l], U[2p+1][2l+1], so
//              the two rows of U that a pair of columns needs are ONE ds_read_b128 per lane (33 KiB instead
//              of 64 KiB, conflict-free: the lanes of a read are contiguous);
//   recurrence each wave runs four rows, the 128 columns two per lane (lane l: columns 2l, 2l + 1).  Column
//              c's weight comes from its owning lane by v_readlane, every lane computes the (uniform) code,
//              fake value and error and updates its own two columns; the four rows' chains are independent
//              and share the U read, so one chain's divide latency hides under the others.  The owning lane
//              keeps code, fake value and error; Err1 (16 x 128) goes to LDS, codes and fake values to
//              global memory with one vector store per lane and row;
//   trailing   W[slab, i2:] -= Err1 @ U[i1:i2, i2:] on v_mfma_f32_16x16x4_f32 (M = 16 is the slab).  The A
//              fragments of Err1 are read from LDS once (32 k-steps, 32 VGPRs); a wave takes 64 columns at a
//              time as four MFMA tiles whose columns interleave (tile t, column n <-> n0 + 4 n + t), so
//              the B operand of all four is ONE float4 load per lane straight from global memory in the
//              MFMA's register layout (each element of U is used once per workgroup: no LDS stage) and
//              the C rows of W are float4 loads / stores in place.
//
// Right-looking order: W in global memory is always "the reference's outer W" for the columns behind the
// current block, which is what the group parameters of the reference read (gptq.py:113-117): a group's
// (scale, zero) come from the block-START state of the current block's columns (the lanes' registers
// before the recurrence) and, for groups of 256, from the next block as the last trailing update left it.
//
// Everything is fp32, every product and sum rounded separately as torch's ops round them (no contraction),
// both quotients are IEEE divisions.  No atomics.
#include "common.h"

#pragma clang fp contract(off)

namespace samq {
namespace {

constexpr int GB = 128;                       // column block (blocksize of fasterquant)
constexpr int SLAB = 16;                      // rows per workgroup = M of the MFMA
constexpr int TRI = 64 * 65 / 2;              // float4 entries of the packed triangle
constexpr int ERR_LD = GB + 4;                // Err1 row stride: the A-fragment reads hit every bank twice

__device__ __forceinline__ int tri_off(int p) { return 64 * p - ((p * (p - 1)) >> 1); }

__device__ __forceinline__ float lane_read(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// min / max over aligned groups of N lanes (N a power of two <= 64); every lane gets its group's value
template <int N>
__device__ __forceinline__ void group_minmax(float& mn, float& mx) {
#pragma unroll
  for (int o = 1; o < N; o <<= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
}

// Quantizer.find_params on one slice's min / max
__device__ __forceinline__ void find_params(float mn, float mx, float maxq, float& s, float& z) {
  mn = fminf(mn, 0.f);
  mx = fmaxf(mx, 0.f);
  if (mn == 0.f && mx == 0.f) {
    mn = -1.f;
    mx = 1.f;
  }
  s = (mx - mn) / maxq;
  z = rintf(-mn / s);
}

// GS: 0 = one group per row (groupsize -1), else the group size (32, 64, 128, 256)
template <int GS>
__global__ __launch_bounds__(256) void gptq_quant_kernel(float* __restrict__ W, const float* __restrict__ U,
                                                         uint8_t* __restrict__ codes, float* __restrict__ scale,
                                                         float* __restrict__ zero, int rows, int K, float maxq) {
  __shared__ float4_t Ut[TRI];
  __shared__ float Err[SLAB * ERR_LD];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slab0 = blockIdx.x * SLAB;
  const int G = GS == 0 ? 1 : K / GS;

  int row[4];
  bool live[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    row[j] = slab0 + wave * 4 + j;
    live[j] = row[j] < rows;
  }

  float scv[4], zv[4];   // per lane: the parameters of the group its two columns belong to
  if constexpr (GS == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mn = 0.f, mx = 0.f;
      if (live[j])
        for (int k = 2 * lane; k < K; k += GB) {
          const float2_t v = *(const float2_t*)(W + (size_t)row[j] * K + k);
          mn = fminf(mn, fminf(v.x, v.y));
          mx = fmaxf(mx, fmaxf(v.x, v.y));
        }
      group_minmax<64>(mn, mx);
      find_params(mn, mx, maxq, scv[j], zv[j]);
      if (live[j] && lane == 0) {
        scale[row[j]] = scv[j];
        zero[row[j]] = zv[j];
      }
    }
  }

  for (int i1 = 0; i1 < K; i1 += GB) {
    const int i2 = i1 + GB;

    // ---- stage the diagonal block's upper triangle, load the block-start weights
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int p = it * 4 + wave;
      if (lane >= p) {
        const float* up = U + (size_t)(i1 + 2 * p) * K + i1 + 2 * lane;
        const float2_t r0 = *(const float2_t*)up, r1 = *(const float2_t*)(up + K);
        Ut[tri_off(p) + lane - p] = float4_t{r0.x, r0.y, r1.x, r1.y};
      }
    }
    float2_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      w[j] = live[j] ? *(const float2_t*)(W + (size_t)row[j] * K + i1 + 2 * lane) : float2_t{0.f, 0.f};

    // ---- group parameters from the outer W: block-start values of this block (the registers), and for
    // groups of 256 the next block as it stands in global memory
    if constexpr (GS != 0) {
      if (GS < 256 || (i1 & 255) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float mn = fminf(w[j].x, w[j].y), mx = fmaxf(w[j].x, w[j].y);
          if constexpr (GS == 256) {
            const float2_t v = live[j] ? *(const float2_t*)(W + (size_t)row[j] * K + i2 + 2 * lane) : float2_t{0.f, 0.f};
            mn = fminf(mn, fminf(v.x, v.y));
            mx = fmaxf(mx, fmaxf(v.x, v.y));
          }
          group_minmax<(GS >= 128 ? 64 : GS / 2)>(mn, mx);
          find_params(mn, mx, maxq, scv[j], zv[j]);
          const int c = i1 + 2 * lane;
          if (live[j] && c % GS == 0) {
            scale[(size_t)row[j] * G + c / GS] = scv[j];
            zero[(size_t)row[j] * G + c / GS] = zv[j];
          }
        }
      }
    }
    __syncthreads();

    // ---- the recurrence over the block's 64 column pairs
    float2_t fq[4], cd[4], er[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fq[j] = cd[j] = er[j] = float2_t{0.f, 0.f};
    for (int p = 0; p < 64; ++p) {
      // lanes below p read the tail of the previous pair's entries: in bounds, and they feed only the
      // registers of columns that are already quantised
      const float4_t u = Ut[tri_off(p) + lane - p];
      const float d0 = lane_read(u.x, p), d1 = lane_read(u.w, p);
      const bool own = lane == p;
      float s[4], z[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[j] = lane_read(scv[j], p);
        z[j] = lane_read(zv[j], p);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {   // column 2p
        const float wc = lane_read(w[j].x, p);
        const float q = fminf(fmaxf(rintf(wc / s[j]) + z[j], 0.f), maxq);
        const float f = s[j] * (q - z[j]);
        const float e = (wc - f) / d0;
        w[j].x = w[j].x - e * u.x;
        w[j].y = w[j].y - e * u.y;
        fq[j].x = own ? f : fq[j].x;
        cd[j].x = own ? q : cd[j].x;
        er[j].x = own ? e : er[j].x;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {   // column 2p + 1
        const float wc = lane_read(w[j].y, p);
        const float q = fminf(fmaxf(rintf(wc / s[j]) + z[j], 0.f), maxq);
        const float f = s[j] * (q - z[j]);
        const float e = (wc - f) / d1;
        w[j].x = w[j].x - e * u.z;
        w[j].y = w[j].y - e * u.w;
        fq[j].y = own ? f : fq[j].y;
        cd[j].y = own ? q : cd[j].y;
        er[j].y = own ? e : er[j].y;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *(float2_t*)(Err + (wave * 4 + j) * ERR_LD + 2 * lane) = er[j];
      if (live[j]) {
        const size_t o = (size_t)row[j] * K + i1 + 2 * lane;
        *(float2_t*)(W + o) = fq[j];
        if (codes) *(uint16_t*)(codes + o) = (uint16_t)((uint32_t)cd[j].x | ((uint32_t)cd[j].y << 8));
      }
    }
    __syncthreads();

    // ---- trailing update of the columns behind the block
    if (i2 < K) {
      const int kr = lane >> 4, nc = 4 * (lane & 15);
      float a[32];
#pragma unroll
      for (int s = 0; s < 32; ++s) a[s] = Err[(lane & 15) * ERR_LD + 4 * s + kr];
      for (int n0 = i2 + 64 * wave; n0 < K; n0 += 256) {
        float4_t acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = float4_t{0.f, 0.f, 0.f, 0.f};
        const float* up = U + (size_t)(i1 + kr) * K + n0 + nc;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
          const float4_t b = *(const float4_t*)(up + (size_t)(4 * s) * K);
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b.x, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b.y, acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b.z, acc[2], 0, 0, 0);
          acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b.w, acc[3], 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = slab0 + 4 * kr + v;
          if (r < rows) {
            float4_t* wp = (float4_t*)(W + (size_t)r * K + n0 + nc);
            float4_t x = *wp;
            x.x -= acc[0][v];
            x.y -= acc[1][v];
            x.z -= acc[2][v];
            x.w -= acc[3][v];
            *wp = x;
          }
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace
}  // namespace samq

using namespace samq;

extern "C" int samq_gptq_quant(float* W, const float* U, uint8_t* codes, float* scale, float* zero, int rows, int K,
                               int groupsize, int maxq, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  (void)workspace;
  (void)workspace_bytes;
  SAMQ_REQUIRE(W && U && scale && zero, SAMQ_ERR_INVALID, "gptq_quant: null pointer");
  SAMQ_REQUIRE(rows > 0 && K > 0, SAMQ_ERR_INVALID, "gptq_quant: empty weight");
  SAMQ_REQUIRE(maxq >= 3 && maxq <= 255, SAMQ_ERR_INVALID, "gptq_quant: maxq outside 3..255");
  SAMQ_REQUIRE((((uintptr_t)W | (uintptr_t)U) & 15) == 0 && ((uintptr_t)codes & 1) == 0, SAMQ_ERR_INVALID,
               "gptq_quant: W and U must be 16-byte aligned, codes 2-byte aligned");
  SAMQ_REQUIRE(K % GB == 0, SAMQ_ERR_UNSUPPORTED, "gptq_quant: K must be a multiple of 128");
  SAMQ_REQUIRE(groupsize == -1 || groupsize == 32 || groupsize == 64 || groupsize == 128 || groupsize == 256,
               SAMQ_ERR_UNSUPPORTED, "gptq_quant: groupsize must be -1, 32, 64, 128 or 256");
  SAMQ_REQUIRE(groupsize == -1 || K % groupsize == 0, SAMQ_ERR_UNSUPPORTED,
               "gptq_quant: K must be a multiple of groupsize");
  const dim3 grid((unsigned)((rows + SLAB - 1) / SLAB)), block(256);
  const float mq = (float)maxq;
#define SAMQ_GPTQ_LAUNCH(GS) \
  hipLaunchKernelGGL((gptq_quant_kernel<GS>), grid, block, 0, stream, W, U, codes, scale, zero, rows, K, mq)
  switch (groupsize) {
    case -1: SAMQ_GPTQ_LAUNCH(0); break;
    case 32: SAMQ_GPTQ_LAUNCH(32); break;
    case 64: SAMQ_GPTQ_LAUNCH(64); break;
    case 128: SAMQ_GPTQ_LAUNCH(128); break;
    default: SAMQ_GPTQ_LAUNCH(256); break;
  }
#undef SAMQ_GPTQ_LAUNCH
  SAMQ_LAUNCH_CHECK("gptq_quant launch");
  return SAMQ_OK;
}
