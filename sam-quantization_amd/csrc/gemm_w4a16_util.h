// W4A16 GEMM: helpers shared by the kernel families -- counted vmcnt waits, the int4 -> fp16
// unpack and the LayerNorm-fold epilogue pieces.  Included by gemm_w4a16.hip only.
#pragma once

#include "common.h"

namespace samq {

template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N <= 63, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// int4 -> fp16 unpack of one packed word (8 k-values of one column, nibble order
// [k0,k2,k4,k6 | k1,k3,k5,k7]; nibble group i at bits 4i..4i+3 of both halves).  A nibble on
// mantissa bits 0..3 under the exponent of 1024 is the exact fp16 integer 1024+q; on bits 4..7
// under the exponent of 64 it is 64+q.  So groups 0 and 1 convert in place and groups 2 and 3
// after ONE shift by 8 of the word: 5 bit ops + 4 packed subtractions of (magic + zp) per 8
// weights instead of 7 + 4.  (Bits 8..15 would reach the 5-bit exponent field.)
struct W4Unpack {
  uint32_t m0, m1, g0, g1;   // masks / magics, held in VGPRs (gfx950 VOP3 takes no literal)
  __device__ void init() {
    m0 = 0x000F000Fu; m1 = 0x00F000F0u; g0 = 0x64006400u; g1 = 0x54005400u;
    asm volatile("" : "+v"(m0), "+v"(m1), "+v"(g0), "+v"(g1));
  }
};
struct W4Zero {   // (magic + zero point) splats of one column
  half2_t z1024, z64;
  __device__ void set(int zp) {
    const _Float16 a = (_Float16)(1024 + zp), b = (_Float16)(64 + zp);
    z1024 = half2_t{a, a};
    z64 = half2_t{b, b};
  }
};
__device__ __forceinline__ half8_t w4_unpack(uint32_t w, const W4Unpack& k, const W4Zero& z) {
  const uint32_t w8 = w >> 8;
  const half2_t h0 = __builtin_bit_cast(half2_t, (w & k.m0) | k.g0) - z.z1024;
  const half2_t h1 = __builtin_bit_cast(half2_t, (w & k.m1) | k.g1) - z.z64;
  const half2_t h2 = __builtin_bit_cast(half2_t, (w8 & k.m0) | k.g0) - z.z1024;
  const half2_t h3 = __builtin_bit_cast(half2_t, (w8 & k.m1) | k.g1) - z.z64;
  return half8_t{h0[0], h0[1], h1[0], h1[1], h2[0], h2[1], h3[0], h3[1]};
}
// grouped weights: the exact integers (q - zp) times the group's fp16 scale, one rounding
__device__ __forceinline__ half8_t scale8(half8_t v, half2_t s) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const half2_t h = half2_t{v[2 * i], v[2 * i + 1]} * s;
    v[2 * i] = h[0];
    v[2 * i + 1] = h[1];
  }
  return v;
}

// ---- LayerNorm-fold epilogues (SAMQ_EPI_RESADD_LNF / BIAS_LNF / GELU_LNF, include/samq.h)
struct LnfArgs {
  const float* gamma;   // producer: the next LayerNorm's weight [N]
  const float* gw;      // consumer: gamma . W [N]
  const float* bw;      // consumer: beta . W [N]
  float* stats;         // [M][N_producer / 64][2] partial sums of (x - mu_p), (x - mu_p)^2
  float* mu;            // [M] row mean of the previous LayerNorm (consumer: += delta)
  _Float16* aout;       // producer: f16 (x - mu_p) * gamma [M][N]
  float eps;
  int nblk;             // consumer: K / 64 partial-sum blocks per row
  const _Float16* bias; // consumer: the layer bias (set by the kernel)
};
constexpr bool lnf_producer(int epi) { return epi == SAMQ_EPI_RESADD_LNF; }
constexpr bool lnf_consumer(int epi) { return epi == SAMQ_EPI_BIAS_LNF || epi == SAMQ_EPI_GELU_LNF; }
constexpr bool epi_f32_out(int epi) {
  return epi == SAMQ_EPI_RESADD_F32 || epi == SAMQ_EPI_F32 || epi == SAMQ_EPI_RESADD_LNF;
}

// producer: one f32 residual row chunk (4 columns at col of row) x_new = xo + v (xo: the old
// residual, loaded ahead by the caller), its f16 fold operand and this lane's partial sums; the
// caller reduces the sums over the 16 lanes of a row
__device__ __forceinline__ void lnf_res4(const LnfArgs& L, float* C, int64_t ldc, int N, int64_t row, int col,
                                         float4_t xo, float4_t v, float m, float4_t g, float& s1, float& s2) {
  const float4_t x = xo + v;
  *(float4_t*)(C + row * ldc + col) = x;
  const float4_t d = x - m;
  *(half4_t*)(L.aout + row * N + col) = half4_t{(_Float16)(d[0] * g[0]), (_Float16)(d[1] * g[1]),
                                                (_Float16)(d[2] * g[2]), (_Float16)(d[3] * g[3])};
  s1 = (d[0] + d[1]) + (d[2] + d[3]);
  s2 = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
}
// sum over the 16 lanes of a DPP row (the xor-1, 2, 4, 8 butterfly's order: same bits)
__device__ __forceinline__ float sum16_dpp(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
  return v;
}
// ... reduced over 16 lanes (one row), lane 0 of the 16 writes the block's pair
__device__ __forceinline__ void lnf_stats16(const LnfArgs& L, int N, int64_t row, int col_block, bool valid,
                                            float s1, float s2, int c4) {
  s1 = sum16_dpp(s1);
  s2 = sum16_dpp(s2);
  if (valid && c4 == 0) *(float2_t*)(L.stats + (row * (N / 64) + col_block) * 2) = float2_t{s1, s2};
}
// producer slice of R rows x 64 columns staged in LDS at ep (row pitch P floats): the old residual
// and the row means are all loaded before the first store (no store-to-load ordering per chunk)
template <int R, int P>
__device__ __forceinline__ void lnf_produce_slice(const LnfArgs& L, const float* ep, float* C, int64_t ldc, int N,
                                                  int M, int srow0, int col_base, int lane) {
  constexpr int J = R * 16 / 64;
  const int c4 = lane & 15;
  const int col = col_base + 4 * c4;
  const float4_t g = *(const float4_t*)(L.gamma + col);
  float4_t xo[J];
  float m[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    int64_t row = srow0 + 4 * j + (lane >> 4);
    row = row < M ? row : M - 1;
    xo[j] = *(const float4_t*)(C + row * ldc + col);
    m[j] = L.mu[row];
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int rl = 4 * j + (lane >> 4);
    const int row = srow0 + rl;
    const float4_t v = *(const float4_t*)(ep + rl * P + 4 * c4);
    float s1 = 0.f, s2 = 0.f;
    if (row < M) lnf_res4(L, C, ldc, N, row, col, xo[j], v, m[j], g, s1, s2);
    lnf_stats16(L, N, row, col_base / 64, row < M, s1, s2, c4);
  }
}
// consumer: (delta, rstd) of the workgroup's BM rows into LDS (rowinfo[BM]), mu += delta by the
// workgroups of column tile 0.  The rows' partial sums (BM x nblk float2, contiguous) arrive by
// LDS-DMA (1 KiB pieces dealt over the NW waves, one wait), then one lane per row adds its nblk
// pairs in block order from LDS (the order of the standalone reduction: same bits).  No read
// leaves stats[0 .. M * nblk * 2).
template <int BM, int NW>
__device__ __forceinline__ void lnf_rowinfo_wg(const LnfArgs& L, float2_t* rowinfo, char* sbuf, int M, int row_base,
                                               bool col0, int wave, int lane) {
  static_assert(BM % (NW * 32) == 0 || BM <= NW * 64, "rows per wave");
  const int nfl = 2 * L.nblk;                                 // floats per row
  const int npieces = BM * nfl / 256;                         // 1 KiB pieces (BM * nblk * 8 / 1024)
  const float* base = L.stats + (int64_t)row_base * nfl;
  const int64_t nvalid = (int64_t)(M - row_base) * nfl;       // floats of the rows < M, from base
  const int64_t lim = nvalid - 4;                             // last in-bounds 16-byte chunk
  // A chunk past lim is clamped to it, which leaves the slots of rows >= M with stale pairs (never
  // used).  Where the valid rows end 8 bytes past a 16-byte boundary (rows left and nblk both odd)
  // the chunk holding the last row's last pair is clamped back by one pair as well: that one pair
  // is read from global memory by its row's lane below.  lim < 0 (M = 1, nblk = 1: 8 bytes of
  // stats in all) has no in-bounds chunk: nothing is staged.
  const int tail_rl = (nvalid & 2) != 0 && M - row_base <= BM ? M - row_base - 1 : -1;
  if (lim >= 0) {
    for (int pc = wave; pc < npieces; pc += NW) {
      int64_t off = (int64_t)(pc * 64 + lane) * 4;
      off = off <= lim ? off : lim;
      __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)(base + off), (SAMQ_LDS void*)(sbuf + pc * 1024), 16, 0, 0);
    }
  }
  vm_wait<0>();
  __syncthreads();
  const float inv_k = 1.0f / (float)(L.nblk * 64);
  constexpr int RPW = BM / NW;                                // rows per wave
#pragma unroll
  for (int q = 0; q < (RPW + 63) / 64; ++q) {
    const int rl = wave * RPW + q * 64 + lane;
    if (q * 64 + lane < RPW) {
      const float2_t* sp = (const float2_t*)(sbuf + rl * nfl * 4);
      float s1 = 0.f, s2 = 0.f;
      for (int b = 0; b < L.nblk - 1; ++b) {
        const float2_t v = sp[b];
        s1 += v.x;
        s2 += v.y;
      }
      float2_t last = sp[L.nblk - 1];
      if (rl == tail_rl) last = *(const float2_t*)(base + nvalid - 2);
      s1 += last.x;
      s2 += last.y;
      const float delta = s1 * inv_k;
      const float var = fmaxf(s2 * inv_k - delta * delta, 0.0f);
      rowinfo[rl] = float2_t{delta, rsqrtf(var + L.eps)};
      const int64_t row = row_base + rl;
      if (col0 && row < M) L.mu[row] += delta;
    }
  }
  __syncthreads();
}
// consumer store of 8 columns: y = rstd * (v - delta * gw) + (bw + bias) (-> GELU), f16
template <int EPI>
__device__ __forceinline__ half8_t lnf_out8(float4_t v0, float4_t v1, float2_t ri, const float (&gw)[8],
                                           const float (&bb)[8]) {
  float y[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
  half8_t h;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float t = __builtin_fmaf(ri.y, __builtin_fmaf(-ri.x, gw[e], y[e]), bb[e]);
    if (EPI == SAMQ_EPI_GELU_LNF) t = gelu_fast(t);
    h[e] = (_Float16)t;
  }
  return h;
}

}  // namespace samq
