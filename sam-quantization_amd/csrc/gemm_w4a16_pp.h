// W4A16 ping-pong GEMM kernel (v6, k-phases) with its LDS layout and epilogues.
// Included by gemm_w4a16.hip only.
#pragma once

#include "gemm_w4a16_util.h"

namespace samq {

// Variant flags of the ping-pong kernel: the VAR template argument of pp2_tile / w4a16_gemm_pp2 is
// an OR of these.  The values are part of the kernels' mangled names.
enum : int {
  PP_T_NO_RESTAGE = 1,        // tuning build, timing-only (wrong results): no restaging of the ring
  PP_T_NO_MFMA = 2,           // tuning build, timing-only (wrong results): no MFMA
  PP_MFMA16 = 16,             // v_mfma_f32_16x16x32_f16 fragments instead of 32x32x16
  PP_GROUPED = 512,           // grouped weights (groupsize < K): per-group scale / zero rows
  PP_WAVE_SGPR = 4096,        // the wave index, hence piece choices and addresses, in an SGPR
  PP_DMA_SPREAD = 16384,      // LDS-DMA pieces spread through the MFMA burst instead of after it
  PP_T_NO_EPILOGUE = 32768,   // tuning build, timing-only (wrong results): no epilogue
  PP_TE_STAGED = 65536,       // transposed accumulators + the LDS-staged f16 epilogue
  PP_PERSISTENT = 1 << 20,    // at most one workgroup per CU loops over the tiles
  PP_EARLY_EP = 1 << 21,      // the epilogue's scale / bias loaded before the prologue
  PP_F16T = 1 << 22,          // f16 outputs staged transposed (pp_epilogue_f16t)
  PP_GROUP_REGS = 1 << 23,    // with PP_GROUPED: group rows prefetched into VGPRs, not in the ring
};

// The same epilogue for 16x16x32 accumulators (PP_MFMA16): lane (ql, g)
// of 16-row tile i, 32-column block t, half h holds rows 16i + 4g + r of column 32t + 16h + ql;
// staged per 16-row tile with a padded pitch (WN + 4 floats: the four lane groups' rows land
// on different banks).
// RES (SAMQ_EPI_RESADD_F32): the old residual is read a batch of RES_NB16 slices ahead (res_load,
// common.h).  xpre = the first batch, loaded by the caller before the epilogue's barrier.
constexpr int RES_NB16 = 2;
template <int TM16, int TN, int EPI>
__device__ __forceinline__ void pp_epilogue16(const float4_t (&acc)[TM16][TN][2], const float (&csc)[TN][2],
                                              const float (&cb)[TN][2], char* ep_bytes, void* Cout, int64_t ldc,
                                              int M, int row_base, int col_base, int lane,
                                              const LnfArgs& L = LnfArgs{}, int N = 0,
                                              const float2_t* rowinfo = nullptr, const float4_t* xpre = nullptr) {
  constexpr int WN = TN * 32, EP_ROWS = 16, PITCH = WN + 4;
  static_assert(!(lnf_producer(EPI) || lnf_consumer(EPI)) || WN == 64, "LN fold: 64-column wave tiles");
  constexpr bool RES = EPI == SAMQ_EPI_RESADD_F32;
  static_assert(!RES || TM16 % RES_NB16 == 0, "residual batches");
  constexpr int RJ = res_j(EP_ROWS, WN), RX = RES ? RES_NB16 * RJ : 1;
  float4_t xo[2][RX];   // RES: the old residual of the current and the next batch of slices
  if constexpr (RES) {
#pragma unroll
    for (int k = 0; k < RX; ++k) xo[0][k] = xpre[k];
  }
  float* ep = (float*)ep_bytes;
  const int ql = lane & 15, g = lane >> 4;
  float gw8[8], bb8[8];   // LNF consumer: this lane's 8 columns (fixed over the slices)
  if constexpr (lnf_consumer(EPI)) {
    const int c0 = col_base + 8 * (lane % (WN / 8));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      gw8[e] = L.gw[c0 + e];
      bb8[e] = L.bw[c0 + e] + (L.bias ? (float)L.bias[c0 + e] : 0.0f);
    }
  }
#pragma unroll
  for (int i = 0; i < TM16; ++i) {
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = lnf_consumer(EPI) ? acc[i][t][h][r] * csc[t][h] : acc[i][t][h][r] * csc[t][h] + cb[t][h];
          if (EPI == SAMQ_EPI_BIAS_GELU) v = gelu_fast(v);
          ep[(4 * g + r) * PITCH + 32 * t + 16 * h + ql] = v;
        }
    if constexpr (RES) {   // the next batch's residual: in flight over this batch's staging and stores
      if (i % RES_NB16 == 0 && i + RES_NB16 < TM16) {
#pragma unroll
        for (int b = 0; b < RES_NB16; ++b)
          res_load<EP_ROWS, WN>(&xo[(i / RES_NB16 + 1) & 1][b * RJ], Cout, ldc, M, row_base + (i + RES_NB16 + b) * 16,
                                col_base, lane);
      }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slice is in LDS (same wave reads it)
    const int srow0 = row_base + i * 16;
    if (lnf_producer(EPI)) {
      lnf_produce_slice<EP_ROWS, PITCH>(L, ep, (float*)Cout, ldc, N, M, srow0, col_base, lane);
    } else if (EPI == SAMQ_EPI_RESADD_F32 || EPI == SAMQ_EPI_F32) {
      constexpr int C4 = WN / 4;
#pragma unroll
      for (int j = 0; j < (EP_ROWS * C4 + 63) / 64; ++j) {
        const int idx = j * 64 + lane;
        if (idx < EP_ROWS * C4) {
          const int rl = idx / C4, c4 = idx % C4;
          const int row = srow0 + rl;
          float4_t v = *(const float4_t*)(ep + rl * PITCH + 4 * c4);
          if constexpr (RES) v = res_add(xo[(i / RES_NB16) & 1][(i % RES_NB16) * RJ + j], v);
          if (row < M) *(float4_t*)((float*)Cout + (int64_t)row * ldc + col_base + 4 * c4) = v;
        }
      }
    } else if (lnf_consumer(EPI)) {
      constexpr int C8 = WN / 8;
#pragma unroll
      for (int j = 0; j < (EP_ROWS * C8 + 63) / 64; ++j) {
        const int idx = j * 64 + lane;
        if (idx < EP_ROWS * C8) {
          const int rl = idx / C8, c8 = idx % C8;
          const int row = srow0 + rl;
          const float4_t v0 = *(const float4_t*)(ep + rl * PITCH + 8 * c8);
          const float4_t v1 = *(const float4_t*)(ep + rl * PITCH + 8 * c8 + 4);
          if (row < M) {
            const float2_t ri = rowinfo[row - row_base];
            *(half8_t*)((_Float16*)Cout + (int64_t)row * ldc + col_base + 8 * c8) = lnf_out8<EPI>(v0, v1, ri, gw8, bb8);
          }
        }
      }
    } else {
      constexpr int C8 = WN / 8;
#pragma unroll
      for (int j = 0; j < (EP_ROWS * C8 + 63) / 64; ++j) {
        const int idx = j * 64 + lane;
        if (idx < EP_ROWS * C8) {
          const int rl = idx / C8, c8 = idx % C8;
          const int row = srow0 + rl;
          const float4_t v0 = *(const float4_t*)(ep + rl * PITCH + 8 * c8);
          const float4_t v1 = *(const float4_t*)(ep + rl * PITCH + 8 * c8 + 4);
          if (row < M) {
            const half8_t hv = {(_Float16)v0[0], (_Float16)v0[1], (_Float16)v0[2], (_Float16)v0[3],
                                (_Float16)v1[0], (_Float16)v1[1], (_Float16)v1[2], (_Float16)v1[3]};
            *(half8_t*)((_Float16*)Cout + (int64_t)row * ldc + col_base + 8 * c8) = hv;
          }
        }
      }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);   // reads done before the next slice overwrites
  }
}

// y = acc * s[n] + b[n] (-> GELU / residual add), staged through LDS in EP_ROWS-row slices per
// wave so the global traffic is row-contiguous 16-byte vectors (v3's epilogue)
// RES (SAMQ_EPI_RESADD_F32): the old residual is read one slice ahead of the stores (res_load,
// common.h); xpre = the first slice's, loaded by the caller before the epilogue's barrier
template <int TM, int TN, int EP_ROWS, int EPI>
__device__ __forceinline__ void pp_epilogue(const float16_t (&acc)[TM][TN], const float (&csc)[TN],
                                            const float (&cb)[TN], char* ep_bytes, void* Cout, int64_t ldc,
                                            int M, int row_base, int col_base, int lane,
                                            const LnfArgs& L = LnfArgs{}, int N = 0,
                                            const float2_t* rowinfo = nullptr, const float4_t* xpre = nullptr) {
  constexpr int WN = TN * 32;
  constexpr int NSL = 32 / EP_ROWS;
  constexpr bool RES = EPI == SAMQ_EPI_RESADD_F32;
  constexpr int RJ = RES ? res_j(EP_ROWS, WN) : 1;
  float4_t xo[2][RJ];   // RES: the old residual of the current and the next slice
  if constexpr (RES) {
#pragma unroll
    for (int k = 0; k < RJ; ++k) xo[0][k] = xpre[k];
  }
  static_assert(!(lnf_producer(EPI) || lnf_consumer(EPI)) || WN == 64, "LN fold: 64-column wave tiles");
  float* ep = (float*)ep_bytes;
  const int hsel = lane >> 5;
  constexpr bool F16SWZ = EPI == SAMQ_EPI_BIAS || EPI == SAMQ_EPI_BIAS_GELU;   // staging swizzle (below)
  if constexpr (EPI == SAMQ_EPI_SILU_MUL) {
    // gated MLP: the wave's 64 columns are one 32-column block of the gate (t = 0) and the same
    // block of the up projection (t = 1) -- samq_w4_interleave32 layout; out f16 [M, N / 2] =
    // silu(gate) * up, the 32 output columns of block (col_base / 64)
    static_assert(TN == 2 && EP_ROWS == 32, "SILU_MUL: 64-column wave tiles");
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = (r & 3) + 8 * (r >> 2) + 4 * hsel;
        const float gv = acc[i][0][r] * csc[0], uv = acc[i][1][r] * csc[1];
        ep[rl * 32 + (lane & 31)] = gv / (1.0f + __expf(-gv)) * uv;
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);
      const int srow0 = row_base + i * 32;
#pragma unroll
      for (int j = 0; j < 2; ++j) {   // 32 rows x 4 chunks of 8 columns
        const int idx = j * 64 + lane;
        const int rl = idx >> 2, c8 = idx & 3;
        const int row = srow0 + rl;
        const float4_t v0 = ((const float4_t*)ep)[2 * idx];
        const float4_t v1 = ((const float4_t*)ep)[2 * idx + 1];
        if (row < M) {
          const half8_t h = {(_Float16)v0[0], (_Float16)v0[1], (_Float16)v0[2], (_Float16)v0[3],
                             (_Float16)v1[0], (_Float16)v1[1], (_Float16)v1[2], (_Float16)v1[3]};
          *(half8_t*)((_Float16*)Cout + (int64_t)row * ldc + col_base / 2 + 8 * c8) = h;
        }
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);
    }
    return;
  }
  float gw8[8], bb8[8];   // LNF consumer: this lane's 8 columns (fixed over the slices)
  if constexpr (lnf_consumer(EPI)) {
    const int c0 = col_base + 8 * (lane % (WN / 8));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      gw8[e] = L.gw[c0 + e];
      bb8[e] = L.bw[c0 + e] + (L.bias ? (float)L.bias[c0 + e] : 0.0f);
    }
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
#pragma unroll
      for (int rq = 0; rq < 16 / NSL; rq += 2) {   // accumulator pairs (r, r + 1): packed fp32 math
        const int r = sl * (16 / NSL) + rq;
        const int rl = (r & 3) + 8 * (r >> 2) + 4 * hsel - sl * EP_ROWS;   // row within the slice (r + 1: rl + 1)
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          float2_t v = __builtin_elementwise_fma((float2_t){acc[i][t][r], acc[i][t][r + 1]}, (float2_t)(csc[t]),
                                                 (float2_t)(lnf_consumer(EPI) ? 0.0f : cb[t]));
          if (EPI == SAMQ_EPI_BIAS_GELU) v = gelu_fast2(v);
          // f16 outputs: the 4-column chunk XOR ((rl >> 1) & 1) within each 8 columns, so the two
          // 16-byte reads of a lane group's 4 rows land on distinct banks (gemm_i8_epilogue.h)
          const int cs = (t * 32 + (lane & 31)) ^ (F16SWZ ? 4 * ((rl >> 1) & 1) : 0);
          ep[rl * WN + cs] = v.x;
          ep[(rl + 1) * WN + cs] = v.y;
        }
      }
      const int srow0 = row_base + i * 32 + sl * EP_ROWS;
      const int sn = i * NSL + sl;   // slice number
      if constexpr (RES) {   // the next slice's residual: in flight over this slice's staging and stores
        if (sn + 1 < TM * NSL) res_load<EP_ROWS, WN>(xo[(sn + 1) & 1], Cout, ldc, M, srow0 + EP_ROWS, col_base, lane);
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slice is in LDS (same wave reads it)
      if (lnf_producer(EPI)) {
        lnf_produce_slice<EP_ROWS, WN>(L, ep, (float*)Cout, ldc, N, M, srow0, col_base, lane);
      } else if (lnf_consumer(EPI)) {
        constexpr int C8 = WN / 8;
#pragma unroll
        for (int j = 0; j < (EP_ROWS * C8 + 63) / 64; ++j) {
          const int idx = j * 64 + lane;
          if (idx < EP_ROWS * C8) {
            const int rl = idx / C8, c8 = idx % C8;
            const int row = srow0 + rl;
            const float4_t v0 = ((const float4_t*)ep)[2 * idx];
            const float4_t v1 = ((const float4_t*)ep)[2 * idx + 1];
            if (row < M) {
              const float2_t ri = rowinfo[row - row_base];
              *(half8_t*)((_Float16*)Cout + (int64_t)row * ldc + col_base + 8 * c8) = lnf_out8<EPI>(v0, v1, ri, gw8, bb8);
            }
          }
        }
      } else if (EPI == SAMQ_EPI_RESADD_F32 || EPI == SAMQ_EPI_F32) {
        constexpr int C4 = WN / 4;
#pragma unroll
        for (int j = 0; j < (EP_ROWS * C4 + 63) / 64; ++j) {
          const int idx = j * 64 + lane;
          if (idx < EP_ROWS * C4) {
            const int rl = idx / C4, c4 = idx % C4;
            const int row = srow0 + rl;
            float4_t v = ((const float4_t*)ep)[idx];
            if constexpr (RES) v = res_add(xo[sn & 1][j], v);
            if (row < M) *(float4_t*)((float*)Cout + (int64_t)row * ldc + col_base + 4 * c4) = v;
          }
        }
      } else {
        constexpr int C8 = WN / 8;
#pragma unroll
        for (int j = 0; j < (EP_ROWS * C8 + 63) / 64; ++j) {
          const int idx = j * 64 + lane;
          if (idx < EP_ROWS * C8) {
            const int rl = idx / C8, c8 = idx % C8;
            const int row = srow0 + rl;
            const int sk = (rl >> 1) & 1;   // F16SWZ
            const float4_t v0 = ((const float4_t*)ep)[2 * idx + sk];
            const float4_t v1 = ((const float4_t*)ep)[2 * idx + (1 ^ sk)];
            if (row < M) {
              const half8_t h = {(_Float16)v0[0], (_Float16)v0[1], (_Float16)v0[2], (_Float16)v0[3],
                                 (_Float16)v1[0], (_Float16)v1[1], (_Float16)v1[2], (_Float16)v1[3]};
              *(half8_t*)((_Float16*)Cout + (int64_t)row * ldc + col_base + 8 * c8) = h;
            }
          }
        }
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);   // reads done before the next slice overwrites
    }
  }
}

// f16-output epilogue staged TRANSPOSED (PP_F16T): per 32-row slice the wave
// writes its 64 x 32 (column x row) f16 image -- lane (l32, hsel) packs the 4 consecutive rows of
// one column that accumulator registers 4j .. 4j+3 hold into ONE ds_write_b64 (pitch 72 B: the 16
// lanes of a write group on distinct banks) -- and reads it back row-contiguous with
// ds_read_b64_tr_b16 (T10: lane 4q+p of a 16-lane group addresses image row q = output column, 4
// output rows at 4p; lane i receives output row i, 4 columns), two reads per 16-byte store.  vs
// pp_epilogue: 8 instead of 32 LDS writes per slice and half the staged bytes (f16, not f32).
__device__ __forceinline__ half4_t ep_tr16(uint32_t addr) {
  half4_t r;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}
template <int TM, int TN, int EPI>
__device__ __forceinline__ void pp_epilogue_f16t(const float16_t (&acc)[TM][TN], const float (&csc)[TN],
                                                 const float (&cb)[TN], char* ep_bytes, void* Cout, int64_t ldc,
                                                 int M, int row_base, int col_base, int lane) {
  static_assert(TN == 2, "64-column wave tiles");
  static_assert(EPI == SAMQ_EPI_BIAS || EPI == SAMQ_EPI_BIAS_GELU, "f16 outputs");
  constexpr int PITCH = 72;                              // bytes per image row (32 f16 + 8 pad)
  const int l32 = lane & 31, hsel = lane >> 5;
  const uint32_t img = (uint32_t)(uintptr_t)((const SAMQ_LDS char*)ep_bytes);
  // tr-read addresses: group g (lanes 16g..16g+15), iteration k: pair pi = 4k + g = (16-row half
  // rb = pi & 1, 8-column chunk c8 = pi >> 1); lane 4q+p: image row 8 c8 + q (+4), rows 16 rb + 4p
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3, i16 = lane & 15;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float2_t v0 = __builtin_elementwise_fma((float2_t){acc[i][t][4 * j], acc[i][t][4 * j + 1]}, (float2_t)(csc[t]),
                                                (float2_t)(cb[t]));
        float2_t v1 = __builtin_elementwise_fma((float2_t){acc[i][t][4 * j + 2], acc[i][t][4 * j + 3]},
                                                (float2_t)(csc[t]), (float2_t)(cb[t]));
        if (EPI == SAMQ_EPI_BIAS_GELU) {
          v0 = gelu_fast2(v0);
          v1 = gelu_fast2(v1);
        }
        const half2_t h0 = __builtin_convertvector(v0, half2_t), h1 = __builtin_convertvector(v1, half2_t);
        *(half4_t*)(ep_bytes + (32 * t + l32) * PITCH + (8 * j + 4 * hsel) * 2) = half4_t{h0.x, h0.y, h1.x, h1.y};
      }
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slice image is in LDS
    const int srow0 = row_base + i * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int pi = 4 * k + g, rb = pi & 1, c8 = pi >> 1;
      const uint32_t a = img + (8 * c8 + q) * PITCH + (16 * rb + 4 * pp) * 2;
      half4_t lo = ep_tr16(a), hi = ep_tr16(a + 4 * PITCH);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo), "+v"(hi));
      const int row = srow0 + 16 * rb + i16;
      if (row < M)
        *(half8_t*)((_Float16*)Cout + (int64_t)row * ldc + col_base + 8 * c8) =
            half8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
  }
}

// Staged epilogue of TRANSPOSED 32x32 accumulators (PP_TE_STAGED), f16 outputs: lane (l32, hsel) of
// tile (i, t) holds row 32 i + l32, columns 32 t + 8 j + 4 hsel .. +3 in register group j, so four
// consecutive columns convert to one 8-byte f16 group -> ONE ds_write_b64 per 4 values (the
// row-pitch 144 B keeps the 16 rows of a write group on distinct banks), then row-contiguous
// ds_read_b128 + 16-byte global stores.  The whole WM x WN wave tile is staged at once in the LDS
// the ring frees (f16: 18 KiB per wave).  vs pp_epilogue: 4x fewer LDS write instructions and half
// the staged bytes (f16 instead of f32).
template <int TM, int TN, int EPI>
__device__ __forceinline__ void te_staged_epilogue_f16(const float16_t (&acc)[TM][TN], const _Float16* __restrict__ scales,
                                                       const _Float16* __restrict__ bias, char* ep, void* Cout,
                                                       int64_t ldc, int M, int row_base, int col_base, int lane) {
  static_assert(EPI == SAMQ_EPI_BIAS || EPI == SAMQ_EPI_BIAS_GELU, "f16 outputs");
  constexpr int WN = TN * 32, PITCH = WN * 2 + 16, C8 = WN / 8;
  const int l32 = lane & 31, hsel = lane >> 5;
#pragma unroll
  for (int t = 0; t < TN; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cl = 32 * t + 8 * j + 4 * hsel;
      const half4_t s4 = *(const half4_t*)(scales + col_base + cl);
      const half4_t b4 = bias ? *(const half4_t*)(bias + col_base + cl) : half4_t{0, 0, 0, 0};
      const float2_t sa = {(float)s4[0], (float)s4[1]}, sb = {(float)s4[2], (float)s4[3]};
      const float2_t ba = {(float)b4[0], (float)b4[1]}, bb = {(float)b4[2], (float)b4[3]};
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        float2_t v0 = __builtin_elementwise_fma((float2_t){acc[i][t][4 * j], acc[i][t][4 * j + 1]}, sa, ba);
        float2_t v1 = __builtin_elementwise_fma((float2_t){acc[i][t][4 * j + 2], acc[i][t][4 * j + 3]}, sb, bb);
        if (EPI == SAMQ_EPI_BIAS_GELU) {
          v0 = gelu_fast2(v0);
          v1 = gelu_fast2(v1);
        }
        const half2_t h0 = __builtin_convertvector(v0, half2_t), h1 = __builtin_convertvector(v1, half2_t);
        *(half4_t*)(ep + (32 * i + l32) * PITCH + cl * 2) = half4_t{h0.x, h0.y, h1.x, h1.y};
      }
    }
  __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the wave's own tile is in LDS
#pragma unroll
  for (int it = 0; it < TM * 32 * C8 / 64; ++it) {
    const int idx = it * 64 + lane;
    const int rl = idx / C8, c8 = idx % C8;
    const half8_t h = *(const half8_t*)(ep + rl * PITCH + c8 * 16);
    const int row = row_base + rl;
    if (row < M) *(half8_t*)((_Float16*)Cout + (int64_t)row * ldc + col_base + 8 * c8) = h;
  }
}

// ------------------------------------------------------------------ GEMM v6 (ping-pong, k-phases)
// As v5, but a phase is a K-PART of the tile over ALL of the wave's output tiles: phase p
// multiplies k16-steps [p*KPP, (p+1)*KPP) for TM x TN accumulators, so every phase reads its own
// A fragments (balanced LDS traffic, A registers for one k-part only) and unpacks its own slice
// of the packed B words (balanced VALU); the packed B words of the whole K tile are read in
// phase 0.  STAGES-slot ring: K tile kt+STAGES-1 is staged during tile kt (phases 1..NPH-1).

// Tile (mt, nt) of workgroup bid: XCD x owns the x-th contiguous eighth of the row-major tile
// order (xcd_remap), i.e. whole M-rows of tiles across ALL N tiles.
__device__ __forceinline__ void xcd_tile(int bid, int tiles_m, int tiles_n, int& mt, int& nt) {
  const int t = xcd_remap(bid, tiles_m * tiles_n);
  mt = t / tiles_n;
  nt = t % tiles_n;
}

// Tile geometry and LDS layout of a ping-pong config: the kernel and the launcher both read it
// from here.  A ring stage is the A tile (BM rows x 128 B), the NB packed B blocks (1 KiB each) and,
// for grouped weights whose group row rides in the ring (GROW), that row: BN fp16 scales (GLS
// lanes of 16 bytes) and BN / 8 packed zero words (GLZ lanes).  The epilogue reuses the ring's LDS:
// one f32 slice per wave, then the LayerNorm-fold consumer's (delta, rstd) table (RI_BYTES) and
// its workgroup's row partial sums (BM rows x K/64 float2) in what is left -- LNF_KMAX is the
// largest consumer K that fits (the launcher checks it).
template <int WAVES_M, int TM, int TN, int STAGES, int EPI, int VAR>
struct Pp2Lds {
  static constexpr int NW = 8, WM = TM * 32, WN = TN * 32, BM = WAVES_M * WM, BN = (NW / WAVES_M) * WN;
  static constexpr bool GR = (VAR & PP_GROUPED) != 0, M16 = (VAR & PP_MFMA16) != 0;
  static constexpr bool GRR = GR && (VAR & PP_GROUP_REGS) != 0;   // group rows in registers
  static constexpr bool GROW = GR && !GRR;                        // the group row rides in the ring
  static constexpr int GLS = BN * 2 / 16, GLZ = BN / 32;          // lanes carrying scales / zero words
  static constexpr int GRB = GROW ? (GLS + GLZ) * 16 : 0;
  static constexpr int A_BYTES = BM * 128, NB = BN / 32;
  static constexpr int STAGE = A_BYTES + NB * 1024 + GRB;
  static constexpr int EP_ROWS = WN > 64 ? 16 : 32;
  static constexpr int EP_BYTES = M16 ? 16 * (WN + 4) * 4 : EP_ROWS * WN * 4;
  static constexpr int RI_BYTES = lnf_consumer(EPI) ? BM * 8 : 0;
  static constexpr int SMEM = STAGES * STAGE > NW * EP_BYTES + RI_BYTES ? STAGES * STAGE : NW * EP_BYTES + RI_BYTES;
  static constexpr int LNF_KMAX = ((SMEM - NW * EP_BYTES - RI_BYTES) / (BM * 8)) * 64;
};

__host__ __device__ constexpr int pp2_pre(int p, int npw, int nph, int first) {   // pieces before phase p
  return p <= first ? 0 : (npw * (p - first)) / (nph - first);
}
template <int N>
__device__ __forceinline__ void vm_wait_le(int n) {   // s_waitcnt vmcnt(n) for a uniform n <= N
  if constexpr (N > 0) {
    if (n >= N) { vm_wait<N>(); return; }
    vm_wait_le<N - 1>(n);
  } else {
    vm_wait<0>();
  }
}

template <int WAVES_M, int TM, int TN, int NPH, int STAGES, int LA, int EPI, int VAR = 0>
__device__ __forceinline__
void pp2_tile(const _Float16* __restrict__ A, int64_t lda, const u32x4* __restrict__ Wp,
                    const _Float16* __restrict__ scales, const uint32_t* __restrict__ qzeros,
                    const _Float16* __restrict__ bias, void* __restrict__ Cout, int64_t ldc,
                    int M, int N, int K, int kpg, LnfArgs lnf, int bid) {
  using Lds = Pp2Lds<WAVES_M, TM, TN, STAGES, EPI, VAR>;
  constexpr int NW = Lds::NW, WAVES_N = NW / WAVES_M;
  constexpr int WM = Lds::WM, WN = Lds::WN, BM = Lds::BM, BN = Lds::BN;
  constexpr int BK = 64, ROWB = BK * 2;
  constexpr int A_BYTES = Lds::A_BYTES, NB = Lds::NB, STAGE = Lds::STAGE, SMEM = Lds::SMEM;
  constexpr int EP_ROWS = Lds::EP_ROWS, EP_BYTES = Lds::EP_BYTES, RI_BYTES = Lds::RI_BYTES;
  static_assert(A_BYTES == BM * ROWB, "A tile: 128-byte rows");
  // PP_GROUPED: grouped weights (groupsize = 64 kpg < K).  The K tile that starts a group carries
  // one more LDS-DMA piece, the group row of the whole tile: BN fp16 scales (lanes 0 .. BN/8-1) and
  // BN/8 packed zero words (the next BN/32 lanes; the rest idle), GRB bytes behind the B pieces.
  // Wave 0 issues it (compile-time slot NPW - 1, in the last phase); every wave reads its columns
  // of tile kt+1's row in the MFMA half of tile kt's last phase -- after the barrier that follows
  // every wave's retire wait for tile kt+1, wave 0's included -- and converts them in tile kt+1's
  // phase 0.  The unpack scales the exact integers once in fp16, fp16((q - zp) * s) (the v3
  // kernels' semantics); the epilogue's per-channel scale is 1.
  constexpr bool GR = Lds::GR;
  // PP_GROUP_REGS (with GR), register rows: each lane loads its own columns' group scale and zero
  // word straight into VGPRs (global loads in inline asm, so the compiler adds no wait of its own --
  // its waitcnt pass would wait vmcnt(0) on the loop-carried registers), issued in the
  // MFMA half of a group's first K tile for the NEXT group, before that phase's LDS-DMA pieces.
  // They count in the ring's vmcnt arithmetic (gl below) and a counted wait at the next group's
  // start retires them.  The ring then carries no group row: 4 slots / lookahead 3 like the
  // per-channel cfg 57, instead of 3 / 2 (4 x 40 KiB fill the 160 KiB LDS).
  constexpr bool GRR = Lds::GRR;
  constexpr bool GROW = Lds::GROW;                    // the group row rides in the ring
  constexpr int GLS = Lds::GLS, GLZ = Lds::GLZ;       // lanes carrying scales / zero words
  static_assert(!GR || GLS + GLZ <= 64, "group row: one lane per 16 bytes");
  // PP_MFMA16: v_mfma_f32_16x16x32_f16 fragments (same tile, LDS bytes and unpack count; the chip
  // holds a higher clock on this shape under load, MI355X_MICROARCH.md 'DVFS give-back' item 7)
  constexpr bool M16 = Lds::M16;
  constexpr int NA = BM / 8, NT = NA + NB + (GROW ? 1 : 0);
  constexpr int NGL = GRR ? 2 * TN * (M16 ? 2 : 1) : 0;   // GRR: loads per lane per group
  constexpr int NPW = (NT + NW - 1) / NW;
  constexpr int KPP = 4 / NPH;
  // K tile kt+LA is staged during tile kt (slot of tile kt+LA-STAGES, last read during tile kt-1
  // at the latest), its pieces issued behind the MFMA bursts: a wave's MFMA half of phase 0
  // starts after the barrier that ends every read of tile kt-1 (both groups' load halves of
  // tile kt-1's last phase lie before it, and their lgkmcnt waits precede their MFMAs), so all
  // phases may restage (WAR).  The retire wait for tile kt+1 sits in the load half of the last
  // phase, before the barrier after which the first group reads it (RAW).
  constexpr int PRE_LAST = pp2_pre(NPH - 1, NPW, NPH, 0);
  // PP_TE_STAGED: transposed accumulators + the LDS-staged f16 epilogue (te_staged_epilogue_f16)
  constexpr bool TES = (VAR & PP_TE_STAGED) != 0;
  static_assert(!TES || (!M16 && !GR && (EPI == SAMQ_EPI_BIAS || EPI == SAMQ_EPI_BIAS_GELU)), "TES: f16 outputs, 32x32");
  static_assert(!TES || 8 * TM * 32 * (TN * 64 + 16) <= 163840, "TES staging");
  // timing-only (tuning build, wrong results): no ring restaging / no MFMA / no epilogue
  constexpr bool T_NO_RESTAGE = (VAR & PP_T_NO_RESTAGE) != 0, T_NO_MFMA = (VAR & PP_T_NO_MFMA) != 0;
  constexpr bool T_NO_EPILOGUE = (VAR & PP_T_NO_EPILOGUE) != 0;
  // PP_DMA_SPREAD: LDS-DMA pieces spread through the MFMA burst (see the MFMA half)
  constexpr bool DMA_SPREAD = (VAR & PP_DMA_SPREAD) != 0;
  static_assert(!DMA_SPREAD || !(TES || T_NO_MFMA), "DMA spread: product MFMA halves only");
  constexpr int KS32 = 2 / NPH;                  // M16: k32 steps per phase
  static_assert(!M16 || NPH <= 2, "M16: one or two phases per K tile");
  static_assert(NPH >= 1 && 4 % NPH == 0, "phases");
  static_assert(LA >= 2 && LA < STAGES, "ring");
  static_assert((LA - 2) * (NPW + NGL) + PRE_LAST + NGL <= 63, "vmcnt");
  static_assert(!GRR || 3 * NPW <= 63, "vmcnt (group start)");
  static_assert(SMEM <= 160 * 1024, "LDS");

  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // PP_WAVE_SGPR (and GR): the wave index -- hence piece choices and addresses -- in an SGPR
  constexpr bool RFL = GR || (VAR & PP_WAVE_SGPR) != 0;
  const int wave = RFL ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int grp = wave >> 2;
  const int tiles_n = N / BN;
  const int tiles_m = (M + BM - 1) / BM;
  int m0, n0;
  xcd_tile(bid, tiles_m, tiles_n, m0, n0);
  m0 *= BM;
  n0 *= BN;
  const int kt_count = K / BK;

  const char* src[NPW];
  int dst[NPW];
  int step[NPW];
  // GR: pieces dealt j = i * 8 + wave (interleaved) instead of wave * NPW + i; the A / B pieces
  // fill slots i < NPW - 1; slot NPW - 1 of wave 0 is the group row
  static_assert(!GROW || ((NA + NB) % NW == 0 && NPW == (NA + NB) / NW + 1), "group row slot");
  static_assert(!GROW || pp2_pre(NPH - 1, NPW, NPH, 0) <= NPW - 1, "group row issued in the last phase");
#pragma unroll
  for (int i = 0; i < NPW; ++i) {
    int j = GR ? i * NW + wave : wave * NPW + i;
    j = j < NT ? j : NT - 1;
    if (GROW && i == NPW - 1) {
      if (lane < GLS) {
        src[i] = (const char*)(scales + n0 + 8 * lane);
        step[i] = N * 2;
      } else {
        const int l = lane - GLS < GLZ ? lane - GLS : 0;
        src[i] = (const char*)(qzeros + n0 / 8 + 4 * l);
        step[i] = (N / 8) * 4;
      }
      dst[i] = A_BYTES + NB * 1024;
    } else if (j < NA) {
      const int row = j * 8 + (lane >> 3);
      const int c = (lane & 7) ^ ((row >> 1) & 7);
      int gr = m0 + row;
      gr = gr < M ? gr : M - 1;
      src[i] = (const char*)(A + (int64_t)gr * lda + c * 8);
      dst[i] = j * 1024;
      step[i] = BK * 2;
    } else {
      const int nt = n0 / 32 + (j - NA);
      src[i] = (const char*)(Wp + ((int64_t)nt * kt_count) * 64 + lane);
      dst[i] = A_BYTES + (j - NA) * 1024;
      step[i] = 64 * 16;
    }
  }
  auto issue = [&](int kt, int slot, int i0, int i1) {
#pragma unroll
    for (int i = 0; i < NPW; ++i)
      if (i >= i0 && i < i1) {
        if (GROW && i == NPW - 1) {
          // wave 0, and only for a K tile that starts a group (uniform: wave is an SGPR)
          if (wave == 0 && kt % kpg == 0) {
            if (lane < GLS + GLZ)
              __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)(src[i] + (int64_t)(kt / kpg) * step[i]),
                                               (SAMQ_LDS void*)(smem + slot * STAGE + dst[i]), 16, 0, 0);
          }
        } else {
          __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)(src[i] + (int64_t)kt * step[i]),
                                           (SAMQ_LDS void*)(smem + slot * STAGE + dst[i]), 16, 0, 0);
        }
      }
  };
  // GR: the raw group row values of this lane's columns (read after the retire wait of their tile)
  // and the fp16 scale splats (set from them where a group starts)
  half2_t gsc[TN], gsc16[TN][2];
  uint32_t graw_s[TN][2] = {}, graw_z[TN][2] = {};
  auto gread = [&](int slot_) {
    const char* gp = smem + slot_ * STAGE + A_BYTES + NB * 1024;
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int h = 0; h < (M16 ? 2 : 1); ++h) {
        const int cl = wn * WN + (M16 ? 32 * t + 16 * h + (lane & 15) : 32 * t + (lane & 31));
        graw_s[t][h] = *(const uint16_t*)(gp + 2 * cl);
        graw_z[t][h] = *(const uint32_t*)(gp + BN * 2 + 4 * (cl >> 3)) >> (4 * (cl & 7));
      }
  };
  // GR: LDS-DMA pieces this wave issues for K tile t (wave 0 adds the group row where a group starts)
  auto npieces = [&](int t) -> int { return GROW ? NPW - 1 + (wave == 0 && t % kpg == 0 ? 1 : 0) : NPW; };
  // GRR: the register-row loads of a group are issued in the MFMA half of the previous group's first
  // tile t0, right before K tile t0 + LA's pieces; gl(kt + j) = such loads precede tile kt + j's
  // pieces (t0 = kt + j - LA starts a group and a group follows it).  t0 % kpg from the position
  // gk of tile kt in its group: (gk + j - LA) mod kpg, at most LA - 2 additions of kpg -- not a
  // loop over t0 (that SALU chain sat in every last-phase load half: lin2, 80 K tiles, +38 %)
  auto gl = [&](int kt_, int j, int gk_) -> bool {
    if (!GRR) return false;
    const int t0 = kt_ + j - LA;
    if (t0 < 0 || t0 + kpg >= kt_count) return false;
    int r = gk_ + j - LA;
    while (r < 0) r += kpg;
    return r == 0;
  };
  auto gload = [&](int gi) {   // GRR: this lane's columns of group gi into graw_s / graw_z (no wait)
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int h = 0; h < (M16 ? 2 : 1); ++h) {
        const int c = n0 + wn * WN + (M16 ? 32 * t + 16 * h + (lane & 15) : 32 * t + (lane & 31));
        const _Float16* sp = scales + (int64_t)gi * N + c;
        const uint32_t* zp = qzeros + (int64_t)gi * (N / 8) + (c >> 3);
        asm volatile("global_load_ushort %0, %1, off" : "+v"(graw_s[t][h]) : "v"(sp));
        asm volatile("global_load_dword %0, %1, off" : "+v"(graw_z[t][h]) : "v"(zp));
      }
  };

  int col[TN];
  W4Zero zc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    col[t] = n0 + wn * WN + t * 32 + (lane & 31);
    const uint32_t zw = qzeros[col[t] >> 3];
    zc[t].set((int)((zw >> (4 * (col[t] & 7))) & 0xFu) + 1);
  }
  W4Unpack ku;
  ku.init();

  float16_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int hsel = lane >> 5;
  int a_off[TM], a_swz[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int rr = wm * WM + i * 32 + (lane & 31);
    a_off[i] = rr * ROWB;
    a_swz[i] = (rr >> 1) & 7;
  }

  // M16 state: 16-row tiles i, column halves h of each 32-column block t; lane (ql, g16) holds
  // column 32t + 16h + ql and k = 32 s + 8 g16 .. +7, whose packed word (layout 1: column c,
  // k chunk kb at word kb / 2 of lane c + 32 (kb & 1)) is word 2 s + (g16 >> 1) of lane
  // 16h + ql + 32 (g16 & 1) in the staged B block
  const int ql = lane & 15, g16 = lane >> 4;
  float4_t acc16[M16 ? 2 * TM : 1][TN][2];
  W4Zero zc16[TN][2];
  int a_off16[M16 ? 2 * TM : 1], a_swz16[M16 ? 2 * TM : 1];
  if constexpr (M16) {
#pragma unroll
    for (int i = 0; i < 2 * TM; ++i) {
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) acc16[i][t][h] = float4_t{0.f, 0.f, 0.f, 0.f};
      const int rr = wm * WM + i * 16 + ql;
      a_off16[i] = rr * ROWB;
      a_swz16[i] = (rr >> 1) & 7;
    }
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = n0 + wn * WN + 32 * t + 16 * h + ql;
        zc16[t][h].set((int)((qzeros[c >> 3] >> (4 * (c & 7))) & 0xFu) + 1);
      }
  }

  // PP_EARLY_EP: the epilogue's per-channel scale / bias of this lane's columns loaded before
  // the prologue's LDS-DMA pieces (the prologue's retire wait covers them) and kept in VGPRs over
  // the main loop, instead of loaded after it, where their latency sits behind the epilogue barrier
  constexpr bool EARLY_EP = (VAR & PP_EARLY_EP) != 0;
  static_assert(!EARLY_EP || !(GR || TES || lnf_consumer(EPI) || lnf_producer(EPI)), "early epilogue operands");
  constexpr int NEC = EARLY_EP ? (M16 ? 2 * TN : TN) : 1;
  _Float16 esc[NEC], ebi[NEC];
  if constexpr (EARLY_EP) {
#pragma unroll
    for (int e = 0; e < NEC; ++e) {
      const int c = M16 ? n0 + wn * WN + 32 * (e >> 1) + 16 * (e & 1) + (lane & 15) : col[e];
      esc[e] = scales[c];
      ebi[e] = bias ? bias[c] : (_Float16)0.0f;
    }
  }
  // ---- prologue: K tiles 0 .. LA-1 in flight, tile 0 retired + visible; group 1 lags a barrier
  const int pro = kt_count < LA ? kt_count : LA;
  if (GRR) gload(0);   // older than every piece: the prologue's retire wait for tile 0 covers it
#pragma unroll
  for (int j = 0; j < LA; ++j)
    if (j < pro) issue(j, j, 0, NPW);
  {
    int newer = 0;
#pragma unroll
    for (int j = 1; j < LA; ++j) newer += j < pro ? npieces(j) : 0;
    vm_wait_le<(LA - 1) * NPW>(newer);
  }
  __builtin_amdgcn_s_barrier();
  if (GROW) gread(0);   // tile 0's row: wave 0's retire wait precedes the barrier above
  if (grp) __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  int slot = 0;
  int gk = 0;   // GR: K tiles since the current group's first
  int gidx = 0; // GR: the current group
  for (int kt = 0; kt < kt_count; ++kt) {
    const char* st = smem + slot * STAGE;
    const int ahead = kt + LA;
    const bool pf = ahead < kt_count && !T_NO_RESTAGE;
    const int sa = slot + LA >= STAGES ? slot + LA - STAGES : slot + LA;   // (kt + LA) % STAGES
    u32x4 bw[TN];
    uint32_t bw16[TN][2][2];
    static_for<NPH>([&](auto pc_) {   // phases: p a constant (folds the DMA piece schedule)
      constexpr int p = decltype(pc_)::value;
      // ---------------- load half
      if (p == NPH - 1 && kt + 1 < kt_count) {
        // K tile kt+1 retired: newer = whole tiles kt+2 .. kt+LA-1 + this tile's pieces so far.
        // Per-channel steady state (every later tile whole, restaging on): a compile-time count --
        // the runtime form is a ~40-SALU / 15-branch decision tree on the load half's stream
        if (!GR && pf && kt + LA < kt_count) {
          vm_wait<(LA - 2) * NPW + PRE_LAST>();
        } else if (GRR && LA == 3 && NPH > 1 && kpg == 2 && pf && kt + LA < kt_count) {
          // GRR, two K tiles per group (G = 128): of the two tiles kt - 1, kt exactly one starts a
          // group, so one set of register-row loads is newer -- a constant count, no decision tree
          vm_wait<(LA - 2) * NPW + PRE_LAST + NGL>();
        } else {
          int newer = pf ? PRE_LAST : 0;
          if (NPH > 1 && GRR && gk == 0 && kt + kpg < kt_count) newer += NGL;   // gl(ahead)   // this tile's register-row loads (phase 0)
#pragma unroll
          for (int j = 2; j < LA; ++j) newer += (kt + j < kt_count ? npieces(kt + j) : 0) + (gl(kt, j, gk) ? NGL : 0);
          vm_wait_le<(LA - 2) * (NPW + NGL) + PRE_LAST + NGL>(newer);
        }
      }
      if (GR && p == 0 && gk == 0) {   // first K tile of a group: its scale / zero splats
        if constexpr (GRR) {
          // the group's loads were issued kpg tiles ago, before the pieces of tiles kt - kpg + LA ..
          // kt + LA - 1 (those that exist); everything older has retired once at most that many
          // remain.  (kt == 0: the prologue's wait covered them.)  The empty asm re-defines the
          // registers after the wait, so nothing reading them is scheduled above it.
          if (kt > 0) {
            int left = kt_count - (kt - kpg + LA);
            left = T_NO_RESTAGE || left < 0 ? 0 : left > kpg ? kpg : left;
            if (kpg == 2 && left == 2)
              vm_wait<2 * NPW>();
            else
              vm_wait_le<3 * NPW>(left * NPW);
          }
#pragma unroll
          for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int h = 0; h < (M16 ? 2 : 1); ++h) {
              asm volatile("" : "+v"(graw_s[t][h]), "+v"(graw_z[t][h]));
              graw_s[t][h] &= 0xFFFFu;
              graw_z[t][h] >>= 4 * ((n0 + wn * WN + (M16 ? 32 * t + 16 * h + (lane & 15) : 32 * t + (lane & 31))) & 7);
            }
        }
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
          for (int h = 0; h < (M16 ? 2 : 1); ++h) {
            // fp16 bits: 1024 + zp = 0x6400 + zp, 64 + zp = 0x5400 + 16 zp (exact), splatted
            const uint32_t zp = (graw_z[t][h] & 0xFu) + 1u;
            W4Zero z;
            z.z1024 = __builtin_bit_cast(half2_t, (0x6400u + zp) * 0x10001u);
            z.z64 = __builtin_bit_cast(half2_t, (0x5400u + 16u * zp) * 0x10001u);
            const half2_t sc2 = __builtin_bit_cast(half2_t, graw_s[t][h] * 0x10001u);
            if constexpr (M16) { zc16[t][h] = z; gsc16[t][h] = sc2; } else { zc[t] = z; gsc[t] = sc2; }
          }
      }
      if (M16 && p == 0) {
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const char* bp = st + A_BYTES + (wn * TN + t) * 1024 + (16 * h + ql + 32 * (g16 & 1)) * 16 + 4 * (g16 >> 1);
            bw16[t][h][0] = *(const uint32_t*)bp;         // k32 step 0
            bw16[t][h][1] = *(const uint32_t*)(bp + 8);   // k32 step 1
          }
      } else if (p == 0) {
#pragma unroll
        for (int t = 0; t < TN; ++t) bw[t] = *(const u32x4*)(st + A_BYTES + (wn * TN + t) * 1024 + lane * 16);
      }
      half8_t af16[M16 ? 2 * TM : 1][KS32], bf16[TN][2][KS32];
      if constexpr (M16) {
#pragma unroll
        for (int s = 0; s < KS32; ++s) {
          const int k32 = p * KS32 + s;
#pragma unroll
          for (int i = 0; i < 2 * TM; ++i)
            af16[i][s] = *(const half8_t*)(st + a_off16[i] + (((4 * k32 + g16) ^ a_swz16[i]) << 4));
#pragma unroll
          for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              bf16[t][h][s] = w4_unpack(bw16[t][h][k32], ku, zc16[t][h]);
              if (GR) bf16[t][h][s] = scale8(bf16[t][h][s], gsc16[t][h]);
            }
        }
      }
      half8_t af[TM][KPP];
      half8_t bf[TN][KPP];
      if constexpr (!M16) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int s = 0; s < KPP; ++s)
            af[i][s] = *(const half8_t*)(st + a_off[i] + (((2 * (p * KPP + s) + hsel) ^ a_swz[i]) << 4));
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
          for (int s = 0; s < KPP; ++s) {
            bf[t][s] = w4_unpack(bw[t][p * KPP + s], ku, zc[t]);
            if (GR) bf[t][s] = scale8(bf[t][s], gsc[t]);
          }
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // ---------------- MFMA half
      __builtin_amdgcn_s_setprio(1);
      if constexpr (DMA_SPREAD) {
        // the phase's LDS-DMA pieces spread through the MFMA burst (one after every NMF / np
        // MFMAs) instead of after it: issued after the last MFMA they queue behind the other
        // MFMA-half waves' pieces in the TA while the MFMA pipe drains, and the partner group
        // waits at the barrier for that tail (per-segment stamps: MFMA half ~690 cycles for 512)
        constexpr int P0 = pp2_pre(p, NPW, NPH, 0), NP = pp2_pre(p + 1, NPW, NPH, 0) - P0;
        constexpr int NMF = M16 ? KS32 * 2 * TM * TN * 2 : KPP * TM * TN;
        static_for<NMF>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          if constexpr (M16) {
            constexpr int s = q / (2 * TM * TN * 2), i = (q / (TN * 2)) % (2 * TM), t = (q / 2) % TN, h = q % 2;
            acc16[i][t][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af16[i][s], bf16[t][h][s], acc16[i][t][h], 0, 0, 0);
          } else {
            constexpr int s = q / (TM * TN), i = (q / TN) % TM, t = q % TN;
            acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][s], bf[t][s], acc[i][t], 0, 0, 0);
          }
          static_for<NPW>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if constexpr (k < NP && q + 1 == ((2 * k + 1) * NMF) / (2 * NP)) {
              __builtin_amdgcn_sched_barrier(0);
              if (pf) issue(ahead, sa, P0 + k, P0 + k + 1);
              __builtin_amdgcn_sched_barrier(0);
            }
          });
        });
      } else if constexpr (M16) {
#pragma unroll
        for (int s = 0; s < KS32; ++s)
#pragma unroll
          for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
            for (int t = 0; t < TN; ++t)
#pragma unroll
              for (int h = 0; h < 2; ++h)
                acc16[i][t][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af16[i][s], bf16[t][h][s], acc16[i][t][h], 0, 0, 0);
      } else {
#pragma unroll
        for (int s = 0; s < KPP; ++s)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int t = 0; t < TN; ++t) {
              if (T_NO_MFMA) {
                acc[i][t][0] += (float)af[i][s][0] * (float)bf[t][s][1];
              } else {   // TES: W^T . A^T, so a lane's accumulator registers run along N
                acc[i][t] = TES ? __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[t][s], af[i][s], acc[i][t], 0, 0, 0)
                                : __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][s], bf[t][s], acc[i][t], 0, 0, 0);
              }
            }
      }
      // the next-next tile's LDS-DMA pieces behind this MFMA burst (the wave would only wait at
      // the barrier otherwise; WAR-safe in every phase: see header)
      // GRR: the next group's register rows, older than tile ahead's pieces (gl(ahead))
      if (GRR && p == 0 && gk == 0 && kt + kpg < kt_count) gload(gidx + 1);   // == gl(ahead)
      if (pf && !DMA_SPREAD) issue(ahead, sa, pp2_pre(p, NPW, NPH, 0), pp2_pre(p + 1, NPW, NPH, 0));
      // GR: tile kt+1 starts a group -> its row into registers (every wave's retire wait for tile
      // kt+1, wave 0's included, precedes the barrier that opened this MFMA half)
      if (GROW && p == NPH - 1 && kt + 1 < kt_count && gk + 1 == kpg)
        gread(slot + 1 == STAGES ? 0 : slot + 1);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    });
    slot = slot == STAGES - 1 ? 0 : slot + 1;
    if (GR) {
      gidx += gk + 1 == kpg ? 1 : 0;
      gk = gk + 1 == kpg ? 0 : gk + 1;
    }
  }
  if (!grp) __builtin_amdgcn_s_barrier();   // balance group 1's extra barrier

  if constexpr (T_NO_EPILOGUE) {   // keeps the sums alive
    float z = 0.f;
    if constexpr (M16) {
#pragma unroll
      for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
        for (int t = 0; t < TN; ++t) z += acc16[i][t][0][0] + acc16[i][t][1][3];
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int t = 0; t < TN; ++t) z += acc[i][t][0] + acc[i][t][15];
    }
    if (z == 1234.5f) ((float*)Cout)[tid] = z;
    return;
  }
  if constexpr (TES) {
    constexpr int WB = TM * 32 * (TN * 64 + 16);
    __syncthreads();   // every wave is done with the ring
    te_staged_epilogue_f16<TM, TN, EPI>(acc, scales, bias, smem + wave * WB, Cout, ldc, M, m0 + wm * WM, n0 + wn * WN,
                                        lane);
    return;
  }
  // fp32 residual (SAMQ_EPI_RESADD_F32): the old values are read a batch of slices ahead of the
  // stores (res_load, common.h), the first batch here -- behind the scale / bias loads, which
  // return first, and before the barrier, so it is in flight over both.
  constexpr bool RES = EPI == SAMQ_EPI_RESADD_F32;
  constexpr int RES_R = M16 ? 16 : EP_ROWS, RES_NB = M16 ? RES_NB16 : 1;
  constexpr int RES_J = res_j(RES_R, WN), RES_NX = RES ? RES_NB * RES_J : 1;
  float4_t xpre[RES_NX];
  auto res_first = [&]() {
    if constexpr (RES) {
#pragma unroll
      for (int b = 0; b < RES_NB; ++b)
        res_load<RES_R, WN>(xpre + b * RES_J, Cout, ldc, M, m0 + wm * WM + b * RES_R, n0 + wn * WN, lane);
    }
  };
  if constexpr (M16) {
    float csc16[TN][2], cb16[TN][2];
    if constexpr (EARLY_EP || GR) {
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int c = n0 + wn * WN + 32 * t + 16 * h + ql;
          csc16[t][h] = EARLY_EP ? (float)esc[EARLY_EP ? 2 * t + h : 0] : GR ? 1.0f : (float)scales[c];
          cb16[t][h] = EARLY_EP ? (float)ebi[EARLY_EP ? 2 * t + h : 0] : bias ? (float)bias[c] : 0.0f;
        }
      res_first();
    } else {
      // this lane's scales and biases as one batch of raw loads behind a single wait (bias null: 0)
      const HOpt bo(bias, scales);
      _Float16 rs[TN][2];
      uint32_t rb[TN][2];
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int c = n0 + wn * WN + 32 * t + 16 * h + ql;
          rs[t][h] = scales[c];
          rb[t][h] = bo.raw(c);
        }
      res_first();
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          csc16[t][h] = (float)rs[t][h];
          cb16[t][h] = bo.f32(rb[t][h]);
        }
    }
    __syncthreads();
    float2_t* rowinfo = (float2_t*)(smem + NW * EP_BYTES) + wm * WM;
    lnf.bias = bias;
    if constexpr (lnf_consumer(EPI))
      lnf_rowinfo_wg<BM, NW>(lnf, (float2_t*)(smem + NW * EP_BYTES), smem + NW * EP_BYTES + RI_BYTES, M, m0, n0 == 0,
                             wave, lane);
    pp_epilogue16<2 * TM, TN, EPI>(acc16, csc16, cb16, smem + wave * EP_BYTES, Cout, ldc, M, m0 + wm * WM,
                                   n0 + wn * WN, lane, lnf, N, rowinfo, xpre);
    return;
  }
  float csc[TN], cb[TN];
  if constexpr (EARLY_EP || GR) {
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      csc[t] = EARLY_EP ? (float)esc[EARLY_EP ? t : 0] : GR ? 1.0f : (float)scales[col[t]];
      cb[t] = EARLY_EP ? (float)ebi[EARLY_EP ? t : 0] : bias ? (float)bias[col[t]] : 0.0f;
    }
    res_first();
  } else {
    const HOpt bo(bias, scales);
    _Float16 rs[TN];           // one batch of raw loads behind a single wait (bias null: 0)
    uint32_t rb[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      rs[t] = scales[col[t]];
      rb[t] = bo.raw(col[t]);
    }
    res_first();
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      csc[t] = (float)rs[t];
      cb[t] = bo.f32(rb[t]);
    }
  }
  __syncthreads();
  float2_t* rowinfo = (float2_t*)(smem + NW * EP_BYTES) + wm * WM;
  lnf.bias = bias;
  if constexpr (lnf_consumer(EPI))
    lnf_rowinfo_wg<BM, NW>(lnf, (float2_t*)(smem + NW * EP_BYTES), smem + NW * EP_BYTES + RI_BYTES, M, m0, n0 == 0,
                           wave, lane);
  if constexpr ((VAR & PP_F16T) != 0) {
    static_assert(EPI == SAMQ_EPI_BIAS || EPI == SAMQ_EPI_BIAS_GELU, "transposed f16 staging: f16 outputs");
    static_assert(EP_BYTES >= 64 * 72, "transposed f16 staging image");
    pp_epilogue_f16t<TM, TN, EPI>(acc, csc, cb, smem + wave * EP_BYTES, Cout, ldc, M, m0 + wm * WM, n0 + wn * WN, lane);
    return;
  }
  pp_epilogue<TM, TN, EP_ROWS, EPI>(acc, csc, cb, smem + wave * EP_BYTES, Cout, ldc, M, m0 + wm * WM, n0 + wn * WN,
                                    lane, lnf, N, rowinfo, xpre);
}

// The ping-pong GEMM kernel: one tile per workgroup, or (PP_PERSISTENT) a grid of at
// most one workgroup per CU looping over the tiles t = blockIdx.x, + gridDim.x, ... -- the tile's
// epilogue stores drain while the next tile's prologue DMA and first K tiles run (a one-tile
// workgroup holds its CU until its stores are acknowledged).  gridDim.x % 8 == 0 keeps every tile
// on the XCD its one-tile launch would give it (xcd_remap's t % 8 map).
template <int WAVES_M, int TM, int TN, int NPH, int STAGES, int LA, int EPI, int VAR = 0>
__global__ __launch_bounds__(512, 1)
void w4a16_gemm_pp2(const _Float16* __restrict__ A, int64_t lda, const u32x4* __restrict__ Wp,
                    const _Float16* __restrict__ scales, const uint32_t* __restrict__ qzeros,
                    const _Float16* __restrict__ bias, void* __restrict__ Cout, int64_t ldc,
                    int M, int N, int K, int kpg, LnfArgs lnf) {
  if constexpr ((VAR & PP_PERSISTENT) != 0) {
    using Lds = Pp2Lds<WAVES_M, TM, TN, STAGES, EPI, VAR>;
    constexpr int BM = Lds::BM, BN = Lds::BN;
    const int ntiles = ((M + BM - 1) / BM) * (N / BN);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
      pp2_tile<WAVES_M, TM, TN, NPH, STAGES, LA, EPI, VAR>(A, lda, Wp, scales, qzeros, bias, Cout, ldc, M, N, K, kpg,
                                                           lnf, t);
      __syncthreads();   // the epilogue's LDS reads before the next tile's ring DMA
    }
  } else {
    pp2_tile<WAVES_M, TM, TN, NPH, STAGES, LA, EPI, VAR>(A, lda, Wp, scales, qzeros, bias, Cout, ldc, M, N, K, kpg, lnf,
                                                         blockIdx.x);
  }
}

}  // namespace samq
