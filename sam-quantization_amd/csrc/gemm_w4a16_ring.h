// W4A16 GEMM kernels v1 (register-staged B, double-buffered A) and v3 (3-stage LDS-DMA ring).
// Included by gemm_w4a16.hip only.
#pragma once

#include "gemm_w4a16_util.h"

namespace samq {

// ------------------------------------------------------------------ GEMM v1
template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI, bool GROUPED>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N)
void w4a16_gemm_kernel(const _Float16* __restrict__ A, int64_t lda,
                       const u32x4* __restrict__ Wp,
                       const _Float16* __restrict__ scales,
                       const uint32_t* __restrict__ qzeros,
                       const _Float16* __restrict__ bias,
                       void* __restrict__ Cout, int64_t ldc,
                       int M, int N, int K, int groupsize) {
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int WM = BM / WAVES_M;
  constexpr int WN = BN / WAVES_N;
  constexpr int TM = WM / 32;
  constexpr int TN = WN / 32;
  constexpr int BK = 64;
  constexpr int ROWB = BK * 2;                 // 128 bytes per A row in LDS
  constexpr int TILE_BYTES = BM * ROWB;
  constexpr int GLDS_PER_WAVE = BM / 8 / NW;   // 1 KiB (8 rows) per wave-instruction
  static_assert(TM >= 1 && TN >= 1 && GLDS_PER_WAVE >= 1, "bad tile");

  __shared__ __attribute__((aligned(16))) char smem[2 * TILE_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;

  const int tiles_n = N / BN;
  const int tiles_m = (M + BM - 1) / BM;
  const int nwg = tiles_m * tiles_n;
  const int bid = xcd_remap(blockIdx.x, nwg);
  const int tm = bid / tiles_n;
  const int tn = bid % tiles_n;
  const int m0 = tm * BM;
  const int n0 = tn * BN;
  const int kt_count = K / BK;

  // ---- A staging: this wave's global_load_lds sources (row clamp at M-1)
  const _Float16* a_src[GLDS_PER_WAVE];
  int a_dst[GLDS_PER_WAVE];
#pragma unroll
  for (int i = 0; i < GLDS_PER_WAVE; ++i) {
    const int r0 = (wave * GLDS_PER_WAVE + i) * 8;
    const int row = r0 + (lane >> 3);
    const int p = lane & 7;
    const int c = p ^ ((row >> 1) & 7);
    int gr = m0 + row;
    gr = gr < M ? gr : M - 1;
    a_src[i] = A + (int64_t)gr * lda + c * 8;
    a_dst[i] = r0 * ROWB;
  }
  auto stage_a = [&](int kt, int buf) {
#pragma unroll
    for (int i = 0; i < GLDS_PER_WAVE; ++i) {
      __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)(a_src[i] + kt * BK),
                                       (SAMQ_LDS void*)(smem + buf * TILE_BYTES + a_dst[i]), 16, 0, 0);
    }
  };

  // ---- B fragments (packed): per n-tile one dwordx4 per lane per K tile
  const int ncol_tile0 = (n0 + wn * WN) / 32;
  const u32x4* b_ptr[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) b_ptr[t] = Wp + ((int64_t)(ncol_tile0 + t) * kt_count) * 64 + lane;

  // per-lane output column of each n-tile
  int col[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) col[t] = n0 + wn * WN + t * 32 + (lane & 31);

  auto load_zc = [&](int g, half2_t* zc, half2_t* sc) {
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const uint32_t zw = qzeros[(int64_t)g * (N / 8) + (col[t] >> 3)];
      const int zp = (int)((zw >> (4 * (col[t] & 7))) & 0xFu) + 1;
      const _Float16 z = (_Float16)(1024 + zp);
      zc[t] = half2_t{z, z};
      if (GROUPED) {
        const _Float16 s = scales[(int64_t)g * N + col[t]];
        sc[t] = half2_t{s, s};
      }
    }
  };

  half2_t zc[TN], sc[TN];
  load_zc(0, zc, sc);
  int cur_group = 0;

  float16_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // LDS read offsets for the A fragments of this wave (row part), k-chunk added per step
  int a_row[TM];
  int a_swz[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int rr = wm * WM + i * 32 + (lane & 31);
    a_row[i] = rr * ROWB;
    a_swz[i] = (rr >> 1) & 7;
  }
  const int hsel = lane >> 5;

  // unpack constants held in VGPRs (opaque to the compiler) so (x & M) | MAGIC fuses into one
  // v_and_or_b32 (gfx950 VOP3 takes no literal operands)
  uint32_t kMask = 0x000F000Fu, kMagic = 0x64006400u;
  asm volatile("" : "+v"(kMask), "+v"(kMagic));

  // prologue
  stage_a(0, 0);
  u32x4 bcur[TN], bnext[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) bcur[t] = b_ptr[t][0];
  __syncthreads();

  for (int kt = 0; kt < kt_count; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < kt_count) {
      stage_a(kt + 1, buf ^ 1);
#pragma unroll
      for (int t = 0; t < TN; ++t) bnext[t] = b_ptr[t][(int64_t)(kt + 1) * 64];
    }
    if (GROUPED) {
      const int g = (kt * BK) / groupsize;
      if (g != cur_group) {
        load_zc(g, zc, sc);
        cur_group = g;
      }
    }
    const char* abase = smem + buf * TILE_BYTES;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      half8_t af[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int c = 2 * s + hsel;
        af[i] = *(const half8_t*)(abase + a_row[i] + ((c ^ a_swz[i]) << 4));
      }
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const uint32_t w = bcur[t][s];
        half8_t bf;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t bits = ((w >> (4 * i)) & kMask) | kMagic;
          half2_t h = __builtin_bit_cast(half2_t, bits) - zc[t];
          if (GROUPED) h = h * sc[t];
          bf[2 * i] = h[0];
          bf[2 * i + 1] = h[1];
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
          acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf, acc[i][t], 0, 0, 0);
      }
    }
    __syncthreads();
    if (kt + 1 < kt_count) {
#pragma unroll
      for (int t = 0; t < TN; ++t) bcur[t] = bnext[t];
    }
  }

  // ---- epilogue
  float csc[TN], cb[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    csc[t] = GROUPED ? 1.0f : (float)scales[col[t]];
    cb[t] = bias ? (float)bias[col[t]] : 0.0f;
  }
  // fp32 residual: the old values of a 32-row tile are all read before its first store (rows past
  // M clamped: read, never stored; common.h res_load)
  constexpr bool RES = EPI == SAMQ_EPI_RESADD_F32;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    float xo[RES ? 16 : 1][TN];
    if constexpr (RES) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int row = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
        row = row < M ? row : M - 1;
#pragma unroll
        for (int t = 0; t < TN; ++t) xo[r][t] = ((const float*)Cout)[(int64_t)row * ldc + col[t]];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
      if (row >= M) continue;
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        float v = acc[i][t][r] * csc[t] + cb[t];
        if (EPI == SAMQ_EPI_BIAS_GELU) v = gelu_erf(v);
        if (EPI == SAMQ_EPI_RESADD_F32) {
          float* cp = (float*)Cout + (int64_t)row * ldc + col[t];
          *cp = xo[RES ? r : 0][t] + v;
        } else if (EPI == SAMQ_EPI_F32) {
          ((float*)Cout)[(int64_t)row * ldc + col[t]] = v;
        } else {
          ((_Float16*)Cout)[(int64_t)row * ldc + col[t]] = (_Float16)v;
        }
      }
    }
  }
}

// ------------------------------------------------------------------ GEMM v3 (3-stage LDS-DMA ring)
// Both operands reach LDS by global_load_lds: A (BM rows x 128 B, XOR-swizzled through the
// source address) and B (BN/32 packed 1-KiB fragment blocks, already in lane order); a 3-slot
// ring keeps two K tiles in flight behind counted vmcnt waits and ONE raw s_barrier per K tile
// (no vmcnt(0) drain in the loop).  Fragment reads: A ds_read_b128 (conflict-free swizzle),
// B ds_read_b128 lane-linear.
template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI, bool GROUPED>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N)
void w4a16_gemm_v3(const _Float16* __restrict__ A, int64_t lda, const u32x4* __restrict__ Wp,
                   const _Float16* __restrict__ scales, const uint32_t* __restrict__ qzeros,
                   const _Float16* __restrict__ bias, void* __restrict__ Cout, int64_t ldc,
                   int M, int N, int K, int groupsize) {
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int WM = BM / WAVES_M;
  constexpr int WN = BN / WAVES_N;
  constexpr int TM = WM / 32;
  constexpr int TN = WN / 32;
  constexpr int BK = 64;
  constexpr int ROWB = BK * 2;
  constexpr int A_BYTES = BM * ROWB;
  constexpr int NA = BM / 8;                 // A pieces (1 KiB = 8 rows) per stage
  constexpr int NB = BN / 32;                // B pieces (one packed n-tile block) per stage
  constexpr int NT = NA + NB;
  constexpr int NPW = (NT + NW - 1) / NW;    // glds per wave per stage
  constexpr int STAGE = A_BYTES + NB * 1024;
  constexpr int STAGES = 3;
  static_assert(TM >= 1 && TN >= 1 && NPW <= 15, "bad tile");
  constexpr int EP_BYTES = 32 * WN * 4;                // epilogue: one 32-row slice per wave, f32
  constexpr int SMEM = STAGES * STAGE > NW * EP_BYTES ? STAGES * STAGE : NW * EP_BYTES;

  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int tiles_n = N / BN;
  const int tiles_m = (M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int m0 = (bid / tiles_n) * BM;
  const int n0 = (bid % tiles_n) * BN;
  const int kt_count = K / BK;

  // ---- this wave's LDS-DMA pieces: global source (per lane) and LDS offset (wave-uniform)
  const char* src[NPW];
  int dst[NPW];
  int64_t step[NPW];   // source advance per K tile (bytes)
#pragma unroll
  for (int i = 0; i < NPW; ++i) {
    int j = wave * NPW + i;
    j = j < NT ? j : NT - 1;   // surplus slots re-issue the last piece (same bytes, same place)
    if (j < NA) {
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
  auto issue = [&](int kt, int slot) {
#pragma unroll
    for (int i = 0; i < NPW; ++i)
      __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)(src[i] + kt * step[i]),
                                       (SAMQ_LDS void*)(smem + slot * STAGE + dst[i]), 16, 0, 0);
  };

  int col[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) col[t] = n0 + wn * WN + t * 32 + (lane & 31);
  W4Zero zc[TN];
  half2_t sc[TN];
  auto load_zc = [&](int g) {
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const uint32_t zw = qzeros[(int64_t)g * (N / 8) + (col[t] >> 3)];
      zc[t].set((int)((zw >> (4 * (col[t] & 7))) & 0xFu) + 1);
      if (GROUPED) {
        const _Float16 s = scales[(int64_t)g * N + col[t]];
        sc[t] = half2_t{s, s};
      }
    }
  };
  load_zc(0);
  int cur_group = 0;

  W4Unpack ku;
  ku.init();

  float16_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  int a_off[TM], a_swz[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int rr = wm * WM + i * 32 + (lane & 31);
    a_off[i] = rr * ROWB;
    a_swz[i] = (rr >> 1) & 7;
  }
  const int hsel = lane >> 5;

  issue(0, 0);
  if (kt_count > 1) issue(1, 1);
  int slot = 0;
  for (int kt = 0; kt < kt_count; ++kt) {
    if (kt + 1 < kt_count) vm_wait<NPW>(); else vm_wait<0>();
    __builtin_amdgcn_s_barrier();          // tile kt visible to all; slot (kt+2)%3 free
    if (kt + 2 < kt_count) {
      int s2 = slot + 2;
      s2 = s2 >= STAGES ? s2 - STAGES : s2;
      issue(kt + 2, s2);
    }
    if (GROUPED) {
      const int g = (kt * BK) / groupsize;
      if (g != cur_group) { load_zc(g); cur_group = g; }
    }
    const char* abase = smem + slot * STAGE;
    u32x4 bw[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) bw[t] = *(const u32x4*)(abase + A_BYTES + (wn * TN + t) * 1024 + lane * 16);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      half8_t af[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *(const half8_t*)(abase + a_off[i] + (((2 * s + hsel) ^ a_swz[i]) << 4));
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const uint32_t w = bw[t][s];
        half8_t bf = w4_unpack(w, ku, zc[t]);
        if (GROUPED) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const half2_t h = half2_t{bf[2 * i], bf[2 * i + 1]} * sc[t];
            bf[2 * i] = h[0];
            bf[2 * i + 1] = h[1];
          }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf, acc[i][t], 0, 0, 0);
      }
    }
    slot = slot + 1 == STAGES ? 0 : slot + 1;
  }

  // ---- epilogue: y = acc * s[n] + b[n] (-> GELU), staged through LDS per 32-row slice so the
  // global traffic is row-contiguous 16-byte vectors (f16: 8 columns / lane; f32 residual:
  // 4 columns / lane read-modify-write) instead of one 2- or 4-byte access per accumulator.
  float csc[TN], cb[TN];
  {
    const HOpt bo(bias, scales);
    _Float16 rs[TN];           // one batch of raw loads behind a single wait (bias null: 0)
    uint32_t rb[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      rs[t] = GROUPED ? (_Float16)1.0f : scales[col[t]];
      rb[t] = bo.raw(col[t]);
    }
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      csc[t] = GROUPED ? 1.0f : (float)rs[t];
      cb[t] = bo.f32(rb[t]);
    }
  }
  const int row_base = m0 + wm * WM;
  const int col_base = n0 + wn * WN;
  // fp32 residual: the old values a 32-row slice ahead of the stores (res_load, common.h), the
  // first slice's before the barrier
  constexpr bool RES = EPI == SAMQ_EPI_RESADD_F32;
  constexpr int RJ = RES ? res_j(32, WN) : 1;
  float4_t xo[2][RJ];
  if constexpr (RES) res_load<32, WN>(xo[0], Cout, ldc, M, row_base, col_base, lane);
  __syncthreads();                                      // every wave is done with the ring
  float* ep = (float*)(smem + wave * EP_BYTES);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = (r & 3) + 8 * (r >> 2) + 4 * hsel;   // row within the slice
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        float v = acc[i][t][r] * csc[t] + cb[t];
        if (EPI == SAMQ_EPI_BIAS_GELU) v = gelu_fast(v);
        ep[rl * WN + t * 32 + (lane & 31)] = v;
      }
    }
    if constexpr (RES) {
      if (i + 1 < TM) res_load<32, WN>(xo[(i + 1) & 1], Cout, ldc, M, row_base + (i + 1) * 32, col_base, lane);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slice is in LDS (same wave reads it)
    if (EPI == SAMQ_EPI_RESADD_F32 || EPI == SAMQ_EPI_F32) {
      constexpr int C4 = WN / 4;                        // float4 per slice row
#pragma unroll
      for (int j = 0; j < 32 * C4 / 64; ++j) {
        const int idx = j * 64 + lane;
        const int rl = idx / C4, c4 = idx % C4;
        const int row = row_base + i * 32 + rl;
        float4_t v = ((const float4_t*)ep)[idx];
        if constexpr (RES) v = res_add(xo[i & 1][j], v);
        if (row < M) *(float4_t*)((float*)Cout + (int64_t)row * ldc + col_base + 4 * c4) = v;
      }
    } else {
      constexpr int C8 = WN / 8;                        // 8-column chunks per slice row
#pragma unroll
      for (int j = 0; j < (32 * C8 + 63) / 64; ++j) {
        const int idx = j * 64 + lane;
        if (idx < 32 * C8) {
          const int rl = idx / C8, c8 = idx % C8;
          const int row = row_base + i * 32 + rl;
          const float4_t v0 = ((const float4_t*)ep)[2 * idx];
          const float4_t v1 = ((const float4_t*)ep)[2 * idx + 1];
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

}  // namespace samq
