// Int8 GEMM on a 2- or 3-slot LDS-DMA ring (W8 and W4 weights, grouped W4, implicit-GEMM A).
// Included by gemm_i8.hip only.
#pragma once

#include "gemm_i8_epilogue.h"

namespace samq {

enum { BF_W8 = 0, BF_W4 = 1 };

// Implicit-GEMM A operand (AG != 0): the int8 codes are gathered from an image / feature map
// instead of an [M, K] matrix, 16 contiguous bytes per LDS-DMA lane:
//   AG_PATCH  x int8 [B, Cin, S, S] (NCHW), P = 16: A[t, (c, kh, kw)] = x[b, c, gy*16+kh, gx*16+kw]
//             (fq_vit PatchEmbed QConv2d on the image codes, fq_vit image_encoder.py PatchEmbed)
//   AG_3X3    x int8 [B, G, G, Cin] (NHWC), pad 1: A[t, (ky, kx, c)] = x[b, gy+ky-1, gx+kx-1, c], 0 outside
//             (neck QConv2d 3x3, image_encoder.py:88-104; weight codes permuted to (n, ky, kx, c))
enum { AG_ROWS = 0, AG_PATCH = 1, AG_3X3 = 2 };
struct I8Gather { int S, G, Cin; };
__device__ __attribute__((aligned(16))) int8_t g_zero_i8[16];


template <int N>
__device__ __forceinline__ void vm_wait_i8() {
  static_assert(N >= 0 && N <= 15, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Same machinery as the W4A16 v3 kernel (gemm_w4a16_ring.h): LDS ring fed by global_load_lds (A
// rows XOR-swizzled through the source address, B pre-packed in fragment order), counted vmcnt
// waits + one s_barrier per K tile, XCD-aware tile remap, LDS-staged 16-byte vector epilogue.
// K tile = 128 int8 = the same 128-byte A rows as the fp16 kernel.
// GRP (W4 only): grouped GPTQ weights, w = s[g, n] (q - zp[g, n]) with g = k / groupsize and the
// groupsize a multiple of the 128-deep K tile (ep_args.kpg tiles per group).  The int32 MFMA sums of
// one group are exact (|sum| <= 128 * 127 * 16 per tile); at each group end they are scaled by the
// group's f32 scale into f32 accumulators (one fma per element) and restarted; the zero point of
// the group is applied per byte in the unpack as for per-channel weights.  wscale is the f32
// [G, N] scale table; the next group's zero / scale words are loaded one K tile ahead, before the
// tile's LDS-DMA pieces (so the ring's counted vmcnt covers them).
// EpiArgs = I8EpiZp (W8 only): activations with zero points -- the epilogue adds col_offset and
// carries the quantisers' zero points, the 3x3 gather pads with the zero-point code (I8EpiZp,
// gemm_i8_epilogue.h); the main loop is the same.
// EpiArgs = I8EpiPtf: Power-of-Two Factor activations.  Epilogue: per-column exponents of the output
// quantiser and the residual.  Main loop (AG_ROWS): masked-pass replay for an INPUT with per-k
// exponents -- A has ep_args.k_tiles_a K tiles and the kernel's K runs P <= 4 times over them (the A
// tile index is a running counter modulo k_tiles_a) against P stacked weight copies, pass p holding
// W[n, k] where exp[k] == e_p (descending, the last 0) and 0 elsewhere; after the last tile of pass
// p < P - 1 the int32 sums are shifted left by k_shift[p] = e_p - e_{p+1} (Horner), which gives
// sum_k a_k 2^exp[k] W[n, k] exactly (the host checks 255 * 128 * 2^max_exp * K_A < 2^31).
template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI, int BFMT, int STAGES, int AG = AG_ROWS, bool GRP = false,
          typename EpiArgs = I8Epi>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N)
void i8_gemm_kernel(const int8_t* __restrict__ A, int64_t lda, const char* __restrict__ Wp,
                    const float* __restrict__ wscale, const uint32_t* __restrict__ qzeros,
                    const float* __restrict__ bias, void* __restrict__ Cout, int64_t ldc,
                    int M, int N, int K, EpiArgs ep_args, I8Gather ga) {
  constexpr bool ZP = std::is_base_of<I8EpiZp, EpiArgs>::value;
  constexpr bool PTF = std::is_same<EpiArgs, I8EpiPtf>::value;
  static_assert(!ZP || (BFMT == BF_W8 && !GRP), "zero points: W8 weights");
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int WM = BM / WAVES_M;
  constexpr int WN = BN / WAVES_N;
  constexpr int TM = WM / 32;
  constexpr int TN = WN / 32;
  constexpr int BK = 128;                     // int8 k per tile = 128-byte A rows
  constexpr int ROWB = BK;
  constexpr int A_BYTES = BM * ROWB;
  constexpr int PPB = BFMT == BF_W8 ? 4 : 2;  // 1-KiB pieces per (32-column, 128-k) block
  constexpr int NA = BM / 8;
  constexpr int NB = (BN / 32) * PPB;
  constexpr int NT = NA + NB;
  constexpr int NPW = (NT + NW - 1) / NW;
  constexpr int STAGE = A_BYTES + NB * 1024;
  static_assert(TM >= 1 && TN >= 1 && NPW <= 15, "bad tile");
  static_assert(!GRP || (BFMT == BF_W4 && AG == AG_ROWS), "grouped: W4 weights, row-major A");

  __shared__ __attribute__((aligned(16))) char smem[STAGES * STAGE];

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

  const char* src[NPW];
  int dst[NPW];
  int64_t step[NPW];
  int gtok[NPW], gck[NPW];   // AG: token (b, gy, gx) and in-tile byte offset of each A piece's lane
#pragma unroll
  for (int i = 0; i < NPW; ++i) {
    int j = wave * NPW + i;
    j = j < NT ? j : NT - 1;
    if (j < NA) {
      const int row = j * 8 + (lane >> 3);
      const int c = (lane & 7) ^ ((row >> 1) & 7);
      int gr = m0 + row;
      gr = gr < M ? gr : M - 1;
      src[i] = (const char*)(A + (int64_t)gr * lda + c * 16);
      gtok[i] = gr;
      gck[i] = c * 16;
      dst[i] = j * 1024;
      step[i] = BK;
    } else {
      const int jb = j - NA;
      const int nt = n0 / 32 + jb / PPB;
      src[i] = Wp + (((int64_t)nt * kt_count) * PPB + (jb % PPB)) * 1024 + lane * 16;
      dst[i] = A_BYTES + jb * 1024;
      step[i] = PPB * 1024;
    }
  }
  auto a_gather = [&](int i, int kt) -> const char* {
    const int t = gtok[i], k = kt * BK + gck[i];
    const int gg = ga.G * ga.G;
    const int b = t / gg, rem = t - b * gg, gy = rem / ga.G, gx = rem - gy * ga.G;
    if (AG == AG_PATCH) {   // k = (c * 16 + kh) * 16 + kw, kw = 0..15 contiguous
      const int ckh = k >> 4;
      const int c = ckh >> 4, kh = ckh & 15;
      return (const char*)(A + (((int64_t)b * ga.Cin + c) * ga.S + gy * 16 + kh) * ga.S + gx * 16);
    }
    const int tap = k / ga.Cin, c0 = k - tap * ga.Cin;   // AG_3X3: k = (ky * 3 + kx) * Cin + c
    const int sy = gy + tap / 3 - 1, sx = gx + tap % 3 - 1;
    if (sy < 0 || sy >= ga.G || sx < 0 || sx >= ga.G) {
      if constexpr (ZP) return (const char*)ep_args.pad16;   // a padded 0.0 is the code zp
      else return (const char*)g_zero_i8;
    }
    return (const char*)(A + (((int64_t)b * ga.G + sy) * ga.G + sx) * ga.Cin + c0);
  };
  int ka_next = 0;   // PTF: the A tile of the next issue, kt mod k_tiles_a (issue runs kt = 0, 1, 2, ...)
  auto issue = [&](int kt, int slot) {
    int ka = kt;
    if constexpr (PTF) {
      ka = ka_next;
      ka_next = ka_next + 1 == ep_args.k_tiles_a ? 0 : ka_next + 1;
    }
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
      const char* p = src[i] + kt * step[i];
      if constexpr (PTF) {
        if (wave * NPW + i < NA) p = src[i] + ka * step[i];
      }
      if (AG != AG_ROWS && wave * NPW + i < NA) p = a_gather(i, kt);
      __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)p, (SAMQ_LDS void*)(smem + slot * STAGE + dst[i]), 16,
                                       0, 0);
    }
  };

  int col[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) col[t] = n0 + wn * WN + t * 32 + (lane & 31);
  uint32_t zpx[TN];
  if (BFMT == BF_W4) {
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const uint32_t zw = qzeros[col[t] >> 3];
      zpx[t] = (((zw >> (4 * (col[t] & 7))) & 0xFu) + 1u) * 0x01010101u;
    }
  }

  int16_t_v acc[TM][TN];
  float16_t facc[GRP ? TM : 1][GRP ? TN : 1];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[i][j][r] = 0;
        if constexpr (GRP) facc[i][j][r] = 0.f;
      }
  const int kpg = GRP ? ep_args.kpg : 1;
  float gsc[TN], nsc[TN];   // GRP: the current / next group's scales of this lane's columns
  uint32_t nzp[TN];
  if constexpr (GRP) {
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      gsc[t] = wscale[col[t]];
      nsc[t] = gsc[t];
      nzp[t] = zpx[t];
    }
  }

  int a_off[TM], a_swz[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int rr = wm * WM + i * 32 + (lane & 31);
    a_off[i] = rr * ROWB;
    a_swz[i] = (rr >> 1) & 7;
  }
  const int hsel = lane >> 5;
  uint32_t kLo = 0x0F0F0F0Fu;
  asm volatile("" : "+v"(kLo));

  int ptile = 0, pass = 0;   // PTF: tiles done in the current pass, the pass
  issue(0, 0);
  if (STAGES > 2 && kt_count > 1) issue(1, 1);
  int slot = 0;
  for (int kt = 0; kt < kt_count; ++kt) {
    if (STAGES > 2) {
      if (kt + 1 < kt_count) vm_wait_i8<NPW>(); else vm_wait_i8<0>();
      __builtin_amdgcn_s_barrier();
      if (GRP && kt + 1 < kt_count && (kt + 1) % kpg == 0) {   // next group's zero / scale words
        const int g = (kt + 1) / kpg;
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          const uint32_t zw = qzeros[(int64_t)g * (N / 8) + (col[t] >> 3)];
          nzp[t] = (((zw >> (4 * (col[t] & 7))) & 0xFu) + 1u) * 0x01010101u;
          nsc[t] = wscale[(int64_t)g * N + col[t]];
        }
      }
      if (kt + 2 < kt_count) {
        int s2 = slot + 2;
        s2 = s2 >= STAGES ? s2 - STAGES : s2;
        issue(kt + 2, s2);
      }
    } else {
      vm_wait_i8<0>();
      __builtin_amdgcn_s_barrier();            // tile kt landed; everyone is done with tile kt-1
      if (GRP && kt + 1 < kt_count && (kt + 1) % kpg == 0) {
        const int g = (kt + 1) / kpg;
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          const uint32_t zw = qzeros[(int64_t)g * (N / 8) + (col[t] >> 3)];
          nzp[t] = (((zw >> (4 * (col[t] & 7))) & 0xFu) + 1u) * 0x01010101u;
          nsc[t] = wscale[(int64_t)g * N + col[t]];
        }
      }
      if (kt + 1 < kt_count) issue(kt + 1, slot ^ 1);
    }
    const char* abase = smem + slot * STAGE;
    const char* bbase = abase + A_BYTES + (wn * TN) * PPB * 1024 + lane * 16;
    u32x4 bw[TN][2];
    if (BFMT == BF_W4) {
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        bw[t][0] = *(const u32x4*)(bbase + (t * PPB + 0) * 1024);
        bw[t][1] = *(const u32x4*)(bbase + (t * PPB + 1) * 1024);
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int4_t af[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *(const int4_t*)(abase + a_off[i] + (((2 * s + hsel) ^ a_swz[i]) << 4));
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        int4_t bf;
        if (BFMT == BF_W8) {
          bf = *(const int4_t*)(bbase + (t * PPB + s) * 1024);
        } else {
          const uint32_t w0 = bw[t][s >> 1][2 * (s & 1)];
          const uint32_t w1 = bw[t][s >> 1][2 * (s & 1) + 1];
          bf[0] = w4_to_i8(w0 & kLo, zpx[t]);
          bf[1] = w4_to_i8((w0 >> 4) & kLo, zpx[t]);
          bf[2] = w4_to_i8(w1 & kLo, zpx[t]);
          bf[3] = w4_to_i8((w1 >> 4) & kLo, zpx[t]);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) acc[i][t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[i], bf, acc[i][t], 0, 0, 0);
      }
    }
    if constexpr (PTF) {   // end of a pass that is not the last: the sums move up to the next exponent
      if (++ptile == ep_args.k_tiles_a) {
        ptile = 0;
        if (kt + 1 < kt_count) {
          const int sh = pass == 0 ? ep_args.k_shift[0] : (pass == 1 ? ep_args.k_shift[1] : ep_args.k_shift[2]);
          ++pass;
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int t = 0; t < TN; ++t)
#pragma unroll
              for (int r = 0; r < 16; ++r) acc[i][t][r] = (int)((uint32_t)acc[i][t][r] << sh);
        }
      }
    }
    if (GRP && ((kt + 1) % kpg == 0 || kt + 1 == kt_count)) {   // group end: scale the exact sums in
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            facc[i][t][r] = __builtin_fmaf((float)acc[i][t][r], gsc[t], facc[i][t][r]);
            acc[i][t][r] = 0;
          }
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        zpx[t] = nzp[t];
        gsc[t] = nsc[t];
      }
    }
    if (STAGES > 2) slot = slot + 1 == STAGES ? 0 : slot + 1;
    else slot ^= 1;
  }

  // ---- epilogue (LDS-staged per 32-row slice, in the ring's LDS)
  static_assert(NW * 32 * WN * 4 <= STAGES * STAGE, "epilogue staging does not fit the LDS ring");
  __syncthreads();
  if constexpr (GRP)
    i8_epilogue<TM, TN, WN, EPI, false, float16_t>(facc, col, nullptr, bias, ep_args, (float*)(smem + wave * 32 * WN * 4),
                                                   Cout, ldc, M, m0 + wm * WM, n0 + wn * WN, lane);
  else
    i8_epilogue<TM, TN, WN, EPI>(acc, col, wscale, bias, ep_args, (float*)(smem + wave * 32 * WN * 4), Cout, ldc, M,
                                 m0 + wm * WM, n0 + wn * WN, lane);
}

}  // namespace samq
