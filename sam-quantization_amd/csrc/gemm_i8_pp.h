// W4A8 ping-pong GEMM kernel (int4 weights x int8 activations, 256x256 tiles).
// Included by gemm_i8.hip only.
#pragma once

#include "gemm_i8_epilogue.h"

namespace samq {

// Flags of the ping-pong kernel: the FLAGS template argument of i8_gemm_pp2 is an OR of these.
// The values are part of the kernels' mangled names.
enum : int {
  I8PP_ROW_SUMS = 1,         // zero point through the row sums of A (cfg 86) instead of per weight (85)
  I8PP_RS_IN = 2,            // with I8PP_ROW_SUMS: the sums come from the producer of A (ep_args.rs_in)
  I8PP_T_NO_MFMA = 4,        // tuning build, timing-only (wrong results): no MFMA
  I8PP_T_NO_RESTAGE = 8,     // tuning build, timing-only (wrong results): no restaging of the ring
  I8PP_T_NO_EPILOGUE = 16,   // tuning build, timing-only (nothing written): no epilogue
};

__host__ __device__ constexpr int i8_pre(int p, int npw, int nph) {   // pieces issued before phase p
  return (npw * p) / nph;
}
template <int N>
__device__ __forceinline__ void i8_vm_wait_le(int n) {   // s_waitcnt vmcnt(n) for a uniform n <= N
  if constexpr (N > 0) {
    if (n >= N) { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); return; }
    i8_vm_wait_le<N - 1>(n);
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

// The W4A16 ping-pong structure (gemm_w4a16_pp.h w4a16_gemm_pp2) on the int8 MFMA: 256x256 tiles,
// 8 waves (2 x 4, 128x64 each) in two groups one s_barrier apart, so the two waves of a SIMD
// alternate -- one issues its MFMA burst (s_setprio 1) while the other reads its A fragments and
// its B piece from LDS and unpacks int4 -> int8; the LDS-DMA pieces of K tile kt+LA are issued
// behind the MFMA bursts of tile kt.  K tile = 128 int8 (128-byte A rows, one 2-KiB layout-3 block
// per 32 columns); phase p of a K tile = k32 steps 2p, 2p+1 = B piece p, so each phase reads its own
// A fragments and unpacks its own piece.  WAR / RAW: as w4a16_gemm_pp2 (the slot restaged during
// tile kt held tile kt+LA-STAGES <= kt-1, whose last reads were consumed before the barrier that
// opens the MFMA half of tile kt's phase 0 for either group; the retire wait for tile kt+1 sits in
// the load half of the last phase, before the barrier after which the first group reads it).
//
// Zero point: without I8PP_ROW_SUMS subtracted per weight in the unpack (w4_to_i8).  With it the
// MFMA multiplies the raw nibbles q (an AND per 4 weights instead of OR / SUB / XOR on top) and the
// epilogue subtracts zp[n] * S[m], S[m] = sum_k a[m, k].  Integer-exact: identical outputs.
// Without I8PP_RS_IN, S is accumulated from the staged A tile by v_dot4
// against ones (wave wn sums the 32 rows of its M block wn, 8 dot4 + 2 LDS reads per phase); with
// it, S is loaded once from ep_args.rs_in -- older than every LDS-DMA piece, so the ring's counted
// waits retire it on the way.  Either way the 4 waves of an M half share the sums through LDS at
// the end.
template <int EPI, int FLAGS = 0>
__global__ __launch_bounds__(512, 1)
void i8_gemm_pp2(const int8_t* __restrict__ A, int64_t lda, const char* __restrict__ Wp,
                 const float* __restrict__ wscale, const uint32_t* __restrict__ qzeros,
                 const float* __restrict__ bias, void* __restrict__ Cout, int64_t ldc, int M, int N, int K,
                 I8Epi ep_args) {
  constexpr int STAGES = 3, LA = 2;            // ring slots, K tiles in flight ahead of the MFMAs
  constexpr int NW = 8, WAVES_N = 4, TM = 4, TN = 2;
  constexpr int WM = TM * 32, WN = TN * 32;
  constexpr int BM = 2 * WM, BN = WAVES_N * WN;
  constexpr int BK = 128, ROWB = BK;
  constexpr int A_BYTES = BM * ROWB;
  constexpr int PPB = 2;                       // W4 layout 3: two 1-KiB pieces per (32 columns, 128 k)
  constexpr int NA = BM / 8, NB = (BN / 32) * PPB, NT = NA + NB;
  constexpr int NPW = (NT + NW - 1) / NW;
  constexpr int STAGE = A_BYTES + NB * 1024;
  constexpr int NPH = 2;
  constexpr int PRE_LAST = i8_pre(NPH - 1, NPW, NPH);
  constexpr int EP_BYTES = 32 * WN * 4;
  constexpr int SMEM = STAGES * STAGE > NW * EP_BYTES ? STAGES * STAGE : NW * EP_BYTES;
  static_assert(LA >= 2 && LA < STAGES, "ring");
  static_assert((LA - 2) * NPW + PRE_LAST <= 63 && (LA - 1) * NPW <= 63, "vmcnt");
  static_assert(SMEM <= 160 * 1024 && NW * EP_BYTES + BM * 4 <= SMEM, "LDS");
  constexpr bool ZPS = (FLAGS & I8PP_ROW_SUMS) != 0, RSIN = ZPS && (FLAGS & I8PP_RS_IN) != 0;
  constexpr bool T_NO_MFMA = (FLAGS & I8PP_T_NO_MFMA) != 0, T_NO_RESTAGE = (FLAGS & I8PP_T_NO_RESTAGE) != 0;
  constexpr bool T_NO_EPILOGUE = (FLAGS & I8PP_T_NO_EPILOGUE) != 0;

  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int grp = wave >> 2;
  const int tiles_n = N / BN;
  const int tiles_m = (M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int m0 = (bid / tiles_n) * BM;
  const int n0 = (bid % tiles_n) * BN;
  const int kt_count = K / BK;

  const char* src[NPW];
  int dst[NPW];
  int step[NPW];
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
  auto issue = [&](int kt, int slot, int i0, int i1) {
#pragma unroll
    for (int i = 0; i < NPW; ++i)
      if (i >= i0 && i < i1)
        __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)(src[i] + (int64_t)kt * step[i]),
                                         (SAMQ_LDS void*)(smem + slot * STAGE + dst[i]), 16, 0, 0);
  };

  int col[TN];
  uint32_t zpx[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    col[t] = n0 + wn * WN + t * 32 + (lane & 31);
    const uint32_t zw = qzeros[col[t] >> 3];
    zpx[t] = (((zw >> (4 * (col[t] & 7))) & 0xFu) + 1u) * 0x01010101u;
  }
  int16_t_v acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
  const int hsel = lane >> 5;
  int a_off[TM], a_swz[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int rr = wm * WM + i * 32 + (lane & 31);
    a_off[i] = rr * ROWB;
    a_swz[i] = (rr >> 1) & 7;
  }
  uint32_t kLo = 0x0F0F0F0Fu;
  asm volatile("" : "+v"(kLo));
  static_assert(!ZPS || TM == WAVES_N, "row sums: wave wn sums M block wn");
  const int rs_row = wm * WM + wn * 32 + (lane & 31);
  const int rs_off = rs_row * ROWB, rs_swz = (rs_row >> 1) & 7;
  int rsum = 0;
  if constexpr (RSIN) {
    const int r = m0 + rs_row;
    rsum = ep_args.rs_in[r < M ? r : M - 1];
  }

  // ---- prologue: K tiles 0 .. LA-1 in flight, tile 0 retired + visible; group 1 lags a barrier
  const int pro = kt_count < LA ? kt_count : LA;
#pragma unroll
  for (int j = 0; j < LA; ++j)
    if (j < pro) issue(j, j, 0, NPW);
  i8_vm_wait_le<(LA - 1) * NPW>((pro - 1) * NPW);
  __builtin_amdgcn_s_barrier();
  if (grp) __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  int slot = 0;
  for (int kt = 0; kt < kt_count; ++kt) {
    const char* st = smem + slot * STAGE;
    const int ahead = kt + LA;
    const bool pf = ahead < kt_count && !T_NO_RESTAGE;
    const int sa = slot + LA >= STAGES ? slot + LA - STAGES : slot + LA;   // (kt + LA) % STAGES
    static_for<NPH>([&](auto pc_) {
      constexpr int p = decltype(pc_)::value;
      // ---------------- load half
      if (p == NPH - 1 && kt + 1 < kt_count) {
        // K tile kt+1 retired: newer = whole tiles kt+2 .. kt+LA-1 + this tile's pieces so far
        // (steady state: a compile-time count instead of the runtime SALU decision tree)
        if (pf && kt + LA < kt_count) {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"((LA - 2) * NPW + PRE_LAST) : "memory");
        } else {
          int newer = pf ? PRE_LAST : 0;
#pragma unroll
          for (int j = 2; j < LA; ++j) newer += kt + j < kt_count ? NPW : 0;
          i8_vm_wait_le<(LA - 2) * NPW + PRE_LAST>(newer);
        }
      }
      u32x4 bw[TN];
#pragma unroll
      for (int t = 0; t < TN; ++t) bw[t] = *(const u32x4*)(st + A_BYTES + ((wn * TN + t) * PPB + p) * 1024 + lane * 16);
      int4_t af[TM][2];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          af[i][s] = *(const int4_t*)(st + a_off[i] + (((2 * (2 * p + s) + hsel) ^ a_swz[i]) << 4));
      if constexpr (ZPS && !RSIN) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int4_t x = *(const int4_t*)(st + rs_off + (((2 * (2 * p + s) + hsel) ^ rs_swz) << 4));
#pragma unroll
          for (int e = 0; e < 4; ++e) rsum = __builtin_amdgcn_sdot4(x[e], 0x01010101, rsum, false);
        }
      }
      int4_t bf[TN][2];
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const uint32_t w0 = bw[t][2 * s], w1 = bw[t][2 * s + 1];
          if (ZPS) {
            bf[t][s] = int4_t{(int)(w0 & kLo), (int)((w0 >> 4) & kLo), (int)(w1 & kLo), (int)((w1 >> 4) & kLo)};
            continue;
          }
          bf[t][s][0] = w4_to_i8(w0 & kLo, zpx[t]);
          bf[t][s][1] = w4_to_i8((w0 >> 4) & kLo, zpx[t]);
          bf[t][s][2] = w4_to_i8(w1 & kLo, zpx[t]);
          bf[t][s][3] = w4_to_i8((w1 >> 4) & kLo, zpx[t]);
        }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // ---------------- MFMA half
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int t = 0; t < TN; ++t) {
            if (T_NO_MFMA) acc[i][t][0] += af[i][s][0] ^ bf[t][s][1];
            else acc[i][t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[i][s], bf[t][s], acc[i][t], 0, 0, 0);
          }
      if (pf) issue(ahead, sa, i8_pre(p, NPW, NPH), i8_pre(p + 1, NPW, NPH));
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    });
    slot = slot == STAGES - 1 ? 0 : slot + 1;
  }
  if (!grp) __builtin_amdgcn_s_barrier();   // balance group 1's extra barrier

  if constexpr (T_NO_EPILOGUE) {   // sums kept alive
    int z = rsum;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int t = 0; t < TN; ++t) z += acc[i][t][0] + acc[i][t][15];
    if (z == 123456789) ((int*)Cout)[tid] = z;
    return;
  }
  __syncthreads();
  if constexpr (ZPS) {
    int* s_lds = (int*)(smem + NW * EP_BYTES);
    if constexpr (!RSIN) rsum += __shfl_xor(rsum, 32, 64);   // the two k halves of the row
    if (lane < 32) s_lds[rs_row] = rsum;
    __syncthreads();
    int zpv[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) zpv[t] = -(int)(zpx[t] & 0xFFu);
    i8_epilogue<TM, TN, WN, EPI, true>(acc, col, wscale, bias, ep_args, (float*)(smem + wave * EP_BYTES), Cout, ldc,
                                       M, m0 + wm * WM, n0 + wn * WN, lane, s_lds + wm * WM, zpv);
    return;
  }
  i8_epilogue<TM, TN, WN, EPI>(acc, col, wscale, bias, ep_args, (float*)(smem + wave * EP_BYTES), Cout, ldc, M,
                               m0 + wm * WM, n0 + wn * WN, lane);
}

}  // namespace samq
