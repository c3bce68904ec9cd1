// Epilogue of the int8-activation GEMMs, shared by the 3-slot ring kernel (gemm_i8_ring.h) and the
// W4A8 ping-pong kernel (gemm_i8_pp.h).  Included through those two by gemm_i8.hip only.
#pragma once

#include "common.h"

namespace samq {

struct I8Epi {
  float a_scale, mid_scale, res_scale, out_scale;
  const int8_t* R;
  int64_t ldr;
  int rmod;               // > 0: residual row = output row % rmod (pos_embed codes shared by images)
  int kpg;                // grouped W4 (GRP kernels): K tiles (128) per weight group
  // W4A8 row sums: rs_in = S[m] = sum_k A[m, k] of the int8 input rows, emitted by the producer of
  // A (LN-q, the lin1 epilogue) so the ping-pong kernel does not recompute it per column tile;
  // rs_out (int8-code epilogues): S of the OUTPUT rows accumulated with one int32 atomic per row
  // and 16 x (WN / 16) codes -- the caller zeroes it first
  const int* rs_in;
  int* rs_out;
  // Q8 epilogue (the W8A8 qkv GEMM): the codes of columns >= v16_col0 (the V third) are also
  // stored as fp16 values (exact small integers) into v16 [rows, ldv] at column c - v16_col0, so
  // the attention stages V without an int8 -> fp16 conversion per key row
  _Float16* v16;
  int v16_col0;
  int64_t ldv;
};

// Activations with zero points (samq_i8_gemm_zp / samq_w8a8_conv_gemm_zp; W8 ring kernels, int8-code
// epilogues): the kernels instantiated on I8EpiZp take
//   col_offset  int32 [N] (null = 0), added to every row's int32 sum at the head of the epilogue: the
//               INPUT's zero point, -zp_a * sum_k W[n, k] (sum_k (a - zp_a) w = sum a w - zp_a sum w,
//               exact in int32; folded into the float bias it would nearly cancel against the sum);
//   mid_zp / res_zp / out_zp  the zero points of the mid quantiser, the residual codes and the output
//               quantiser (integers in [-128, 127] as floats; q8_exact2_zp, common.h);
//   pad16       AG_3X3: 16 bytes of the input's zero-point code, the gather's source outside the map
//               (a padded 0.0 is the code zp_a), so col_offset holds for border pixels too.
// The symmetric kernels keep I8Epi: their arguments and code are untouched.
struct I8EpiZp : I8Epi {
  const int* col_offset;
  float mid_zp, res_zp, out_zp;
  const int8_t* pad16;
};

// Power-of-Two Factor activations (samq_i8_gemm_ptf / samq_w8a8_conv_gemm_ptf): a PTF quantiser is
// (s0, zp, exp[C]) with the channel's scale s0 * 2^exp[c], exp[c] in 0..3 (fq_vit observer/ptf.py).
// The kernels instantiated on I8EpiPtf take, beside the I8EpiZp fields,
//   out_exp   uint8 [N] (null = 0): the OUTPUT quantiser's exponents.  x * 2^-e is exact and
//             fl(x / (s * 2^e)) = fl(x / s) * 2^-e, so the unchanged quotient chain runs on x * 2^-e;
//   res_exp   uint8 [N] (null = 0, Q8_RES): the residual value is ((R - res_zp) << e) * res_scale;
//   k_tiles_a / k_shift  the INPUT's exponents along K by masked-pass replay (gemm_i8_ring.h): A has
//             k_tiles_a K tiles, the kernel's K is P * k_tiles_a * 128 over P stacked masked weight
//             copies; after the last tile of pass p < P - 1 the int32 sums are shifted left by k_shift[p].
// Both arrays null and P = 1: bit-identical to the I8EpiZp kernels.
struct I8EpiPtf : I8EpiZp {
  const uint8_t* out_exp;
  const uint8_t* res_exp;
  int k_tiles_a;
  int k_shift[3];
};

// 2^e (e in -3..3) as a float, built in the exponent field
__device__ __forceinline__ float ptf_pow2(int e) { return __builtin_bit_cast(float, (uint32_t)(127 + e) << 23); }

// The W4 unpack of both kernels: four nibbles q (one per byte) minus the zero point zpx (zp in
// every byte) as int8 -- bytes(q) | 0x80 minus zp per byte never borrows, ^0x80 -> int8
__device__ __forceinline__ int w4_to_i8(uint32_t nib, uint32_t zpx) {
  return (int)(((nib | 0x80808080u) - zpx) ^ 0x80808080u);
}

// y = float(acc) * (a_scale * wscale[n]) + bias[n] (-> GELU / residual / int8 quantiser) of one
// 32-row slice i of the wave's accumulator tile, staged through LDS (ep = this wave's 32 x WN f32
// slice) so the global traffic is row-contiguous 16-byte vectors.
// ZPS: the sums exclude the zero point (acc = sum a * q) and the epilogue subtracts zp[n] * S[m]
// (zpv = MINUS this lane's zp per column block, ssum = S of the wave's WM rows; int32-exact, on
// the full-rate 24-bit multiply: |zp| <= 16, |S| <= 128 K < 2^23).
// Grouped W4 (float accumulators, the group scales already applied): wscale == nullptr, the
// factor is a_scale alone.
// SAMQ_EPI_RESADD_F32: the old residual is read one slice ahead of the stores (res_load,
// common.h): xcur = this slice's, loaded by the previous slice (the first by i8_epilogue); xnext,
// where not null, receives slice i + 1's before this slice's stores; scb = the factors and biases
// of this lane's columns, loaded once per tile by i8_epilogue (reloaded per slice, their waits
// would drain the residual loads).
template <int TM, int TN, int WN, int EPI, bool ZPS = false, typename AccV = int16_t_v, typename EpiArgs = I8Epi>
__device__ __forceinline__ void i8_epilogue_slice(int i, const AccV (&acc)[TM][TN], const int (&col)[TN],
                                                  const float* __restrict__ wscale, const float* __restrict__ bias,
                                                  const EpiArgs& ep_args, float* ep, void* __restrict__ Cout,
                                                  int64_t ldc, int M, int row_base, int col_base, int lane,
                                                  const int* ssum = nullptr, const int* zpv = nullptr,
                                                  const float4_t* xcur = nullptr, float4_t* xnext = nullptr,
                                                  const float* scb = nullptr) {
  constexpr bool RESB = EPI == SAMQ_EPI_RESADD_F32;
  constexpr bool ZP = std::is_base_of<I8EpiZp, EpiArgs>::value;   // activations with zero points
  constexpr bool PTF = std::is_same<EpiArgs, I8EpiPtf>::value;    // ... and per-column power-of-two factors
  static_assert(!ZP || (!ZPS && (EPI == SAMQ_EPI_Q8 || EPI == SAMQ_EPI_Q8_GELU || EPI == SAMQ_EPI_Q8_RES)),
                "zero points: W8 weights, int8-code epilogues");
  const int hsel = lane >> 5;
  float csc[TN], cb[TN];
  int coff[ZP ? TN : 1];
  float zp_mid = 0.f, zp_res = 0.f, zp_out = 0.f;
  if constexpr (ZP) {
#pragma unroll
    for (int t = 0; t < TN; ++t) coff[t] = ep_args.col_offset ? ep_args.col_offset[col[t]] : 0;
    zp_mid = ep_args.mid_zp;
    zp_res = ep_args.res_zp;
    zp_out = ep_args.out_zp;
  }
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    if constexpr (RESB) {
      csc[t] = scb[t];
      cb[t] = scb[TN + t];
    } else {
      csc[t] = wscale ? ep_args.a_scale * wscale[col[t]] : ep_args.a_scale;
      cb[t] = bias ? bias[col[t]] : 0.0f;
    }
  }
  constexpr bool GELU = EPI == SAMQ_EPI_BIAS_GELU || EPI == SAMQ_EPI_Q8_GELU;
  const float inv_out = ep_args.out_scale > 0.f ? 1.0f / ep_args.out_scale : 0.f;   // q8_exact (common.h)
  const float inv_mid = ep_args.mid_scale > 0.f ? 1.0f / ep_args.mid_scale : 0.f;
  // q8_exact2 clamps (260: a quotient of -255.5 still rounds into the code range under a zero point of 127)
  const float lim_out = (ZP ? 260.0f : 130.0f) * ep_args.out_scale, lim_mid = (ZP ? 260.0f : 130.0f) * ep_args.mid_scale;
  // staging swizzle: the readers below take 64 B (int8 path: 16 columns, 4 ds_read_b128) or 32 B
  // (f16 path: 8 columns, 2 reads) of one row per lane, and a ds_read_b128 lane group spans 4 rows
  // whose k-th 16-byte chunks sat on the same banks (PMC: 3.9 M conflict cycles per W4A8 lin1
  // launch at M = 16384, profiles/r4_pmc_i8_pp2_m16384.txt).  Column c of slice row r is stored at
  // c ^ swz(r), swz = 4 * key: the 4-column chunk within each 16 (int8) / 8 (f16) columns XOR
  // key = (r >> 1) & 3 / & 1, so read k of the group's rows lands on distinct banks; rows r, r + 1
  // (r even) share the key, so a lane's accumulator pair still stores with one ds_write2
  constexpr bool Q8OUT = EPI == SAMQ_EPI_Q8 || EPI == SAMQ_EPI_Q8_GELU || EPI == SAMQ_EPI_Q8_RES;
  constexpr bool F16OUT = EPI == SAMQ_EPI_BIAS || EPI == SAMQ_EPI_BIAS_GELU;
  constexpr int SWZ = (Q8OUT && WN % 16 == 0) ? 1 : (F16OUT && WN % 8 == 0) ? 2 : 0;
  auto swz = [](int row) { return SWZ == 1 ? 4 * ((row >> 1) & 3) : SWZ == 2 ? 4 * ((row >> 1) & 1) : 0; };
  {
    // accumulator pairs (r, r + 1) = slice rows (rl, rl + 1): packed fp32; four rows x TN columns
    // at a time are dequantised and their GELU chains run in lockstep (gelu_r16_n: 2 TN pairs)
#pragma unroll
    for (int r0 = 0; r0 < 16; r0 += 4) {
      float2_t y[2 * TN];
#pragma unroll
      for (int r = r0; r < r0 + 4; r += 2) {
        const int rl = (r & 3) + 8 * (r >> 2) + 4 * hsel;
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          auto a0 = acc[i][t][r], a1 = acc[i][t][r + 1];
          if constexpr (ZPS) {   // v_mad_i32_i24 (zpv = -zp; |S| <= 128 K < 2^23: K < 65536 checked at launch)
            a0 += __mul24(zpv[t], ssum[i * 32 + rl]);
            a1 += __mul24(zpv[t], ssum[i * 32 + rl + 1]);
          }
          if constexpr (ZP) {   // the input's zero point: -zp_a * sum_k W[n, k], exact in int32
            a0 += coff[t];
            a1 += coff[t];
          }
          y[((r - r0) / 2) * TN + t] = __builtin_elementwise_fma((float2_t){(float)a0, (float)a1}, (float2_t)(csc[t]),
                                                                 (float2_t)(cb[t]));
        }
      }
      if constexpr (EPI == SAMQ_EPI_BIAS_GELU) {   // fp16 out: within one fp16 step down the negative tail
#pragma unroll
        for (int n = 0; n < 2 * TN; ++n) y[n] = gelu_erfc2(y[n]);
      } else if constexpr (GELU) {
        gelu_r16_n<2 * TN>(y);
      }
#pragma unroll
      for (int r = r0; r < r0 + 4; r += 2) {
        const int rl = (r & 3) + 8 * (r >> 2) + 4 * hsel;
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          const float2_t v = y[((r - r0) / 2) * TN + t];
          const int cs = (t * 32 + (lane & 31)) ^ swz(rl);   // rl even: swz(rl + 1) == swz(rl)
          ep[rl * WN + cs] = v.x;
          ep[(rl + 1) * WN + cs] = v.y;
        }
      }
    }
    if constexpr (RESB) {   // the next slice's residual: in flight over this slice's staging and stores
      if (xnext) res_load<32, WN>(xnext, Cout, ldc, M, row_base + (i + 1) * 32, col_base, lane);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (EPI == SAMQ_EPI_RESADD_F32 || EPI == SAMQ_EPI_F32) {
      constexpr int C4 = WN / 4;
#pragma unroll
      for (int j = 0; j < 32 * C4 / 64; ++j) {
        const int idx = j * 64 + lane;
        const int rl = idx / C4, c4 = idx % C4;
        const int row = row_base + i * 32 + rl;
        float4_t v = ((const float4_t*)ep)[idx];
        if constexpr (RESB) v = res_add(xcur[j], v);
        if (row < M) *(float4_t*)((float*)Cout + (int64_t)row * ldc + col_base + 4 * c4) = v;
      }
    } else if (EPI == SAMQ_EPI_BIAS || EPI == SAMQ_EPI_BIAS_GELU) {
      constexpr int C8 = WN / 8;
#pragma unroll
      for (int j = 0; j < (32 * C8 + 63) / 64; ++j) {
        const int idx = j * 64 + lane;
        if (idx < 32 * C8) {
          const int rl = idx / C8, c8 = idx % C8;
          const int row = row_base + i * 32 + rl;
          const int f4 = rl * (WN / 4) + 2 * c8, sk = swz(rl) / 4;   // float4s of the 8 columns
          const float4_t v0 = ((const float4_t*)ep)[f4 + sk];
          const float4_t v1 = ((const float4_t*)ep)[f4 + (1 ^ sk)];
          if (row < M) {
            const half8_t h = {(_Float16)v0[0], (_Float16)v0[1], (_Float16)v0[2], (_Float16)v0[3],
                               (_Float16)v1[0], (_Float16)v1[1], (_Float16)v1[2], (_Float16)v1[3]};
            *(half8_t*)((_Float16*)Cout + (int64_t)row * ldc + col_base + 8 * c8) = h;
          }
        }
      }
    } else {   // int8 codes, 16 columns per lane-store
      constexpr int C16 = WN / 16;
      static_assert(C16 >= 1 && 64 % C16 == 0, "int8 store: a row's lanes are C16 consecutive lanes");
#pragma unroll
      for (int j = 0; j < (32 * C16 + 63) / 64; ++j) {
        const int idx = j * 64 + lane;
        int rsum = 0;   // this lane's 16 codes summed (rs_out)
        if (idx < 32 * C16) {
          const int rl = idx / C16, c16 = idx % C16;
          const int row = row_base + i * 32 + rl;
          if (row < M) {
            float v[16];
            const int f4 = rl * (WN / 4) + 4 * c16, sk = swz(rl) / 4;   // float4s of the 16 columns
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float4_t f = ((const float4_t*)ep)[f4 + (e ^ sk)];
              v[4 * e] = f[0]; v[4 * e + 1] = f[1]; v[4 * e + 2] = f[2]; v[4 * e + 3] = f[3];
            }
            u32x4 res;
            if (EPI == SAMQ_EPI_Q8_RES)
              res = *(const u32x4*)(ep_args.R + (int64_t)(ep_args.rmod > 0 ? row % ep_args.rmod : row) * ep_args.ldr +
                                    col_base + 16 * c16);
            u32x4 oexp = {0u, 0u, 0u, 0u}, rexp = {0u, 0u, 0u, 0u};   // PTF: the 16 columns' exponent bytes
            if constexpr (PTF) {
              if (ep_args.out_exp) oexp = *(const u32x4*)(ep_args.out_exp + col_base + 16 * c16);
              if (EPI == SAMQ_EPI_Q8_RES && ep_args.res_exp)
                rexp = *(const u32x4*)(ep_args.res_exp + col_base + 16 * c16);
            }
            u32x4 o;
            float vq[EPI == SAMQ_EPI_Q8 ? 16 : 1];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              float cq[4];
#pragma unroll
              for (int b = 0; b < 4; b += 2) {
                float2_t x = {v[4 * w + b], v[4 * w + b + 1]};
                if constexpr (ZP) {
                  if (EPI == SAMQ_EPI_Q8_RES) {
                    if (ep_args.mid_scale > 0.f)
                      x = (q8_exact2_zp(x, ep_args.mid_scale, inv_mid, lim_mid, zp_mid) - (float2_t)(zp_mid)) *
                          ep_args.mid_scale;
                    float2_t rc = float2_t{(float)(int8_t)((res[w] >> (8 * b)) & 0xFFu),
                                           (float)(int8_t)((res[w] >> (8 * b + 8)) & 0xFFu)} -
                                  (float2_t)(zp_res);   // code - zp: exact
                    if constexpr (PTF)                  // (code - zp) << e: exact
                      rc = rc * float2_t{ptf_pow2((int)((rexp[w] >> (8 * b)) & 3u)),
                                         ptf_pow2((int)((rexp[w] >> (8 * b + 8)) & 3u))};
                    const float2_t rv = rc * ep_args.res_scale;
                    x = rv + x;
                  }
                  if constexpr (PTF)   // the column's output scale is out_scale * 2^e
                    x = x * float2_t{ptf_pow2(-(int)((oexp[w] >> (8 * b)) & 3u)),
                                     ptf_pow2(-(int)((oexp[w] >> (8 * b + 8)) & 3u))};
                  // Q8_GELU: the reciprocal-multiply quotient as in the symmetric kernel (q8_recip2), the
                  // zero point added before the rounding; q8_pack4 saturates
                  const float2_t q = EPI == SAMQ_EPI_Q8_GELU ? q8_recip2(x, inv_out, zp_out)
                                                             : q8_exact2_zp(x, ep_args.out_scale, inv_out, lim_out, zp_out);
                  cq[b] = q.x;
                  cq[b + 1] = q.y;
                  continue;
                }
                if (EPI == SAMQ_EPI_Q8_RES) {
                  if (ep_args.mid_scale > 0.f) x = q8_exact2(x, ep_args.mid_scale, inv_mid, lim_mid) * ep_args.mid_scale;
                  const float2_t rv = float2_t{(float)(int8_t)((res[w] >> (8 * b)) & 0xFFu),
                                               (float)(int8_t)((res[w] >> (8 * b + 8)) & 0xFFu)} * ep_args.res_scale;
                  x = rv + x;
                }
                const float2_t q = EPI == SAMQ_EPI_Q8_GELU ? q8_recip2(x, inv_out)
                                                           : q8_exact2(x, ep_args.out_scale, inv_out, lim_out);
                cq[b] = q.x;
                cq[b + 1] = q.y;
                if constexpr (EPI == SAMQ_EPI_Q8) {
                  vq[4 * w + b] = q.x;
                  vq[4 * w + b + 1] = q.y;
                }
              }
              o[w] = q8_pack4(cq[0], cq[1], cq[2], cq[3]);
            }
            *(u32x4*)((int8_t*)Cout + (int64_t)row * ldc + col_base + 16 * c16) = o;
            if constexpr (EPI == SAMQ_EPI_Q8 && !ZP) {   // (no fp16 V copy under zero points)
              // v16_col0 is a multiple of 64 (samq_w8a8_gemm_v16): a wave of at most 64 columns, at a
              // multiple of WN, lies wholly on one side of it
              static_assert(WN <= 64 && 64 % WN == 0, "v16 store: a wave's columns must not straddle v16_col0");
              if (ep_args.v16 && col_base >= ep_args.v16_col0) {   // (uniform: a wave's columns are in one third)
                half8_t h0, h1;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  h0[e] = (_Float16)vq[e];
                  h1[e] = (_Float16)vq[8 + e];
                }
                _Float16* vp = ep_args.v16 + (int64_t)row * ep_args.ldv + (col_base - ep_args.v16_col0) + 16 * c16;
                *(half8_t*)vp = h0;
                *(half8_t*)(vp + 8) = h1;
              }
            }
            if (ep_args.rs_out) {
#pragma unroll
              for (int w = 0; w < 4; ++w) rsum = __builtin_amdgcn_sdot4((int)o[w], 0x01010101, rsum, false);
            }
          }
        }
        if (ep_args.rs_out) {   // the row's C16 lanes reduce, one int32 atomic per row of the slice
#pragma unroll
          for (int off = 1; off < C16; off <<= 1) rsum += __shfl_xor(rsum, off, 64);
          const int rl = idx / C16, row = row_base + i * 32 + rl;
          if (idx < 32 * C16 && idx % C16 == 0 && row < M) atomicAdd(ep_args.rs_out + row, rsum);
        }
      }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
  }
}

// All TM slices of the wave's tile
template <int TM, int TN, int WN, int EPI, bool ZPS = false, typename AccV = int16_t_v, typename EpiArgs = I8Epi>
__device__ __forceinline__ void i8_epilogue(const AccV (&acc)[TM][TN], const int (&col)[TN],
                                            const float* __restrict__ wscale, const float* __restrict__ bias,
                                            const EpiArgs& ep_args, float* ep, void* __restrict__ Cout, int64_t ldc,
                                            int M, int row_base, int col_base, int lane,
                                            const int* ssum = nullptr, const int* zpv = nullptr) {
  if constexpr (EPI == SAMQ_EPI_RESADD_F32) {
    float4_t xo[2][res_j(32, WN)];   // the old residual of the current and the next slice
    res_load<32, WN>(xo[0], Cout, ldc, M, row_base, col_base, lane);
    float scb[2 * TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      scb[t] = wscale ? ep_args.a_scale * wscale[col[t]] : ep_args.a_scale;
      scb[TN + t] = bias ? bias[col[t]] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
      i8_epilogue_slice<TM, TN, WN, EPI, ZPS, AccV>(i, acc, col, wscale, bias, ep_args, ep, Cout, ldc, M, row_base,
                                                    col_base, lane, ssum, zpv, xo[i & 1],
                                                    i + 1 < TM ? xo[(i + 1) & 1] : nullptr, scb);
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
      i8_epilogue_slice<TM, TN, WN, EPI, ZPS, AccV>(i, acc, col, wscale, bias, ep_args, ep, Cout, ldc, M, row_base,
                                                    col_base, lane, ssum, zpv);
  }
}

}  // namespace samq
