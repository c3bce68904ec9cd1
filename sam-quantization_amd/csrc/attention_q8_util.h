// Shared pieces of the W8A8 attention kernels (attention_q8.hip): the launch parameters, the D = 80 tail
// fragments, the rel-pos MFMA block, the softmax numerator table, and the score quantiser, row maximum
// and table lookup that the row64 and window kernels have in common.  The offset move, the 32-key P.V
// step, the output store, the pad-token codes and the int8 -> fp16 unpack stay written out in each
// kernel: as helpers they compute the same values, but the compiler then allocates and schedules the
// kernels differently (1 - 1.5 % either way on the MI355X).
#pragma once

#include "common.h"

namespace samq {

struct AttnQ8Params {
  const int8_t* qkv;        // [B, H, W, 3, heads, D] codes (D = 64 or 80)
  const float* qkv_bias;    // [3 * C] f32 or null (pad tokens)
  const float* relh;        // [2S-1, D] f32
  const float* relw;        // [2S-1, D] f32
  int8_t* out;              // [B, H, W, C] codes
  int B, H, W, heads, C, S, window, nwh, nww, L;   // B, heads: read by no kernel; they keep the offsets of
                                                  // the fields behind them, which the compiled kernels carry
  const _Float16* v16;      // optional [B, H, W, C] fp16 copy of the V codes (samq_w8a8_gemm_v16)
  int row0;                 // row range (samq_rel_attention_q8_rows): global -- first query grid row
                            // (grid z = rows); windows -- first window row (nwh = the range's rows)
  float qk_scale, s_qkv, s_a1, s_a2, s_out;
  float inv_a1, inv_a2, k2;   // 1/s_a1, 1/s_a2, s_a2*log2(e)
};

// Activations with zero points (samq_rel_attention_q8_zp): the kernels instantiated with ZP take this
// struct instead; the symmetric kernels keep AttnQ8Params and with it their argument layout.  With
// z = zp_qkv, codes q, k, v and D the head dim:
//   q.k    sum_d (q - z)(k - z) = sum q k + (-z) sum_d k - z sum_d q + D z^2, all on the int8 MFMA: the
//          accumulator tile is seeded with this lane's query constant D z^2 - z sum_d q (q8_zp_seed) and
//          a second v_mfma_i32_16x16x64_i8 of the same K fragment against the constant operand -z in
//          every byte adds (-z) sum_d k of each key -- no per-score VALU work and no key sums in LDS
//          (these loops are VALU-bound; the MFMA pipe has the room).  -z = 128 (z = -128) does not fit a
//          byte: the operand is then 64 and the MFMA runs twice (zc_twice).
//   rel    the query codes are unpacked to fp16 as q - z (exact: |q - z| <= 255).
//   scores code1 = clamp(rint(st c1 + z1)), code2 = clamp(rint((code1 - z1) k12 + (rel_h + rel_w) /
//          s_a2 + z2)) = clamp(rint(fma(code1, k12, rh + rw + zfold))), zfold = z2 - z1 k12 folded into
//          the per-lane rel_w registers.  The softmax is shift-invariant and the P table works on code
//          differences d = c - m in [-255, lazyc], codes still in [-128, 127]: nothing else changes.
//   P.V    V is staged as v - z (exact in fp16), so O / l s_qkv is the output value as before, then the
//          output quantiser with z_out.  (O - z l on the raw codes cancels: on the 4096 keys of the
//          64 x 64 grid the fp32 accumulation error of sum P v, ~1e-4 of |z|, is 1e-3 of an output code
//          at a fine s_out -- 1.75e-4 of the codes of the exact-tie test moved.)
//   pads   tokens outside the image: clamp(rint(bias / s + z)), or the code z without a bias.
struct AttnQ8ParamsZp : AttnQ8Params {
  float z_qkv, z_a1, z_a2, z_out, zfold;
  int zi_qkv, dz2;          // z as int; D z^2
  int zc;                   // the constant B operand: -z (64 for z = -128) in every byte
  int zc_twice;             // z = -128: the constant MFMA runs twice
};
template <bool ZP> struct AttnQ8ParamsOf { typedef AttnQ8Params type; };
template <> struct AttnQ8ParamsOf<true> { typedef AttnQ8ParamsZp type; };

typedef int int4v __attribute__((ext_vector_type(4)));

// sum_d q[d] over a lane's 16 (+ 16 tail) query codes, reduced over the four lane groups that share a
// query, into the accumulator seed D z^2 - z sum_d q of that query's column
__device__ __forceinline__ int4v q8_zp_seed(const AttnQ8ParamsZp& p, int4v qfrag, int4v qtail) {
  int s = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s = __builtin_amdgcn_sdot4(qfrag[e], 0x01010101, s, false);
    s = __builtin_amdgcn_sdot4(qtail[e], 0x01010101, s, false);   // zero at D = 64 and in lane groups 1..3
  }
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  const int cq = p.dz2 - p.zi_qkv * s;
  return int4v{cq, cq, cq, cq};
}
// seed + (-z) sum_d k of the 16 keys of K fragment kf (wave-uniform branch for z = -128)
__device__ __forceinline__ int4v q8_zp_ksum(const AttnQ8ParamsZp& p, int4v kf, int4v acc) {
  const int4v c = {p.zc, p.zc, p.zc, p.zc};
  acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, c, acc, 0, 0, 0);
  if (p.zc_twice) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, c, acc, 0, 0, 0);
  return acc;
}
// pad-token codes under a zero point: 16 codes of bias[0..15] (null: the code z) as four dwords
__device__ __forceinline__ u32x4 q8_zp_pad16(const float* bias, float s, float z) {
  u32x4 w = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int c = (int)(bias ? q8_exact_zp(bias[e], s, 1.0f / s, z) : z);
    w[e >> 2] |= ((uint32_t)c & 0xFFu) << (8 * (e & 3));
  }
  return w;
}

// LDS pitches of the row64 and window kernels.  K rows at 96 bytes: the ds_read_b128 fragment reads
// (16 rows x 16 bytes per lane group) are conflict-free in all four lane groups -- at 80 bytes three lane
// pairs of every group share a bank.  V rows (fp16, row-major) at 80 halves: a 32-lane group of a tr
// read takes 8 key rows x 32 bytes, row r starting at bank 40 r mod 64 = 8 (5 r mod 8), a permutation of
// the eight 8-bank slots, for every tile t (a tile shifts all rows alike); 72 halves puts key quads 0 / 7,
// 88 rows 0 / 3 and 96 rows 0 / 4 on the same banks.  At D = 80 the V row is exactly the pitch (no pad)
// and the K row fits the 96, so the LDS per workgroup is the same at both head dims.
constexpr int Q8_KP = 96, Q8_VP = 80;

__device__ __forceinline__ float aq8(float v, float s) {
  return q8_exact(v, s, 1.0f / s);   // s is a kernel argument: the reciprocal is hoisted
}
// Head dim D is a template parameter of every kernel: 64 (vit_b, vit_l) or 80 (vit_h).  D = 80 is 5
// sixteen-byte pieces per token and head; dims 64..79 enter q.k through a second
// v_mfma_i32_16x16x64_i8 into the same int32 tile, lane group 0 holding the 16 dims and groups 1..3
// zero in BOTH operands.  Equal pass counts along an accumulate chain: the cheaper 16x16x32_i8 (4
// passes instead of 8) must not be chained onto the 16x16x64 result -- with SrcC = the previous vDst the
// compiler leaves the two back to back, which the hardware covers for MFMAs of equal pass count only
// (the 4-pass one read the tile before the 8-pass one had written it).  These loops are VALU-bound, so
// the MFMA pipe has the room.
// Dims 64..79 of the token whose head starts at ``base``, in lane group 0; zero in groups 1..3.
__device__ __forceinline__ int4v q8_tail(const int8_t* base, int g) {
  const int4v v = *(const int4v*)(base + 64);
  const int4v z = {0, 0, 0, 0};
  return g == 0 ? v : z;
}
// the same for a pad token; ``bias`` = the head's first bias value
__device__ __forceinline__ int4v q8_tail_bias(const float* bias, float s, int g) {
  int4v w = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 16; ++e) w[e >> 2] |= ((int)q8_exact(bias[64 + e], s, 1.0f / s) & 0xFF) << (8 * (e & 3));
  const int4v z = {0, 0, 0, 0};
  return g == 0 ? w : z;
}

// 16 int8 codes -> fp16 (exact), as the two 16-byte halves of a row-major V row
__device__ __forceinline__ void q8_unpack16(u32x4 w, half8_t& h0, half8_t& h1) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    h0[e] = (_Float16)(float)(int8_t)((w[e >> 2] >> (8 * (e & 3))) & 0xFFu);
    h1[e] = (_Float16)(float)(int8_t)((w[2 + (e >> 2)] >> (8 * (e & 3))) & 0xFFu);
  }
}

// q8_unpack16 as code - z (zero-point kernels: V staged as v - z; exact in fp16)
__device__ __forceinline__ void q8_unpack16_zp(u32x4 w, half8_t& h0, half8_t& h1, float z) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    h0[e] = (_Float16)((float)(int8_t)((w[e >> 2] >> (8 * (e & 3))) & 0xFFu) - z);
    h1[e] = (_Float16)((float)(int8_t)((w[2 + (e >> 2)] >> (8 * (e & 3))) & 0xFFu) - z);
  }
}

// 8 int8 codes -> fp16 (exact); MASKED: all zero unless ``on``
template <bool MASKED>
__device__ __forceinline__ half8_t q8_unpack8(uint2 cw, bool on) {
  half8_t qb;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const _Float16 v = (_Float16)(float)(int8_t)((((e < 4) ? cw.x : cw.y) >> (8 * (e & 3))) & 0xFFu);
    qb[e] = MASKED ? (on ? v : (_Float16)0.f) : v;
  }
  return qb;
}
// the same as code - z (zero-point kernels; exact in fp16: |code - z| <= 255)
template <bool MASKED>
__device__ __forceinline__ half8_t q8_unpack8_zp(uint2 cw, bool on, float z) {
  half8_t qb;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const _Float16 v = (_Float16)((float)(int8_t)((((e < 4) ? cw.x : cw.y) >> (8 * (e & 3))) & 0xFFu) - z);
    qb[e] = MASKED ? (on ? v : (_Float16)0.f) : v;
  }
  return qb;
}

// K row pitch in LDS (bytes) of the generic kernel: 80 at D = 64; a D = 80 row is 80 bytes itself, so it
// takes the 96 of the row64 / window kernels
template <int D> constexpr int q8_kpitch() { return D == 64 ? 80 : Q8_KP; }

// rel_h / rel_w for the 16 queries of a wave that share the query grid row qy, by MFMA:
// rel[kk][q] = s_qkv * sum_d code_q[d] * R[qy - kk + side - 1][d] (both tables by the query ROW: the
// reference's quirk) for the 16 key rows / columns kk = 16 bb + m of block bb.  A operand row m = the
// table row of kk; B = the int8 query codes, exact in fp16; the f32 tables enter as fp16 hi + lo pairs
// (|R - hi - lo| <= 2^-22 |R|), so the sums carry fp32-level error like a scalar fp32 dot product.
// Lane (ql, g) receives rel[16 bb + 4 g + i][query ql], i = 0..3.  ``qcodes_lane``: query ql's codes.
// D = 80 = 2 x 32 + 16: dims 64..79 go through a third, half-filled 16x16x32 step -- lane groups 0 / 1
// hold dims 64 + 8 g .. + 7, groups 2 / 3 read what 0 / 1 read and zero it in BOTH operands (a table
// value times a zero code would still be NaN for an Inf) -- rather than a 16x16x16: one opcode along
// the accumulate chain (see q8_tail).
// ZP: the codes enter as code - zq (q8_unpack8_zp).
template <int D, bool ZP = false>
__device__ __forceinline__ void q8_rel_block(const AttnQ8Params& p, const int8_t* qcodes_lane, int qy, int side,
                                             int bb, int lane, float4_t& rh4, float4_t& rw4, float zq = 0.f) {
  const int ql = lane & 15, g = lane >> 4;
  int r = qy - (16 * bb + ql) + side - 1;      // table row of this lane's A row (kk = 16 bb + ql)
  r = r < 0 ? 0 : (r > 2 * side - 2 ? 2 * side - 2 : r);   // rows past the window: any valid row (masked)
  rh4 = float4_t{0.f, 0.f, 0.f, 0.f};
  rw4 = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    const uint2 cw = *(const uint2*)(qcodes_lane + 32 * s + 8 * g);   // codes of query ql, dims 32s+8g..+7
    half8_t qb;
    if constexpr (ZP) qb = q8_unpack8_zp<false>(cw, true, zq);
    else qb = q8_unpack8<false>(cw, true);
#pragma unroll
    for (int tab = 0; tab < 2; ++tab) {
      const float* src = (tab ? p.relw : p.relh) + (int64_t)r * D + 32 * s + 8 * g;
      const float4_t x0 = *(const float4_t*)src, x1 = *(const float4_t*)(src + 4);
      half8_t hi, lo;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = e < 4 ? x0[e] : x1[e - 4];
        hi[e] = (_Float16)x;
        lo[e] = (_Float16)(x - (float)hi[e]);
      }
      float4_t& d = tab ? rw4 : rh4;
      d = __builtin_amdgcn_mfma_f32_16x16x32_f16(hi, qb, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_16x16x32_f16(lo, qb, d, 0, 0, 0);
    }
  }
  if constexpr (D % 32 == 16) {
    constexpr int T0 = D - 16;
    const bool on = g < 2;
    const int toff = T0 + 8 * (g & 1);          // groups 2 / 3 read what 0 / 1 read, and zero it
    const uint2 cw = *(const uint2*)(qcodes_lane + toff);
    half8_t qb;
    if constexpr (ZP) qb = q8_unpack8_zp<true>(cw, on, zq);
    else qb = q8_unpack8<true>(cw, on);
#pragma unroll
    for (int tab = 0; tab < 2; ++tab) {
      const float* src = (tab ? p.relw : p.relh) + (int64_t)r * D + toff;
      const float4_t x0 = *(const float4_t*)src, x1 = *(const float4_t*)(src + 4);
      half8_t hi, lo;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = on ? (e < 4 ? x0[e] : x1[e - 4]) : 0.f;
        hi[e] = (_Float16)x;
        lo[e] = (_Float16)(x - (float)hi[e]);
      }
      float4_t& d = tab ? rw4 : rh4;
      d = __builtin_amdgcn_mfma_f32_16x16x32_f16(hi, qb, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_16x16x32_f16(lo, qb, d, 0, 0, 0);
    }
  }
  rh4 = rh4 * p.s_qkv;
  rw4 = rw4 * p.s_qkv;
}

// ---------------------------------------------------------------- softmax numerator table
// The score codes are integers and the softmax offset m is one of them, so P = exp2((c - m) k2) takes
// at most 256 + lazyc distinct values, d = c - m in [-255, lazyc].  Entry BASE + d holds P split as fp16
// hi (low half) + lo (high half) -- the B operands of the P.V MFMAs -- and entries below BASE - 255 hold
// 0: a score costs one LDS read and half a v_perm instead of fma + exp2 + three conversions + a
// subtraction.  P = exp2(fl(d k2)) here vs exp2(fl(c k2 - fl(m k2))) computed directly: last-bit
// differences of fp32 P, below the 2^-22 of the hi + lo split.
//   row64:  BASE = 256, every key is real; entry 0 (d = -256, never addressed) is the one zero.
//   window: BASE = 528, masked slots carry the code -400, whose entry -400 - m + 528 is at most 256 <
//           BASE - 255 = 273 for any offset m >= -128: every score, masked or not, is one lookup.
// Lazy offset: m moves only when a code exceeds it by more than lazyc = min(8 / k2, 255) codes, so
// P <= 2^8, far inside fp16 (O and l carry the same offset), and most chunks skip the O / l rescale.
constexpr int PTAB_BASE = 256, PTAB = PTAB_BASE + 256;
constexpr int PTABW_BASE = 528, PTABW = PTABW_BASE + 256;
__device__ __forceinline__ int q8_ptab_lazy(float k2) {   // lazy offset threshold in codes
  return (int)fminf(floorf(8.0f / k2), 255.0f);
}
template <int BASE, int NT>
__device__ __forceinline__ void q8_ptab_fill(uint32_t* ptab, float k2, int lazyc, int tid) {
  for (int i = tid; i <= BASE + lazyc; i += NT) {
    const float pv = i < BASE - 255 ? 0.0f : __builtin_amdgcn_exp2f((float)(i - BASE) * k2);
    const _Float16 h = (_Float16)pv, l = (_Float16)(pv - (float)h);
    ptab[i] = (uint32_t)__builtin_bit_cast(uint16_t, h) | ((uint32_t)__builtin_bit_cast(uint16_t, l) << 16);
  }
}
// P^T fragments (hi, lo) of 8 scores from their table words (v_perm: two per pair of scores)
__device__ __forceinline__ void q8_ptab_unpack(const uint32_t (&w)[8], half8_t& bhi, half8_t& blo) {
  uint32_t hi[4], lo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    hi[j] = __builtin_amdgcn_perm(w[2 * j + 1], w[2 * j], 0x05040100u);
    lo[j] = __builtin_amdgcn_perm(w[2 * j + 1], w[2 * j], 0x07060302u);
  }
  bhi = __builtin_bit_cast(half8_t, hi);
  blo = __builtin_bit_cast(half8_t, lo);
}

// ---------------------------------------------------------------- score codes
// Biased codes: a score code c is kept as the float y = MAG + c, MAG = 1.5 * 2^23.  The add rounds
// half-even exactly (|x| < 2^22), the clamp works on y, and the bits of y are MAGB + c, so the table
// address of a code is one v_lshl_add of its bits -- no float -> int conversion per score.  The offset m
// is kept in the same form.
constexpr float Q8_MAG = 12582912.0f;
constexpr int Q8_MAGB = 0x4B400000;

// The two score quantisers of the reference (reciprocal multiply, round-half-even, clamp):
// c = q8(q8(st * qk_scale, s_a1) * s_a1 + rel_h + rel_w, s_a2), with c1 = qk_scale / s_a1 and the second
// argument as fma(code1, k12 = s_a1 / s_a2, rh + rw = (rel_h + rel_w) / s_a2) -- 8 instead of 10 VALU per
// score.  NOT bit-exact: pre-scaled terms in another addition order than (code1 * s_a1 + rel_h + rel_w)
// / s_a2, so a code can move by one at a .5 tie (bounded by test_w8a8_stage_local_parity).  The
// pre-quantisation values differ from the reference's by fp32 summation order anyway, so a correctly
// rounded division would buy no parity.  Returns the biased code.  rh and rw are passed apart and added
// here, after q1: summed at the call site, the compiler schedules the score loops differently.
__device__ __forceinline__ float q8_score(int st, float c1, float k12, float rh, float rw) {
  const float q1 = __builtin_amdgcn_fmed3f(__builtin_rintf((float)st * c1), -128.f, 127.f);
  return __builtin_amdgcn_fmed3f(fmaf(q1, k12, rh + rw) + Q8_MAG, Q8_MAG - 128.f, Q8_MAG + 127.f);
}

// q8_score with the zero points z1 (first quantiser) and, folded into rw by the caller together with
// -z1 k12, z2: code1 = clamp(rint(st c1 + z1)), code2 = clamp(rint(fma(code1, k12, rh + rw)))
__device__ __forceinline__ float q8_score_zp(int st, float c1, float z1, float k12, float rh, float rw) {
  const float q1 = __builtin_amdgcn_fmed3f(__builtin_rintf(fmaf((float)st, c1, z1)), -128.f, 127.f);
  return __builtin_amdgcn_fmed3f(fmaf(q1, k12, rh + rw) + Q8_MAG, Q8_MAG - 128.f, Q8_MAG + 127.f);
}

__device__ __forceinline__ float q8max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float q8_max16(const float (&c)[4][4]) {   // v_max3 chain
  float v = q8max3(c[0][0], c[0][1], c[0][2]);
  v = q8max3(v, c[0][3], c[1][0]);
  v = q8max3(v, c[1][1], c[1][2]);
  v = q8max3(v, c[1][3], c[2][0]);
  v = q8max3(v, c[2][1], c[2][2]);
  v = q8max3(v, c[2][3], c[3][0]);
  v = q8max3(v, c[3][1], c[3][2]);
  return fmaxf(v, c[3][3]);
}

// LDS read of the table entry of a biased code y: byte address (bits(y) << 2) + tbase, tbase = ptab +
// 4 (BASE - m_code - MAGB) mod 2^32 (recomputed by the kernels wherever the offset m moves)
__device__ __forceinline__ uint32_t q8_ptab_word(float y, uint32_t tbase) {
  const uint32_t a = ((uint32_t)__builtin_bit_cast(int, y) << 2) + tbase;
  return *(const SAMQ_LDS uint32_t*)(uintptr_t)a;
}

}  // namespace samq
