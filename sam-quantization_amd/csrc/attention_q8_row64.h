// W8A8 global attention over a 64 x 64 grid (the global blocks of the SAM encoders, 4096 keys).
//
// A workgroup = one query grid row (64 queries, 4 waves x 16); key row kh is chunk kh (64 keys), so the
// height term rel_h is one value per chunk and the width term rel_w a fixed per-lane set (registers).
// Per chunk and wave:
//   S^T = K.Q^T on 4 (D = 80: 8, see q8_tail) x v_mfma_i32_16x16x64_i8, exact int32; lane = query ql,
//       keys 16 bb + 4 g + i;
//   the two score quantisers as biased integer codes (q8_score);
//   online softmax on the codes with a lazy offset (attention_q8_util.h), P from the table;
//   O^T += V^T.P^T on 16x16x32 f16 MFMAs, P split hi + lo (both fp16, |P - hi - lo| ~ 2^-22 |P|), V^T
//       fragments by ds_read_b64_tr_b16 from the row-major fp16 V; the row sums l come from the same
//       MFMAs against an all-ones operand (fp32 sums of the same hi + lo).
// Staging: a chunk's K codes (int8) and V (fp16, row-major: converted once from the codes, or with V16
// copied from the producer's fp16 copy p.v16, two 16-byte pieces per thread and unit, no conversion) go
// through a 2-deep LDS ring with 16-byte stores.  Two register sets: chunk ch + 2 is loaded while chunk
// ch is computed and chunk ch + 1 (loaded one chunk earlier) is stored -- two chunks of math cover each
// load's latency.  One barrier per chunk: it makes chunk ch + 1 visible, and the buffer it was stored to
// was last read before the previous barrier.
// LDS: K rows at Q8_KP, V rows at Q8_VP (conflict-free: attention_q8_util.h); the prologue's query
// staging aliases V buffer 1, which nothing touches until the store of chunk 1 after the prologue
// barrier; no rel_w table in LDS.  51456 bytes at both head dims: three workgroups per CU, so the 768
// workgroups of a vit_b launch are all resident at once.
// D = 80 staging: the 5th piece of each key (dims 64..79) is 64 K pieces + 64 (int8 V) or 128 (fp16 V)
// V pieces per chunk on top of the 256 threads' one piece of dims 0..63 each, so every thread issues
// one more 16-byte load per chunk, its source picked by the wave -- wave 0: K tail of key = lane; int8
// V: wave 1 the V tail; fp16 V: waves 1 / 2 its two halves; the remaining waves repeat wave 0's load (a
// cache hit) and store nothing.  All loads stay unconditional (the last chunks re-load a clamped row),
// so the compiler's waits stay counted.  The tail K fragment read (ds_read_b128 at byte 64 of row ql in
// lane group 0, groups 1..3 all re-reading row 0: a broadcast) is conflict-free too.
#pragma once

#include "attention_q8_util.h"

namespace samq {

template <int D, int NWQ, bool V16 = false, bool ZP = false>
__global__ __launch_bounds__(64 * NWQ, 3) void rel_attention_q8_row64_kernel(typename AttnQ8ParamsOf<ZP>::type p) {
  static_assert(D == 64 || D == 80, "head dim");
  static_assert(!(ZP && V16), "zero points: int8 V only");
  constexpr int QD = D;
  constexpr int G = 64, KC = 64;
  constexpr int KP = Q8_KP, VP = Q8_VP;
  constexpr int NT = 64 * NWQ;
  constexpr int UNITS = KC * 4;                  // 16-byte pieces of dims 0..63 of one chunk's K (and of its V)
  static_assert(UNITS % NT == 0, "staging");
  constexpr int UPT = UNITS / NT;
  static_assert(D == 64 || (NWQ == 4 && KC == 64), "tail staging: one key per lane, roles by wave");
  __shared__ __attribute__((aligned(16))) int8_t k_lds[2][KC * KP];
  __shared__ __attribute__((aligned(16))) _Float16 v_lds[2][KC * VP];
  int8_t(*q_lds)[16 * KP] = (int8_t(*)[16 * KP])(void*)&v_lds[1][0];   // prologue only
  static_assert(NWQ * 16 * KP <= KC * VP * 2, "query staging inside V buffer 1");
  __shared__ float rh_lds[NWQ][16 * (G + 1)];
  __shared__ uint32_t ptab[PTAB];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int g = lane >> 4;
  const int ql = lane & 15;
  const int qlt = g == 0 ? ql : 0;   // D = 80: K row of the tail fragment (groups 1..3 re-read row 0: a broadcast, no bank conflict)
  const int C = p.C;
  const int head = blockIdx.y;
  const int b = blockIdx.x;
  const int qy = p.row0 + blockIdx.z;           // query grid row of this workgroup
  const int lazyc = q8_ptab_lazy(p.k2);
  q8_ptab_fill<PTAB_BASE, NT>(ptab, p.k2, lazyc, tid);   // visible after the first barrier below
  const int qx = wave * 16 + ql;
  const int64_t ts = 3 * (int64_t)C;
  const int8_t* img = p.qkv + (int64_t)b * G * G * ts;

  // ---- K / V staging: piece u = key * 4 + part (16 bytes of dims 16 part .. +15)
  u32x4 kreg[2][UPT], vreg[2][V16 ? 2 * UPT : UPT];
  u32x4 treg[2];                                 // D = 80: this thread's tail piece (role by wave: see above)
  const _Float16* v16img = V16 ? p.v16 + (int64_t)b * G * G * C : nullptr;
  // tail source of key = lane in key row 0, bytes; key rows are G tokens apart
  const int8_t* tsrc = nullptr;
  int64_t tstep = 0;
  const int trole = V16 ? (wave == 3 ? 0 : wave) : (wave & 1);   // 0: K; 1: V (fp16 V: first half); 2: fp16 V second half
  if constexpr (D == 80) {
    if (V16 && trole > 0) {
      tsrc = (const int8_t*)(v16img + (int64_t)lane * C + head * QD + 64 + 8 * (trole - 1));
      tstep = (int64_t)G * C * 2;
    } else {
      tsrc = img + (int64_t)lane * ts + (1 + trole) * C + head * QD + 64;
      tstep = (int64_t)G * ts;
    }
  }
  auto load = [&](int kh, int r) {
    if constexpr (D == 80) treg[r] = *(const u32x4*)(tsrc + kh * tstep);
#pragma unroll
    for (int j = 0; j < UPT; ++j) {
      const int u = tid + j * NT, key = u >> 2, part = u & 3;
      const int8_t* tp = img + ((int64_t)kh * G + key) * ts + head * QD + part * 16;
      kreg[r][j] = *(const u32x4*)(tp + C);
      if constexpr (V16) {
        const _Float16* vp = v16img + ((int64_t)kh * G + key) * C + head * QD + part * 16;
        vreg[r][2 * j] = *(const u32x4*)vp;
        vreg[r][2 * j + 1] = *(const u32x4*)(vp + 8);
      } else {
        vreg[r][j] = *(const u32x4*)(tp + 2 * C);
      }
    }
  };
  auto store = [&](int buf, int r) {
    if constexpr (D == 80) {
      if constexpr (V16) {
        if (wave == 0) *(u32x4*)(&k_lds[buf][lane * KP + 64]) = treg[r];
        else if (wave < 3) *(u32x4*)(&v_lds[buf][lane * VP + 64 + 8 * (wave - 1)]) = treg[r];
      } else if (wave == 0) {
        *(u32x4*)(&k_lds[buf][lane * KP + 64]) = treg[r];
      } else if (wave == 1) {
        half8_t h0, h1;
        if constexpr (ZP) q8_unpack16_zp(treg[r], h0, h1, p.z_qkv);
        else q8_unpack16(treg[r], h0, h1);
        *(half8_t*)(&v_lds[buf][lane * VP + 64]) = h0;
        *(half8_t*)(&v_lds[buf][lane * VP + 64 + 8]) = h1;
      }
    }
#pragma unroll
    for (int j = 0; j < UPT; ++j) {
      const int u = tid + j * NT, key = u >> 2, part = u & 3;
      *(u32x4*)(&k_lds[buf][key * KP + part * 16]) = kreg[r][j];
      if constexpr (V16) {
        *(u32x4*)(&v_lds[buf][key * VP + part * 16]) = vreg[r][2 * j];
        *(u32x4*)(&v_lds[buf][key * VP + part * 16 + 8]) = vreg[r][2 * j + 1];
      } else {
        half8_t h0, h1;
        if constexpr (ZP) q8_unpack16_zp(vreg[r][j], h0, h1, p.z_qkv);   // V as v - z
        else q8_unpack16(vreg[r][j], h0, h1);
        *(half8_t*)(&v_lds[buf][key * VP + part * 16]) = h0;
        *(half8_t*)(&v_lds[buf][key * VP + part * 16 + 8]) = h1;
      }
    }
  };
  load(0, 0);
  load(1, 1);

  // ---- this wave's 16 queries (codes) and their rel-pos terms (q8_rel_block, table rows qy - k + 63
  // for both).  Lane (g, ql) gets the terms of query ql at k = 16 bb + 4 g + i: rel_w straight into the
  // registers the score loop reads, rel_h into LDS (one value per key row per chunk)
  const int4v qfrag = *(const int4v*)(img + ((int64_t)qy * G + qx) * ts + head * QD + g * 16);
  *(int4v*)(&q_lds[wave][ql * KP + g * 16]) = qfrag;
  int4v qtail = {0, 0, 0, 0};
  if constexpr (D == 80) {
    qtail = q8_tail(img + ((int64_t)qy * G + qx) * ts + head * QD, g);
    if (g == 0) *(int4v*)(&q_lds[wave][ql * KP + 64]) = qtail;
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);   // this wave's query codes are in LDS (wave-private rows: no barrier)
  float rwr[4][4];
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) {
    float4_t rh4, rw4;
    if constexpr (ZP) q8_rel_block<D, true>(p, &q_lds[wave][ql * KP], qy, G, bb, lane, rh4, rw4, p.z_qkv);
    else q8_rel_block<D>(p, &q_lds[wave][ql * KP], qy, G, bb, lane, rh4, rw4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rh_lds[wave][ql * (G + 1) + 16 * bb + 4 * g + i] = rh4[i];
      rwr[bb][i] = rw4[i];
    }
  }
  store(0, 0);
  __syncthreads();   // chunk 0 staged; the rel_h rows and the P table visible; q_lds dead
  const float* rhq = &rh_lds[wave][ql * (G + 1)];

  const float c1 = p.qk_scale * p.inv_a1, inv2 = p.inv_a2, k2 = p.k2, k12 = p.s_a1 * p.inv_a2;
#pragma unroll
  for (int bb = 0; bb < 4; ++bb)
#pragma unroll
    for (int i = 0; i < 4; ++i) rwr[bb][i] *= inv2;
  int4v zseed = {0, 0, 0, 0};
  if constexpr (ZP) {
#pragma unroll
    for (int bb = 0; bb < 4; ++bb)
#pragma unroll
      for (int i = 0; i < 4; ++i) rwr[bb][i] += p.zfold;
    zseed = q8_zp_seed(p, qfrag, qtail);
  }
  const float lazy = (float)lazyc;
  const int trow = ql >> 2, tcol = 4 * (ql & 3);
  const half8_t ones = {1, 1, 1, 1, 1, 1, 1, 1};
  float m = -INFINITY;                           // softmax offset, biased like the codes
  uint32_t tbase = 0;
  const uint32_t ptab_addr = (uint32_t)(uintptr_t)(SAMQ_LDS void*)ptab;
  float4_t acc[QD / 16], lacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < QD / 16; ++t) acc[t] = float4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll 2
  for (int ch = 0; ch < G; ++ch) {
    const int buf = ch & 1;
    load(ch + 2 < G ? ch + 2 : G - 1, buf);      // register set of chunk ch (stored one chunk ago)
    const float rh_row = rhq[ch] * inv2;
    float c[4][4];
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      const int4v kf = *(const int4v*)(&k_lds[buf][(bb * 16 + ql) * KP + g * 16]);
      int4v z = {0, 0, 0, 0};
      if constexpr (ZP) {
        z = q8_zp_ksum(p, kf, zseed);
        if constexpr (D == 80) z = q8_zp_ksum(p, q8_tail(&k_lds[buf][(bb * 16 + qlt) * KP], g), z);
      }
      int4v st = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qfrag, z, 0, 0, 0);
      if constexpr (D == 80)
        st = __builtin_amdgcn_mfma_i32_16x16x64_i8(q8_tail(&k_lds[buf][(bb * 16 + qlt) * KP], g), qtail, st, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (ZP) c[bb][i] = q8_score_zp(st[i], c1, p.z_a1, k12, rh_row, rwr[bb][i]);
        else c[bb][i] = q8_score(st[i], c1, k12, rh_row, rwr[bb][i]);
      }
    }
    const float cmax = max_rows4(q8_max16(c));
    if (cmax > m + lazy) {   // per query column: move the offset, rescale O and l
      const float alpha = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((m - cmax) * k2);
#pragma unroll
      for (int t = 0; t < QD / 16; ++t) acc[t] = acc[t] * alpha;
      lacc = lacc * alpha;
      m = cmax;
      tbase = ptab_addr + 4u * (uint32_t)(PTAB_BASE - (__builtin_bit_cast(int, cmax) - Q8_MAGB) - Q8_MAGB);
    }
    uint32_t pw[2][8];
#pragma unroll
    for (int j = 0; j < 16; ++j) pw[j >> 3][j & 7] = q8_ptab_word(c[j >> 2][j & 3], tbase);
    const _Float16* vb = &v_lds[buf][0];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      half8_t bhi, blo;
      q8_ptab_unpack(pw[s2], bhi, blo);
#pragma unroll
      for (int t = 0; t < QD / 16; ++t) {
        const _Float16* a0 = vb + (32 * s2 + 4 * g + trow) * VP + t * 16 + tcol;
        const half4_t lo = __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((SAMQ_LDS short4_t*)a0));
        const half4_t hi = __builtin_bit_cast(
            half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((SAMQ_LDS short4_t*)(a0 + 16 * VP)));
        const half8_t af = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bhi, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, blo, acc[t], 0, 0, 0);
      }
      lacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, bhi, lacc, 0, 0, 0);
      lacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, blo, lacc, 0, 0, 0);
    }
    store(buf ^ 1, buf ^ 1);                    // chunk ch + 1 (register set (ch + 1) & 1; the last is a dummy); the other
    __syncthreads();                            // buffer was last read before the previous barrier
  }

  int8_t* op = p.out + (((int64_t)b * G + qy) * G + qx) * C + head * QD;
  const float lsum = lacc[0];
#pragma unroll
  for (int t = 0; t < QD / 16; ++t) {
    uint32_t w = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (ZP) {
        const float o = acc[t][i] / lsum * p.s_qkv;
        w |= ((uint32_t)(int)q8_exact_zp(o, p.s_out, 1.0f / p.s_out, p.z_out) & 0xFFu) << (8 * i);
        continue;
      }
      const float o = acc[t][i] / lsum * p.s_qkv;
      w |= ((uint32_t)(int)aq8(o, p.s_out) & 0xFFu) << (8 * i);
    }
    *(uint32_t*)(op + t * 16 + 4 * g) = w;
  }
}

}  // namespace samq
