// W8A8 windowed attention (S = SW <= 16; the launcher uses it for SAM's 14 x 14 windows), key rows of 16
// slots.
//
// A workgroup = NWQ query rows of one (window, head): one wave per query row (16 slots, query
// (wave, ql), slots ql >= SW idle), so a wave's rel-pos terms are one MFMA block (q8_rel_block).  The
// whole window's keys are staged once, key (kh, kw) in slot 16 kh + kw (slots kw >= SW zero and
// masked), so a 16-key block is exactly one key row: rel_h is one value per block and rel_w a fixed
// per-lane set (kw = 4 g + i, registers) -- no index decode and no table reads per score.  Scores,
// quantisers, lazy-offset softmax from the P table, P.V and row sums as in the row64 kernel
// (attention_q8_row64.h); masked slots carry the biased code MAG - 400, which reads a zero of the table.
// NWQ < SW: a workgroup takes NWQ of the SW query rows (blockIdx.z = which), each staging the whole
// window's K / V -- 14 x 14 windows of vit_b at B = 1 are 300 (window, head) items on 256 CUs; as 600
// half-items of 7 waves they spread as ~2.3 per CU instead of 44 CUs running two whole items in turn.
// LDS: K rows at Q8_KP, V rows at Q8_VP (conflict-free: attention_q8_util.h); <14, 7> takes 74816
// bytes at both head dims, two workgroups per CU, which leaves no room for the P table: it is built in
// q_lds's bytes after the barrier that ends the prologue's last read of q_lds, and a second barrier
// makes it visible.
#pragma once

#include "attention_q8_util.h"

namespace samq {

template <int D, int SW, int NWQ = SW, bool ZP = false>
// two workgroups per CU: LDS <= 80 KiB and (HIP's second bound = waves per SIMD) <= 512 / (waves / 2) VGPRs
__global__ __launch_bounds__(64 * NWQ, (2 * NWQ + 3) / 4) void rel_attention_q8_win_kernel(typename AttnQ8ParamsOf<ZP>::type p) {
  static_assert(D == 64 || D == 80, "head dim");
  constexpr int QD = D, PARTS = D / 16;                   // 16-byte pieces per token and head
  constexpr int SLOTS = 16 * SW, KP = Q8_KP, VP = Q8_VP;
  static_assert(SW % NWQ == 0, "query rows split evenly");
  constexpr int NCH = (SW + 3) / 4;                        // chunks of up to 4 key rows (64 slots)
  static_assert(SW <= 16, "one window per workgroup");
  __shared__ __attribute__((aligned(16))) int8_t k_lds[SLOTS * KP];
  __shared__ __attribute__((aligned(16))) _Float16 v_lds[SLOTS * VP];
  __shared__ __attribute__((aligned(16))) int8_t q_lds[NWQ][16 * KP];
  __shared__ float rh_lds[NWQ][16 * (SW + 1)];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int g = lane >> 4;
  const int ql = lane & 15;
  const int qlt = g == 0 ? ql : 0;   // D = 80: K row of the tail fragment (groups 1..3 re-read row 0: a broadcast, no bank conflict)
  const int C = p.C;
  const int head = blockIdx.y;
  const int per = p.nwh * p.nww;
  const int b = blockIdx.x / per;
  const int wy = p.row0 + (blockIdx.x % per) / p.nww;
  const int wx = blockIdx.x % p.nww;
  auto tok_ptr = [&](int ty, int tx, bool& inimg) -> const int8_t* {
    const int y = wy * SW + ty, x = wx * SW + tx;
    inimg = y < p.H && x < p.W;
    return p.qkv + (((int64_t)b * p.H + y) * p.W + x) * (3 * C);
  };

  // ---- stage K codes and V (fp16, row-major) of every key slot; pad tokens = q8(qkv bias)
  for (int u = tid; u < SLOTS * PARTS; u += 64 * NWQ) {
    const int slot = PARTS == 4 ? u >> 2 : u / PARTS, part = PARTS == 4 ? u & 3 : u % PARTS;
    const int kh = slot >> 4, kw = slot & 15;
    u32x4 kc = {0u, 0u, 0u, 0u}, vc = {0u, 0u, 0u, 0u};
    if (kh < SW && kw < SW) {
      bool inimg;
      const int8_t* tp = tok_ptr(kh, kw, inimg);
      if (inimg) {
        kc = *(const u32x4*)(tp + C + head * QD + part * 16);
        vc = *(const u32x4*)(tp + 2 * C + head * QD + part * 16);
      } else if constexpr (ZP) {   // pad token: the codes of the bias, or of 0.0
        kc = q8_zp_pad16(p.qkv_bias ? p.qkv_bias + C + head * QD + part * 16 : nullptr, p.s_qkv, p.z_qkv);
        vc = q8_zp_pad16(p.qkv_bias ? p.qkv_bias + 2 * C + head * QD + part * 16 : nullptr, p.s_qkv, p.z_qkv);
      } else if (p.qkv_bias) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kq = (int)aq8(p.qkv_bias[C + head * QD + part * 16 + e], p.s_qkv);
          const int vq = (int)aq8(p.qkv_bias[2 * C + head * QD + part * 16 + e], p.s_qkv);
          kc[e >> 2] |= ((uint32_t)kq & 0xFFu) << (8 * (e & 3));
          vc[e >> 2] |= ((uint32_t)vq & 0xFFu) << (8 * (e & 3));
        }
      }
    }
    *(u32x4*)(&k_lds[slot * KP + part * 16]) = kc;
    half8_t h0, h1;
    if constexpr (ZP) {
      q8_unpack16_zp(vc, h0, h1, p.z_qkv);   // V as v - z
    } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      h0[e] = (_Float16)(float)(int8_t)((vc[e >> 2] >> (8 * (e & 3))) & 0xFFu);
      h1[e] = (_Float16)(float)(int8_t)((vc[2 + (e >> 2)] >> (8 * (e & 3))) & 0xFFu);
    }
    }
    *(half8_t*)(&v_lds[slot * VP + part * 16]) = h0;
    *(half8_t*)(&v_lds[slot * VP + part * 16 + 8]) = h1;
  }

  // ---- this wave's query row qy (queries qx = ql < SW) and its rel-pos terms (table rows qy - k +
  // SW - 1 for both); rel_w for kw = 4 g + i into registers
  const bool q_in = ql < SW;
  const int qy = blockIdx.z * NWQ + wave, qx = q_in ? ql : 0;
  bool q_ok = false;
  int4v qfrag = {0, 0, 0, 0};
  int4v qtail = {0, 0, 0, 0};                    // D = 80: dims 64..79 (q8_tail)
  if (q_in) {
    const int8_t* tp = tok_ptr(qy, qx, q_ok);
    if (q_ok) {
      qfrag = *(const int4v*)(tp + head * QD + g * 16);
      if constexpr (D == 80) qtail = q8_tail(tp + head * QD, g);
    } else if (p.qkv_bias) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int qq = (int)aq8(p.qkv_bias[head * QD + g * 16 + e], p.s_qkv);
        qfrag[e >> 2] |= (qq & 0xFF) << (8 * (e & 3));
      }
      if constexpr (D == 80) qtail = q8_tail_bias(p.qkv_bias + head * QD, p.s_qkv, g);
    }
  }
  *(int4v*)(&q_lds[wave][ql * KP + g * 16]) = qfrag;
  if constexpr (D == 80)
    if (g == 0) *(int4v*)(&q_lds[wave][ql * KP + 64]) = qtail;
  __builtin_amdgcn_s_waitcnt(0xC07F);   // this wave's query codes are in LDS (wave-private rows: no barrier)
  float rwr[4];
  {
    float4_t rh4, rw4;
    if constexpr (ZP) q8_rel_block<D, true>(p, &q_lds[wave][ql * KP], qy, SW, 0, lane, rh4, rw4, p.z_qkv);
    else q8_rel_block<D>(p, &q_lds[wave][ql * KP], qy, SW, 0, lane, rh4, rw4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rwr[i] = rw4[i];
      if (4 * g + i < SW) rh_lds[wave][ql * (SW + 1) + 4 * g + i] = rh4[i];
    }
  }
  __syncthreads();   // K / V staged; this wave's rel_h rows visible; q_lds read for the last time
  static_assert(sizeof(q_lds) >= PTABW * 4, "P table alias");
  uint32_t* ptab = (uint32_t*)&q_lds[0][0];
  const int lazyc = q8_ptab_lazy(p.k2);
  q8_ptab_fill<PTABW_BASE, 64 * NWQ>(ptab, p.k2, lazyc, tid);
  __syncthreads();   // the P table visible
  const float* rhq = &rh_lds[wave][ql * (SW + 1)];

  const float c1 = p.qk_scale * p.inv_a1, inv2 = p.inv_a2, k2 = p.k2, k12 = p.s_a1 * p.inv_a2;
#pragma unroll
  for (int i = 0; i < 4; ++i) rwr[i] *= inv2;
  int4v zseed = {0, 0, 0, 0};
  if constexpr (ZP) {
#pragma unroll
    for (int i = 0; i < 4; ++i) rwr[i] += p.zfold;
    zseed = q8_zp_seed(p, qfrag, qtail);
  }
  const float lazy = (float)lazyc;
  constexpr float MASKC = Q8_MAG - 400.f;        // masked slots: a table entry below PTABW_BASE - 255, P = 0
  uint32_t tbase = 0;
  const uint32_t ptab_addr = (uint32_t)(uintptr_t)(SAMQ_LDS void*)ptab;
  const int trow = ql >> 2, tcol = 4 * (ql & 3);
  const half8_t ones = {1, 1, 1, 1, 1, 1, 1, 1};
  float m = -INFINITY;                           // softmax offset, biased like the codes
  float4_t acc[QD / 16], lacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < QD / 16; ++t) acc[t] = float4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int nb = SW - 4 * ch < 4 ? SW - 4 * ch : 4;   // key rows in this chunk (compile-time after unroll)
    float c[4][4];
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      if (bb >= nb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) c[bb][i] = MASKC;
        continue;
      }
      const int kh = 4 * ch + bb;
      const float rh_row = rhq[kh] * inv2;
      const int4v kf = *(const int4v*)(&k_lds[(kh * 16 + ql) * KP + g * 16]);
      int4v z = {0, 0, 0, 0};
      if constexpr (ZP) {
        z = q8_zp_ksum(p, kf, zseed);
        if constexpr (D == 80) z = q8_zp_ksum(p, q8_tail(&k_lds[(kh * 16 + qlt) * KP], g), z);
      }
      int4v st = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qfrag, z, 0, 0, 0);
      if constexpr (D == 80)
        st = __builtin_amdgcn_mfma_i32_16x16x64_i8(q8_tail(&k_lds[(kh * 16 + qlt) * KP], g), qtail, st, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float cq;
        if constexpr (ZP) cq = q8_score_zp(st[i], c1, p.z_a1, k12, rh_row, rwr[i]);
        else cq = q8_score(st[i], c1, k12, rh_row, rwr[i]);
        c[bb][i] = 4 * g + i < SW ? cq : MASKC;
      }
    }
    const float cmax = max_rows4(q8_max16(c));
    if (cmax > m + lazy) {   // per query column: move the offset, rescale O and l
      const float alpha = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((m - cmax) * k2);
#pragma unroll
      for (int t = 0; t < QD / 16; ++t) acc[t] = acc[t] * alpha;
      lacc = lacc * alpha;
      m = cmax;
      tbase = ptab_addr + 4u * (uint32_t)(PTABW_BASE - (__builtin_bit_cast(int, cmax) - Q8_MAGB) - Q8_MAGB);
    }
    const _Float16* vb = &v_lds[(ch * 64) * VP];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      if (2 * s2 >= nb) continue;   // both key rows of this k32 step are past the window
      uint32_t pw[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pw[j] = q8_ptab_word(c[2 * s2 + (j >> 2)][j & 3], tbase);
      half8_t bhi, blo;
      q8_ptab_unpack(pw, bhi, blo);
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
  }

  if (q_ok) {
    int8_t* op = p.out + (((int64_t)b * p.H + (wy * SW + qy)) * p.W + (wx * SW + qx)) * C + head * QD;
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
}

}  // namespace samq
