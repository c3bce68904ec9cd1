// W8A8 attention, generic kernel: any window <= 16 (except SAM's 14, attention_q8_win.h) and any global
// grid up to 64 x 64 (except 64 itself, attention_q8_row64.h).
//
// Grid (images * windows, heads, query tiles of 16 * NWQ); a wave owns 16 queries.  RESIDENT (windows,
// S * S <= KC = 256 keys): all keys staged once by the 13 or 16 waves; otherwise 64-key chunks
// double-buffered through LDS, chunk ch + 1 staged while chunk ch is computed, one barrier per chunk
// (it makes chunk ch + 1 visible and ends every wave's reads of buffer ch & 1 before it is refilled).
// Layout: S^T = K.Q^T per 16-key block (lane = one query ql, keys 16 bb + 4 g + i), so P^T feeds the
// P.V MFMA's B operand from the same registers.  K codes in LDS as [key][q8_kpitch] bytes, V^T as fp16
// [d][key] at pitch KC + 8 halves (a scalar transposed store per element).  Keys are decoded per score
// (key -> (kh, kw), the rel terms from two LDS tables), and the softmax is the direct online form, one
// exp2 per score with the offset moved at every new maximum: by design NOT the table arithmetic of the
// row64 / window kernels (tests pin both).  The score quantisers multiply by the hoisted reciprocals
// (see q8_score for why that costs no parity), here in the reference's own order (v1 + rel_h) + rel_w.
#pragma once

#include "attention_q8_util.h"

namespace samq {

template <int D, bool RESIDENT, int NWQ, int KC, int MAXS, bool ZP = false>
__global__ __launch_bounds__(64 * NWQ) void rel_attention_q8_kernel(typename AttnQ8ParamsOf<ZP>::type p) {
  static_assert(D == 64 || D == 80, "head dim");
  constexpr int QD = D, KPITCH = q8_kpitch<D>();
  constexpr int PARTS = D / 16;                  // 16-byte pieces per token and head
  constexpr int NBUF = RESIDENT ? 1 : 2;
  constexpr int VTP = KC + 8;                    // V^T row pitch (halves)
  __shared__ __attribute__((aligned(16))) int8_t k_lds[NBUF][KC * KPITCH];
  __shared__ __attribute__((aligned(16))) _Float16 vt_lds[NBUF][QD * VTP];
  __shared__ __attribute__((aligned(16))) int8_t q_lds[NWQ][16 * KPITCH];
  __shared__ float rh_lds[NWQ][16 * (MAXS + 1)];
  __shared__ float rw_lds[NWQ][16 * (MAXS + 1)];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int g = lane >> 4;
  const int ql = lane & 15;
  const int qlt = g == 0 ? ql : 0;   // D = 80: K row of the tail fragment (groups 1..3 re-read row 0: a broadcast, no bank conflict)
  const int S = p.S, L = p.L, C = p.C;
  const int head = blockIdx.y;
  int b, wy = 0, wx = 0;
  if (p.window > 0) {
    const int per = p.nwh * p.nww;
    b = blockIdx.x / per;
    wy = p.row0 + (blockIdx.x % per) / p.nww;
    wx = blockIdx.x % p.nww;
  } else {
    b = blockIdx.x;
  }
  const float invS = 1.0f / (float)S;

  // local token index -> (row, col) in the window / grid and validity in the image
  auto tok = [&](int t, int& ty, int& tx) {
    ty = (int)(((float)t + 0.5f) * invS);
    tx = t - ty * S;
  };
  auto tok_ptr = [&](int ty, int tx, bool& inimg) -> const int8_t* {
    const int y = wy * S + ty, x = wx * S + tx;
    inimg = y < p.H && x < p.W;
    return p.qkv + (((int64_t)b * p.H + y) * p.W + x) * (3 * C);
  };

  // ---- stage keys [c0, c0 + KC) of K (codes) and V^T (fp16) into buffer buf
  auto stage = [&](int c0, int buf) {
    for (int u = tid; u < KC * PARTS; u += 64 * NWQ) {
      const int key = u % KC, part = u / KC;
      const int kk = c0 + key;
      u32x4 kc = {0u, 0u, 0u, 0u}, vc = {0u, 0u, 0u, 0u};
      if (kk < L) {
        int ty, tx;
        tok(kk, ty, tx);
        bool inimg;
        const int8_t* tp = tok_ptr(ty, tx, inimg);
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
      *(u32x4*)(&k_lds[buf][key * KPITCH + part * 16]) = kc;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float vf = (float)(int8_t)((vc[e >> 2] >> (8 * (e & 3))) & 0xFFu);
        if constexpr (ZP) vf -= p.z_qkv;   // V as v - z (exact in fp16)
        vt_lds[buf][(part * 16 + e) * VTP + key] = (_Float16)vf;
      }
    }
  };

  // ---- this wave's 16 queries: codes (B operand of S^T = K.Q^T) and the rel-pos terms
  const int q0 = blockIdx.z * (16 * NWQ) + wave * 16;
  const int qt = q0 + ql;
  int qy = 0, qx = 0;
  bool q_ok = false;
  int4v qfrag = {0, 0, 0, 0};
  int4v qtail = {0, 0, 0, 0};                    // D = 80: dims 64..79 (q8_tail)
  if (qt < L) {
    tok(qt, qy, qx);
    bool inimg;
    const int8_t* tp = tok_ptr(qy, qx, inimg);
    q_ok = inimg;
    if (inimg) {
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
  *(int4v*)(&q_lds[wave][ql * KPITCH + g * 16]) = qfrag;
  if constexpr (D == 80)
    if (g == 0) *(int4v*)(&q_lds[wave][ql * KPITCH + 64]) = qtail;
  __builtin_amdgcn_s_waitcnt(0xC07F);   // this wave's query codes are in LDS (wave-private rows: no barrier)
  {
    // rel_h[q][kh] = sum_d (code_q[d] * s_qkv) * Rh[qy - kh + S - 1][d];  rel_w likewise with Rw and
    // the same ROW index qy (the reference's quirk).  16 lanes share one table row.
    const int pairs = 16 * S;
    for (int pi = lane; pi < pairs; pi += 64) {
      const int qi = pi & 15, kk = pi >> 4;
      const int qtt = q0 + qi;
      int ty = 0, tx = 0;
      if (qtt < L) tok(qtt, ty, tx);
      const int ridx = ty - kk + S - 1;
      const float* th = p.relh + (int64_t)ridx * QD;
      const float* tw = p.relw + (int64_t)ridx * QD;
      float ah = 0.f, aw = 0.f;
#pragma unroll 1
      for (int d4 = 0; d4 < QD / 16; ++d4) {
        const u32x4 cw = *(const u32x4*)(&q_lds[wave][qi * KPITCH + d4 * 16]);
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const float4_t h4 = *(const float4_t*)(th + d4 * 16 + e4 * 4);
          const float4_t w4 = *(const float4_t*)(tw + d4 * 16 + e4 * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float qf = (float)(int8_t)((cw[e4] >> (8 * e)) & 0xFFu);
            if constexpr (ZP) qf -= p.z_qkv;   // code - z: exact
            qf *= p.s_qkv;
            ah = fmaf(qf, h4[e], ah);
            aw = fmaf(qf, w4[e], aw);
          }
        }
      }
      rh_lds[wave][qi * (MAXS + 1) + kk] = ah;
      rw_lds[wave][qi * (MAXS + 1) + kk] = aw;
    }
  }

  const int nchunks = (L + 63) / 64;
  float m = -INFINITY, lsum = 0.f;
  float4_t acc[QD / 16];
#pragma unroll
  for (int t = 0; t < QD / 16; ++t) acc[t] = float4_t{0.f, 0.f, 0.f, 0.f};
  const float* rhq = &rh_lds[wave][ql * (MAXS + 1)];
  const float* rwq = &rw_lds[wave][ql * (MAXS + 1)];
  const float inv1 = p.inv_a1, inv2 = p.inv_a2, sa1 = p.s_a1;
  int4v zseed = {0, 0, 0, 0};
  if constexpr (ZP) zseed = q8_zp_seed(p, qfrag, qtail);

  if (RESIDENT) {
    for (int c0 = 0; c0 < L; c0 += KC) stage(c0, 0);   // KC >= L: one pass
  } else {
    stage(0, 0);
  }
  __syncthreads();   // the first keys staged; the rel tables visible

  for (int ch = 0; ch < nchunks; ++ch) {
    const int buf = RESIDENT ? 0 : (ch & 1);
    const int koff = RESIDENT ? ch * 64 : 0;             // key offset inside the staged buffer
    if (!RESIDENT && ch + 1 < nchunks) stage((ch + 1) * 64, buf ^ 1);
    // ---- S^T block scores
    float c2[4][4];
    float cmax = -INFINITY;
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      const int4v kf = *(const int4v*)(&k_lds[buf][(koff + bb * 16 + ql) * KPITCH + g * 16]);
      int4v z = {0, 0, 0, 0};
      if constexpr (ZP) {
        z = q8_zp_ksum(p, kf, zseed);
        if constexpr (D == 80) z = q8_zp_ksum(p, q8_tail(&k_lds[buf][(koff + bb * 16 + qlt) * KPITCH], g), z);
      }
      int4v st = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qfrag, z, 0, 0, 0);
      if constexpr (D == 80)
        st = __builtin_amdgcn_mfma_i32_16x16x64_i8(q8_tail(&k_lds[buf][(koff + bb * 16 + qlt) * KPITCH], g), qtail, st,
                                                   0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = ch * 64 + bb * 16 + 4 * g + i;
        float c = -INFINITY;
        if (key < L) {
          int kh, kw;
          tok(key, kh, kw);
          const float v = (float)st[i] * p.qk_scale;
          if constexpr (ZP) {   // rint(x / s + z), value (code - z) s; the softmax below works on code differences
            const float v1 = (fminf(fmaxf(__builtin_rintf(v * inv1 + p.z_a1), -128.f), 127.f) - p.z_a1) * sa1;
            const float t = (v1 + rhq[kh]) + rwq[kw];
            c = fminf(fmaxf(__builtin_rintf(t * inv2 + p.z_a2), -128.f), 127.f);
          } else {
          const float v1 = fminf(fmaxf(__builtin_rintf(v * inv1), -128.f), 127.f) * sa1;
          const float t = (v1 + rhq[kh]) + rwq[kw];
          c = fminf(fmaxf(__builtin_rintf(t * inv2), -128.f), 127.f);
          }
        }
        c2[bb][i] = c;
        cmax = fmaxf(cmax, c);
      }
    }
    cmax = max_rows4(cmax);
    if (cmax > m) {
      const float alpha = m == -INFINITY ? 0.f : exp2f((m - cmax) * p.k2);
      lsum *= alpha;
#pragma unroll
      for (int t = 0; t < QD / 16; ++t) acc[t] = acc[t] * alpha;
      m = cmax;
    }
    float (&pr)[4][4] = c2;   // probabilities overwrite the score codes in place
    // exp(s_a2 * (c - m)) with c, m integer codes (exact difference); exp2 of a pre-scaled
    // argument is within a few ulps of the reference's exp(x - max x)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pv = c2[bb][i] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((c2[bb][i] - m) * p.k2);
        pr[bb][i] = pv;
        lsum += pv;
      }
    // ---- O^T += V^T . P^T  (two 32-key steps, P split hi + lo)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      half8_t bhi, blo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pv = pr[2 * s2 + (j >> 2)][j & 3];
        const _Float16 h = (_Float16)pv;
        bhi[j] = h;
        blo[j] = (_Float16)(pv - (float)h);
      }
#pragma unroll
      for (int t = 0; t < QD / 16; ++t) {
        const _Float16* vr = &vt_lds[buf][(t * 16 + ql) * VTP + koff + 32 * s2 + 4 * g];
        const half4_t a0 = *(const half4_t*)vr;
        const half4_t a1 = *(const half4_t*)(vr + 16);
        const half8_t af = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bhi, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, blo, acc[t], 0, 0, 0);
      }
    }
    if (!RESIDENT) __syncthreads();   // chunk ch+1 staged; everyone done reading buffer buf
  }

  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  if (q_ok) {
    int8_t* op = p.out + (((int64_t)b * p.H + (wy * S + qy)) * p.W + (wx * S + qx)) * C + head * QD;
    // shift-and-or packing in all three kernels, not q8_pack4: v_cvt_i32_f32 turns a NaN quotient into
    // code 0, v_cvt_pk_u8_f32 into -128
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
