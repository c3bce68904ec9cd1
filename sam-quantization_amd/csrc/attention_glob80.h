// Global attention for the ViT-H global blocks on the 32x32 MFMA.  Included by attention.hip only.
//
// ViT-H global blocks (64 x 64 grid, head dim 80) on v_mfma_f32_32x32x16_f16: the 32x32 form
// issues half the MFMA instructions per FLOP of 16x16x32 (each holds the SIMD's vector issue for
// 8 of its 32 cycles, MI355X_MICROARCH.md constants) and D = 80 is 5 k16-steps, no padding.
//  * a wave owns one query tile of 32 queries of ONE grid row qh (so the width table row
//    qh - kw + 63 is one A operand for the whole tile: reference quirk 1 keeps both tables on qh);
//    8 waves = 4 grid rows per workgroup, 16 workgroups per (image, head), one workgroup per CU;
//  * key row kh (64 keys) = two 32-key tiles: S^T = K.Q^T + TW (5 MFMAs each, TW[kt] = log2e q.Rw
//    as the C input, computed once per tile by the same MFMA form); TH[q, kh] = log2e q.Rh, fp16-
//    rounded like the reference's rel_h, kept per wave in LDS and added to the C input together
//    with the softmax offset (see coff below);
//  * a lane holds 32 scores of ONE query (its partner lane ^ 32 the other 32): the row max is
//    in-register + one cross-lane step; lazy exp2 offset (moves only past +8); P stays in the
//    score registers' order, which IS the B operand of O^T += V^T . P^T (k-slot 8h + j <-> key
//    16u + 4h + j (j < 4) / 16u + 8 + 4h + j - 4);
//  * V^T fragments by ds_read_b64_tr_b16 from 4-key x 32-dim chunks (256 contiguous bytes per
//    read group: conflict-free); d-block 2 covers dims 64..95, its rows 80..95 read as 1.0 (a
//    ones region per ring slot, see the V layout below) so the same MFMAs produce the softmax row
//    sums (no extra MFMA, no VALU sum);
//  * K pieces lane-linear (lane l of piece (kt, s) = key 32 kt + l % 32, dims 16 s + 8 (l / 32):
//    the A fragment read is ds_read_b128 at l * 16); key rows stream through a 5-slot LDS ring
//    (20 KiB of K / V per row, LDS-DMA, 20 pieces over 8 waves), two barriers per key row (the
//    two-group ping-pong below), the next row's Q.K^T MFMAs issued ahead of the current row's
//    softmax.
#pragma once

#include "attention_util.h"

namespace samq {

__global__ __launch_bounds__(512, 1) void glob80_attention_kernel(AttnParams p) {
  constexpr int D = 80, S = 64, KS = 5;
  constexpr int NSLOT = 5;                        // key-row ring slots
  // V of a key row (round 4): dims 0..63 (16 key quads x 512 B) | dims 64..79 (16 quads x 128 B) |
  // 128 B pad | 2 KiB of fp16 ones written once per slot, so the lanes of d-block 2 that hold rows
  // 80..95 (the softmax row sums) read 1.0 from LDS at their own base (+2176: the other 32 banks)
  // instead of masking 4 dwords per P.V step (the round-3 layout: 16 key quads x (256 + 256 + 128 B)
  // interleaved, rows 80..95 forced to 1.0 in registers).
  constexpr int VB = 10 * 1024;                   // V dims 0..63
  constexpr int V2B = 18 * 1024;                  // V dims 64..79
  constexpr int ONESB = V2B + 2048 + 128;         // the ones (+2176 from V2B)
  constexpr int ROWB = ONESB + 2048;              // one key row's ring slot
  constexpr int THB = 64 * 32 * 2;                // per wave: fp16 TH[kh][q]
  __shared__ __attribute__((aligned(16))) char smem[NSLOT * ROWB + 8 * THB];
  static_assert(NSLOT * ROWB + 8 * THB <= 160 * 1024, "LDS");

  _Float16* th_lds = (_Float16*)(smem + NSLOT * ROWB);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2;                       // waves w, w + 4 share a SIMD
  const int l32 = lane & 31, h = lane >> 5;
  // XCD-aware 1-D grid: the 16 query blocks of one (image, head) on one XCD (shared K/V in its L2)
  const int nqb = p.nqb, pairs = p.heads * p.units;
  const int xcd = blockIdx.x & 7, kk = blockIdx.x >> 3;
  const int pair = xcd * (pairs >> 3) + kk / nqb;
  const int qblk = kk % nqb;
  const int head = pair % p.heads;
  const int b = pair / p.heads;
  const int C = p.C;
  const int qh = 4 * qblk + (wave >> 1);           // this wave's query grid row
  const int qw0 = 32 * (wave & 1);
  const _Float16* img = p.qkv + (int64_t)b * S * S * p.tok_stride;

  // ---- K / V staging: 20 pieces per key row; wave w issues pieces w, w + 8 (, w + 16 for w < 4)
  constexpr int NI = 3;
  const int npc = wave < 4 ? 3 : 2;
  const _Float16* src0[NI];
  int dst[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int v = wave + 8 * i;
    int key, dim;
    if (v < 10) {                                  // K piece (kt, s): lane-linear A fragments
      key = 32 * (v / 5) + l32;
      dim = C + 16 * (v % 5) + 8 * h;
    } else {                                       // V: dims 0..63 (pieces 10..17), 64..79 (18, 19)
      const int gl = 64 * (v - 10) + lane;
      if (v < 18) {                                // 16 key quads x (256 + 256 B)
        const int kq = gl >> 5, w = gl & 31;
        key = 4 * kq + ((w & 15) >> 2);
        dim = 2 * C + 32 * (w >> 4) + 8 * (w & 3);
      } else {                                     // 16 key quads x 128 B
        const int g2 = gl - 512, kq = g2 >> 3, w = g2 & 7;
        key = 4 * kq + (w >> 1);
        dim = 2 * C + 64 + 8 * (w & 1);
      }
      key = key < S ? key : S - 1;
    }
    src0[i] = img + (int64_t)key * p.tok_stride + head * D + dim;
    dst[i] = v * 1024;
  }
  const int64_t rowstride = (int64_t)S * p.tok_stride;
  auto issue = [&](int kh, int slot) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      if (i < npc)
        __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)(src0[i] + kh * rowstride),
                                         (SAMQ_LDS void*)(smem + slot * ROWB + dst[i]), 16, 0, 0);
  };
#pragma unroll
  for (int r = 0; r < NSLOT - 1; ++r) issue(r, r);

  // ---- Q^T fragments (B operand): lane = query qw0 + l32, dims 16 s + 8 h (fp16(q * scale * log2e))
  const float qscale = p.scale * LOG2E;
  half8_t qf[KS];
  {
    const _Float16* qp = img + ((int64_t)qh * S + qw0 + l32) * p.tok_stride + head * D + 8 * h;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      half8_t v = *(const half8_t*)(qp + 16 * s);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (_Float16)__builtin_fmaf((float)v[j], qscale, 0.0f);
      qf[s] = v;
    }
  }
  // ---- rel-pos terms: TW[kt] (score layout, the C input) and TH -> LDS (fp16, per wave)
  const float inv_scale = 1.0f / p.scale;
  float16_t tw[2];
  _Float16* thw = th_lds + wave * (64 * 32);
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const _Float16* tab = which ? p.relw : p.relh;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const int r = qh - (32 * kt + l32) + S - 1;   // table row of this lane's A row (key column / key row)
      const _Float16* rp = tab + (int64_t)r * D + 8 * h;
      float16_t a = {};
#pragma unroll
      for (int s = 0; s < KS; ++s) a = mfma32(*(const half8_t*)(rp + 16 * s), qf[s], a);
      a = a * inv_scale;
      if (which) {
        tw[kt] = a;
      } else {
#pragma unroll
        for (int r2 = 0; r2 < 16; ++r2) {
          const int kh = 32 * kt + 8 * (r2 >> 2) + 4 * h + (r2 & 3);
          thw[kh * 32 + l32] = (_Float16)a[r2];
        }
      }
    }
  }

  // ---- V^T fragment addresses (ds_read_b64_tr_b16): lane 4q + p of its 16-lane group reads
  // key 4 kq + q, dims 16 g16 + 4p .. of the chunk; d-block 2 lanes g16 = 1 (dims 80..95) read
  // the slot's ones
  const int i16 = lane & 15, g16 = (lane >> 4) & 1;
  const int tq = i16 >> 2, tp = i16 & 3;
  constexpr int QB = 512, QB2 = 128;   // bytes per key quad (dims 0..63 / 64..79)
  const uint32_t vb01 = lds_addr(smem + VB) + h * QB + tq * 64 + g16 * 32 + tp * 8;
  const uint32_t vb2 = lds_addr(smem + V2B) + h * QB2 + tq * 32 + tp * 8 + g16 * (ONESB - V2B);
  {   // the ones of every ring slot (read only after the barrier below)
    const u32x4 one4 = {0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u};
    for (int i = tid; i < NSLOT * 128; i += 512)
      *(u32x4*)(smem + (i >> 7) * ROWB + ONESB + (i & 127) * 16) = one4;
  }

  float16_t o[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) o[d] = float16_t{};
  float m = -INFINITY;
  float16_t sc[2];
  half8_t pb[2][2];

  half8_t kf[2][KS];
  auto kread = [&](const char* kb) {   // K fragments of a key row (A operands, lane-linear pieces)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s = 0; s < KS; ++s) kf[kt][s] = *(const half8_t*)(kb + (kt * 5 + s) * 1024 + lane * 16);
  };
  // coff (round 4): the next row's TH and softmax offset enter its Q.K^T as part of the C input
  // (C = TW + (TH[kh] - offset), a per-lane scalar added in the MFMA segment), so the softmax
  // segment -- the longer of the two -- runs exp2 straight on the scores (32 fewer v_sub per row
  // than subtracting the offset there): 204.1 vs 209.6 us per 2-image launch, outputs within 3e-5
  // (profiles/r4_i.attn.log)
  float coff = (float)thw[l32];   // TH of the next row (here row 0) minus the offset baked into its scores
  auto qk = [&] {   // S^T = K . Q^T + TW + coff for the two 32-key tiles of a key row
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      float16_t a = tw[kt] + coff;
#pragma unroll
      for (int s = 0; s < KS; ++s) a = mfma32(kf[kt][s], qf[s], a);
      sc[kt] = a;
    }
  };
  // Online softmax (exp2 domain), lane = one query, 32 of its 64 keys.  P is computed with the
  // offset m of the PREVIOUS rows, so the exp2s do not wait for this row's max (whose reduction +
  // cross-lane step + compare is a serial chain): the max runs beside them and only decides
  //  * m moves by > 8 (lazy offset): applied after this row's P.V, before the next row's P
  //    (O *= exp2(m - m_new) there; P and O of this row share the old offset);
  //  * this row's P could exceed 2^15 (fp16 range): rare slow path, O rescaled and P recomputed
  //    with the new offset now (always taken for row 0, m = -inf).
  float m_pend = -INFINITY;
  bool pend = false;
  // moff = the offset baked into the current row's scores (m after the pending move, 0 for row 0
  // whose m is -inf); the scores are then s + TH - moff and P = exp2(score)
  float moff = 0.f;
  auto softmax = [&](int kh) {
    if (__any(pend)) {   // last row's deferred offset move (moff already includes it)
      const float alpha = pend ? __builtin_amdgcn_exp2f(m - m_pend) : 1.0f;
      m = pend ? m_pend : m;
#pragma unroll
      for (int d = 0; d < 3; ++d) o[d] = o[d] * alpha;
      pend = false;
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) pb[kt][u][j] = (_Float16)__builtin_amdgcn_exp2f(sc[kt][8 * u + j]);
    // fence: keep the fast-path exp2s ahead of the max chain (the compiler otherwise sinks them
    // into the not-unsafe branch, behind the serial max3 / permlane / compare chain)
    asm volatile("" : "+v"(pb[0][0]), "+v"(pb[0][1]), "+v"(pb[1][0]), "+v"(pb[1][1]));
    float mx = max3f(sc[0][0], sc[0][1], sc[0][2]);
    float my = max3f(sc[1][0], sc[1][1], sc[1][2]);
#pragma unroll
    for (int r = 3; r + 1 < 16; r += 2) {
      mx = max3f(mx, sc[0][r], sc[0][r + 1]);
      my = max3f(my, sc[1][r], sc[1][r + 1]);
    }
    mx = max3f(mx, my, fmaxf(sc[0][15], sc[1][15]));
    {   // lane ^ 32 (the query's other 32 keys): one VALU permlane swap instead of an LDS bpermute
        // (v_permlane32_swap of mx with itself: result 0 holds mx[l & 31], result 1 mx[32 + (l & 31)])
      const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(int, mx), __builtin_bit_cast(int, mx),
                                                       false, false);
      mx = fmaxf(__builtin_bit_cast(float, (int)sw[0]), __builtin_bit_cast(float, (int)sw[1]));
    }
    const float mrow = mx + moff;
    const bool unsafe = !(mrow <= m + 15.0f);   // (m = -inf: unsafe)
    if (__any(unsafe)) {
      const float mnew = unsafe ? mrow : m;
      const float alpha = unsafe ? __builtin_amdgcn_exp2f(m - mnew) : 1.0f;
      m = mnew;
#pragma unroll
      for (int d = 0; d < 3; ++d) o[d] = o[d] * alpha;
      const float delta = m - moff;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int j = 0; j < 8; ++j) pb[kt][u][j] = (_Float16)__builtin_amdgcn_exp2f(sc[kt][8 * u + j] - delta);
    }
    pend = mrow > m + 8.0f;
    m_pend = mrow;
    if (kh + 1 < S) {
      const float th = (float)thw[(kh + 1) * 32 + l32];
      moff = pend ? m_pend : m;
      coff = th - moff;
    }
  };
  // V^T fragments of k16-step t = (kt, u): six ds_read_b64_tr_b16 (lo / hi key quads x 3 d-blocks)
  auto vread = [&](auto tc, uint32_t rb, half4_t (&lo)[3], half4_t (&hi)[3]) {
    constexpr int t = decltype(tc)::value;
    constexpr int KQ = 8 * (t >> 1) + 4 * (t & 1);   // key quad of slot j < 4 (+h); j >= 4: +2
    lo[0] = ds_read_tr16_off<KQ * QB>(vb01 + rb);
    hi[0] = ds_read_tr16_off<(KQ + 2) * QB>(vb01 + rb);
    lo[1] = ds_read_tr16_off<KQ * QB + 256>(vb01 + rb);
    hi[1] = ds_read_tr16_off<(KQ + 2) * QB + 256>(vb01 + rb);
    lo[2] = ds_read_tr16_off<KQ * QB2>(vb2 + rb);
    hi[2] = ds_read_tr16_off<(KQ + 2) * QB2>(vb2 + rb);
  };
  auto pv = [&](int slot) {   // O^T += V^T . P^T: 4 k16-steps x 3 d-blocks, next step's reads in flight
    const uint32_t rb = slot * ROWB;
    half4_t lo[2][3], hi[2][3];
    vread(std::integral_constant<int, 0>{}, rb, lo[0], hi[0]);
    static_for<4>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      constexpr int cb = t & 1;
      if constexpr (t + 1 < 4) {
        vread(std::integral_constant<int, t + 1>{}, rb, lo[cb ^ 1], hi[cb ^ 1]);
        asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(lo[cb][0]), "+v"(hi[cb][0]), "+v"(lo[cb][1]), "+v"(hi[cb][1]),
                     "+v"(lo[cb][2]), "+v"(hi[cb][2]));
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo[cb][0]), "+v"(hi[cb][0]), "+v"(lo[cb][1]), "+v"(hi[cb][1]),
                     "+v"(lo[cb][2]), "+v"(hi[cb][2]));
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const half8_t va = {lo[cb][d][0], lo[cb][d][1], lo[cb][d][2], lo[cb][d][3],
                            hi[cb][d][0], hi[cb][d][1], hi[cb][d][2], hi[cb][d][3]};
        o[d] = mfma32(va, pb[t >> 1][t & 1], o[d]);
      }
    });
  };

  // ---- key-row loop as a two-group ping-pong (MI355X_MICROARCH.md "Two waves per SIMD"): per
  // key row a VALU segment (softmax of row kh + the K fragment reads of row kh+1) and an MFMA
  // segment (P.V of row kh, Q.K^T of row kh+1), one barrier apart; waves 4..7 (group 1) run one
  // barrier behind waves 0..3, so each SIMD pairs one wave's softmax with its partner's MFMAs.
  // Barrier n: group 0's VALU segment of row kh lies between barriers 2kh-1 and 2kh, its MFMA
  // segment between 2kh and 2kh+1; group 1's one barrier later.  Ring of 5 slots, row r in slot
  // r % 5:
  //  * row kh+4 is staged at the start of the MFMA segment of row kh into row kh-1's slot, whose
  //    last reads (group 1's P.V of row kh-1) ended at that segment's opening barrier;
  //  * row r is first read by group 0's VALU segment of row r-1 (after barrier 2r-3), so every
  //    wave retires its pieces of row r before barrier 2r-3: group 0 at the end of its MFMA
  //    segment of row r-2, group 1 at the end of its VALU segment of row r-2.
  // The asm fences pin the softmax results and K fragments to their segment (the compiler would
  // otherwise sink the exp2s past the barrier into the MFMA segment).
  wait_vmcnt<0>();
  __syncthreads();   // rows 0..3 landed; TH visible
  kread(smem);
  qk();
  if (grp) __builtin_amdgcn_s_barrier();
  // segment fences: empty volatile asm that "redefines" the registers crossing a barrier, so the
  // compiler can neither hoist the next row's softmax into the MFMA segment nor sink either
  // segment's work across its barrier
  auto fence_sc = [&] {
    asm volatile("" : "+v"(sc[0]), "+v"(sc[1]), "+v"(o[0]), "+v"(o[1]), "+v"(o[2]) :: "memory");
  };
  auto fence_pk = [&] {
    asm volatile("" : "+v"(pb[0][0]), "+v"(pb[0][1]), "+v"(pb[1][0]), "+v"(pb[1][1]), "+v"(kf[0][0]),
                 "+v"(kf[0][1]), "+v"(kf[0][2]), "+v"(kf[0][3]), "+v"(kf[0][4]) :: "memory");
    asm volatile("" : "+v"(kf[1][0]), "+v"(kf[1][1]), "+v"(kf[1][2]), "+v"(kf[1][3]), "+v"(kf[1][4]),
                 "+v"(o[0]), "+v"(o[1]), "+v"(o[2]) :: "memory");
  };
  // ring slots as rotating wave-uniform counters (no per-row modulo); constant vmcnt counts per
  // group: group 0 (waves 0..3) issues 3 pieces per row, group 1 two
  static_assert(NI == 3, "vmcnt counts below: 3 / 2 pieces per row for group 0 / 1");
  int j = 0;   // kh % NSLOT
  for (int kh = 0; kh < S; ++kh) {
    const int j1 = j == NSLOT - 1 ? 0 : j + 1, j4 = j == 0 ? NSLOT - 1 : j - 1;
    fence_sc();
    softmax(kh);
    if (kh + 1 < S) kread(smem + j1 * ROWB);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    fence_pk();
    if (grp && kh + 2 < S) {   // row kh+2 (row kh+3 newer)
      if (kh + 3 < S) wait_vmcnt<2>();
      else wait_vmcnt<0>();
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    fence_pk();
    __builtin_amdgcn_s_setprio(1);
    // row kh+4 into row kh-1's slot, ahead of the P.V step's V^T reads
    if (kh + 4 < S) issue(kh + 4, j4);
    pv(j);
    if (kh + 1 < S) qk();
    fence_sc();
    __builtin_amdgcn_s_setprio(0);
    if (!grp && kh + 2 < S) {   // row kh+2 (rows kh+3, kh+4 newer)
      if (kh + 4 < S) wait_vmcnt<6>();
      else if (kh + 3 < S) wait_vmcnt<3>();
      else wait_vmcnt<0>();
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    j = j1;
  }
  if (!grp) __builtin_amdgcn_s_barrier();   // balance group 1's extra barrier

  // ---- normalise + store: lane = query (qh, qw0 + l32), dims 32 db + 8 c + 4 h .. + 3
  const float inv = 1.0f / o[2][8];
  const int64_t dst_tok = (((int64_t)b * p.H + qh) * p.W + qw0 + l32) * C + head * D;
#pragma unroll
  for (int db = 0; db < 3; ++db)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (db == 2 && c >= 2) continue;
      const float4_t v = {o[db][4 * c], o[db][4 * c + 1], o[db][4 * c + 2], o[db][4 * c + 3]};
      attn_store4(p, dst_tok + 32 * db + 8 * c + 4 * h, v * inv);
    }
}

}  // namespace samq
