// Attention with decomposed relative-position bias, the general kernel: every grid side the
// library accepts (resident for S <= 16, streaming for S = 32 / 64), rel-pos tables or precomputed
// bias tensors.  Included by attention.hip only.
//
// Structure (gfx950, wave64, v_mfma_f32_16x16x32_f16, 7-8 waves per workgroup = 2 waves/SIMD):
//  * work unit = (window or image, head, block of query tiles); a query tile is 16 queries of
//    ONE grid row (rows padded to SP = 16 / 32 / 64 slots), so a tile has one query row qh;
//  * keys are consumed one GRID ROW at a time (SP slots).  For key row kh the scores are
//        s[q, kw] = q.k * scale + TH[q, kh] + TW[q, kw]
//    TW[q, kw] = q . Rw[qh - kw + S - 1] is identical for every key row: it is computed once per
//    query tile by MFMA directly in the score-tile register layout and fed as the C input of
//    every Q.K^T; TH[q, kh] = q . Rh[qh - kh + S - 1] is constant along the row, so it is folded
//    into the running max instead of being added per score.  (Both tables are indexed by the
//    query ROW qh: reference quirk 1.)
//  * scores are computed transposed (S^T = K . Q^T): each lane owns one query, row reductions are
//    in-register + 2 cross-lane steps; P feeds O^T += V^T . P^T as the B operand with a permuted
//    k order that V^T supplies through ds_read_b64_tr_b16 from the row-major V tile;
//  * K / V rows reach LDS by global_load_lds (no VGPR round trip): windows (S <= 16) are staged
//    whole before the loop (no barrier inside it); global attention streams key rows through a
//    3-deep LDS ring with counted vmcnt and one raw s_barrier per row;
//  * online softmax in the exp2 domain with f32 statistics; the O rescale is skipped when no
//    query of the wave raised its max (alpha == 1 exactly, bit-identical results).
#pragma once

#include "attention_util.h"

namespace samq {

constexpr int REL_QT = 2;   // query tiles per wave (the launcher sizes the grid by it)

template <int D, int SP, int NW, bool RESIDENT, bool PRECOMP, int RS = 16, int SC = 0>
__global__ __launch_bounds__(64 * NW, 1) void rel_attention_kernel(AttnParams p) {
  constexpr int QT = REL_QT;
  constexpr int KT = SP / 16;                  // key tiles per key row
  constexpr int DT = D / 16;                   // output d tiles
  constexpr int KS = (D + 31) / 32;            // k32 steps of Q.K^T (D=80 -> 3, last half-zero)
  constexpr int D8 = D / 8;                    // 16-byte chunks per token
  constexpr int ROWB = SP * D * 2;             // bytes of one key row (K or V) in LDS
  // RESIDENT: the keys of the whole (<= RS x RS) grid packed with row pitch S, plus 16 - S slack
  // keys so the 16-slot tile of the last row stays in bounds (slots >= S are masked)
  constexpr int RKEYS = RS * RS + 16 - RS;
  constexpr int UNIT_CHUNKS = RESIDENT ? 2 * RKEYS * D8 : 2 * SP * D8;
  constexpr int NI = (UNIT_CHUNKS + 64 * NW - 1) / (64 * NW);   // glds per wave per unit
  constexpr int BUFB = NI * NW * 1024;
  constexpr int NBUF = RESIDENT ? 1 : 3;
  constexpr int TH_ROWS = RESIDENT ? 16 : SP;   // >= 16: the TH tile writes 16 rows
  constexpr int TH_BYTES = NW * QT * TH_ROWS * 16 * 4;
  static_assert(D == 64 || D == 80, "head dim");
  static_assert(!RESIDENT || SP == 16, "resident mode holds <= 16 rows of 16 slots");

  __shared__ __attribute__((aligned(16))) char smem[NBUF * BUFB + TH_BYTES];
  float* th_lds = (float*)(smem + NBUF * BUFB);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int ql = lane & 15;
  const int g = lane >> 4;
  // XCD-aware order for the streaming (global) path: the grid is 1-D and the query blocks of one
  // (image, head) all land on one XCD (workgroups are dealt round-robin over the 8 XCDs), so that
  // XCD's L2 serves their shared K/V stream instead of every XCD fetching every head's keys
  int qblk = blockIdx.x, head = blockIdx.y, unit = blockIdx.z;
  // p.nqb > 0 only on the 1-D launch (launch_attn sets it there); a 3-D launch whose y / z
  // extents happen to be 1 (heads * units == 1) keeps blockIdx as is
  if (!RESIDENT && p.nqb > 0) {
    const int nqb = p.nqb, pairs = p.heads * p.units;
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int pair = xcd * (pairs >> 3) + k / nqb;
    qblk = k % nqb;
    head = pair % p.heads;
    unit = pair / p.heads;
  }
  const int S = SC ? SC : p.S;   // grid side, compile-time where the dispatcher knows it
  const int b = unit / p.upi;
  const int wi = unit % p.upi;
  const int Y0 = (wi / p.nwx) * S;
  const int X0 = (wi % p.nwx) * S;
  const int C = p.C;
  const float qscale = p.scale * LOG2E;

  // 0 = real token, 1 = window pad (q/k/v = bias), 2 = slot beyond the row (masked / unused)
  auto tok_kind = [&](int y, int x) -> int {
    if (x >= S || y >= S) return 2;
    return (Y0 + y < p.H && X0 + x < p.W) ? 0 : 1;
  };
  auto tok_ptr = [&](int y, int x) -> const _Float16* {
    return p.qkv + (((int64_t)b * p.H + (Y0 + y)) * p.W + (X0 + x)) * p.tok_stride;
  };

  // ---------------------------------------------------------------- K/V staging (LDS-DMA)
  // chunk c of a unit -> LDS byte c*16; unit layout [K|V][key][D] (STREAM: one row of SP slots;
  // RESIDENT: key r*S + x of the whole grid)
  // per-lane sources for key row 0 (STREAM) / the whole grid (RESIDENT); a STREAM row kh is the
  // same pattern kh grid rows further down, so the loop only adds kh * rowstride
  const _Float16* src0[NI];
  bool adv[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = (wave * NI + i) * 64 + lane;
    const _Float16* src = g_zero16;
    bool real = false;
    if (c < UNIT_CHUNKS) {
      constexpr int HALF = UNIT_CHUNKS / 2;
      const bool isv = c >= HALF;
      const int cc = isv ? c - HALF : c;
      const int key = cc / D8, d8 = cc % D8;
      const int r = RESIDENT ? key / S : 0;
      const int slot = RESIDENT ? key % S : key;
      const int kind = r < S ? tok_kind(r, slot) : 2;
      const int off = (isv ? 2 * C : C) + head * D + d8 * 8;
      if (kind == 0) { src = tok_ptr(r, slot) + off; real = true; }
      else if (kind == 1 && p.qkv_bias) src = p.qkv_bias + off;
    }
    src0[i] = src;
    adv[i] = real && !RESIDENT;
  }
  const int64_t rowstride = (int64_t)p.W * p.tok_stride;
  auto issue = [&](int row0, int buf) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const _Float16* src = adv[i] ? src0[i] + row0 * rowstride : src0[i];
      __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)src,
                                       (SAMQ_LDS void*)(smem + buf * BUFB + (wave * NI + i) * 1024), 16, 0, 0);
    }
  };

  // start the K/V traffic first, it overlaps the Q / rel-pos prologue
  issue(0, 0);
  if (!RESIDENT && S > 1) issue(1, 1);

  // ---------------------------------------------------------------- Q fragments (scaled)
  const bool kin3 = 64 + 8 * g < D;   // this lane group holds real d in the last k-step
  half8_t qf[QT][KS];
  int qrow[QT], qcol0[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qi = (qblk * NW + wave) * QT + t;
    qrow[t] = qi / KT;
    qcol0[t] = (qi % KT) * 16;
    const int kind = tok_kind(qrow[t], qcol0[t] + ql);
    const _Float16* src = nullptr;
    if (kind == 0) src = tok_ptr(qrow[t], qcol0[t] + ql) + head * D;
    else if (kind == 1 && p.qkv_bias) src = p.qkv_bias + head * D;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      half8_t v = {};
      if (src && (s < 2 || kin3)) v = *(const half8_t*)(src + 32 * s + 8 * g);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (_Float16)((float)v[j] * qscale);
      qf[t][s] = v;
    }
  }

  // ---------------------------------------------------------------- rel-pos terms
  float4_t tw[QT][KT];
  const float inv_scale = 1.0f / p.scale;  // (Qs . R) / scale = log2e * (q . R)
  float* th_w = th_lds + wave * (QT * TH_ROWS * 16);
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qh = qrow[t] < S ? qrow[t] : S - 1;
    if (!PRECOMP) {
#pragma unroll
      for (int which = 0; which < 2; ++which) {
        const _Float16* tab = which ? p.relw : p.relh;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          int r = qh - (kt * 16 + ql) + S - 1;     // table row of this lane's A-operand row
          r = r < 0 ? 0 : r;
          const _Float16* rp = tab + (int64_t)r * D;
          float4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            half8_t ra = {};
            if (s < 2 || kin3) ra = *(const half8_t*)(rp + 32 * s + 8 * g);
            a = __builtin_amdgcn_mfma_f32_16x16x32_f16(ra, qf[t][s], a, 0, 0, 0);
          }
          a = a * inv_scale;
          if (which) {
            tw[t][kt] = a;
          } else {
#pragma unroll
            for (int r2 = 0; r2 < 4; ++r2) th_w[(t * TH_ROWS + kt * 16 + 4 * g + r2) * 16 + ql] = a[r2];
          }
        }
      }
    } else {
      // precomputed bias tensors [B'*heads][S][S][S]: rel_h[.., qh, qw, kh], rel_w[.., qh, qw, kw]
      const int qw = qcol0[t] + ql;
      const bool ok = qw < S && qrow[t] < S;
      const int64_t base = ((((int64_t)unit * p.heads + head) * S + qh) * S + (ok ? qw : 0)) * S;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
        for (int r2 = 0; r2 < 4; ++r2) {
          const int kk = kt * 16 + 4 * g + r2;
          const bool kin = ok && kk < S;
          tw[t][kt][r2] = kin ? (float)p.relw[base + kk] * LOG2E : 0.f;
          th_w[(t * TH_ROWS + kk) * 16 + ql] = kin ? (float)p.relh[base + kk] * LOG2E : 0.f;
        }
      }
    }
  }

  // SP >= 32: the softmax denominator is accumulated by the P.V MFMAs themselves (one more
  // 16x16x32 against an all-ones A operand per 32 keys, rescaled with O) instead of one VALU add
  // per score plus the cross-lane reduction -- the softmax VALU is what bounds this kernel.
  constexpr bool MSUM = SP >= 32;
  float m[QT], l[QT];
  float4_t o[QT][DT], lacc[QT];
  const half8_t ones = {1, 1, 1, 1, 1, 1, 1, 1};
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    m[t] = -INFINITY;
    l[t] = 0.f;
    lacc[t] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < DT; ++d) o[t][d] = float4_t{0.f, 0.f, 0.f, 0.f};
  }
  const bool mask_slots = S < SP;
  const int trow = ql >> 2;            // ds_read_b64_tr_b16: lane 4q+p of a 16-lane group reads
  const int tcol = 4 * (ql & 3);       // block row q, columns 4p..4p+3; receives column (lane&15)

  if (RESIDENT) {
    wait_vmcnt<0>();
    __syncthreads();   // K/V of the whole window + TH visible
  } else {
    __syncthreads();   // TH visible (the K/V ring is ordered by counted vmcnt + s_barrier below)
  }

  // ---- per key row: scores (QK), online softmax, O += P.V -- as lambdas so the streaming loop
  // can software-pipeline them (see below)
  using PB = half8_t[QT][(SP + 31) / 32];
  auto qk = [&](const char* kb, float4_t (&sc)[QT][KT]) {
      // ---- scores S^T = K . Q^T (+ TW as the C input)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const char* krow = kb + (kt * 16 + ql) * (D * 2);
        half8_t kf[KS];
        // unconditional: lanes past D in the last k-step read the next key's bytes (finite K/V
        // data of the LDS image) against zero Q dims -- no v_mov zero-fill per fragment
#pragma unroll
        for (int s = 0; s < KS; ++s) kf[s] = *(const half8_t*)(krow + (32 * s + 8 * g) * 2);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
          float4_t a = tw[t][kt];
#pragma unroll
          for (int s = 0; s < KS; ++s) a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[s], qf[t][s], a, 0, 0, 0);
          sc[t][kt] = a;
        }
      }

  };
  auto soft = [&](int kh, float4_t (&sc)[QT][KT], PB& pb, half4_t (&pb16)[QT]) {
    // ---- online softmax (exp2 domain); TH[q, kh] is constant along the row
    bool any_rescale = false;
    float alpha[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      if (mask_slots) {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (kt * 16 + 4 * g + r >= S) sc[t][kt][r] = -INFINITY;
      }
      float mx;
      if constexpr (KT == 1) {
        mx = max3f(sc[t][0][0], sc[t][0][1], fmaxf(sc[t][0][2], sc[t][0][3]));
      } else {   // two max3 chains (no canonicalising v_max of a lone fmaxf)
        mx = max3f(sc[t][0][0], sc[t][0][1], sc[t][0][2]);
        float my = max3f(sc[t][1][0], sc[t][1][1], sc[t][1][2]);
        mx = max3f(mx, sc[t][0][3], sc[t][1][3]);
#pragma unroll
        for (int kt = 2; kt < KT; kt += 2) {
          mx = max3f(mx, sc[t][kt][0], sc[t][kt][1]);
          my = max3f(my, sc[t][kt + 1][0], sc[t][kt + 1][1]);
          mx = max3f(mx, sc[t][kt][2], sc[t][kt][3]);
          my = max3f(my, sc[t][kt + 1][2], sc[t][kt + 1][3]);
        }
        mx = fmaxf(mx, my);
      }
      mx = max_rows4(mx);
      const float th = th_w[(t * TH_ROWS + kh) * 16 + ql];
      // lazy rescale: the exp2 offset m only moves when the row max exceeds it by > 8 (P <= 2^8,
      // far inside fp16; O and l carry the same offset, so O / l is unchanged) -- most key rows
      // then skip the O rescale, whose packed multiplies beside the MFMAs bound this loop
      const float mrow = mx + th;
      const bool up = mrow > m[t] + 8.0f;
      const float mnew = up ? mrow : m[t];
      alpha[t] = up ? __builtin_amdgcn_exp2f(m[t] - mnew) : 1.0f;
      any_rescale |= up;
      m[t] = mnew;
      const float corr = mnew - th;
      float rs = 0.f;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(sc[t][kt][r] - corr);
          sc[t][kt][r] = e;
          if (!MSUM) rs += e;
        }
      if (!MSUM) l[t] = l[t] * alpha[t] + rs;
      if (SP == 16) {
        pb16[t] = half4_t{(_Float16)sc[t][0][0], (_Float16)sc[t][0][1], (_Float16)sc[t][0][2], (_Float16)sc[t][0][3]};
      } else {
#pragma unroll
        for (int s = 0; s < SP / 32; ++s) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pb[t][s][r] = (_Float16)sc[t][2 * s][r];
            pb[t][s][4 + r] = (_Float16)sc[t][2 * s + 1][r];
          }
        }
      }
    }
    if (__any(any_rescale)) {
#pragma unroll
      for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int d = 0; d < DT; ++d) o[t][d] = o[t][d] * alpha[t];
#pragma unroll
      for (int t = 0; t < QT; ++t)
        if (MSUM) lacc[t] = lacc[t] * alpha[t];
    }

  };
  auto pv = [&](const char* vb, PB& pb, half4_t (&pb16)[QT]) {
    // ---- O^T += V^T . P^T  (V^T fragments by hardware-transposed LDS reads of row-major V)
    // one base address per key row, the (d, s) offsets as the instruction's immediate
    const uint32_t vbase = lds_addr(vb + ((4 * g + trow) * D + tcol) * 2);
    static_for<DT>([&](auto dc_) {
      constexpr int d = decltype(dc_)::value;
      if constexpr (SP == 16) {
        half4_t va = ds_read_tr16_off<(d * 16) * 2>(vbase);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(va));
#pragma unroll
        for (int t = 0; t < QT; ++t) o[t][d] = __builtin_amdgcn_mfma_f32_16x16x16f16(va, pb16[t], o[t][d], 0, 0, 0);
      } else {
        constexpr int NS = SP / 32;
        half4_t lo[NS], hi[NS];
        static_for<NS>([&](auto sc_) {
          constexpr int s_ = decltype(sc_)::value;
          lo[s_] = ds_read_tr16_off<((32 * s_) * D + d * 16) * 2>(vbase);
          hi[s_] = ds_read_tr16_off<((32 * s_ + 16) * D + d * 16) * 2>(vbase);
        });
        if constexpr (NS == 2) {
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo[0]), "+v"(hi[0]), "+v"(lo[1]), "+v"(hi[1]));
        } else {
#pragma unroll
          for (int s = 0; s < NS; ++s) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo[s]), "+v"(hi[s]));
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const half8_t va = {lo[s][0], lo[s][1], lo[s][2], lo[s][3], hi[s][0], hi[s][1], hi[s][2], hi[s][3]};
#pragma unroll
          for (int t = 0; t < QT; ++t) o[t][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb[t][s], o[t][d], 0, 0, 0);
        }
      }
    });
    if constexpr (MSUM) {
      constexpr int NS = SP / 32;
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int t = 0; t < QT; ++t) lacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pb[t][s], lacc[t], 0, 0, 0);
    }
  };

  if (RESIDENT) {
    for (int kh = 0; kh < S; ++kh) {
      const char* kb = smem + kh * S * (D * 2);
      float4_t sc[QT][KT];
      PB pb;
      half4_t pb16[QT];
      qk(kb, sc);
      soft(kh, sc, pb, pb16);
      pv(kb + (UNIT_CHUNKS / 2) * 16, pb, pb16);
    }
  } else {
    // Streaming (global) attention, software-pipelined by one key row: the Q.K^T MFMAs of row
    // kh+1 are issued ahead of the softmax of row kh (independent registers), so the MFMA tail
    // drains under the first softmax VALU work (with the MFMA row sums: 507 -> 474 us at ViT-H
    // B=4; forcing a finer MFMA/VALU interleave with sched_group_barrier spills, and the
    // softmax's max -> reduce -> exp chain leaves little to interleave).  Ring: row r in slot
    // r % 3; at the top of iteration kh row kh+1 is retired (nothing newer in flight) and, after
    // the barrier that also ends every read of row kh-1, row kh+2 is staged into row kh-1's slot.
    float4_t scA[QT][KT], scB[QT][KT];
    PB pb;
    half4_t pb16[QT];
    if (S > 1) wait_vmcnt<NI>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();   // row 0 landed for every wave
    qk(smem, scA);
    auto step = [&](int kh, float4_t (&cur)[QT][KT], float4_t (&nxt)[QT][KT]) {
      if (kh + 1 < S) {
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();   // row kh+1 landed for every wave; row kh-1 fully consumed
        if (kh + 2 < S) issue(kh + 2, (kh + 2) % 3);
        qk(smem + ((kh + 1) % 3) * BUFB, nxt);
      }
      soft(kh, cur, pb, pb16);
      pv(smem + (kh % 3) * BUFB + ROWB, pb, pb16);
    };
    for (int kh = 0; kh < S; kh += 2) {   // S is even on this path (32 or 64)
      step(kh, scA, scB);
      step(kh + 1, scB, scA);
    }
  }

  // ---------------------------------------------------------------- normalise + store
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    float lt = l[t];
    if (MSUM) {
      lt = lacc[t][0];
    } else {
      lt += __shfl_xor(lt, 16, 64);
      lt += __shfl_xor(lt, 32, 64);
    }
    const int x = qcol0[t] + ql;
    if (tok_kind(qrow[t], x) != 0) continue;
    const float inv = 1.0f / lt;
    const int64_t dst = (((int64_t)b * p.H + (Y0 + qrow[t])) * p.W + (X0 + x)) * C + head * D;
#pragma unroll
    for (int d = 0; d < DT; ++d) attn_store4(p, dst + d * 16 + 4 * g, o[t][d] * inv);
  }
}

}  // namespace samq
