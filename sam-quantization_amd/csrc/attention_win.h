// Windowed attention (14 x 14) with in-kernel decomposed relative-position bias.  Included by
// attention.hip only.
//
// The 14x14-window blocks (28 of 32 in ViT-H).  One (window, head) item per 4-wave workgroup, TWO
// workgroups per CU (LDS < 80 KiB, <= 256 VGPRs): the partner workgroup runs out of phase, so
// one's HBM wait, softmax VALU and MFMA runs overlap the other's (no barrier couples them), and the
// hardware deals the 800 items of a 2-image ViT-H launch dynamically over the 512 slots.
//  * LDS image of an item: per key row kh (16 key slots; slots 14, 15 duplicate slot 13 and are
//    masked) NPC 1-KiB pieces, each written by ONE global_load_lds_dwordx4 whose lanes pick their
//    own sources:  K piece s: position l = (g, ql) holds key ql, dims 32 s + 8 g  -- read back by
//    lane l itself (ds_read_b128 at l * 16: the A operand of k-step s, conflict-free);  V piece:
//    position (g8, slot ^ 8 (g8 & 1)) holds key slot, dims 32 dblk + 8 g8 -- the XOR spreads the
//    ds_read_b64_tr_b16 reads of V^T over all 64 banks.  (D = 80: K dims 64..79 and V dims 64..79
//    share one piece; lanes of k-step 2 past dim 79 read V bytes against zero Q dims.)
//    Sources are one 64-bit add per piece (row stride); window pad tokens (past the image) read
//    the qkv bias, as the reference's zero-padded tokens do after the qkv Linear.
//  * query rows in passes of two 16-slot tiles per wave (rows 2w, 2w+1 then 8+2w, 9+2w); per tile
//    TW[q, kw] = q . Rw[qh - kw + 13] and TH[q, kh] = q . Rh[qh - kh + 13] (both indexed by the
//    query ROW qh: reference quirk 1) come out of 2 x KS MFMAs in the score layout; TW is the C
//    input of every key row's Q.K^T, TH[q, kh] is added to it per row (lane-local after one LDS
//    exchange; TH is rounded to fp16 as the reference's rel_h is);
//  * S^T = K.Q^T per key row (16 x 16 tile, each lane owns one query), one exact softmax over the
//    window's keys in the exp2 domain, O^T += V^T.P^T two key rows per MFMA with P^T in the score
//    registers' own k order, the row sum as one more MFMA against ones.
// Unscaled Q (round 4): Q enters the MFMAs unscaled (exact fp16 qkv values) and the scores stay in
// unscaled units S_u = q.k + (q.Rw + fp16(q.Rh)) / scale, the sm scale and log2e applied inside the
// softmax's exp2 argument (one fma per score, as the subtraction it replaces): no fp16 rounding of
// q * scale * log2e (a 2^-12 relative error on every score), and TH rounded to fp16 where the
// reference rounds rel_h (q . Rh, unscaled).  Against the scaled-Q form it replaced: 35.6 vs 36.2 us
// per ViT-H 2-image launch, fp16 output 1.59e-3 vs 1.95e-3 max-abs from the fp32 oracle, W4A8 store
// codes off by one 1.7e-3 vs 2.5e-3 (profiles/r4_m.win.log).
// PHL (round 4, the W4A8 int8-code store): P enters P.V as fp16 hi + lo (P - hi, |P - hi - lo| ~
// 2^-22 |P|, the split of attention_q8_row64.h) -- two MFMAs per P.V step and for the row sums -- so the
// output carries fp32-level error instead of fp16 P's 2^-12, before the proj QAct's quantiser
#pragma once

#include "attention_util.h"

namespace samq {

// pieces of the window kernel
template <int D, bool PHL = false>
struct Win {
  static constexpr int S = 14, QT = 2;
  static constexpr int KS = D == 80 ? 3 : 2;            // k32 steps of Q.K^T
  static constexpr int DT = D / 16;                     // output d tiles
  static constexpr int NPC = D == 80 ? 5 : 4;           // 1-KiB pieces per key row
  static constexpr int ROWB = NPC * 1024;
  static constexpr int KVB = S * ROWB;                  // one item's K/V image
  static constexpr int V0 = (NPC - 2) * 1024;           // V dims 0..31 piece (dims 32..63 follow)
  static constexpr int TAB = (2 * S - 1) * D;           // elements per rel-pos table
  static constexpr int TABB = ((2 * TAB * 2 + 1023) / 1024) * 1024;   // both tables, whole pieces
  static_assert(D == 64 || D == 80, "head dim");

  struct Geo { const _Float16* tok0; int b, Y0, X0, head, nrow, ncol; };

  __device__ static __forceinline__ Geo geo(const AttnParams& p, int item) {
    Geo o;
    const int unit = item / p.heads;
    o.head = item - unit * p.heads;
    o.b = unit / p.upi;
    const int wi = unit - o.b * p.upi;
    const int wy = wi / p.nwx;
    o.Y0 = wy * S;
    o.X0 = (wi - wy * p.nwx) * S;
    o.nrow = p.H - o.Y0 < S ? p.H - o.Y0 : S;           // rows / columns inside the image
    o.ncol = p.W - o.X0 < S ? p.W - o.X0 : S;
    o.tok0 = p.qkv + (((int64_t)o.b * p.H + o.Y0) * p.W + o.X0) * p.tok_stride;
    return o;
  }

  // both rel-pos tables -> LDS, pieces i0, i0 + istep, ... (one wave's share)
  __device__ static __forceinline__ void issue_tables(const AttnParams& p, char* tab, int lane, int i0, int istep) {
    for (int i = i0; i < TABB / 1024; i += istep) {
      const int c = i * 64 + lane;                       // 16-byte chunk of [relh | relw]
      const int tc = c < TAB / 8 ? c : c - TAB / 8;
      const _Float16* src = c < 2 * (TAB / 8) ? (c < TAB / 8 ? p.relh : p.relw) + 8 * tc : g_zero16;
      __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)src, (SAMQ_LDS void*)(tab + i * 1024), 16, 0, 0);
    }
  }

  // key rows kh0, kh0 + khstep, ... of one item -> its LDS image (one global_load_lds per piece)
  __device__ static __forceinline__ void issue_rows(const AttnParams& p, const Geo& G, char* kv, int lane, int kh0,
                                                    int khstep) {
    const int ql = lane & 15, g = lane >> 4;
    const int64_t ts = p.tok_stride, rowstride = (int64_t)p.W * ts;
    const _Float16* src[NPC];
    int64_t step[NPC];
    const _Float16* pad[NPC];
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      int col, ch;
      if (j < KS - (D == 80 ? 1 : 0) || (D == 80 && j == 2 && lane < 32)) {   // K: (g, ql)
        col = ql;
        ch = p.C + G.head * D + 32 * j + 8 * g;
      } else {                                                                // V: (g8, slot ^ 8 (g8 & 1))
        const bool comb = D == 80 && j == 2;             // upper half of the shared K/V piece
        const int g8 = comb ? g - 2 : g;
        const int dblk = comb ? 2 : j - (NPC - 2);
        col = ql ^ (8 * (g8 & 1));
        ch = 2 * p.C + G.head * D + 32 * dblk + 8 * g8;
      }
      col = col < S - 1 ? col : S - 1;
      pad[j] = p.qkv_bias ? p.qkv_bias + ch : g_zero16;
      const bool real = col < G.ncol;
      src[j] = real ? G.tok0 + (int64_t)col * ts + ch + kh0 * rowstride : pad[j];
      step[j] = real ? khstep * rowstride : 0;
    }
    for (int kh = kh0; kh < S; kh += khstep) {
      const bool rowreal = kh < G.nrow;
#pragma unroll
      for (int j = 0; j < NPC; ++j) {
        __builtin_amdgcn_global_load_lds((const SAMQ_GLOBAL void*)(rowreal ? src[j] : pad[j]),
                                         (SAMQ_LDS void*)(kv + kh * ROWB + j * 1024), 16, 0, 0);
        src[j] += step[j];
      }
    }
  }

  // raw Q of one tile (query row r, slots ql; dims 32 s + 8 g; zero past D and for slots 14, 15)
  __device__ static __forceinline__ void load_q(const AttnParams& p, const Geo& G, int r, int lane, half8_t (&q)[KS]) {
    const int ql = lane & 15, g = lane >> 4;
    const bool inwin = ql < S && r < S;
    const bool real = inwin && r < G.nrow && ql < G.ncol;
    const _Float16* base = real ? G.tok0 + ((int64_t)r * p.W + ql) * p.tok_stride + G.head * D
                                : ((inwin && p.qkv_bias) ? p.qkv_bias + G.head * D : nullptr);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const _Float16* a = (base && 32 * s + 8 * g < D) ? base + 32 * s + 8 * g : g_zero16;
      asm volatile("" : "+v"(a));
      q[s] = *(const SAMQ_GLOBAL half8_t*)a;
    }
  }

  // query rows row0, row0 + 1 of one item: rel-pos terms, S^T = K.Q^T + TW + TH, exact softmax,
  // O^T = V^T.P^T, normalise, store.  after_qk() runs once the scores are in registers (the
  // caller's prefetch of the next tiles' Q into qf goes there: qf is dead by then).
  template <typename F>
  __device__ static __forceinline__ void tiles(const AttnParams& p, const Geo& G, const char* kv, const char* tab,
                                               half8_t (&qf)[QT][KS], int row0, int lane, F&& after_qk) {
    const int ql = lane & 15, g = lane >> 4;
    const float qscale = p.scale * LOG2E;                // applied inside the softmax's exp2 argument
    const float inv_scale = 1.0f / p.scale;              // rel-pos terms in the scores' unscaled units
    const _Float16* tabh = (const _Float16*)tab;
    // ---- rel-pos table fragments (A operands: row i = key column / key row) from the LDS copy
    half8_t relh[QT][KS], relw[QT][KS];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      int idx = row0 + t - ql + S - 1;
      idx = idx < 0 ? 0 : idx;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        int dd = 32 * s + 8 * g;
        dd = dd < D ? dd : dd - 16;                      // k-step-2 lanes past D: any in-bounds row bytes
        relh[t][s] = *(const half8_t*)(tabh + idx * D + dd);
        relw[t][s] = *(const half8_t*)(tabh + TAB + idx * D + dd);
      }
    }
    // ---- rel-pos terms of the (unscaled) Q
    float4_t tw[QT];
    half8_t th[QT][2];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      float4_t a = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(relw[t][s], qf[t][s], a, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(relh[t][s], qf[t][s], c, 0, 0, 0);
      }
      a = a * inv_scale;                 // (q . Rw) / scale; c = q . Rh is rounded below like rel_h
      if (g == 3) { a[2] = -INFINITY; a[3] = -INFINITY; }   // key slots 14, 15
      tw[t] = a;
      // lane (g, ql) holds TH[kh = 4g..4g+3][query ql]; gather kh 0..15 of its query from the
      // lanes (g', ql) (fp16, as the reference rounds rel_h)
      union { half4_t h; uint32_t u[2]; } mine;
      mine.h = half4_t{(_Float16)c[0], (_Float16)c[1], (_Float16)c[2], (_Float16)c[3]};
      union { half8_t h[2]; uint32_t u[8]; } all;
#pragma unroll
      for (int gg = 0; gg < 4; ++gg)
#pragma unroll
        for (int w = 0; w < 2; ++w) all.u[2 * gg + w] = (uint32_t)__shfl((int)mine.u[w], ql + 16 * gg, 64);
      th[t][0] = all.h[0];
      th[t][1] = all.h[1];
    }

    // ---- scores S^T = K.Q^T + TW + TH for all key rows (next row's K fragments in flight)
    float4_t sc[QT][S];
    half8_t kf[2][KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) kf[0][s] = *(const half8_t*)(kv + s * 1024 + lane * 16);
#pragma unroll
    for (int kh = 0; kh < S; ++kh) {
      if (kh + 1 < S) {
#pragma unroll
        for (int s = 0; s < KS; ++s) kf[(kh + 1) & 1][s] = *(const half8_t*)(kv + (kh + 1) * ROWB + s * 1024 + lane * 16);
      }
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        const float h = (float)th[t][kh >> 3][kh & 7] * inv_scale;
        float4_t a = tw[t] + h;
#pragma unroll
        for (int s = 0; s < KS; ++s) a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kh & 1][s], qf[t][s], a, 0, 0, 0);
        sc[t][kh] = a;
      }
      __builtin_amdgcn_sched_barrier(0);   // no hoisting of later rows' C inputs (register pressure)
    }
    after_qk();

    // ---- exact softmax over the window (exp2 domain)
    half8_t pb[QT][S / 2];
    half8_t pl[PHL ? QT : 1][PHL ? S / 2 : 1];   // PHL: the lo parts
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      // two independent max3 chains (no canonicalising v_max of a lone fmaxf)
      float mx = max3f(sc[t][0][0], sc[t][0][1], sc[t][0][2]);
      float my = max3f(sc[t][1][0], sc[t][1][1], sc[t][1][2]);
      mx = max3f(mx, sc[t][0][3], sc[t][1][3]);
#pragma unroll
      for (int kh = 2; kh < S; kh += 2) {
        mx = max3f(mx, sc[t][kh][0], sc[t][kh][1]);
        my = max3f(my, sc[t][kh + 1][0], sc[t][kh + 1][1]);
        mx = max3f(mx, sc[t][kh][2], sc[t][kh][3]);
        my = max3f(my, sc[t][kh + 1][2], sc[t][kh + 1][3]);
      }
      mx = fmaxf(mx, my);
      mx = max_rows4(mx);
      // P = exp2((S_u - max) * scale * log2e) as one fma per score
      const float nmx = -mx * qscale;
      if constexpr (PHL) {
#pragma unroll
        for (int pr = 0; pr < S / 2; ++pr)
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[t][2 * pr + (r >> 2)][r & 3], qscale, nmx));
            const _Float16 hi = (_Float16)e;
            pb[t][pr][r] = hi;
            pl[PHL ? t : 0][PHL ? pr : 0][r] = (_Float16)(e - (float)hi);
          }
      } else {
#pragma unroll
        for (int pr = 0; pr < S / 2; ++pr)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pb[t][pr][r] = (_Float16)__builtin_amdgcn_exp2f(__builtin_fmaf(sc[t][2 * pr][r], qscale, nmx));
            pb[t][pr][4 + r] = (_Float16)__builtin_amdgcn_exp2f(__builtin_fmaf(sc[t][2 * pr + 1][r], qscale, nmx));
          }
      }
    }

    // ---- O^T = V^T . P^T (two key rows per MFMA), l = ones . P^T
    // V^T fragment address of this lane (ds_read_b64_tr_b16: lane 4q+p of a group reads key slot
    // 4g + q, dims 4p..4p+3 of the tile's 16; the V pieces' XOR layout)
    const int tq = ql >> 2, tp = ql & 3;
    const int vslot = 4 * g + tq;
    const uint32_t vlane = lds_addr(kv) + (((tp >> 1) * 16 + (vslot ^ (8 * (tp >> 1)))) * 16 + (tp & 1) * 8);
    const half8_t ones = {1, 1, 1, 1, 1, 1, 1, 1};
    float4_t o[QT][DT], lsum[QT];   // first written by the pr = 0 MFMAs (zero C operand)
    const float4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    half4_t vlo[2][DT], vhi[2][DT];
    // V^T fragments of key rows (2 pr, 2 pr + 1) for all d tiles (immediate offsets from two bases)
    auto vread = [&](auto prc, half4_t (&lo)[DT], half4_t (&hi)[DT]) {
      constexpr int PR = decltype(prc)::value;
      constexpr int HB = PR >= 4 ? 32768 : 0;
      const uint32_t base = vlane + HB;
      static_for<DT>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
        constexpr int VO = d < 4 ? V0 + (d >> 1) * 1024 + (d & 1) * 512 : 2 * 1024 + 512;
        lo[d] = ds_read_tr16_off<(2 * PR) * ROWB + VO - HB>(base);
        hi[d] = ds_read_tr16_off<(2 * PR + 1) * ROWB + VO - HB>(base);
      });
    };
    vread(std::integral_constant<int, 0>{}, vlo[0], vhi[0]);
    static_for<S / 2>([&](auto prc) {
      constexpr int pr = decltype(prc)::value;
      constexpr int cb = pr & 1;
      if constexpr (pr + 1 < S / 2) vread(std::integral_constant<int, pr + 1>{}, vlo[cb ^ 1], vhi[cb ^ 1]);
      // this pair's fragments landed (the next pair's 2*DT reads may still be in flight)
      if constexpr (DT == 5) {
        if (pr + 1 < S / 2)
          asm volatile("s_waitcnt lgkmcnt(10)" : "+v"(vlo[cb][0]), "+v"(vlo[cb][1]), "+v"(vlo[cb][2]), "+v"(vlo[cb][3]),
                       "+v"(vlo[cb][4]), "+v"(vhi[cb][0]), "+v"(vhi[cb][1]), "+v"(vhi[cb][2]), "+v"(vhi[cb][3]), "+v"(vhi[cb][4]));
        else
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vlo[cb][0]), "+v"(vlo[cb][1]), "+v"(vlo[cb][2]), "+v"(vlo[cb][3]),
                       "+v"(vlo[cb][4]), "+v"(vhi[cb][0]), "+v"(vhi[cb][1]), "+v"(vhi[cb][2]), "+v"(vhi[cb][3]), "+v"(vhi[cb][4]));
      } else {
        if (pr + 1 < S / 2)
          asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(vlo[cb][0]), "+v"(vlo[cb][1]), "+v"(vlo[cb][2]), "+v"(vlo[cb][3]),
                       "+v"(vhi[cb][0]), "+v"(vhi[cb][1]), "+v"(vhi[cb][2]), "+v"(vhi[cb][3]));
        else
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vlo[cb][0]), "+v"(vlo[cb][1]), "+v"(vlo[cb][2]), "+v"(vlo[cb][3]),
                       "+v"(vhi[cb][0]), "+v"(vhi[cb][1]), "+v"(vhi[cb][2]), "+v"(vhi[cb][3]));
      }
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        const half8_t va = {vlo[cb][d][0], vlo[cb][d][1], vlo[cb][d][2], vlo[cb][d][3],
                            vhi[cb][d][0], vhi[cb][d][1], vhi[cb][d][2], vhi[cb][d][3]};
#pragma unroll
        for (int t = 0; t < QT; ++t) {
          o[t][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb[t][pr], pr ? o[t][d] : zero4, 0, 0, 0);
          if constexpr (PHL) o[t][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pl[t][pr], o[t][d], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        lsum[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pb[t][pr], pr ? lsum[t] : zero4, 0, 0, 0);
        if constexpr (PHL) lsum[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pl[t][pr], lsum[t], 0, 0, 0);
      }
    });

    // ---- normalise + store (token-major [B, H, W, C])
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const int r = row0 + t;
      if (r >= G.nrow || ql >= G.ncol) continue;
      const float inv = __builtin_amdgcn_rcpf(lsum[t][0]);
      const int64_t dst = (((int64_t)G.b * p.H + (G.Y0 + r)) * p.W + (G.X0 + ql)) * p.C + G.head * D;
#pragma unroll
      for (int d = 0; d < DT; ++d) attn_store4(p, dst + d * 16 + 4 * g, o[t][d] * inv);
    }
  }
};

// One item per 4-wave workgroup, two workgroups per CU (rows 2w, 2w+1 then 8+2w, 9+2w).  (A
// persistent form -- one 8-wave workgroup per CU, wave 7 streaming the next item's K/V into a second
// buffer while waves 0..6 compute -- measured 37.9 vs 37.0 us per 2-image ViT-H launch.)
template <int D, bool PHL = false>
__global__ __launch_bounds__(256, 2) void win_attention_kernel(AttnParams p, int items) {
  using W = Win<D, PHL>;
  static_assert(W::KVB + W::TABB <= 80 * 1024, "two workgroups per CU");
  __shared__ __attribute__((aligned(16))) char smem[W::KVB + W::TABB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // consecutive items (the heads of one window: K/V cache lines shared across head slices) on one XCD
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  if (item >= items) return;
  const typename W::Geo G = W::geo(p, item);
  char* tab = smem + W::KVB;
  W::issue_tables(p, tab, lane, wave, 4);
  W::issue_rows(p, G, smem, lane, wave, 4);
  half8_t qf[W::QT][W::KS];
#pragma unroll
  for (int t = 0; t < W::QT; ++t) W::load_q(p, G, 2 * wave + t, lane, qf[t]);
  wait_vmcnt<0>();
  __syncthreads();   // the item's K/V image and the tables are complete
  const int npass = 8 + 2 * wave < W::S ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    const int row0 = 8 * pass + 2 * wave;
    W::tiles(p, G, smem, tab, qf, row0, lane, [&] {
      if (pass + 1 < npass) {
#pragma unroll
        for (int t = 0; t < W::QT; ++t) W::load_q(p, G, row0 + 8 + t, lane, qf[t]);
      }
    });
  }
}

}  // namespace samq
