// W8A8 attention of the SAM mask decoder's two-way transformer on int8 codes (gfx950): the part of
// fq_vit/models/sam/transformer.py Attention.forward between the input projections and out_proj
// (:520-537) -- head split, q.k^T / sqrt(D), qact_attn1, softmax, p.v, head merge, qact2.
//
//   a_ij = q8(float(sum_d q_id k_jd) * (s_q s_k / sqrt(D)), s_a1)      int32 sum exact
//   p_ij = exp((a_ij - m_i) s_a1),  m_i = max_j a_ij                   fp32, on the integer codes
//   out  = q8((sum_j p_ij v_jd) s_v / sum_j p_ij, s_out)
//
// No relative positions, no windows, Nq != Nk: nothing of the encoder's MFMA kernels
// (attention_q8.hip) applies, and the whole decoder attention is ~0.2 GFLOP -- latency, not
// throughput.  One launch per attention, int8 dot products on v_dot4_i32_i8, two launch branches:
//
//   few queries (Nq <= 16) against many keys (tokens x image): one workgroup per (batch, head,
//     QT queries); every lane owns keys j = tid, tid + NT, ... and keeps an online softmax
//     (integer running max, fp32 sum and p.v) per query in registers.  The partial states of the
//     lanes, then of the waves (LDS), are combined exactly: the running maxima are integer codes,
//     so the rescale factors exp((m_part - m) s_a1) are the same numbers any split produces.
//   many queries or few keys (image x tokens, tokens x tokens): one lane per (query, head), the
//     keys / values of the head staged through LDS KT at a time (broadcast reads), the same online
//     softmax per lane; no reduction.
//
// The softmax numerators are a function of the integer code difference alone (the property the
// encoder kernels' 256-entry table uses); here exp2 is evaluated on that difference directly -- a
// table would cost a workgroup barrier per launch for a few thousand v_exp.
#include "common.h"

namespace samq {

struct AttnPlainParams {
  const int8_t* q;
  const int8_t* k;
  const int8_t* v;
  int8_t* out;
  int B, Nq, Nk, H;
  float kscale;   // s_q s_k / sqrt(D)
  float s_a1, k2; // k2 = s_a1 log2(e)
  float s_v, s_out;
};

constexpr int AP_NEG = -100000;   // running max of a lane that has seen no key

template <int D>
__device__ __forceinline__ int dot_codes(const int (&a)[D / 4], const int (&b)[D / 4]) {
  int acc = 0;
#pragma unroll
  for (int e = 0; e < D / 4; ++e) acc = __builtin_amdgcn_sdot4(a[e], b[e], acc, false);
  return acc;
}

__device__ __forceinline__ float code_f(int w, int e) { return (float)(int8_t)((w >> (8 * e)) & 0xFF); }

// one key into one query's online softmax state
template <int D>
__device__ __forceinline__ void ap_update(int a, const int (&vw)[D / 4], float k2, int& m, float& l, float (&o)[D]) {
  if (a > m) {
    const float f = __builtin_amdgcn_exp2f((float)(m - a) * k2);   // m == AP_NEG: exp2(-huge) = 0
    l *= f;
#pragma unroll
    for (int d = 0; d < D; ++d) o[d] *= f;
    m = a;
  }
  const float p = __builtin_amdgcn_exp2f((float)(a - m) * k2);
  l += p;
#pragma unroll
  for (int d = 0; d < D; ++d) o[d] = fmaf(p, code_f(vw[d / 4], d & 3), o[d]);
}

template <int D>
__device__ __forceinline__ int ap_score(const AttnPlainParams& p, int dot, float inv_a1) {
  return (int)q8_exact((float)dot * p.kscale, p.s_a1, inv_a1);
}

// D output values of one query -> D int8 codes at dst (16-byte aligned)
template <int D>
__device__ __forceinline__ void ap_store(const AttnPlainParams& p, const float (&o)[D], float l, int8_t* dst) {
  const float inv_out = 1.0f / p.s_out, lim = 130.0f * p.s_out;
  uint32_t w[D / 4];
#pragma unroll
  for (int e = 0; e < D / 4; ++e) {
    float2_t x0 = {o[4 * e] * p.s_v / l, o[4 * e + 1] * p.s_v / l};
    float2_t x1 = {o[4 * e + 2] * p.s_v / l, o[4 * e + 3] * p.s_v / l};
    const float2_t c0 = q8_exact2(x0, p.s_out, inv_out, lim), c1 = q8_exact2(x1, p.s_out, inv_out, lim);
    w[e] = q8_pack4(c0.x, c0.y, c1.x, c1.y);
  }
#pragma unroll
  for (int e = 0; e < D / 16; ++e) ((u32x4*)dst)[e] = u32x4{w[4 * e], w[4 * e + 1], w[4 * e + 2], w[4 * e + 3]};
}

// ---------------------------------------------------------------- few queries, keys over the lanes
// grid (B * H, ceil(Nq / QT)), NW waves.  LDS: per wave and query (m, l, o[D]).
template <int D, int QT, int NW>
__global__ __launch_bounds__(64 * NW) void attention_q8_plain_keys_kernel(AttnPlainParams p) {
  constexpr int NT = 64 * NW, DW = D / 4;
  __shared__ float part[NW][QT][D + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / p.H, h = blockIdx.x % p.H, q0 = blockIdx.y * QT;
  const int HD = p.H * D;
  const float inv_a1 = 1.0f / p.s_a1;

  int qw[QT][DW];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int qi = q0 + i < p.Nq ? q0 + i : p.Nq - 1;   // a tail query repeats the last one; never stored
    const int* src = (const int*)(p.q + ((int64_t)b * p.Nq + qi) * HD + h * D);
#pragma unroll
    for (int e = 0; e < DW; ++e) qw[i][e] = src[e];
  }
  int m[QT];
  float l[QT], o[QT][D];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    m[i] = AP_NEG;
    l[i] = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) o[i][d] = 0.f;
  }
  for (int j = tid; j < p.Nk; j += NT) {
    const int64_t off = ((int64_t)b * p.Nk + j) * HD + h * D;
    int kw[DW], vw[DW];
#pragma unroll
    for (int e = 0; e < DW / 4; ++e) {
      const int4_t kk = ((const int4_t*)(p.k + off))[e], vv = ((const int4_t*)(p.v + off))[e];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        kw[4 * e + c] = kk[c];
        vw[4 * e + c] = vv[c];
      }
    }
#pragma unroll
    for (int i = 0; i < QT; ++i) ap_update<D>(ap_score<D>(p, dot_codes<D>(qw[i], kw), inv_a1), vw, p.k2, m[i], l[i], o[i]);
  }
  // lanes -> wave: exact rescale to the wave's integer max, then sums
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    int mw = m[i];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mw = max(mw, __shfl_xor(mw, s, 64));
    const float f = m[i] == AP_NEG ? 0.f : __builtin_amdgcn_exp2f((float)(m[i] - mw) * p.k2);
    const float lw = wave_sum(l[i] * f);
    if (lane == 0) {
      part[wave][i][0] = (float)mw;
      part[wave][i][1] = lw;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float od = wave_sum(o[i][d] * f);
      if (lane == 0) part[wave][i][2 + d] = od;
    }
  }
  __syncthreads();
  // waves -> workgroup: lane i < QT finishes query q0 + i
  if (tid < QT && q0 + tid < p.Nq) {
    int mg = AP_NEG;
    for (int w = 0; w < NW; ++w) mg = max(mg, (int)part[w][tid][0]);
    float lg = 0.f, og[D];
#pragma unroll
    for (int d = 0; d < D; ++d) og[d] = 0.f;
    for (int w = 0; w < NW; ++w) {
      const int mw = (int)part[w][tid][0];
      const float f = mw == AP_NEG ? 0.f : __builtin_amdgcn_exp2f((float)(mw - mg) * p.k2);
      lg = fmaf(part[w][tid][1], f, lg);
#pragma unroll
      for (int d = 0; d < D; ++d) og[d] = fmaf(part[w][tid][2 + d], f, og[d]);
    }
    ap_store<D>(p, og, lg, p.out + ((int64_t)b * p.Nq + q0 + tid) * HD + h * D);
  }
}

// ---------------------------------------------------------------- one lane per query
// grid (ceil(Nq / 64 NW), B * H); the head's keys / values through LDS, KT at a time
template <int D, int NW>
__global__ __launch_bounds__(64 * NW) void attention_q8_plain_rows_kernel(AttnPlainParams p) {
  constexpr int NT = 64 * NW, DW = D / 4, KT = 64;
  __shared__ int ks[KT][DW], vs[KT][DW];
  const int tid = threadIdx.x;
  const int b = blockIdx.y / p.H, h = blockIdx.y % p.H;
  const int HD = p.H * D;
  const int qi = blockIdx.x * NT + tid;
  const bool live = qi < p.Nq;
  const float inv_a1 = 1.0f / p.s_a1;
  int qw[DW];
  {
    const int* src = (const int*)(p.q + ((int64_t)b * p.Nq + (live ? qi : p.Nq - 1)) * HD + h * D);
#pragma unroll
    for (int e = 0; e < DW; ++e) qw[e] = src[e];
  }
  int m = AP_NEG;
  float l = 0.f, o[D];
#pragma unroll
  for (int d = 0; d < D; ++d) o[d] = 0.f;
  for (int j0 = 0; j0 < p.Nk; j0 += KT) {
    const int nk = min(KT, p.Nk - j0);
    __syncthreads();   // the previous tile has been read
    for (int idx = tid; idx < nk * DW; idx += NT) {
      const int64_t off = ((int64_t)b * p.Nk + j0 + idx / DW) * HD + h * D;
      ks[idx / DW][idx % DW] = ((const int*)(p.k + off))[idx % DW];
      vs[idx / DW][idx % DW] = ((const int*)(p.v + off))[idx % DW];
    }
    __syncthreads();
    for (int j = 0; j < nk; ++j) {
      int kw[DW], vw[DW];
#pragma unroll
      for (int e = 0; e < DW; ++e) {
        kw[e] = ks[j][e];
        vw[e] = vs[j][e];
      }
      ap_update<D>(ap_score<D>(p, dot_codes<D>(qw, kw), inv_a1), vw, p.k2, m, l, o);
    }
  }
  if (live) ap_store<D>(p, o, l, p.out + ((int64_t)b * p.Nq + qi) * HD + h * D);
}

}  // namespace samq

using namespace samq;

extern "C" int samq_attention_q8_plain(const int8_t* q, const int8_t* k, const int8_t* v, int8_t* out, int B, int Nq,
                                       int Nk, int heads, int hd, float s_q, float s_k, float s_v, float s_a1,
                                       float s_out, hipStream_t stream) {
  SAMQ_REQUIRE(B >= 0 && Nq >= 0 && Nk >= 0 && heads > 0, SAMQ_ERR_INVALID, "attention_q8_plain: bad shape");
  SAMQ_REQUIRE(hd == 16 || hd == 32, SAMQ_ERR_UNSUPPORTED, "attention_q8_plain: head_dim must be 16 or 32");
  SAMQ_REQUIRE((int64_t)heads * hd <= 256, SAMQ_ERR_UNSUPPORTED, "attention_q8_plain: heads * head_dim must be <= 256");
  if (B == 0 || Nq == 0) return SAMQ_OK;   // no query: nothing to write, data pointers may be null
  SAMQ_REQUIRE(Nk >= 1, SAMQ_ERR_INVALID, "attention_q8_plain: a softmax over no key");
  SAMQ_REQUIRE(q && k && v && out, SAMQ_ERR_INVALID, "attention_q8_plain: null pointer");
  SAMQ_REQUIRE(s_q > 0.f && s_k > 0.f && s_v > 0.f && s_a1 > 0.f && s_out > 0.f, SAMQ_ERR_INVALID,
               "attention_q8_plain: scales must be > 0");
  SAMQ_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0, SAMQ_ERR_INVALID,
               "attention_q8_plain: pointers must be 16-byte aligned");
  SAMQ_REQUIRE((int64_t)B * heads < 65536 && (int64_t)B * Nq * heads * hd < ((int64_t)1 << 40) &&
               Nq < (1 << 30) && Nk < (1 << 30), SAMQ_ERR_UNSUPPORTED, "attention_q8_plain: shape too large");
  AttnPlainParams p{q, k, v, out, B, Nq, Nk, heads,
                    (float)((double)s_q * (double)s_k / sqrt((double)hd)), s_a1,
                    (float)((double)s_a1 * 1.4426950408889634), s_v, s_out};
  if (Nq <= 16 && Nk > 64) {   // keys over the lanes
    const int nw = Nk > 2048 ? 8 : (Nk > 512 ? 4 : (Nk > 128 ? 2 : 1));
#define AP_KEYS(D_, QT_, NW_)                                                                              \
  hipLaunchKernelGGL((attention_q8_plain_keys_kernel<D_, QT_, NW_>), dim3(B * heads, (Nq + QT_ - 1) / QT_), \
                     dim3(64 * NW_), 0, stream, p)
#define AP_KEYS_NW(D_, QT_)              \
  do {                                   \
    if (nw == 8) AP_KEYS(D_, QT_, 8);    \
    else if (nw == 4) AP_KEYS(D_, QT_, 4); \
    else if (nw == 2) AP_KEYS(D_, QT_, 2); \
    else AP_KEYS(D_, QT_, 1);            \
  } while (0)
    if (hd == 16) AP_KEYS_NW(16, 4);
    else AP_KEYS_NW(32, 2);
#undef AP_KEYS_NW
#undef AP_KEYS
  } else {
    const unsigned by = (unsigned)(B * heads);
    if (Nq <= 64) {
      if (hd == 16) hipLaunchKernelGGL((attention_q8_plain_rows_kernel<16, 1>), dim3(1, by), dim3(64), 0, stream, p);
      else hipLaunchKernelGGL((attention_q8_plain_rows_kernel<32, 1>), dim3(1, by), dim3(64), 0, stream, p);
    } else {
      const unsigned bx = (unsigned)((Nq + 255) / 256);
      if (hd == 16) hipLaunchKernelGGL((attention_q8_plain_rows_kernel<16, 4>), dim3(bx, by), dim3(256), 0, stream, p);
      else hipLaunchKernelGGL((attention_q8_plain_rows_kernel<32, 4>), dim3(bx, by), dim3(256), 0, stream, p);
    }
  }
  SAMQ_LAUNCH_CHECK("attention_q8_plain launch");
  return SAMQ_OK;
}
