// Mask post-processing: Sam.postprocess_masks (two bilinear resizes with a crop between them), the mask
// threshold, the three pixel counts of calculate_stability_score and batched_mask_to_box, in one pass over
// the low-res logits.  Nothing of the padded-input or the original size is ever written in fp32: per mask
// the kernel reads lh * lw logits and writes H * W mask bytes and eight integers.
//
// The composition of the two resizes is separable and banded.  An output row y reads two ADJACENT rows
// j0, j0 + 1 of the padded-input image (stage 2), each of which reads two adjacent low-res rows (stage 1),
// and the two pairs overlap or touch: together at most three consecutive low-res rows R .. R + 2.  So
//   v(y, x) = sum_{a < 3} sum_{b < 3} wy[a] wx[b] low[R(y) + a][C(x) + b]
// with the four weight products of each axis folded (edge clamps included) into three weights.  Every
// coordinate follows torch's fp32 rule (area_pixel_compute_source_index, align_corners = False).  When the
// input size equals the original size stage 2 is the identity and a two-tap instance runs (TAPS = 2).
//
// Work split: a workgroup of four waves owns a band of bh = 4 rw output rows by 256 output columns of one
// mask; wave w owns rows w rw .. w rw + rw - 1 of the band, a lane four consecutive columns.  The low-res
// rectangle the band can touch is staged in LDS once (fp32; fp16 logits are converted here).  Per wave:
//   columns  a lane folds its four columns' base C and weights once and keeps them in registers;
//   rows     lane i folds output row i of the wave's rows; the row loop broadcasts (R, wy) by v_readlane,
//            so the row weights are SGPR operands of the FMAs;
//   window   R never decreases: the horizontal three-tap values of low-res rows R .. R + 2 stay in
//            registers (3 x 4 floats) and only new rows are formed (TAPS LDS reads and FMAs per column);
//   output   TAPS FMAs per pixel, three compares; the four mask bytes of a lane go out as one dword
//            (rows of an odd W are not dword aligned: the store is an unaligned global_store_dword),
//            the ragged last lane of a row stores bytes;
//   counts   s_bcnt1 of the three ballots per column, accumulated in SGPRs; the column-occupancy ballots
//            are ORed over the rows (first / last set lane = x extremes), the row extremes are scalar
//            compares: no cross-lane reduction at all;
//   combine  the four waves' counts and boxes meet in LDS and leave as ONE row of eight integers per
//            workgroup in the caller's workspace; mask_post_finish (one wave per mask, same stream) sums /
//            min-maxes a mask's rows in a fixed order and writes its stats row (empty mask -> box 0, 0, 0,
//            0).  No atomics: folded into the stats row directly, the ~10^3 same-address atomics of one
//            mask serialise (measured: N = 3 took longer than N = 192).
// All lanes of a wave read the SAME staged row at a time, so the row stride takes no part in bank
// conflicts; the rows are stored densely.  fp32 throughout; MFMA has no use for a 3-tap band.
#include "common.h"

#include <limits.h>

namespace samq {
namespace {

constexpr int MP_COLS = 256;                  // output columns per wave / workgroup (4 per lane)
constexpr int MP_LDS_MAX = 48 * 1024;         // staged rectangle, bytes

struct MaskPostArgs {
  int lh, ih, iw, H, W;
  int rw, bh;                 // rows per wave, rows per workgroup (<= 4 rw)
  int rows_cap, cols_cap;     // staged rectangle
  int col_tiles;
  float sy, sx;               // stage-2 scales ih / H, iw / W as torch forms them
  float thr, thr_hi, thr_lo;
};

template <int TAPS>
struct Fold {
  int base;
  float w[TAPS];
};

// stage 1 (low -> padded input, scale exactly 1/4): the two source indices and the weight of the second
__device__ __forceinline__ void stage1(int j, int lh, int& i0, int& i1, float& lam) {
  const float src = fmaxf(0.25f * ((float)j + 0.5f) - 0.5f, 0.f);
  i0 = min((int)src, lh - 1);
  i1 = i0 + (i0 < lh - 1 ? 1 : 0);
  lam = src - (float)i0;
}

// one axis of output index dst: the first low-res index it reads and the folded weights of base .. base + TAPS - 1
template <int TAPS>
__device__ __forceinline__ Fold<TAPS> fold_axis(int dst, float scale, int in2, int lh) {
  Fold<TAPS> f;
  if constexpr (TAPS == 2) {
    int i0, i1;
    float lam;
    stage1(dst, lh, i0, i1, lam);
    f.base = i0;
    f.w[0] = i1 == i0 ? (1.f - lam) + lam : 1.f - lam;
    f.w[1] = i1 == i0 ? 0.f : lam;
  } else {
    const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    const int j0 = min((int)src, in2 - 1), j1 = j0 + (j0 < in2 - 1 ? 1 : 0);
    const float mu = src - (float)j0, nu = 1.f - mu;
    int a0, a1, b0, b1;
    float la, lb;
    stage1(j0, lh, a0, a1, la);
    stage1(j1, lh, b0, b1, lb);
    f.base = a0;
    const float c0 = nu * (1.f - la), c1 = nu * la, c2 = mu * (1.f - lb), c3 = mu * lb;
    const int d1 = a1 - a0, d2 = b0 - a0, d3 = b1 - a0;   // 0 .. 2
#pragma unroll
    for (int a = 0; a < 3; ++a)
      f.w[a] = (((a == 0 ? c0 : 0.f) + (d1 == a ? c1 : 0.f)) + (d2 == a ? c2 : 0.f)) + (d3 == a ? c3 : 0.f);
  }
  return f;
}

__device__ __forceinline__ float lane_readf(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

typedef uint32_t u32_unaligned __attribute__((aligned(1)));

// one wave per mask: fold the mask's per-workgroup rows (counts add, box min / max), fixed order
__global__ __launch_bounds__(64) void mask_post_finish(const int* __restrict__ part, int* __restrict__ stats,
                                                       int wgs) {
  const int lane = threadIdx.x;
  const int* pm = part + (size_t)blockIdx.x * wgs * 8;
  int v[7] = {0, 0, 0, INT_MAX, INT_MAX, -1, -1};
  for (int g = lane; g < wgs; g += 64) {
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] += pm[g * 8 + j];
    v[3] = min(v[3], pm[g * 8 + 3]);
    v[4] = min(v[4], pm[g * 8 + 4]);
    v[5] = max(v[5], pm[g * 8 + 5]);
    v[6] = max(v[6], pm[g * 8 + 6]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] += __shfl_xor(v[j], o, 64);
    v[3] = min(v[3], __shfl_xor(v[3], o, 64));
    v[4] = min(v[4], __shfl_xor(v[4], o, 64));
    v[5] = max(v[5], __shfl_xor(v[5], o, 64));
    v[6] = max(v[6], __shfl_xor(v[6], o, 64));
  }
  if (lane < 8) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) r = lane == j ? v[j] : r;
    stats[(size_t)blockIdx.x * 8 + lane] = (lane >= 3 && v[2] == 0) ? 0 : r;
  }
}

template <int TAPS, bool F16>
__global__ __launch_bounds__(256) void mask_post_kernel(const void* __restrict__ low, uint8_t* __restrict__ mask,
                                                        int* __restrict__ part, const MaskPostArgs p) {
  extern __shared__ float stage[];
  __shared__ int wpart[4][8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x / p.col_tiles, c0 = (blockIdx.x % p.col_tiles) * MP_COLS;
  const int band0 = blockIdx.y * p.bh, band1 = min(band0 + p.bh, p.H);

  // ---- stage the low-res rectangle of this band and column tile; indices past the last low-res row /
  // column repeat it (those taps carry weight 0), so every staged word is a real logit
  const int Rlo = fold_axis<TAPS>(band0, p.sy, p.ih, p.lh).base;
  const int Clo = fold_axis<TAPS>(c0, p.sx, p.iw, p.lh).base;
  const size_t lbase = (size_t)n * p.lh * p.lh;
  for (int r = wave; r < p.rows_cap; r += 4) {
    const size_t ro = lbase + (size_t)min(Rlo + r, p.lh - 1) * p.lh;
    for (int c = lane; c < p.cols_cap; c += 64) {
      const size_t o = ro + min(Clo + c, p.lh - 1);
      stage[r * p.cols_cap + c] = F16 ? (float)((const _Float16*)low)[o] : ((const float*)low)[o];
    }
  }

  // ---- this lane's four columns
  const int x0 = c0 + 4 * lane;
  int cb[4];
  float wx[4][TAPS];
  unsigned long long live[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const Fold<TAPS> f = fold_axis<TAPS>(min(x0 + k, p.W - 1), p.sx, p.iw, p.lh);
    cb[k] = min(max(f.base - Clo, 0), p.cols_cap - TAPS);
#pragma unroll
    for (int b = 0; b < TAPS; ++b) wx[k][b] = f.w[b];
    live[k] = __ballot(x0 + k < p.W);
  }

  // ---- the wave's rows: lane i folds row y0 + i
  const int y0 = band0 + wave * p.rw, y1 = min(y0 + p.rw, band1);
  const Fold<TAPS> fy = fold_axis<TAPS>(min(y0 + lane, p.H - 1), p.sy, p.ih, p.lh);
  __syncthreads();

  auto hrow = [&](int r, float (&h)[4]) {
    const float* s = stage + min(max(r - Rlo, 0), p.rows_cap - 1) * p.cols_cap;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float acc = wx[k][0] * s[cb[k]];
#pragma unroll
      for (int b = 1; b < TAPS; ++b) acc = fmaf(wx[k][b], s[cb[k] + b], acc);
      h[k] = acc;
    }
  };

  float hw[TAPS][4];
  int cur = -TAPS - 1;    // low-res row of hw[0]; R >= 0, so the first row fills the whole window
  unsigned n_area = 0, n_hi = 0, n_lo = 0;
  unsigned long long colm[4] = {0, 0, 0, 0};
  int ymin = INT_MAX, ymax = -1;
  uint8_t* mp = mask ? mask + (size_t)n * p.H * p.W + (size_t)y0 * p.W + x0 : nullptr;
  const bool whole = x0 + 3 < p.W;

  for (int i = 0; i < y1 - y0; ++i) {   // no trip for a wave past the band's end
    const int R = __builtin_amdgcn_readlane(fy.base, i);
    float wy[TAPS];
#pragma unroll
    for (int a = 0; a < TAPS; ++a) wy[a] = lane_readf(fy.w[a], i);

    const int d = R - cur;
    if (d != 0) {
      if (d < 0 || d >= TAPS) {
#pragma unroll
        for (int a = 0; a < TAPS; ++a) hrow(R + a, hw[a]);
      } else if (d == 1) {
#pragma unroll
        for (int a = 0; a + 1 < TAPS; ++a)
#pragma unroll
          for (int k = 0; k < 4; ++k) hw[a][k] = hw[a + 1][k];
        hrow(R + TAPS - 1, hw[TAPS - 1]);
      } else {   // d == 2 (three taps only)
#pragma unroll
        for (int k = 0; k < 4; ++k) hw[0][k] = hw[TAPS - 1][k];
#pragma unroll
        for (int a = 1; a < TAPS; ++a) hrow(R + a, hw[a]);
      }
      cur = R;
    }

    uint32_t word = 0;
    unsigned long long any = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v = wy[0] * hw[0][k];
#pragma unroll
      for (int a = 1; a < TAPS; ++a) v = fmaf(wy[a], hw[a][k], v);
      const bool m = v > p.thr;
      const unsigned long long bm = __ballot(m) & live[k];
      n_area += __popcll(bm);
      n_hi += __popcll(__ballot(v > p.thr_hi) & live[k]);
      n_lo += __popcll(__ballot(v > p.thr_lo) & live[k]);
      colm[k] |= bm;
      any |= bm;
      word |= (m ? 1u : 0u) << (8 * k);
    }
    if (any) {
      ymin = min(ymin, y0 + i);
      ymax = y0 + i;
    }
    if (mp) {
      if (whole) {
        *(u32_unaligned*)mp = word;
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (x0 + k < p.W) mp[k] = (uint8_t)((word >> (8 * k)) & 1u);
      }
      mp += p.W;
    }
  }

  if (lane == 0) {
    int xmin = INT_MAX, xmax = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (colm[k]) {
        xmin = min(xmin, c0 + 4 * (int)__builtin_ctzll(colm[k]) + k);
        xmax = max(xmax, c0 + 4 * (63 - (int)__builtin_clzll(colm[k])) + k);
      }
    int* w = wpart[wave];
    w[0] = (int)n_hi, w[1] = (int)n_lo, w[2] = (int)n_area, w[3] = xmin, w[4] = ymin, w[5] = xmax, w[6] = ymax;
  }
  __syncthreads();
  if (tid < 7) {
    int r = wpart[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const int o = wpart[w][tid];
      r = tid < 3 ? r + o : tid < 5 ? min(r, o) : max(r, o);
    }
    // blockIdx.x is mask-major, so a mask's col_tiles * gridDim.y rows are contiguous
    part[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 8 + tid] = r;
  }
}

// low-res rows (columns) a run of `count` output rows (columns) can touch, from the first one's base:
// the stage-2 index moves by at most (count - 1) s + 1, a quarter of that plus one in low-res rows, plus
// the TAPS rows of the last output row; one more for the fp32 rounding of the device's coordinates
int staged_extent(int count, double s, int taps, int lh) {
  const int e = (int)(0.25 * ((count - 1) * s + 1.0)) + 2 + taps;
  return e < lh + taps - 1 ? e : lh + taps - 1;
}

// the launch plan of one call: the guards of the C entry, the band height, the staged rectangle
int plan(int N, int lh, int lw, int img_size, int ih, int iw, int H, int W, MaskPostArgs& p, int& bands) {
  SAMQ_REQUIRE(N > 0 && N < (1 << 27), SAMQ_ERR_INVALID, "mask_postprocess: mask count outside 0 .. 2^27");
  SAMQ_REQUIRE(lh >= 1 && lh == lw, SAMQ_ERR_INVALID, "mask_postprocess: the low-res masks must be square");
  SAMQ_REQUIRE(lh <= (1 << 20) && img_size == 4 * lh, SAMQ_ERR_INVALID,
               "mask_postprocess: img_size must be 4 times the low-res side");
  SAMQ_REQUIRE(ih >= 1 && iw >= 1 && H >= 1 && W >= 1, SAMQ_ERR_INVALID, "mask_postprocess: sizes must be >= 1");
  SAMQ_REQUIRE(ih <= img_size && iw <= img_size, SAMQ_ERR_INVALID, "mask_postprocess: input_size exceeds img_size");
  SAMQ_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), SAMQ_ERR_INVALID, "mask_postprocess: H * W must be below 2^31");
  const bool ident = ih == H && iw == W;
  const int taps = ident ? 2 : 3;
  p.lh = lh, p.ih = ih, p.iw = iw, p.H = H, p.W = W;
  p.sy = (float)ih / (float)H, p.sx = (float)iw / (float)W;
  p.col_tiles = (W + MP_COLS - 1) / MP_COLS;
  SAMQ_REQUIRE((int64_t)N * p.col_tiles < ((int64_t)1 << 31), SAMQ_ERR_UNSUPPORTED, "mask_postprocess: too many masks");

  // rows per wave: 16, fewer while the grid would leave most of the device idle (one click: N = 3)
  int rw = 16, nw = 4;
  while (rw > 4 && (int64_t)N * p.col_tiles * ((H + 4 * rw - 1) / (4 * rw)) < 1024) rw >>= 1;
  const double sy = ident ? 1.0 : (double)ih / H, sx = ident ? 1.0 : (double)iw / W;
  p.cols_cap = staged_extent(W < MP_COLS ? W : MP_COLS, sx, taps, lh);
  for (;;) {   // a steep downscale spreads a band over many low-res rows: shrink the band until it fits
    p.rows_cap = staged_extent(rw * nw, sy, taps, lh);
    if ((size_t)p.rows_cap * p.cols_cap * sizeof(float) <= (size_t)MP_LDS_MAX) break;
    if (rw > 1) rw >>= 1;
    else if (nw > 1) nw >>= 1;
    else return fail(SAMQ_ERR_UNSUPPORTED, "mask_postprocess: one output row's low-res taps exceed the LDS stage");
  }
  p.rw = rw, p.bh = rw * nw;
  bands = (H + p.bh - 1) / p.bh;
  SAMQ_REQUIRE(bands <= 65535, SAMQ_ERR_UNSUPPORTED, "mask_postprocess: too many row bands");
  return SAMQ_OK;
}

}  // namespace
}  // namespace samq

using namespace samq;

extern "C" size_t samq_mask_postprocess_workspace(int N, int lh, int lw, int img_size, int ih, int iw, int H, int W) {
  MaskPostArgs p;
  int bands;
  if (N <= 0 || plan(N, lh, lw, img_size, ih, iw, H, W, p, bands) != SAMQ_OK) return 0;
  return (size_t)N * p.col_tiles * bands * 8 * sizeof(int);
}

extern "C" int samq_mask_postprocess(const void* low, int low_f16, int N, int lh, int lw, int img_size, int ih, int iw,
                                     int H, int W, float thr, float off, uint8_t* mask, int32_t* stats,
                                     void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (N == 0) return SAMQ_OK;
  MaskPostArgs p;
  int bands;
  if (const int st = plan(N, lh, lw, img_size, ih, iw, H, W, p, bands)) return st;
  SAMQ_REQUIRE(off >= 0.f, SAMQ_ERR_INVALID, "mask_postprocess: offset must be >= 0");
  SAMQ_REQUIRE(low && stats && workspace, SAMQ_ERR_INVALID, "mask_postprocess: null pointer");
  SAMQ_REQUIRE(((uintptr_t)low & (low_f16 ? 1 : 3)) == 0 && (((uintptr_t)stats | (uintptr_t)workspace) & 3) == 0,
               SAMQ_ERR_INVALID, "mask_postprocess: misaligned pointer");
  const int wgs = p.col_tiles * bands;   // per mask
  SAMQ_REQUIRE(workspace_bytes >= (size_t)N * wgs * 8 * sizeof(int), SAMQ_ERR_INVALID,
               "mask_postprocess: workspace too small");
  p.thr = thr, p.thr_hi = (float)((double)thr + (double)off), p.thr_lo = (float)((double)thr - (double)off);
  const size_t lds = (size_t)p.rows_cap * p.cols_cap * sizeof(float);
  const bool ident = ih == H && iw == W;
  int* part = (int*)workspace;

  const dim3 grid((unsigned)(N * p.col_tiles), (unsigned)bands), block(256);
#define SAMQ_MP_LAUNCH(T, F) hipLaunchKernelGGL((mask_post_kernel<T, F>), grid, block, lds, stream, low, mask, part, p)
  if (ident) {
    if (low_f16) SAMQ_MP_LAUNCH(2, true); else SAMQ_MP_LAUNCH(2, false);
  } else {
    if (low_f16) SAMQ_MP_LAUNCH(3, true); else SAMQ_MP_LAUNCH(3, false);
  }
#undef SAMQ_MP_LAUNCH
  hipLaunchKernelGGL(mask_post_finish, dim3((unsigned)N), dim3(64), 0, stream, (const int*)part, stats, wgs);
  SAMQ_LAUNCH_CHECK("mask_postprocess launch");
  return SAMQ_OK;
}
