// Next click of the RITM click simulator (Clicker._get_next_click with padding): from a predicted mask and a
// ground truth on the device, the exact squared Euclidean distance transform of the false-negative and the
// false-positive mask (each padded by a ring of zeros), the first deepest pixel of the larger error region and
// the IoU counts -- eight integers per mask, no mask or distance image copied to the host.  Integers only:
//   d2(y, x) = min over x' in [-1, W] of (x - x')^2 + g(y, x')^2,   g(y, -1) = g(y, W) = 0,
//   g(y, x)  = distance from (y, x) to the nearest zero of column x, with zeros at y = -1 and y = H
// (separable and exact), so ties break the same way on every run.  Four launches on one stream, no atomics:
//
//   nc_bits    one wave per 64 columns x 64 rows (a SEGMENT): a lane owns a column and packs the segment's
//              fn / fp bits into one 64-bit word each (rows of pred / gt are read coalesced, eight rows in
//              flight); the words go to the workspace ([segment][map][W], 1/4 byte per pixel).  It has seen
//              every pixel, so it also counts inter / union (lane-private adds, one wave fold at the end).
//   nc_colg    same grid.  Inside a segment g is bit arithmetic on the lane's word: the run of ones ending at
//              row i is clz((~m) << (63 - i)), the run starting there ctz((~m) >> i).  Where a run reaches the
//              segment's end it continues through the CARRY: the distance from the segment's first (last) row
//              to the nearest zero above (below), found by walking the column's words of the other segments --
//              whole words of ones add 64, the first other word ends the walk with one clz / ctz, the virtual
//              zeros at -1 and H end it otherwise.  At most H / 64 - 1 <= 63 coalesced 8-byte reads per lane;
//              "nearest zero above / below" compose min-plus, so no look-back and no second pass over pixels.
//              g of both maps leaves as one dword per pixel (uint16 fn | uint16 fp << 16).
//   nc_rows    a workgroup of four waves owns RB rows; wave w takes map w & 1 and every second row.  The
//              row's g (uint16) sits in the wave's LDS slice, framed by four zeros on each side: slot -1 and
//              slot W ARE the padded ring, the other three absorb the unrolled probes.  A lane owns pixels
//              x = lane + 64 j (neighbouring lanes read neighbouring LDS halves: unit stride).  It
//              starts from best = g(y, x)^2 and probes x -+ k, k = 1, 2, .., four k per trip, while
//              k^2 < best: the four probes of one side are consecutive halves (hipcc of ROCm 7.2 merges
//              them into one 8-byte read), a probe then costs one v_mad_u32_u24 and a share of the min
//              tree.  Probes past the stopping k only offer candidates that are no smaller than the
//              minimum, so the unroll is exact.  A row whose g is all zero (one ballot) and pixels with g = 0 cost nothing.  The
//              clicked list lives in two VGPRs (lane j holds click j): one ballot per row says whether the row
//              holds a click at all.  (d2, first index) folds as d2 << 32 | (2^32 - 1 - index) under max: per
//              lane, across the wave by shuffles, across the waves in LDS, one row per workgroup out.
//   nc_finish  one wave per mask folds the workgroups' rows in a fixed order and writes the eight integers.
#include "common.h"

namespace samq {
namespace {

constexpr int NC_SEG = 64;        // rows per column segment: one bit each of a 64-bit word
constexpr int NC_COLS = 64;       // columns per wave / workgroup of nc_bits and nc_colg
constexpr int NC_PAD = 4;         // zeros on each side of a staged row = probes per trip of the search
constexpr int NC_MAX_SIDE = 4096; // g <= 2048 fits uint16, d2 <= 2^23 fits int32
constexpr int NC_MAX_CLICKS = 64;

struct NextClickPlan {
  int segs, col_tiles, rb, row_blocks, stride;
  size_t off_part, off_g, off_cnt, bytes;
};

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const u64 t = ((u64)hi << 32) | lo;
    v = t > v ? t : v;
  }
  return v;
}

__global__ __launch_bounds__(64) void nc_bits(const uint8_t* __restrict__ pred, const int8_t* __restrict__ gt,
                                              u64* __restrict__ bits, int* __restrict__ cnt, int H, int W, int segs,
                                              int col_tiles, int ignore) {
  const int lane = threadIdx.x;
  const int n = blockIdx.x / col_tiles, tile = blockIdx.x % col_tiles, s = blockIdx.y;
  const int x = tile * NC_COLS + lane, y0 = s * NC_SEG;
  const bool col = x < W;
  const size_t base = (size_t)n * H * W + (col ? x : 0);
  u64 mfn = 0, mfp = 0;
  int inter = 0, uni = 0;
  for (int i0 = 0; i0 < NC_SEG && y0 + i0 < H; i0 += 8) {
    uint8_t p[8];
    int8_t t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int y = y0 + i0 + j;
      const bool ok = col && y < H;
      const size_t o = base + (size_t)(ok ? y : y0) * W;   // a row of this mask either way
      p[j] = col ? pred[o] : 0;
      t[j] = col ? gt[o] : 0;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool keep = col && y0 + i0 + j < H && t[j] != ignore;
      const bool obj = t[j] == 1, pr = p[j] != 0;
      mfn |= (u64)(keep && obj && !pr) << (i0 + j);
      mfp |= (u64)(keep && !obj && pr) << (i0 + j);
      inter += keep && obj && pr;
      uni += keep && (obj || pr);
    }
  }
  if (col) {
    u64* b = bits + ((size_t)n * segs + s) * 2 * W + x;
    b[0] = mfn;
    b[W] = mfp;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    inter += __shfl_xor(inter, o, 64);
    uni += __shfl_xor(uni, o, 64);
  }
  if (lane < 2) cnt[((size_t)blockIdx.x * segs + s) * 2 + lane] = lane ? uni : inter;
}

// distance from the first row of segment s to the nearest zero above it (>= 1; the zero at y = -1 ends it)
__device__ __forceinline__ int carry_above(const u64* col, size_t seg_stride, int s) {
  int acc = 1;
  for (int t = s - 1; t >= 0; --t) {
    const u64 z = ~col[(size_t)t * seg_stride];
    if (z) return acc + (int)__builtin_clzll(z);
    acc += NC_SEG;
  }
  return acc;
}
// distance from row 63 of segment s to the nearest zero below it; rows past H are zero bits of the last word,
// and a last word of 64 ones ends at the zero at y = H
__device__ __forceinline__ int carry_below(const u64* col, size_t seg_stride, int s, int segs) {
  int acc = 1;
  for (int t = s + 1; t < segs; ++t) {
    const u64 z = ~col[(size_t)t * seg_stride];
    if (z) return acc + (int)__builtin_ctzll(z);
    acc += NC_SEG;
  }
  return acc;
}

__global__ __launch_bounds__(64) void nc_colg(const u64* __restrict__ bits, uint32_t* __restrict__ g, int H, int W,
                                              int segs, int col_tiles) {
  const int n = blockIdx.x / col_tiles, tile = blockIdx.x % col_tiles, s = blockIdx.y;
  const int x = tile * NC_COLS + (int)threadIdx.x, y0 = s * NC_SEG;
  if (x >= W) return;
  const size_t seg_stride = 2 * (size_t)W;
  const u64* col = bits + (size_t)n * segs * seg_stride + x;   // [segment][map][W]
  const u64 m[2] = {col[s * seg_stride], col[s * seg_stride + W]};
  int up[2], dn[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    up[k] = carry_above(col + k * W, seg_stride, s);
    dn[k] = carry_below(col + k * W, seg_stride, s, segs);
  }
  uint32_t* out = g + ((size_t)n * H + y0) * W + x;
  const int len = min(NC_SEG, H - y0);
  for (int i = 0; i < len; ++i) {
    uint32_t v[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const u64 za = (~m[k]) << (63 - i), zb = (~m[k]) >> i;
      const int a = za ? (int)__builtin_clzll(za) : i + up[k];
      const int b = zb ? (int)__builtin_ctzll(zb) : 63 - i + dn[k];
      v[k] = (uint32_t)min(a, b);
    }
    out[(size_t)i * W] = v[0] | (v[1] << 16);
  }
}

__global__ __launch_bounds__(256) void nc_rows(const uint32_t* __restrict__ g, const int* __restrict__ clicked, int K,
                                               int H, int W, int rb, int row_blocks, int stride,
                                               int* __restrict__ d2, u64* __restrict__ part) {
  extern __shared__ uint16_t staged[];
  __shared__ u64 wkey[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, map = wave & 1;
  const int n = blockIdx.x / row_blocks, r0 = (blockIdx.x % row_blocks) * rb;
  uint16_t* row = staged + wave * stride + NC_PAD;   // row[-4 .. -1] and row[W .. W + 3] stay zero
  if (lane < NC_PAD) row[lane - NC_PAD] = 0, row[W + lane] = 0;
  int cy = -1, cx = -1;
  if (lane < K) cy = clicked[((size_t)n * K + lane) * 2], cx = clicked[((size_t)n * K + lane) * 2 + 1];

  u64 key = 0xFFFFFFFFull;   // d2 = 0 at pixel (0, 0): what an all-zero map selects
  for (int j = wave >> 1; j < rb; j += 2) {   // the same trip count in every wave: rb is even
    const int y = r0 + j;
    const bool live = y < H;
    const size_t ro = ((size_t)n * H + (live ? y : 0)) * W;
    unsigned any = 0;
    __syncthreads();   // the previous row's probes are done
    if (live)
      for (int x = lane; x < W; x += 64) {
        const uint32_t v = g[ro + x];
        const unsigned gv = map ? v >> 16 : v & 0xFFFFu;
        row[x] = (uint16_t)gv;
        any |= gv;
      }
    __syncthreads();
    if (!live || (!__ballot(any != 0) && !d2)) continue;
    const unsigned long long hit = __ballot(cy == y);
    for (int xb = 0; xb < W; xb += 64) {
      const int x = xb + lane;
      const bool act = x < W;
      const unsigned gx = act ? row[x] : 0;
      unsigned best = gx * gx;
      for (int k = 1; (unsigned)(k * k) < best; k += NC_PAD) {
#pragma unroll
        for (int u = 0; u < NC_PAD; ++u) {
          const unsigned a = row[x - k - u], b = row[x + k + u], kk = (unsigned)((k + u) * (k + u));
          best = min(best, min(a * a + kk, b * b + kk));
        }
      }
      if (d2 && act) d2[(((size_t)n * 2 + map) * H + y) * W + x] = (int)best;
      for (unsigned long long h = hit; h; h &= h - 1)
        if (x == __builtin_amdgcn_readlane(cx, (int)__builtin_ctzll(h))) best = 0;
      if (best) {
        const u64 c = ((u64)best << 32) | (0xFFFFFFFFu - (unsigned)(y * W + x));
        key = c > key ? c : key;
      }
    }
  }
  key = wave_max_u64(key);
  if (lane == 0) wkey[wave] = key;
  __syncthreads();
  if (tid < 2) part[(size_t)blockIdx.x * 2 + tid] = wkey[tid] > wkey[tid + 2] ? wkey[tid] : wkey[tid + 2];
}

// one wave per mask: the row blocks' keys (max) and the segments' counts (sum), in a fixed order
__global__ __launch_bounds__(64) void nc_finish(const u64* __restrict__ part, const int* __restrict__ cnt,
                                                int* __restrict__ out, int row_blocks, int cnt_rows, int W) {
  const int lane = threadIdx.x, n = blockIdx.x;
  u64 kfn = 0xFFFFFFFFull, kfp = 0xFFFFFFFFull;
  for (int r = lane; r < row_blocks; r += 64) {
    const u64 a = part[((size_t)n * row_blocks + r) * 2], b = part[((size_t)n * row_blocks + r) * 2 + 1];
    kfn = a > kfn ? a : kfn;
    kfp = b > kfp ? b : kfp;
  }
  int inter = 0, uni = 0;
  for (int r = lane; r < cnt_rows; r += 64) {
    inter += cnt[((size_t)n * cnt_rows + r) * 2];
    uni += cnt[((size_t)n * cnt_rows + r) * 2 + 1];
  }
  kfn = wave_max_u64(kfn), kfp = wave_max_u64(kfp);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    inter += __shfl_xor(inter, o, 64);
    uni += __shfl_xor(uni, o, 64);
  }
  if (lane == 0) {
    const int fn_max = (int)(kfn >> 32), fp_max = (int)(kfp >> 32);
    const bool pos = fn_max > fp_max;   // a tie is a negative click
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(pos ? kfn : kfp);
    int* o = out + (size_t)n * 8;
    o[0] = pos, o[1] = (int)(idx / (unsigned)W), o[2] = (int)(idx % (unsigned)W), o[3] = fn_max, o[4] = fp_max;
    o[5] = inter, o[6] = uni, o[7] = 0;
  }
}

// the guards of the C entry, the grid and the workspace layout of one call
int plan(int n, int H, int W, NextClickPlan& p) {
  SAMQ_REQUIRE(n >= 1 && n < (1 << 16), SAMQ_ERR_INVALID, "next_click: mask count outside 1 .. 65535");
  SAMQ_REQUIRE(H >= 1 && W >= 1 && H <= NC_MAX_SIDE && W <= NC_MAX_SIDE, SAMQ_ERR_INVALID,
               "next_click: H and W must be 1 .. 4096");
  p.segs = (H + NC_SEG - 1) / NC_SEG;
  p.col_tiles = (W + NC_COLS - 1) / NC_COLS;
  // rows per workgroup of the row pass: 16, fewer while the grid would leave most of the device idle
  p.rb = 16;
  while (p.rb > 2 && (int64_t)n * ((H + p.rb - 1) / p.rb) < 2048) p.rb >>= 1;
  p.row_blocks = (H + p.rb - 1) / p.rb;
  p.stride = (W + 2 * NC_PAD + 7) & ~7;
  const size_t bits = (size_t)n * p.segs * 2 * W * sizeof(u64);
  p.off_part = bits;
  p.off_g = p.off_part + (size_t)n * p.row_blocks * 2 * sizeof(u64);
  p.off_cnt = p.off_g + (size_t)n * H * W * sizeof(uint32_t);
  p.bytes = (p.off_cnt + (size_t)n * p.col_tiles * p.segs * 2 * sizeof(int) + 7) & ~(size_t)7;   // g is 4 n H W
  return SAMQ_OK;
}

}  // namespace
}  // namespace samq

using namespace samq;

extern "C" size_t samq_next_click_workspace(int n, int H, int W) {
  NextClickPlan p;
  if (n <= 0 || plan(n, H, W, p) != SAMQ_OK) return 0;
  return p.bytes;
}

extern "C" int samq_next_click(const uint8_t* pred, const int8_t* gt, const int32_t* clicked, int K, int n, int H,
                               int W, int ignore_label, int32_t* out, int32_t* d2, void* workspace,
                               size_t workspace_bytes, hipStream_t stream) {
  if (n == 0) return SAMQ_OK;
  NextClickPlan p;
  if (const int st = plan(n, H, W, p)) return st;
  SAMQ_REQUIRE(K >= 0 && K <= NC_MAX_CLICKS, SAMQ_ERR_INVALID, "next_click: K must be 0 .. 64");
  SAMQ_REQUIRE(pred && gt && out && workspace && (clicked || K == 0), SAMQ_ERR_INVALID, "next_click: null pointer");
  SAMQ_REQUIRE((((uintptr_t)out | (uintptr_t)d2 | (uintptr_t)clicked) & 3) == 0 && ((uintptr_t)workspace & 7) == 0,
               SAMQ_ERR_INVALID, "next_click: misaligned pointer");
  SAMQ_REQUIRE(workspace_bytes >= p.bytes, SAMQ_ERR_INVALID, "next_click: workspace too small");
  char* ws = (char*)workspace;
  u64* bits = (u64*)ws;
  u64* part = (u64*)(ws + p.off_part);
  uint32_t* g = (uint32_t*)(ws + p.off_g);
  int* cnt = (int*)(ws + p.off_cnt);

  const dim3 cgrid((unsigned)(n * p.col_tiles), (unsigned)p.segs);
  hipLaunchKernelGGL(nc_bits, cgrid, dim3(64), 0, stream, pred, gt, bits, cnt, H, W, p.segs, p.col_tiles, ignore_label);
  hipLaunchKernelGGL(nc_colg, cgrid, dim3(64), 0, stream, (const u64*)bits, g, H, W, p.segs, p.col_tiles);
  hipLaunchKernelGGL(nc_rows, dim3((unsigned)(n * p.row_blocks)), dim3(256), 4 * (size_t)p.stride * sizeof(uint16_t),
                     stream, (const uint32_t*)g, clicked, K, H, W, p.rb, p.row_blocks, p.stride, d2, part);
  hipLaunchKernelGGL(nc_finish, dim3((unsigned)n), dim3(64), 0, stream, (const u64*)part, (const int*)cnt, out,
                     p.row_blocks, p.col_tiles * p.segs, W);
  SAMQ_LAUNCH_CHECK("next_click launch");
  return SAMQ_OK;
}
