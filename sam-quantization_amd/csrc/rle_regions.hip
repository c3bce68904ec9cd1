// Small-region removal on the run-length encoding itself:
//   remove_small_regions(mask, min_area, "holes") then (.., "islands")      (segment_anything/utils/amg.py)
// per mask of a CSR batch as samq_mask_rle_* writes it, with no mask image anywhere.  Connected components with
// 8-connectivity are taken over vertical SEGMENTS: a run cut at the column boundaries (flat index a multiple
// of H), (column X, rows [y_lo, y_hi), value).  The segments of a mask tile [0, H W) in flat order, so one
// array of start positions holds them (segment g ends where g + 1 starts), every column starts a segment, and
// a mask of R runs has at most R + W - 1 of them.
//
// Two segments of equal value are joined when
//   * they lie in neighbouring columns and rows [y_lo - 1, y_hi + 1) of one meet rows [y_lo, y_hi) of the other,
//   * or they follow each other in one column (equal values there exist only after a hole fill).
// The last pixel of a column and the first of the next are no neighbours, although one run may cover both.
//
// label (one workgroup per mask, then one wave for the new offsets):
//   runs      block scan of the run lengths -> run starts; a second block scan of the per-run segment counts
//             -> the first segment of every run (both into the workspace).
//   segments  segment g finds its run by binary search in the scanned segment counts and writes its start and
//             value; the segment with y_lo == 0 writes col_first[X].
//   holes     union-find over the value-0 segments: a segment binary-searches col_first[X - 1] .. col_first[X]
//             for the first left neighbour ending at or below y_lo, walks while the neighbour starts at or above
//             y_hi, and unions with those of its value.  Parents are int32 indices; find halves paths; union
//             hooks the LARGER root under the smaller with atomicCAS, so the root of a component is its first
//             segment in Fortran order whatever the interleaving.  After a barrier every segment walks to its
//             root (reading only), stores it as its parent and adds its length to the root's area; components
//             below min_area flip to 1.
//   islands   the same over the value-1 segments of the filled mask.  If a component is small, only those that
//             are not small stay; if none is left the largest stays, a block max over (area, -root): an exact
//             tie goes to the component holding the earliest pixel in column-major order.
//   count     a transition sits where a segment's final value differs from the previous one's (0 before the
//             first); their number, the box, the area and the flag go to `stats`, the final values stay in the
//             workspace.
// write (one workgroup per mask): block scan of the transition flags -> their flat positions in rank order,
//   then the run lengths into the new row.
// Parents and areas live in LDS (the launch's dynamic LDS) when the mask has at most RGN_LDS_SEGS segments,
// else in the mask's workspace slice: the same code, instantiated on either pointer.  Integer atomics only
// (compare-and-swap on parents, add on areas), and the outcome of both is order independent: the output is
// the same on every run.
//
// Run lengths are clamped (negative -> 0, running start -> H W, the last run closes at H W) and row bounds are
// clamped to [0, total_in], so a row that breaks the contract changes only its own result: every index stays
// inside the buffers the caller sized.
#include "common.h"

namespace samq {
namespace {

constexpr int RGN_THREADS = 256;
constexpr int RGN_WAVES = RGN_THREADS / 64;
constexpr int RGN_CHUNK = 4 * RGN_THREADS;    // items per block-scan step, four per thread
// Segments whose parents and areas (8 bytes each) fit the dynamic LDS of one workgroup: 128 KiB of gfx950's
// 160 KiB, the rest left to the static reduction scratch.
constexpr int RGN_LDS_SEGS = 16384;

struct RgnArgs {
  int n, H, W, HW, min_area;
  int lds_segs;         // segments the launch's dynamic LDS holds
  int64_t total_in;     // entries of the input counts
};

// workspace of mask i, in ints: run_start (R + 1), seg_base (R + 1), then pos, val, parent, area (R + W each)
// and col_first (W + 1): 6 R + 5 W + 3.  After all masks: (segments, transitions) per mask.
struct RgnSlice {
  int R;
  const int* counts;
  int *run_start, *seg_base, *pos, *val, *parent, *area, *col_first;
};

__host__ __device__ inline int64_t rgn_per_mask(int W) { return 5 * (int64_t)W + 3; }
__host__ __device__ inline int64_t rgn_ws_ints(int n, int64_t total_in, int W) {
  return 6 * total_in + (int64_t)n * (rgn_per_mask(W) + 2);
}

__device__ __forceinline__ RgnSlice rgn_slice(const int64_t* __restrict__ offsets, const int* __restrict__ counts,
                                              int* __restrict__ ws, const RgnArgs& p, int i) {
  int64_t lo = offsets[i], hi = offsets[i + 1];
  lo = lo < 0 ? 0 : (lo > p.total_in ? p.total_in : lo);
  hi = hi < lo ? lo : (hi > p.total_in ? p.total_in : hi);
  RgnSlice s;
  s.R = (int)(hi - lo);
  s.counts = counts ? counts + lo : nullptr;
  const int cap = s.R + p.W;
  s.run_start = ws + 6 * lo + (int64_t)i * rgn_per_mask(p.W);
  s.seg_base = s.run_start + s.R + 1;
  s.pos = s.seg_base + s.R + 1;
  s.val = s.pos + cap;
  s.parent = s.val + cap;
  s.area = s.parent + cap;
  s.col_first = s.area + cap;
  return s;
}

__host__ __device__ inline int* rgn_header(int* ws, const RgnArgs& p, int i) {
  return ws + 6 * p.total_in + (int64_t)p.n * rgn_per_mask(p.W) + 2 * (int64_t)i;
}

// sum of `mine` over the threads before this one; `total`: over the block.  Two barriers.
template <typename T>
__device__ __forceinline__ T rgn_block_excl(T mine, T* wsum, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  __syncthreads();
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  T before = incl - mine;
  total = 0;
#pragma unroll
  for (int q = 0; q < RGN_WAVES; ++q) {
    if (q < wave) before += wsum[q];
    total += wsum[q];
  }
  return before;
}

// op over the block, the result in every thread.  Two barriers.
template <typename Op>
__device__ __forceinline__ long long rgn_block_reduce(long long v, Op op, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long r = red[0];
#pragma unroll
  for (int q = 1; q < RGN_WAVES; ++q) r = op(r, red[q]);
  return r;
}

// Other waves hook roots while this one reads: every parent access is a relaxed atomic, never a cached value.
__device__ __forceinline__ int rgn_ld(const int* a) {
  return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rgn_st(int* a, int v) {
  __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Path halving.  A parent is always a smaller index, and only a root (parent[x] == x) is ever hooked, so
// storing an ancestor into a non-root races with nothing.
__device__ __forceinline__ int rgn_find(int* parent, int x) {
  for (;;) {
    const int q = rgn_ld(parent + x);
    if (q == x) return x;
    const int gq = rgn_ld(parent + q);
    if (gq == q) return q;
    rgn_st(parent + x, gq);
    x = gq;
  }
}

__device__ __forceinline__ void rgn_union(int* parent, int a, int b) {
  for (;;) {
    a = rgn_find(parent, a);
    b = rgn_find(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(parent + hi, hi, lo) == hi) return;     // else another wave hooked `hi` first: find again
    a = hi, b = lo;
  }
}

// Components of the segments holding `v`: parent[g] = the component's first segment, area[root] its pixels.
__device__ __forceinline__ void rgn_components(int* parent, int* area, const RgnSlice& s, int S, int H, int v) {
  const int tid = threadIdx.x;
  for (int g = tid; g < S; g += RGN_THREADS) parent[g] = g, area[g] = 0;
  __syncthreads();
  for (int g = tid; g < S; g += RGN_THREADS) {
    if (s.val[g] != v) continue;
    const int p0 = s.pos[g], p1 = s.pos[g + 1], c = p0 / H;
    if (g > s.col_first[c] && s.val[g - 1] == v) rgn_union(parent, g, g - 1);
    if (c == 0) continue;
    // the left column in flat positions: its segment t covers rows [pos[t], pos[t + 1]) - (c - 1) H
    const int first = s.col_first[c - 1], end = s.col_first[c];
    const int lo_f = p0 - H, hi_f = p1 - H;
    int l = first, r = end;
    while (l < r) {             // first t with y_hi(t) > y_lo - 1
      const int m = (l + r) >> 1;
      if (s.pos[m + 1] >= lo_f) r = m; else l = m + 1;
    }
    for (int t = l; t < end && s.pos[t] <= hi_f; ++t)      // while y_lo(t) < y_hi + 1
      if (s.val[t] == v) rgn_union(parent, g, t);
  }
  __syncthreads();
  // Flatten with a find that writes nothing on its way: a halving store of an ancestor read earlier could land
  // on parent[x] AFTER the owner of x has stored its root there, and the next phase reads parent[] as roots.
  for (int g = tid; g < S; g += RGN_THREADS) {
    if (s.val[g] != v) continue;
    int root = g;
    for (int q = rgn_ld(parent + root); q != root; q = rgn_ld(parent + root)) root = q;
    rgn_st(parent + g, root);
    atomicAdd(area + root, s.pos[g + 1] - s.pos[g]);
  }
  __syncthreads();
}

constexpr int RGN_SMALL_HOLE = 1, RGN_SMALL_ISLAND = 2, RGN_LARGE_ISLAND = 4;

// Holes, then islands on the filled values; leaves the final values in s.val.  Returns whether the mask changed
// (the reference's flag: a small island counts even when it is the one that stays).
__device__ __forceinline__ bool rgn_clean(int* parent, int* area, const RgnSlice& s, int S, const RgnArgs& p,
                                          long long* red) {
  const int tid = threadIdx.x;
  const auto bit_or = [](long long a, long long b) { return a | b; };
  const auto max_of = [](long long a, long long b) { return a > b ? a : b; };
  int bits = 0;
  rgn_components(parent, area, s, S, p.H, 0);
  for (int g = tid; g < S; g += RGN_THREADS)
    if (s.val[g] == 0 && area[parent[g]] < p.min_area) s.val[g] = 1, bits |= RGN_SMALL_HOLE;
  __syncthreads();
  rgn_components(parent, area, s, S, p.H, 1);
  long long best = -1;      // (area, -root) of the roots this thread owns
  for (int g = tid; g < S; g += RGN_THREADS) {
    if (s.val[g] != 1) continue;
    const int a = area[parent[g]];
    bits |= a < p.min_area ? RGN_SMALL_ISLAND : RGN_LARGE_ISLAND;
    if (parent[g] == g) best = max_of(best, ((long long)a << 32) | (unsigned)(0x7fffffff - g));
  }
  bits = (int)rgn_block_reduce(bits, bit_or, red);
  if (bits & RGN_SMALL_ISLAND) {
    int winner = -1;        // all islands small: the root of the one that stays
    if (!(bits & RGN_LARGE_ISLAND))
      winner = 0x7fffffff - (int)(rgn_block_reduce(best, max_of, red) & 0xffffffffll);
    for (int g = tid; g < S; g += RGN_THREADS)
      if (s.val[g] == 1) s.val[g] = winner >= 0 ? parent[g] == winner : area[parent[g]] >= p.min_area;
  }
  __syncthreads();
  return (bits & (RGN_SMALL_HOLE | RGN_SMALL_ISLAND)) != 0;
}

__global__ __launch_bounds__(RGN_THREADS) void rle_regions_label(const int64_t* __restrict__ offsets,
                                                                 const int* __restrict__ counts,
                                                                 int* __restrict__ ws, int* __restrict__ stats,
                                                                 const RgnArgs p) {
  extern __shared__ int rgn_lds[];
  __shared__ long long red[RGN_WAVES];
  __shared__ int wsum[RGN_WAVES];
  const int tid = threadIdx.x, i = blockIdx.x;
  const RgnSlice s = rgn_slice(offsets, counts, ws, p, i);
  int* hdr = rgn_header(ws, p, i);
  int* st = stats + 8 * (size_t)i;
  const int R = s.R, H = p.H, HW = p.HW;
  if (R == 0) {     // no row at all: an empty canvas
    if (tid == 0) {
      st[0] = st[1] = st[2] = st[3] = st[4] = st[6] = st[7] = 0, st[5] = 1;
      hdr[0] = hdr[1] = 0;
    }
    return;
  }

  // runs: starts and first segments
  long long carry_len = 0;
  int S = 0;
  for (int c0 = 0; c0 < R; c0 += RGN_CHUNK) {
    const int e = c0 + 4 * tid;
    int len[4], nseg[4];
    long long mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = e + k < R ? s.counts[e + k] : 0;
      len[k] = v < 0 ? 0 : (v > HW ? HW : v);
      mine += len[k];
    }
    long long total_len;
    long long start = carry_len + rgn_block_excl(mine, red, total_len);
    int mine_seg = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = e + k;
      const int a = (int)(start < HW ? start : HW);
      start += len[k];
      const int b = j == R - 1 ? HW : (int)(start < HW ? start : HW);
      nseg[k] = j < R && b > a ? (b - 1) / H - a / H + 1 : 0;
      if (j < R) s.run_start[j] = a;
      mine_seg += nseg[k];
    }
    int total_seg;
    int base = S + rgn_block_excl(mine_seg, wsum, total_seg);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (e + k < R) s.seg_base[e + k] = base;
      base += nseg[k];
    }
    carry_len += total_len;
    S += total_seg;
  }
  if (tid == 0) s.run_start[R] = HW, s.seg_base[R] = S;
  __syncthreads();

  // segments: start, value, first of a column
  for (int g = tid; g < S; g += RGN_THREADS) {
    int l = 0, r = R;           // the last run j with seg_base[j] <= g
    while (r - l > 1) {
      const int m = (l + r) >> 1;
      if (s.seg_base[m] <= g) l = m; else r = m;
    }
    const int a = s.run_start[l], c = a / H + (g - s.seg_base[l]);
    const int start = a > c * H ? a : c * H;
    s.pos[g] = start;
    s.val[g] = l & 1;
    if (start == c * H) s.col_first[c] = g;
  }
  if (tid == 0) s.pos[S] = HW, s.col_first[p.W] = S;
  __syncthreads();

  const bool changed = S <= p.lds_segs ? rgn_clean(rgn_lds, rgn_lds + p.lds_segs, s, S, p, red)
                                       : rgn_clean(s.parent, s.area, s, S, p, red);

  // transitions, box, area
  int trans = 0, x_lo = p.W, x_hi = -1, y_lo = H, y_hi = -1;
  long long area = 0;
  for (int g = tid; g < S; g += RGN_THREADS) {
    const int v = s.val[g];
    trans += v != (g > 0 ? s.val[g - 1] : 0);
    if (!v) continue;
    const int p0 = s.pos[g], p1 = s.pos[g + 1], c = p0 / H;
    x_lo = min(x_lo, c), x_hi = max(x_hi, c);
    y_lo = min(y_lo, p0 - c * H), y_hi = max(y_hi, p1 - c * H - 1);
    area += p1 - p0;
  }
  const auto add = [](long long a, long long b) { return a + b; };
  const auto lo_of = [](long long a, long long b) { return a < b ? a : b; };
  const auto hi_of = [](long long a, long long b) { return a > b ? a : b; };
  trans = (int)rgn_block_reduce(trans, add, red);
  area = rgn_block_reduce(area, add, red);
  x_lo = (int)rgn_block_reduce(x_lo, lo_of, red), x_hi = (int)rgn_block_reduce(x_hi, hi_of, red);
  y_lo = (int)rgn_block_reduce(y_lo, lo_of, red), y_hi = (int)rgn_block_reduce(y_hi, hi_of, red);
  if (tid == 0) {
    const bool any = area > 0;
    st[0] = any ? x_lo : 0, st[1] = any ? y_lo : 0, st[2] = any ? x_hi : 0, st[3] = any ? y_hi : 0;
    st[4] = (int)area, st[5] = !changed, st[6] = S, st[7] = trans;
    hdr[0] = S, hdr[1] = trans;
  }
}

// one wave: offsets[0] = 0, offsets[i + 1] = offsets[i] + transitions_i + 1
__global__ __launch_bounds__(64) void rle_regions_offsets(const int* __restrict__ hdr, int64_t* __restrict__ offsets,
                                                          int n) {
  const int lane = threadIdx.x;
  int64_t carry = 0;
  if (lane == 0) offsets[0] = 0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int i = c0 + lane;
    int64_t incl = i < n ? (int64_t)hdr[2 * i + 1] + 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (i < n) offsets[i + 1] = carry + incl;
    carry += __shfl(incl, 63, 64);
  }
}

__global__ __launch_bounds__(RGN_THREADS) void rle_regions_write(const int64_t* __restrict__ offsets,
                                                                 int* __restrict__ ws,
                                                                 const int64_t* __restrict__ new_offsets,
                                                                 int* __restrict__ out, int64_t new_total,
                                                                 const RgnArgs p) {
  __shared__ int wsum[RGN_WAVES];
  const int tid = threadIdx.x, i = blockIdx.x;
  const RgnSlice s = rgn_slice(offsets, nullptr, ws, p, i);
  const int* hdr = rgn_header(ws, p, i);
  const int S = hdr[0], T = hdr[1];
  const int64_t row = new_offsets[i];
  if (S < 0 || S > s.R + p.W - 1 + (s.R == 0) || T < 0 || T > S) return;    // not the label stage's workspace
  if (row < 0 || row + T + 1 > new_total) return;                             // nor its offsets
  int* tpos = s.parent;       // free again: the transitions' flat positions, in rank order
  int rank0 = 0;
  for (int c0 = 0; c0 < S; c0 += RGN_CHUNK) {
    const int e = c0 + 4 * tid;
    int prev = e > 0 && e - 1 < S ? s.val[e - 1] : 0;
    int flag[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = e + k < S ? s.val[e + k] : prev;
      flag[k] = v != prev;
      mine += flag[k];
      prev = v;
    }
    int total;
    int rank = rank0 + rgn_block_excl(mine, wsum, total);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (flag[k]) tpos[rank++] = s.pos[e + k];
    rank0 += total;
  }
  __syncthreads();
  int* c = out + row;
  for (int j = tid; j <= T; j += RGN_THREADS) c[j] = (j < T ? tpos[j] : p.HW) - (j > 0 ? tpos[j - 1] : 0);
}

int plan(int n, int64_t total_in, int H, int W, int min_area, RgnArgs& p) {
  SAMQ_REQUIRE(n >= 1, SAMQ_ERR_INVALID, "rle_regions: n must be >= 0");
  SAMQ_REQUIRE(H >= 1 && W >= 1, SAMQ_ERR_INVALID, "rle_regions: sizes must be >= 1");
  SAMQ_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), SAMQ_ERR_INVALID, "rle_regions: H * W must be below 2^31");
  SAMQ_REQUIRE(min_area >= 1, SAMQ_ERR_INVALID, "rle_regions: min_area must be >= 1");
  SAMQ_REQUIRE(total_in >= n, SAMQ_ERR_INVALID, "rle_regions: every row holds at least one run");
  // segment indices are int32
  SAMQ_REQUIRE(total_in + W < ((int64_t)1 << 31), SAMQ_ERR_UNSUPPORTED, "rle_regions: too many runs");
  p.n = n, p.H = H, p.W = W, p.HW = H * W, p.min_area = min_area, p.total_in = total_in;
  const int64_t most = total_in - (n - 1) + W - 1;     // segments of the longest possible row
  p.lds_segs = (int)(most < RGN_LDS_SEGS ? most : RGN_LDS_SEGS);
  return SAMQ_OK;
}

}  // namespace
}  // namespace samq

using namespace samq;

extern "C" size_t samq_rle_regions_workspace(int n, int64_t total_in, int H, int W) {
  RgnArgs p;
  if (n <= 0 || plan(n, total_in, H, W, 1, p) != SAMQ_OK) return 0;
  return (size_t)rgn_ws_ints(n, total_in, W) * sizeof(int);
}

#define SAMQ_RGN_COMMON(name, min_area)                                                                        \
  if (n == 0) return SAMQ_OK;                                                                                  \
  RgnArgs p;                                                                                                   \
  if (const int st = plan(n, total_in, H, W, min_area, p)) return st;                                          \
  SAMQ_REQUIRE(offsets && new_offsets && workspace, SAMQ_ERR_INVALID, name ": null pointer");                  \
  SAMQ_REQUIRE((((uintptr_t)offsets | (uintptr_t)new_offsets) & 7) == 0 && ((uintptr_t)workspace & 3) == 0,    \
               SAMQ_ERR_INVALID, name ": misaligned pointer");                                                 \
  SAMQ_REQUIRE(workspace_bytes >= (size_t)rgn_ws_ints(n, total_in, W) * sizeof(int), SAMQ_ERR_INVALID,         \
               name ": workspace too small");                                                                  \
  int* ws = (int*)workspace

extern "C" int samq_rle_regions_label(const int64_t* offsets, const int32_t* counts, int n, int64_t total_in, int H,
                                      int W, int min_area, int64_t* new_offsets, int32_t* stats, void* workspace,
                                      size_t workspace_bytes, hipStream_t stream) {
  SAMQ_RGN_COMMON("rle_regions_label", min_area);
  SAMQ_REQUIRE(counts && stats, SAMQ_ERR_INVALID, "rle_regions_label: null pointer");
  SAMQ_REQUIRE((((uintptr_t)counts | (uintptr_t)stats) & 3) == 0, SAMQ_ERR_INVALID,
               "rle_regions_label: misaligned pointer");
  const size_t lds = (size_t)p.lds_segs * 2 * sizeof(int);
  if (lds > 48 * 1024) {
    static const hipError_t raised = hipFuncSetAttribute((const void*)rle_regions_label,
                                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                                         RGN_LDS_SEGS * 2 * (int)sizeof(int));
    if (raised != hipSuccess) return check_hip(raised, "rle_regions_label: dynamic LDS");
  }
  hipLaunchKernelGGL(rle_regions_label, dim3((unsigned)n), dim3(RGN_THREADS), lds, stream, offsets, counts, ws, stats,
                     p);
  hipLaunchKernelGGL(rle_regions_offsets, dim3(1), dim3(64), 0, stream, (const int*)rgn_header(ws, p, 0), new_offsets,
                     n);
  SAMQ_LAUNCH_CHECK("rle_regions_label launch");
  return SAMQ_OK;
}

extern "C" int samq_rle_regions_write(const int64_t* offsets, int n, int64_t total_in, int H, int W,
                                      const int64_t* new_offsets, void* workspace, size_t workspace_bytes,
                                      int32_t* new_counts, int64_t new_total, hipStream_t stream) {
  SAMQ_RGN_COMMON("rle_regions_write", 1);
  // every row has at least one entry and at most one per segment plus one
  SAMQ_REQUIRE(new_total >= n && new_total <= total_in + (int64_t)n * W, SAMQ_ERR_INVALID,
               "rle_regions_write: new_total is not new_offsets[n] of the label stage");
  SAMQ_REQUIRE(new_counts && ((uintptr_t)new_counts & 3) == 0, SAMQ_ERR_INVALID,
               "rle_regions_write: null or misaligned new_counts");
  hipLaunchKernelGGL(rle_regions_write, dim3((unsigned)n), dim3(RGN_THREADS), 0, stream, offsets, ws, new_offsets,
                     new_counts, new_total, p);
  SAMQ_LAUNCH_CHECK("rle_regions_write launch");
  return SAMQ_OK;
}
