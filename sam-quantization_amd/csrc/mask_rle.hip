// Uncompressed COCO run-length encoding of selected masks placed on a larger canvas:
//   mask_to_rle_pytorch(uncrop_masks(masks[sel], crop_box, H, W))     (segment_anything/utils/amg.py)
// with no padded copy, no transposed copy and no index tensor.  A row of the result is the run lengths of the
// H x W canvas flattened in Fortran order (p = X H + Y), starting with a run of zeros.
//
// A transition sits at flat index p where v(p) != v(p - 1), v(-1) = 0 (so a set pixel (0, 0) gives the
// transition p = 0 and with it the leading run of length 0).  With k transitions t_0 < .. < t_{k-1} the row
// is [t_0, t_1 - t_0, .., H W - t_{k-1}]: k + 1 entries.  In the row-major mask `v(p) != v(p - 1)` is a
// VERTICAL comparison, so the masks are read in their own order; only the order of the output is transposed,
// and that is a scan of per-column counts.  Column x of the mask (canvas column X = x0 + x) owns
//   rows     y = 0 .. h - 1: a transition at X H + y0 + y where m[y][x] != m[y - 1][x]; row 0 compares with
//            the canvas pixel before (X, y0): 0, unless the mask spans the whole canvas height (y0 == 0,
//            h == H: the column seam is live), where it is m[h - 1][x - 1] (0 for x == 0);
//   closing  a set m[h - 1][x] ends its run at X H + y0 + h, unless the next column's row 0 makes that
//            comparison (live seam, x + 1 < w) or the canvas ends there (y0 + h == H, X + 1 == W).
// Canvas columns outside the mask hold no transition of their own.
//
// Three steps, the mask read twice and never written:
//   count    grid (selected mask x 256-column tile, 4 row bands); a WAVE owns a band of RLE_BAND rows, a lane
//            four adjacent columns, one (unaligned) dword per row.  Bytes are normalised to 0x80 / 0, XORed
//            with the row above, and the four columns' counts accumulate as the four bytes of one register
//            (at most RLE_BAND + 1 per byte).  They go to the workspace as int32 [mask][column][band]: the
//            Fortran-order rank of a transition is then a plain exclusive scan of that array.
//   scan     one workgroup per selected mask scans its w x bands counts in place (thread-serial 4, wave scan
//            by shuffles, wave totals and the running carry through LDS) and leaves the mask's total in the
//            workspace tail; one wave turns the n_sel totals into `offsets` (row i holds total_i + 1 entries).
//   write    the count pass again, each lane starting from its scanned offsets and storing the flat position
//            of every transition at offsets[i] + rank; an elementwise kernel (one workgroup per row) then
//            writes counts[j] = pos[j] - pos[j - 1] into a second buffer, with pos[-1] = 0 and the closing
//            run up to H W.
// No atomics: every word of every buffer has one writer, so the output is the same on every run.  An entry of
// `sel` outside [0, N) reads nothing and encodes an empty canvas.
#include "common.h"

namespace samq {
namespace {

constexpr int RLE_COLS = 256;    // columns per wave (4 per lane)
constexpr int RLE_BAND = 64;     // rows per wave
constexpr int RLE_WAVES = 4;     // bands per workgroup

struct RleArgs {
  int N, n_sel, h, w, x0, y0, H, W;
  int col_tiles, bands;
  int seam;       // y0 == 0 && h == H: the last pixel of a column precedes the first of the next
  int bottom;     // y0 + h == H
};

typedef uint32_t u32_unaligned __attribute__((aligned(1)));

// four mask bytes -> 0x80 per non-zero byte
__device__ __forceinline__ uint32_t norm4(uint32_t v) {
  return (((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u;
}

// the lane's four columns of row y; columns at or past w read as 0
__device__ __forceinline__ uint32_t row_word(const uint8_t* __restrict__ m, int w, int y, int x, bool whole) {
  const uint8_t* p = m + (size_t)y * w + x;
  if (whole) return norm4(*(const u32_unaligned*)p);
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (x + k < w) v |= (uint32_t)p[k] << (8 * k);
  return norm4(v);
}

// what row 0 of the lane's columns compares with: the last row of the column to the left across a live seam
__device__ __forceinline__ uint32_t seam_word(const uint8_t* __restrict__ m, const RleArgs& p, int x) {
  uint32_t v = 0;
  if (p.seam) {
    const uint8_t* last = m + (size_t)(p.h - 1) * p.w;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k > 0 && x + k < p.w) v |= (uint32_t)last[x + k - 1] << (8 * k);
  }
  return norm4(v);
}

// the closing transitions of the lane's columns, given their last row
__device__ __forceinline__ uint32_t closing_word(uint32_t last, const RleArgs& p, int x) {
  uint32_t keep = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool next_col = p.seam && x + k + 1 < p.w;
    const bool canvas_end = p.bottom && p.x0 + x + k + 1 == p.W;
    if (x + k < p.w && !next_col && !canvas_end) keep |= 0x80u << (8 * k);
  }
  return last & keep;
}

// WRITE = false: per-(column, band) transition counts into ws.  WRITE = true: ws holds their exclusive scan;
// the flat position of every transition goes to pos[offsets[i] + rank].
template <bool WRITE>
__global__ __launch_bounds__(64 * RLE_WAVES) void mask_rle_pass(const uint8_t* __restrict__ masks,
                                                               const int* __restrict__ sel, int* __restrict__ ws,
                                                               const int64_t* __restrict__ offsets,
                                                               int* __restrict__ pos, const RleArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x / p.col_tiles, x = (blockIdx.x % p.col_tiles) * RLE_COLS + 4 * lane;
  const int band = blockIdx.y * RLE_WAVES + wave;
  if (band >= p.bands || x >= p.w) return;
  const int s = sel[i];
  const bool valid = s >= 0 && s < p.N;     // wave-uniform
  const uint8_t* m = masks + (size_t)(valid ? s : 0) * p.h * p.w;
  const bool whole = x + 3 < p.w;
  const int y_lo = band * RLE_BAND, y_hi = min(y_lo + RLE_BAND, p.h);
  int* cell = ws + ((size_t)i * p.w + x) * p.bands + band;    // column x + k: cell[k * bands]

  int rank[4] = {0, 0, 0, 0};
  int* out = nullptr;
  if constexpr (WRITE) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < p.w) rank[k] = cell[(size_t)k * p.bands];
    out = pos + offsets[i];
  }
  uint32_t acc = 0;
  if (valid) {
    uint32_t prev = y_lo == 0 ? seam_word(m, p, x) : row_word(m, p.w, y_lo - 1, x, whole);
    const int base = (p.x0 + x) * p.H + p.y0;    // flat position of (column x, row 0); + k H per column
    auto emit = [&](uint32_t t, int y) {
      if constexpr (WRITE) {
        if (t) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (t & (0x80u << (8 * k))) out[rank[k]++] = base + k * p.H + y;
        }
      } else {
        acc += t >> 7;
      }
    };
#pragma unroll 8
    for (int y = y_lo; y < y_hi; ++y) {
      const uint32_t cur = row_word(m, p.w, y, x, whole);
      emit(cur ^ prev, y);
      prev = cur;
    }
    if (y_hi == p.h) emit(closing_word(prev, p, x), p.h);
  }
  if constexpr (!WRITE) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < p.w) cell[(size_t)k * p.bands] = (int)((acc >> (8 * k)) & 0xffu);
  }
}

// one workgroup per selected mask: exclusive scan of its `len` counts in place, the total to totals[i]
__global__ __launch_bounds__(256) void mask_rle_scan(int* __restrict__ ws, int* __restrict__ totals, int len) {
  __shared__ int wsum[4];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* a = ws + (size_t)blockIdx.x * len;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int c0 = 0; c0 < len; c0 += 1024) {
    const int e = c0 + 4 * tid;
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = e + k < len ? a[e + k] : 0;
    const int mine = v[0] + v[1] + v[2] + v[3];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = carry_s + incl - mine;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (q < wave) before += wsum[q];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (e + k < len) a[e + k] = before;
      before += v[k];
    }
    __syncthreads();
    if (tid == 255) carry_s = before;
    __syncthreads();
  }
  if (tid == 0) totals[blockIdx.x] = carry_s;
}

// one wave: offsets[0] = 0, offsets[i + 1] = offsets[i] + totals[i] + 1
__global__ __launch_bounds__(64) void mask_rle_offsets(const int* __restrict__ totals, int64_t* __restrict__ offsets,
                                                       int n_sel) {
  const int lane = threadIdx.x;
  int64_t carry = 0;
  if (lane == 0) offsets[0] = 0;
  for (int c0 = 0; c0 < n_sel; c0 += 64) {
    const int i = c0 + lane;
    int64_t incl = i < n_sel ? (int64_t)totals[i] + 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (i < n_sel) offsets[i + 1] = carry + incl;
    carry += __shfl(incl, 63, 64);
  }
}

// one workgroup per row: positions -> run lengths, into a second buffer
__global__ __launch_bounds__(256) void mask_rle_lengths(const int* __restrict__ pos, const int64_t* __restrict__ offsets,
                                                        int* __restrict__ counts, int HW) {
  const int64_t b = offsets[blockIdx.x];
  const int k = (int)(offsets[blockIdx.x + 1] - b) - 1;    // transitions of this row
  const int* pp = pos + b;
  int* c = counts + b;
  for (int j = threadIdx.x; j <= k; j += 256) c[j] = (j < k ? pp[j] : HW) - (j > 0 ? pp[j - 1] : 0);
}

int plan(int N, int n_sel, int h, int w, int x0, int y0, int H, int W, RleArgs& p) {
  SAMQ_REQUIRE(N >= 1 && n_sel >= 1, SAMQ_ERR_INVALID, "mask_rle: mask counts must be >= 1");
  SAMQ_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1, SAMQ_ERR_INVALID, "mask_rle: sizes must be >= 1");
  SAMQ_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), SAMQ_ERR_INVALID, "mask_rle: H * W must be below 2^31");
  SAMQ_REQUIRE(x0 >= 0 && y0 >= 0 && (int64_t)x0 + w <= W && (int64_t)y0 + h <= H, SAMQ_ERR_INVALID,
               "mask_rle: the mask must lie inside the canvas");
  p.N = N, p.n_sel = n_sel, p.h = h, p.w = w, p.x0 = x0, p.y0 = y0, p.H = H, p.W = W;
  p.col_tiles = (w + RLE_COLS - 1) / RLE_COLS;
  p.bands = (h + RLE_BAND - 1) / RLE_BAND;
  p.seam = y0 == 0 && h == H;
  p.bottom = y0 + h == H;
  SAMQ_REQUIRE((int64_t)n_sel * p.col_tiles < ((int64_t)1 << 31), SAMQ_ERR_UNSUPPORTED, "mask_rle: too many masks");
  SAMQ_REQUIRE((p.bands + RLE_WAVES - 1) / RLE_WAVES <= 65535, SAMQ_ERR_UNSUPPORTED, "mask_rle: too many row bands");
  return SAMQ_OK;
}

size_t cells(const RleArgs& p) { return (size_t)p.n_sel * p.w * p.bands; }

}  // namespace
}  // namespace samq

using namespace samq;

extern "C" size_t samq_mask_rle_workspace(int N, int n_sel, int h, int w, int x0, int y0, int H, int W) {
  RleArgs p;
  if (n_sel <= 0 || plan(N, n_sel, h, w, x0, y0, H, W, p) != SAMQ_OK) return 0;
  return (cells(p) + (size_t)n_sel) * sizeof(int);
}

#define SAMQ_RLE_COMMON(name)                                                                                  \
  if (n_sel == 0) return SAMQ_OK;                                                                              \
  RleArgs p;                                                                                                   \
  if (const int st = plan(N, n_sel, h, w, x0, y0, H, W, p)) return st;                                         \
  SAMQ_REQUIRE(masks && sel && offsets && workspace, SAMQ_ERR_INVALID, name ": null pointer");                 \
  SAMQ_REQUIRE((((uintptr_t)sel | (uintptr_t)workspace) & 3) == 0 && ((uintptr_t)offsets & 7) == 0,            \
               SAMQ_ERR_INVALID, name ": misaligned pointer");                                                 \
  SAMQ_REQUIRE(workspace_bytes >= (cells(p) + (size_t)n_sel) * sizeof(int), SAMQ_ERR_INVALID,                  \
               name ": workspace too small");                                                                  \
  int* ws = (int*)workspace;                                                                                   \
  const dim3 grid((unsigned)(n_sel * p.col_tiles), (unsigned)((p.bands + RLE_WAVES - 1) / RLE_WAVES));         \
  const dim3 block(64 * RLE_WAVES)

extern "C" int samq_mask_rle_count(const uint8_t* masks, int N, const int32_t* sel, int n_sel, int h, int w, int x0,
                                   int y0, int H, int W, int64_t* offsets, void* workspace, size_t workspace_bytes,
                                   hipStream_t stream) {
  SAMQ_RLE_COMMON("mask_rle_count");
  hipLaunchKernelGGL(mask_rle_pass<false>, grid, block, 0, stream, masks, sel, ws, (const int64_t*)nullptr,
                     (int*)nullptr, p);
  hipLaunchKernelGGL(mask_rle_scan, dim3((unsigned)n_sel), dim3(256), 0, stream, ws, ws + cells(p), p.w * p.bands);
  hipLaunchKernelGGL(mask_rle_offsets, dim3(1), dim3(64), 0, stream, (const int*)(ws + cells(p)), offsets, n_sel);
  SAMQ_LAUNCH_CHECK("mask_rle_count launch");
  return SAMQ_OK;
}

extern "C" int samq_mask_rle_write(const uint8_t* masks, int N, const int32_t* sel, int n_sel, int h, int w, int x0,
                                   int y0, int H, int W, const int64_t* offsets, void* workspace,
                                   size_t workspace_bytes, int32_t* positions, int32_t* counts, int64_t total,
                                   hipStream_t stream) {
  SAMQ_RLE_COMMON("mask_rle_write");
  // every row has at least one entry and at most one per canvas pixel plus one
  SAMQ_REQUIRE(total >= n_sel && total <= (int64_t)n_sel * ((int64_t)H * W + 1), SAMQ_ERR_INVALID,
               "mask_rle_write: total is not offsets[n_sel] of the count pass");
  SAMQ_REQUIRE(positions && counts && positions != counts, SAMQ_ERR_INVALID,
               "mask_rle_write: positions and counts must be two buffers");
  SAMQ_REQUIRE((((uintptr_t)positions | (uintptr_t)counts) & 3) == 0, SAMQ_ERR_INVALID,
               "mask_rle_write: misaligned pointer");
  hipLaunchKernelGGL(mask_rle_pass<true>, grid, block, 0, stream, masks, sel, ws, offsets, positions, p);
  hipLaunchKernelGGL(mask_rle_lengths, dim3((unsigned)n_sel), dim3(256), 0, stream, (const int*)positions, offsets,
                     counts, H * W);
  SAMQ_LAUNCH_CHECK("mask_rle_write launch");
  return SAMQ_OK;
}
