// fq_vit MinmaxObserver.update on the GPU: running per-row / per-column /
// whole-tensor max and min of a calibration tensor.
//
// Reference: fq_vit/models/ptq/observer/minmax.py:14-29 (update: cur_max / cur_min over dim 1 of
// the reshaped tensor, merged with the running values, reduced to a scalar for layer_wise) and
// observer/base.py:16-29 (reshape_tensor: weights (out, -1) -> stats per row; activations
// channel-last (-1, C).T -> stats per column).  HBM-bound reductions; max/min are exact in any
// order, so results are bit-identical to torch's.  NaN propagates like torch.max / torch.min.
//
// The same reduction serves EmaObserver (observer/ema.py:17-32, init = 1) and OmseObserver's
// statistics (observer/omse.py:14-29).  Further down: samq_order_stats, the exact order statistics
// behind PercentileObserver's quantiles (observer/percentile.py:27-39), and samq_omse_scores, the
// candidate loop of OmseObserver.get_quantization_params (observer/omse.py:38-49).
#include "common.h"

namespace samq {

__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a > b) ? a : b; }
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || a < b) ? a : b; }

template <bool F16>
__device__ __forceinline__ float mm_load(const void* x, int64_t i) {
  if (F16) return (float)((const _Float16*)x)[i];
  return ((const float*)x)[i];
}

// stats per row: one wave per row, lanes stride the row
template <bool F16>
__global__ __launch_bounds__(256) void mm_rows_kernel(const void* __restrict__ x, int64_t rows, int C,
                                                      float* __restrict__ max_io, float* __restrict__ min_io,
                                                      int init) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float mx = -INFINITY, mn = INFINITY;
  bool nan = false;
  for (int c = lane; c < C; c += 64) {
    const float v = mm_load<F16>(x, row * C + c);
    nan |= v != v;
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
  }
  mx = wave_max(mx);
  mn = -wave_max(-mn);
  if (__any(nan)) mx = mn = __builtin_nanf("");
  if (lane == 0) {
    max_io[row] = init ? mx : nan_max(mx, max_io[row]);
    min_io[row] = init ? mn : nan_min(mn, min_io[row]);
  }
}

// stats per column, pass 1: thread = column, blockIdx.y = slab of rows -> ws[split][C]
template <bool F16>
__global__ __launch_bounds__(256) void mm_cols_kernel(const void* __restrict__ x, int64_t rows, int C,
                                                      int64_t rows_per_split, float* __restrict__ ws_max,
                                                      float* __restrict__ ws_min) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
  const int64_t r1 = r0 + rows_per_split < rows ? r0 + rows_per_split : rows;
  float mx = -INFINITY, mn = INFINITY;
  bool nan = false;
  for (int64_t r = r0; r < r1; ++r) {
    const float v = mm_load<F16>(x, r * C + c);
    nan |= v != v;
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
  }
  if (nan) mx = mn = __builtin_nanf("");
  ws_max[(int64_t)blockIdx.y * C + c] = mx;
  ws_min[(int64_t)blockIdx.y * C + c] = mn;
}

// pass 2, per column: fold the splits and the running values
__global__ __launch_bounds__(256) void mm_merge_cols_kernel(const float* __restrict__ ws_max,
                                                            const float* __restrict__ ws_min, int splits, int C,
                                                            float* __restrict__ max_io, float* __restrict__ min_io,
                                                            int init) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float mx = ws_max[c], mn = ws_min[c];
  for (int s = 1; s < splits; ++s) {
    mx = nan_max(mx, ws_max[(int64_t)s * C + c]);
    mn = nan_min(mn, ws_min[(int64_t)s * C + c]);
  }
  max_io[c] = init ? mx : nan_max(mx, max_io[c]);
  min_io[c] = init ? mn : nan_min(mn, min_io[c]);
}

// pass 2, whole tensor: one workgroup folds every partial into the running scalar
__global__ __launch_bounds__(256) void mm_merge_all_kernel(const float* __restrict__ ws_max,
                                                           const float* __restrict__ ws_min, int64_t n,
                                                           float* __restrict__ max_io, float* __restrict__ min_io,
                                                           int init) {
  __shared__ float smx[4], smn[4];
  __shared__ int snan[4];
  float mx = -INFINITY, mn = INFINITY;
  bool nan = false;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const float a = ws_max[i], b = ws_min[i];
    nan |= (a != a) | (b != b);
    mx = fmaxf(mx, a);
    mn = fminf(mn, b);
  }
  mx = wave_max(mx);
  mn = -wave_max(-mn);
  const int wnan = __any(nan) ? 1 : 0;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { smx[w] = mx; smn[w] = mn; snan[w] = wnan; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = smx[0];
    mn = smn[0];
    for (int i = 1; i < 4; ++i) { mx = fmaxf(mx, smx[i]); mn = fminf(mn, smn[i]); }
    if (snan[0] | snan[1] | snan[2] | snan[3]) mx = mn = __builtin_nanf("");
    max_io[0] = init ? mx : nan_max(mx, max_io[0]);
    min_io[0] = init ? mn : nan_min(mn, min_io[0]);
  }
}

static int64_t mm_splits(int64_t rows, int C) {
  // enough row slabs to put ~2 K workgroups on the chip, at least 64 rows each
  const int64_t col_blocks = (C + 255) / 256;
  int64_t s = (2048 + col_blocks - 1) / col_blocks;
  const int64_t max_s = (rows + 63) / 64;
  s = s < max_s ? s : max_s;
  return s < 1 ? 1 : (s > 1024 ? 1024 : s);
}


// ---------------------------------------------------------------- order statistics (radix select)
// Order-preserving uint32 image of an f32: negatives reversed below the positives (-0 and +0 are
// adjacent keys that decode to equal values).  Bits only, so denormals and +-inf keep their place.
__device__ __forceinline__ uint32_t os_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float os_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

constexpr int OS_MAX_RANKS = 4;
constexpr int OS_BINS = 2048;          // 11 / 11 / 10 key bits per pass
constexpr int OS_MAX_GRID = 2048;
struct OsRanks { int64_t r[OS_MAX_RANKS]; };

// device state between the passes, at the head of the workspace (zeroed by the entry point)
struct OsState {
  unsigned long long hist[3][OS_MAX_RANKS][OS_BINS];   // pass 0 uses slot 0 only
  unsigned long long rem[OS_MAX_RANKS];                // rank left inside the selected prefix
  uint32_t prefix[OS_MAX_RANKS];                       // key bits selected so far
};

template <int PASS>
__device__ __forceinline__ void os_count(uint32_t key, uint32_t* hist, int wave, int nranks, const uint32_t* pre) {
  if (PASS == 0) {   // no prefix yet: one histogram serves every rank; a copy per wave spreads the atomics
    atomicAdd(&hist[wave * OS_BINS + (key >> 21)], 1u);
  } else {
    const uint32_t hi = PASS == 1 ? key >> 21 : key >> 10;
    const uint32_t bin = PASS == 1 ? (key >> 10) & 2047u : key & 1023u;
#pragma unroll
    for (int r = 0; r < OS_MAX_RANKS; ++r)
      if (r < nranks && hi == pre[r]) atomicAdd(&hist[r * OS_BINS + bin], 1u);
  }
}

// One histogram pass: per-workgroup LDS histograms (LDS atomics), flushed with vector atomicAdd.
// Each workgroup sees fewer than 2^32 elements (n < 2^40 is required), so the LDS counts cannot wrap.
template <bool F16, int PASS>
__global__ __launch_bounds__(256) void os_hist_kernel(const void* __restrict__ x, int64_t n, int nranks,
                                                      OsState* __restrict__ st, int* __restrict__ nan_flag) {
  __shared__ uint32_t hist[OS_MAX_RANKS * OS_BINS];
  for (int i = threadIdx.x; i < OS_MAX_RANKS * OS_BINS; i += 256) hist[i] = 0;
  uint32_t pre[OS_MAX_RANKS];
#pragma unroll
  for (int r = 0; r < OS_MAX_RANKS; ++r) pre[r] = (PASS > 0 && r < nranks) ? st->prefix[r] : 0u;
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  bool nan = false;
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {   // four loads in flight ahead of the LDS atomics
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = mm_load<F16>(x, i + j * stride);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      nan |= v[j] != v[j];
      os_count<PASS>(os_key(v[j]), hist, wave, nranks, pre);
    }
  }
  for (; i < n; i += stride) {
    const float v = mm_load<F16>(x, i);
    nan |= v != v;
    os_count<PASS>(os_key(v), hist, wave, nranks, pre);
  }
  if (PASS == 0 && __any(nan) && (threadIdx.x & 63) == 0) atomicOr(nan_flag, 1);
  __syncthreads();
  if (PASS == 0) {
    for (int b = threadIdx.x; b < OS_BINS; b += 256) {
      const uint32_t c = hist[b] + hist[OS_BINS + b] + hist[2 * OS_BINS + b] + hist[3 * OS_BINS + b];
      if (c) atomicAdd(&st->hist[0][0][b], (unsigned long long)c);
    }
  } else {
    for (int i = threadIdx.x; i < nranks * OS_BINS; i += 256)
      if (hist[i]) atomicAdd(&st->hist[PASS][i / OS_BINS][i % OS_BINS], (unsigned long long)hist[i]);
  }
}

// Between the passes: wave r walks rank r's histogram to the bin that holds the rank, appends the
// bin to the prefix and keeps the rank's offset inside it.  After the last pass the prefix is the
// whole key and is decoded to out[r].  One workgroup of four waves; nothing goes to the host.
template <int PASS>
__global__ __launch_bounds__(256) void os_select_kernel(OsState* __restrict__ st, OsRanks ranks, int nranks,
                                                        float* __restrict__ out) {
  __shared__ unsigned long long part[OS_MAX_RANKS][64];
  const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int BINS = PASS == 2 ? 1024 : 2048, PER = BINS / 64, BITS = PASS == 2 ? 10 : 11;
  const unsigned long long* h = st->hist[PASS][PASS == 0 ? 0 : (r < nranks ? r : 0)];
  unsigned long long mine = 0;
  for (int j = 0; j < PER; ++j) mine += h[lane * PER + j];
  part[r][lane] = mine;
  __syncthreads();
  if (r >= nranks) return;
  const unsigned long long rem = PASS == 0 ? (unsigned long long)ranks.r[r] : st->rem[r];
  unsigned long long before = 0, total = 0;
  for (int j = 0; j < 64; ++j) {
    if (j < lane) before += part[r][j];
    total += part[r][j];
  }
  // the lane whose 32 (16) bins hold the rank; a rank past the total (never for a valid rank) is
  // pinned to the last non-empty lane so the result stays an element of the input
  const bool holds = rem >= before && rem < before + mine;
  const bool last = rem >= total && mine != 0 && before + mine == total;
  if (holds || last) {
    unsigned long long cum = before;
    int bin = lane * PER;
    for (int j = 0; j < PER; ++j) {
      const unsigned long long c = h[lane * PER + j];
      if (c == 0) continue;
      bin = lane * PER + j;
      if (rem < cum + c) break;
      cum += c;
    }
    const uint32_t prefix = ((PASS == 0 ? 0u : st->prefix[r]) << BITS) | (uint32_t)bin;
    st->prefix[r] = prefix;
    st->rem[r] = rem >= cum ? rem - cum : 0;
    if (PASS == 2) out[r] = os_unkey(prefix);
  }
}

// ---------------------------------------------------------------- omse candidate scores
constexpr int OMSE_MAX_CAND = 96;
constexpr int OMSE_MAX_GRID = 1024;

// Pass 1: every lane keeps one float64 sum per candidate over its grid-strided elements; lanes fold
// through the wave, waves through LDS, the workgroup's sums go to partial[block][cand].  The f32
// steps are torch's separate ops (omse.py:45-49, utils.py:9): IEEE division, no contraction.
template <bool F16>
__global__ __launch_bounds__(256) void omse_scores_kernel(const void* __restrict__ x, int64_t n,
                                                          const float* __restrict__ cand, int ncand, float qmin,
                                                          float qmax, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[4][OMSE_MAX_CAND];
  double acc[OMSE_MAX_CAND];
#pragma unroll
  for (int c = 0; c < OMSE_MAX_CAND; ++c) acc[c] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float nxt = i < n ? mm_load<F16>(x, i) : 0.f;
  for (; i < n; i += stride) {
    const float v = nxt;
    if (i + stride < n) nxt = mm_load<F16>(x, i + stride);   // in flight under the 96 candidates
#pragma unroll
    for (int c = 0; c < OMSE_MAX_CAND; ++c) {
      if (c < ncand) {
        const float s = cand[2 * c], zp = cand[2 * c + 1];
        const float q = fminf(fmaxf(__builtin_rintf(v / s + zp), qmin), qmax);
        const float xq = (q - zp) * s;
        const float d = v - xq;
        acc[c] += (double)(d * d);
      }
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < OMSE_MAX_CAND; ++c) {
    double a = acc[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) wsum[wave][c] = a;
  }
  __syncthreads();
  if (threadIdx.x < ncand) {
    const int c = threadIdx.x;
    partial[(int64_t)blockIdx.x * OMSE_MAX_CAND + c] = (wsum[0][c] + wsum[1][c]) + (wsum[2][c] + wsum[3][c]);
  }
}

// Pass 2: one wave per candidate folds the workgroups' sums in a fixed order (run-to-run identical)
__global__ __launch_bounds__(64) void omse_fold_kernel(const double* __restrict__ partial, int blocks,
                                                       double* __restrict__ sums) {
  const int c = blockIdx.x;
  double a = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 64) a += partial[(int64_t)b * OMSE_MAX_CAND + c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (threadIdx.x == 0) sums[c] = a;
}

// ---------------------------------------------------------------- ptf per-channel scores
// PtfObserver.get_quantization_params (observer/ptf.py:53-72): for every channel c of a row-major
// (rows, C) tensor the four sums over the rows of (x - fq_k(x))^2 under the scales s1 * {1, 2, 4, 8} and
// one zero point, each term in f32 as in omse_scores_kernel.  A workgroup takes 64 channels (a lane a
// column: coalesced rows) and one slab of rows, its four waves every fourth row of the slab; a lane's
// float64 sums fold through LDS in wave order into partial[slab][c][k].
constexpr int PTF_MAX_SLABS = 256;

template <bool F16>
__global__ __launch_bounds__(256) void ptf_scores_kernel(const void* __restrict__ x, int64_t rows, int C,
                                                         int64_t rows_per_slab, float s1, float zp, float qmin,
                                                         float qmax, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[4][64][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < rows ? r0 + rows_per_slab : rows;
  const float sc[4] = {s1, s1 * 2.0f, s1 * 4.0f, s1 * 8.0f};   // exact doublings (ptf.py halves scale8 three times)
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (c < C) {
    for (int64_t r = r0 + wave; r < r1; r += 4) {
      const float v = mm_load<F16>(x, r * C + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float q = fminf(fmaxf(__builtin_rintf(v / sc[k] + zp), qmin), qmax);
        const float xq = (q - zp) * sc[k];
        const float d = v - xq;
        acc[k] += (double)(d * d);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) wsum[wave][lane][k] = acc[k];
  __syncthreads();
  if (wave == 0 && c < C) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      partial[((int64_t)blockIdx.y * C + c) * 4 + k] = (wsum[0][lane][k] + wsum[1][lane][k]) +
                                                       (wsum[2][lane][k] + wsum[3][lane][k]);
  }
}

// the slabs' sums of one (channel, scale) in slab order
__global__ __launch_bounds__(256) void ptf_fold_kernel(const double* __restrict__ partial, int slabs, int64_t n4,
                                                       double* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  double a = 0.0;
  for (int s = 0; s < slabs; ++s) a += partial[(int64_t)s * n4 + i];
  sums[i] = a;
}

static int ptf_slabs(int64_t rows, int C) {
  const int64_t col_blocks = (C + 63) / 64;
  int64_t s = (1024 + col_blocks - 1) / col_blocks;     // ~1 K workgroups
  const int64_t max_s = (rows + 31) / 32;               // at least 32 rows each
  s = s < max_s ? s : max_s;
  return (int)(s < 1 ? 1 : (s > PTF_MAX_SLABS ? PTF_MAX_SLABS : s));
}

static int os_grid(int64_t n) {
  const int64_t g = (n + 256 * 16 - 1) / (256 * 16);   // at least 16 elements per thread
  return (int)(g < 1 ? 1 : (g > OS_MAX_GRID ? OS_MAX_GRID : g));
}
static int omse_grid(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > OMSE_MAX_GRID ? OMSE_MAX_GRID : g));
}

}  // namespace samq

using namespace samq;

extern "C" size_t samq_minmax_workspace(int64_t rows, int C, int axis) {
  if (axis == SAMQ_MM_PER_ROW || rows <= 0 || C <= 0) return 0;
  return (size_t)(2 * mm_splits(rows, C) * C);
}

extern "C" int samq_minmax(const void* x, int64_t rows, int C, int in_f16, int axis, float* max_io, float* min_io,
                           int init, float* workspace, size_t workspace_floats, hipStream_t stream) {
  SAMQ_REQUIRE(x && max_io && min_io, SAMQ_ERR_INVALID, "minmax: null pointer");
  SAMQ_REQUIRE(rows > 0 && C > 0, SAMQ_ERR_INVALID, "minmax: empty tensor (torch.max would raise)");
  SAMQ_REQUIRE(axis == SAMQ_MM_PER_ROW || axis == SAMQ_MM_PER_COL || axis == SAMQ_MM_ALL, SAMQ_ERR_INVALID,
               "minmax: axis must be SAMQ_MM_PER_ROW, SAMQ_MM_PER_COL or SAMQ_MM_ALL");
  if (axis == SAMQ_MM_PER_ROW) {
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (in_f16) hipLaunchKernelGGL((mm_rows_kernel<true>), grid, dim3(256), 0, stream, x, rows, C, max_io, min_io, init);
    else hipLaunchKernelGGL((mm_rows_kernel<false>), grid, dim3(256), 0, stream, x, rows, C, max_io, min_io, init);
    SAMQ_LAUNCH_CHECK("minmax rows launch");
    return SAMQ_OK;
  }
  const int64_t splits = mm_splits(rows, C);
  SAMQ_REQUIRE(workspace && workspace_floats >= (size_t)(2 * splits * C), SAMQ_ERR_INVALID,
               "minmax: workspace smaller than samq_minmax_workspace()");
  const int64_t rps = (rows + splits - 1) / splits;
  float* ws_max = workspace;
  float* ws_min = workspace + splits * C;
  const dim3 grid((unsigned)((C + 255) / 256), (unsigned)splits);
  if (in_f16) hipLaunchKernelGGL((mm_cols_kernel<true>), grid, dim3(256), 0, stream, x, rows, C, rps, ws_max, ws_min);
  else hipLaunchKernelGGL((mm_cols_kernel<false>), grid, dim3(256), 0, stream, x, rows, C, rps, ws_max, ws_min);
  SAMQ_LAUNCH_CHECK("minmax cols launch");
  if (axis == SAMQ_MM_PER_COL)
    hipLaunchKernelGGL(mm_merge_cols_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, ws_max, ws_min,
                       (int)splits, C, max_io, min_io, init);
  else
    hipLaunchKernelGGL(mm_merge_all_kernel, dim3(1), dim3(256), 0, stream, ws_max, ws_min, splits * C, max_io, min_io,
                       init);
  SAMQ_LAUNCH_CHECK("minmax merge launch");
  return SAMQ_OK;
}

// Exact order statistics of a flat tensor -- what PercentileObserver.update needs of
// torch.quantile / np.percentile (observer/percentile.py:27-39): the sorted values at up to four
// zero-based ranks, by a three-pass radix select (11 / 11 / 10 key bits), all ranks in the same passes.
extern "C" size_t samq_order_stats_workspace(int64_t n, int nranks) {
  if (n <= 0 || nranks <= 0 || nranks > OS_MAX_RANKS) return 0;
  return sizeof(OsState);
}

extern "C" int samq_order_stats(const void* x, int64_t n, int in_f16, const int64_t* ranks, int nranks, float* out,
                                int* nan_flag, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  SAMQ_REQUIRE(x && ranks && out && nan_flag, SAMQ_ERR_INVALID, "order_stats: null pointer");
  SAMQ_REQUIRE(n > 0 && n < ((int64_t)1 << 40), SAMQ_ERR_INVALID, "order_stats: n must be in [1, 2^40)");
  SAMQ_REQUIRE(nranks >= 1 && nranks <= OS_MAX_RANKS, SAMQ_ERR_INVALID, "order_stats: 1 to 4 ranks");
  SAMQ_REQUIRE(workspace && workspace_bytes >= sizeof(OsState) && ((uintptr_t)workspace & 7) == 0, SAMQ_ERR_INVALID,
               "order_stats: workspace smaller than samq_order_stats_workspace() or not 8-byte aligned");
  OsRanks rk;
  for (int r = 0; r < OS_MAX_RANKS; ++r) {
    rk.r[r] = r < nranks ? ranks[r] : 0;
    SAMQ_REQUIRE(rk.r[r] >= 0 && rk.r[r] < n, SAMQ_ERR_INVALID, "order_stats: rank outside [0, n)");
  }
  OsState* st = (OsState*)workspace;
  hipError_t e = hipMemsetAsync(st, 0, sizeof(OsState), stream);
  if (e == hipSuccess) e = hipMemsetAsync(nan_flag, 0, sizeof(int), stream);
  if (e != hipSuccess) return check_hip(e, "order_stats memset");
  const dim3 grid((unsigned)os_grid(n)), blk(256);
#define SAMQ_OS_PASS(P)                                                                                          \
  do {                                                                                                           \
    if (in_f16) hipLaunchKernelGGL((os_hist_kernel<true, P>), grid, blk, 0, stream, x, n, nranks, st, nan_flag); \
    else hipLaunchKernelGGL((os_hist_kernel<false, P>), grid, blk, 0, stream, x, n, nranks, st, nan_flag);       \
    SAMQ_LAUNCH_CHECK("order_stats histogram launch");                                                           \
    hipLaunchKernelGGL((os_select_kernel<P>), dim3(1), blk, 0, stream, st, rk, nranks, out);                     \
    SAMQ_LAUNCH_CHECK("order_stats select launch");                                                              \
  } while (0)
  SAMQ_OS_PASS(0);
  SAMQ_OS_PASS(1);
  SAMQ_OS_PASS(2);
#undef SAMQ_OS_PASS
  return SAMQ_OK;
}

// The omse candidate scores in one read of the tensor -- the loop body of
// OmseObserver.get_quantization_params (observer/omse.py:45-49, lp_loss observer/utils.py:9) for up
// to 96 (scale, zero_point) candidates at once: sums[c] = sum_i (x_i - fq_c(x_i))^2, each term in
// f32 exactly as torch's separate ops round it, summed in float64 (the caller divides by n).
extern "C" size_t samq_omse_scores_workspace(int64_t n, int ncand) {
  if (n <= 0 || ncand <= 0 || ncand > OMSE_MAX_CAND) return 0;
  return (size_t)omse_grid(n) * OMSE_MAX_CAND * sizeof(double);
}

extern "C" int samq_omse_scores(const void* x, int64_t n, int in_f16, const float* cand, int ncand, float qmin,
                                float qmax, double* sums, void* workspace, size_t workspace_bytes,
                                hipStream_t stream) {
  SAMQ_REQUIRE(x && cand && sums, SAMQ_ERR_INVALID, "omse_scores: null pointer");
  SAMQ_REQUIRE(n > 0, SAMQ_ERR_INVALID, "omse_scores: empty tensor");
  SAMQ_REQUIRE(ncand >= 1 && ncand <= OMSE_MAX_CAND, SAMQ_ERR_INVALID, "omse_scores: 1 to 96 candidates");
  SAMQ_REQUIRE(qmin <= qmax, SAMQ_ERR_INVALID, "omse_scores: qmin > qmax");
  const int blocks = omse_grid(n);
  SAMQ_REQUIRE(workspace && workspace_bytes >= (size_t)blocks * OMSE_MAX_CAND * sizeof(double) &&
                   ((uintptr_t)workspace & 7) == 0,
               SAMQ_ERR_INVALID, "omse_scores: workspace smaller than samq_omse_scores_workspace() or misaligned");
  double* partial = (double*)workspace;
  if (in_f16)
    hipLaunchKernelGGL((omse_scores_kernel<true>), dim3(blocks), dim3(256), 0, stream, x, n, cand, ncand, qmin, qmax,
                       partial);
  else
    hipLaunchKernelGGL((omse_scores_kernel<false>), dim3(blocks), dim3(256), 0, stream, x, n, cand, ncand, qmin, qmax,
                       partial);
  SAMQ_LAUNCH_CHECK("omse_scores launch");
  hipLaunchKernelGGL(omse_fold_kernel, dim3(ncand), dim3(64), 0, stream, partial, blocks, sums);
  SAMQ_LAUNCH_CHECK("omse_scores fold launch");
  return SAMQ_OK;
}

// The PTF observer's per-channel scores in one read of a row-major (rows, C) tensor (f32, or f16 with
// in_f16): sums[c][k] = sum_r (x[r, c] - fq_k(x[r, c]))^2 for the scales scale1 * 2^k, k = 0..3, and the
// shared zero point, each term in f32 exactly as torch's separate ops round it (observer/ptf.py:55-70),
// summed in float64 in a fixed order (the caller divides by rows).  sums is double [C][4]; the
// workspace (samq_ptf_scores_workspace(rows, C) bytes, 8-byte aligned) is the caller's.
extern "C" size_t samq_ptf_scores_workspace(int64_t rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  return (size_t)ptf_slabs(rows, C) * (size_t)C * 4 * sizeof(double);
}

extern "C" int samq_ptf_scores(const void* x, int64_t rows, int C, int in_f16, float scale1, float zero_point,
                               float qmin, float qmax, double* sums, void* workspace, size_t workspace_bytes,
                               hipStream_t stream) {
  SAMQ_REQUIRE(x && sums, SAMQ_ERR_INVALID, "ptf_scores: null pointer");
  SAMQ_REQUIRE(rows > 0 && C > 0, SAMQ_ERR_INVALID, "ptf_scores: empty tensor");
  SAMQ_REQUIRE(scale1 > 0.f, SAMQ_ERR_INVALID, "ptf_scores: scale1 must be > 0");
  SAMQ_REQUIRE(qmin <= qmax, SAMQ_ERR_INVALID, "ptf_scores: qmin > qmax");
  const int slabs = ptf_slabs(rows, C);
  SAMQ_REQUIRE(workspace && workspace_bytes >= (size_t)slabs * (size_t)C * 4 * sizeof(double) &&
                   ((uintptr_t)workspace & 7) == 0,
               SAMQ_ERR_INVALID, "ptf_scores: workspace smaller than samq_ptf_scores_workspace() or misaligned");
  const int64_t rps = (rows + slabs - 1) / slabs;
  double* partial = (double*)workspace;
  const dim3 grid((unsigned)((C + 63) / 64), (unsigned)slabs);
  if (in_f16)
    hipLaunchKernelGGL((ptf_scores_kernel<true>), grid, dim3(256), 0, stream, x, rows, C, rps, scale1, zero_point, qmin,
                       qmax, partial);
  else
    hipLaunchKernelGGL((ptf_scores_kernel<false>), grid, dim3(256), 0, stream, x, rows, C, rps, scale1, zero_point, qmin,
                       qmax, partial);
  SAMQ_LAUNCH_CHECK("ptf_scores launch");
  const int64_t n4 = (int64_t)C * 4;
  hipLaunchKernelGGL(ptf_fold_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, partial, slabs, n4, sums);
  SAMQ_LAUNCH_CHECK("ptf_scores fold launch");
  return SAMQ_OK;
}
