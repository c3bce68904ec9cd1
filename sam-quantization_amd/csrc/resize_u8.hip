// PIL.Image.resize(..., BILINEAR) of a window of a device-resident uint8 HWC image, bit for bit: the resize of
// ResizeLongestSide.apply_image (segment_anything/utils/transforms.py:26-32) in front of the image encoder.
// Pillow's bilinear resize is an antialiased triangle filter in two passes (Resample.c): per axis of input
// length n and output length m, in fp64 with every step its own IEEE operation (the file is built with
// -ffp-contract=off),
//   scale = n / m, fs = max(scale, 1), support = fs, center(i) = (i + 0.5) scale,
//   lo = max(0, (int)(center - support + 0.5)), hi = min(n, (int)(center + support + 0.5)),
//   w_t = max(0, 1 - |(t + lo - center + 0.5) / fs|), ww = sum_t w_t (increasing t), k_t = (int)(w_t / ww 2^22 + 0.5),
//   out(i) = clamp(((1 << 21) + sum_t k_t pixel(lo + t)) >> 22, 0, 255)   in int32;
// the horizontal pass runs first and rounds to uint8, the vertical pass reads those bytes, and a pass whose axis
// keeps its length is skipped.  One launch, no host table, no workspace:
//
//   tile     a workgroup of four waves owns RZ_TW = 64 output columns x RZ_TH = 16 output rows x 3 channels.
//   tables   threads 0 .. 63 compute lo, the tap count and the k_t of the tile's columns, threads 64 .. 79 those
//            of its rows, into LDS ([index][33] int32: the odd pitch keeps the lanes of a wave, which walk
//            neighbouring columns, on different banks).  fs <= 16 bounds the taps at 2 * 16 + 1 = 33.
//   stage    the vertical taps of the tile span the input rows lo(first row) .. hi(last row), its horizontal
//            taps the pixels lo(first column) .. hi(last column): of each such row exactly that HWC byte span is
//            read, as 16-byte loads at 16-byte aligned addresses (the span widened to the alignment; a chunk
//            that would cross either end of the image is read byte by byte inside it), several rows per trip
//            into a raw LDS buffer.
//   hpass    every thread turns raw bytes into horizontally resized bytes: item = (row, channel, column), lanes
//            along the columns, written PLANAR ([row][channel][64]) so that the vertical pass and the planar
//            output read and write consecutive bytes.  stage / hpass repeat until all rows are done; the
//            resized rows (at most 15 * scale + 2 fs + 2 of 192 bytes) stay in LDS.
//   vpass    item = (output row, channel, four columns): one LDS dword per tap carries four pixels, four int32
//            accumulators in registers, k_t read as a broadcast.  The epilogue writes a dword of four uint8
//            (planar (3, out_h, out_w)), or four floats (x - mean[c]) / std[c] into a zeroed (3, P, P) canvas
//            (Sam.preprocess: tiles and pixels right of out_w / below out_h write 0); a channel flip swaps the
//            planes on the way out.
// LDS is sized per call from the scale (a 2.2x reduction, the 1500 x 2250 workload: 39 resized rows = 7 KB, 27 KB
// in all), not for fs = 16 (274 rows = 51 KB, 71 KB in all).
#include "common.h"

namespace samq {
namespace {

constexpr int RZ_TW = 64;          // output columns of a tile
constexpr int RZ_TH = 16;          // output rows of a tile
constexpr int RZ_MAX_FS = 16;      // largest reduction per axis
constexpr int RZ_TAPS = 2 * RZ_MAX_FS + 1;
constexpr int RZ_ROWB = 3 * RZ_TW; // bytes of a horizontally resized row of the tile
constexpr int RZ_RAW = 8192;       // raw staging buffer, bytes (>= one widened span: 3 * (63 * 16 + 33) + 30)
constexpr int RZ_MAX_OUT = 16384;  // largest output side
constexpr int RZ_THREADS = 256;
constexpr int RZ_PREC = 22;

struct Axis {
  int lo[RZ_TW];
  int cnt[RZ_TW];
  int k[RZ_TW][RZ_TAPS];
};

// bounds and coefficients of output index i of an axis resized from n to m (n != m)
__device__ void axis_coeffs(int i, int n, int m, int& lo_out, int& cnt_out, int* k) {
  const double scale = (double)n / (double)m;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = fs;
  const double center = ((double)i + 0.5) * scale;
  int lo = (int)(center - support + 0.5);
  lo = lo < 0 ? 0 : lo;
  int hi = (int)(center + support + 0.5);
  hi = hi > n ? n : hi;
  int cnt = hi - lo;
  cnt = cnt > RZ_TAPS ? RZ_TAPS : cnt;   // never taken for fs <= 16; keeps the table's row in any case
  double ww = 0.0;
  for (int t = 0; t < cnt; ++t) {
    const double a = ((double)(t + lo) - center + 0.5) / fs;
    const double w = 1.0 - fabs(a);
    ww += w < 0.0 ? 0.0 : w;
  }
  for (int t = 0; t < cnt; ++t) {
    const double a = ((double)(t + lo) - center + 0.5) / fs;
    double w = 1.0 - fabs(a);
    w = w < 0.0 ? 0.0 : w;
    k[t] = (int)(w / ww * 4194304.0 + 0.5);
  }
  lo_out = lo, cnt_out = cnt;
}

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> RZ_PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct ResizeArgs {
  const uint8_t* img;   // window origin: img + (y0 * W + x0) * 3
  const uint8_t* base;  // first byte of the whole image
  const uint8_t* end;   // one past its last byte
  int pitch;            // W * 3
  int in_h, in_w;       // the window
  int out_h, out_w;
  int flip;
  int cap_rows;         // resized rows the dynamic LDS holds
  void* out;
  int out_f32, P;
  const float* mean;
  const float* stdv;
};

__global__ __launch_bounds__(RZ_THREADS) void resize_u8_kernel(ResizeArgs a) {
  __shared__ Axis cx;                      // the tile's columns, then its rows
  __shared__ int ylo[RZ_TH], ycnt[RZ_TH], yk[RZ_TH][RZ_TAPS];
  __shared__ __attribute__((aligned(16))) uint8_t raw[RZ_RAW];
  extern __shared__ __attribute__((aligned(16))) uint8_t hbuf[];   // [cap_rows][3][RZ_TW]

  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * RZ_TW, ty0 = blockIdx.y * RZ_TH;
  const int ncol = min(RZ_TW, a.out_w - tx0), nrow = min(RZ_TH, a.out_h - ty0);   // <= 0: a tile of padding only
  const bool live = ncol > 0 && nrow > 0;
  const bool hskip = a.in_w == a.out_w, vskip = a.in_h == a.out_h;

  if (live) {
    if (tid < RZ_TW) {
      int lo = 0, cnt = 0;
      if (tid < ncol) {
        if (hskip) lo = tx0 + tid, cnt = 1;
        else axis_coeffs(tx0 + tid, a.in_w, a.out_w, lo, cnt, cx.k[tid]);
      }
      cx.lo[tid] = lo, cx.cnt[tid] = cnt;
    } else if (tid < RZ_TW + RZ_TH) {
      const int r = tid - RZ_TW;
      int lo = 0, cnt = 0;
      if (r < nrow) {
        if (vskip) lo = ty0 + r, cnt = 1;
        else axis_coeffs(ty0 + r, a.in_h, a.out_h, lo, cnt, yk[r]);
      }
      ylo[r] = lo, ycnt[r] = cnt;
    }
  }
  __syncthreads();

  int rlo = 0;
  if (live) {
    // lo and hi grow with the index, so the first and the last valid entry bound the tile's taps
    const int clo = cx.lo[0], chi = cx.lo[ncol - 1] + cx.cnt[ncol - 1];
    rlo = ylo[0];
    const int rows = min(ylo[nrow - 1] + ycnt[nrow - 1] - rlo, a.cap_rows);
    const int span = (chi - clo) * 3;                    // bytes of a row that the tile reads
    const int chunks = (span + 15 + 15) / 16;            // 16-byte chunks of the widened span, any alignment
    const int per_trip = min(max(RZ_RAW / (chunks * 16), 1), rows);
    for (int r0 = 0; r0 < rows; r0 += per_trip) {
      const int nr = min(per_trip, rows - r0);
      // stage: nr rows x chunks aligned 16-byte loads
      for (int idx = tid; idx < nr * chunks; idx += RZ_THREADS) {
        const int j = idx / chunks, q = idx - j * chunks;
        const uint8_t* first = a.img + (size_t)(rlo + r0 + j) * a.pitch + (size_t)clo * 3;
        const uint8_t* p = first - ((uintptr_t)first & 15) + (size_t)q * 16;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (p >= a.base && p + 16 <= a.end) {
          v = *(const u32x4*)p;
        } else {
          uint8_t b[16];
#pragma unroll
          for (int e = 0; e < 16; ++e) b[e] = (p + e >= a.base && p + e < a.end) ? p[e] : (uint8_t)0;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[e] = (uint32_t)b[4 * e] | ((uint32_t)b[4 * e + 1] << 8) | ((uint32_t)b[4 * e + 2] << 16) |
                   ((uint32_t)b[4 * e + 3] << 24);
        }
        *(u32x4*)(raw + (size_t)(j * chunks + q) * 16) = v;
      }
      __syncthreads();
      // hpass: item = (row j, channel c, column), lanes along the columns
      for (int idx = tid; idx < nr * RZ_ROWB; idx += RZ_THREADS) {
        const int j = idx / RZ_ROWB, o = idx - j * RZ_ROWB, c = o / RZ_TW, col = o - c * RZ_TW;
        int v = 0;
        if (col < ncol) {
          const uint8_t* first = a.img + (size_t)(rlo + r0 + j) * a.pitch + (size_t)clo * 3;
          const uint8_t* src = raw + j * chunks * 16 + (int)((uintptr_t)first & 15) + (cx.lo[col] - clo) * 3 + c;
          if (hskip) {
            v = src[0];
          } else {
            int acc = 1 << (RZ_PREC - 1);
            const int cnt = cx.cnt[col];
            for (int t = 0; t < cnt; ++t) acc += cx.k[col][t] * (int)src[3 * t];
            v = clip8(acc);
          }
        }
        hbuf[(r0 + j) * RZ_ROWB + o] = (uint8_t)v;
      }
      __syncthreads();
    }
  }

  // vpass and epilogue: item = (output row r, channel c, four columns)
  const int tile_w = a.out_f32 ? min(RZ_TW, a.P - tx0) : ncol;   // columns of the tile that exist in the output
  const int tile_h = a.out_f32 ? min(RZ_TH, a.P - ty0) : nrow;
  const int ld = a.out_f32 ? a.P : a.out_w, planes_h = a.out_f32 ? a.P : a.out_h;
  for (int idx = tid; idx < RZ_TH * 3 * (RZ_TW / 4); idx += RZ_THREADS) {
    const int r = idx / (3 * (RZ_TW / 4)), o = idx - r * (3 * (RZ_TW / 4)), c = o / (RZ_TW / 4), q4 = 4 * (o % (RZ_TW / 4));
    if (r >= tile_h || q4 >= tile_w) continue;
    int px[4] = {0, 0, 0, 0};
    const bool inside = live && r < nrow && q4 < ncol;
    if (inside) {
      const uint8_t* col = hbuf + (ylo[r] - rlo) * RZ_ROWB + c * RZ_TW + q4;
      const int cnt = min(ycnt[r], a.cap_rows - (ylo[r] - rlo));
      if (vskip) {
        const uint32_t w = *(const uint32_t*)col;
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = (int)((w >> (8 * e)) & 255u);
      } else {
        int acc[4] = {1 << (RZ_PREC - 1), 1 << (RZ_PREC - 1), 1 << (RZ_PREC - 1), 1 << (RZ_PREC - 1)};
        for (int t = 0; t < cnt; ++t) {
          const uint32_t w = *(const uint32_t*)(col + t * RZ_ROWB);
          const int k = yk[r][t];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] += k * (int)((w >> (8 * e)) & 255u);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = clip8(acc[e]);
      }
    }
    const int oc = a.flip ? 2 - c : c;
    const size_t at = ((size_t)oc * planes_h + (ty0 + r)) * ld + tx0 + q4;
    const int nvalid = min(4, tile_w - q4);      // columns of this item that exist in the output
    if (a.out_f32) {
      const float mu = a.mean[oc], sd = a.stdv[oc];
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = (inside && q4 + e < ncol) ? ((float)px[e] - mu) / sd : 0.0f;
      float* dst = (float*)a.out + at;
      if (nvalid == 4 && (((uintptr_t)dst) & 15) == 0) {
        *(float4_t*)dst = float4_t{f[0], f[1], f[2], f[3]};
      } else {
        for (int e = 0; e < nvalid; ++e) dst[e] = f[e];
      }
    } else {
      uint8_t* dst = (uint8_t*)a.out + at;
      if (nvalid == 4 && (((uintptr_t)dst) & 3) == 0) {
        *(uint32_t*)dst = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
      } else {
        for (int e = 0; e < nvalid; ++e) dst[e] = (uint8_t)px[e];
      }
    }
  }
}

// resized rows a tile can need: hi(last row) - lo(first row) <= 15 scale + 2 fs + 1, plus one for the roundings
int tile_rows(int n, int m) {
  if (n == m) return RZ_TH;
  const double scale = (double)n / (double)m, fs = scale < 1.0 ? 1.0 : scale;
  const int r = (int)((RZ_TH - 1) * scale + 2.0 * fs) + 2;
  return r < n ? r : n;
}
constexpr int RZ_MAX_ROWS = (RZ_TH - 1) * RZ_MAX_FS + 2 * RZ_MAX_FS + 2;

}  // namespace
}  // namespace samq

using namespace samq;

extern "C" int samq_resize_u8(const uint8_t* img, int H, int W, int x0, int y0, int x1, int y1, int out_h, int out_w,
                              int flip, void* out, int out_f32, const float* pixel_mean, const float* pixel_std,
                              int pad_to, hipStream_t stream) {
  if (!img && out_h >= 0 && out_w >= 0 && (out_h == 0 || out_w == 0)) return SAMQ_OK;
  SAMQ_REQUIRE(out_h >= 1 && out_w >= 1, SAMQ_ERR_INVALID, "resize_u8: empty output");
  SAMQ_REQUIRE(H >= 1 && W >= 1 && x0 >= 0 && y0 >= 0 && x1 <= W && y1 <= H, SAMQ_ERR_INVALID,
               "resize_u8: window outside the image");
  SAMQ_REQUIRE(x1 > x0 && y1 > y0, SAMQ_ERR_INVALID, "resize_u8: empty window");
  const int in_h = y1 - y0, in_w = x1 - x0;
  SAMQ_REQUIRE((int64_t)in_h <= (int64_t)RZ_MAX_FS * out_h && (int64_t)in_w <= (int64_t)RZ_MAX_FS * out_w,
               SAMQ_ERR_UNSUPPORTED, "resize_u8: reduction above 16x on an axis");
  SAMQ_REQUIRE(out_h <= RZ_MAX_OUT && out_w <= RZ_MAX_OUT && pad_to <= RZ_MAX_OUT && W <= (1 << 24), SAMQ_ERR_UNSUPPORTED,
               "resize_u8: output side above 16384 or image wider than 2^24");
  SAMQ_REQUIRE(img && out, SAMQ_ERR_INVALID, "resize_u8: null pointer");
  if (out_f32) {
    SAMQ_REQUIRE(pixel_mean && pixel_std, SAMQ_ERR_INVALID, "resize_u8: the float output needs pixel_mean and pixel_std");
    SAMQ_REQUIRE(pad_to >= out_h && pad_to >= out_w, SAMQ_ERR_INVALID, "resize_u8: pad_to below the output size");
    SAMQ_REQUIRE(((uintptr_t)out & 3) == 0, SAMQ_ERR_INVALID, "resize_u8: misaligned output");
  }
  ResizeArgs a;
  a.base = img;
  a.end = img + (size_t)H * W * 3;
  a.pitch = W * 3;
  a.img = img + ((size_t)y0 * W + x0) * 3;
  a.in_h = in_h, a.in_w = in_w, a.out_h = out_h, a.out_w = out_w;
  a.flip = flip != 0;
  a.cap_rows = tile_rows(in_h, out_h);
  a.out = out, a.out_f32 = out_f32 != 0, a.P = pad_to;
  a.mean = pixel_mean, a.stdv = pixel_std;
  const int gw = a.out_f32 ? pad_to : out_w, gh = a.out_f32 ? pad_to : out_h;
  const dim3 grid((unsigned)((gw + RZ_TW - 1) / RZ_TW), (unsigned)((gh + RZ_TH - 1) / RZ_TH));
  const size_t lds = (size_t)a.cap_rows * RZ_ROWB;
  if (lds > 32 * 1024) {   // with the static tables past the default limit of a workgroup
    static const hipError_t raised = hipFuncSetAttribute((const void*)resize_u8_kernel,
                                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                                         RZ_MAX_ROWS * RZ_ROWB);
    if (raised != hipSuccess) return check_hip(raised, "resize_u8: dynamic LDS");
  }
  hipLaunchKernelGGL(resize_u8_kernel, grid, dim3(RZ_THREADS), lds, stream, a);
  SAMQ_LAUNCH_CHECK("resize_u8 launch");
  return SAMQ_OK;
}
