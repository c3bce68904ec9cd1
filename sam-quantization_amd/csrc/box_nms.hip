// Greedy box non-maximum suppression with torchvision.ops.nms's arithmetic, the sweep included on the device.
// Input: the boxes already in rank order (descending score, equal scores by ascending index: a stable sort
// in the caller) and `order`, each rank's original index.  Box j is dropped when a kept box i of higher rank has
//   inter / (area_i + area_j - inter) > thr,   inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1)),
// every operation its own fp32 IEEE operation (this file is built without contraction and with the
// correctly rounded division): 0 / 0 is NaN, compares false, and the box stays.
//
// nms_bits    one wave per upper-triangular 64 x 64 tile of the (rank x rank) suppression matrix.  Lane r
//             holds row box r and its area in registers; the 64 column boxes sit one per lane and reach the
//             loop as SGPR operands by v_readlane (no LDS).  Each lane builds one 64-bit word, bits at or left
//             of the diagonal and columns past n cleared, and stores bits[r][tile_col]: n * ceil(n / 64)
//             words; the tiles below the diagonal are never written and never read.
// nms_sweep   ONE workgroup, thread t owning the running "removed" word of columns 64 t .. 64 t + 63 in a
//             register (512 threads cover the 32768 boxes the entry accepts).  Rows go 64 at a time.  The
//             only true dependency inside a block of 64 rows is its diagonal tile: lane r of every wave holds
//             row r's diagonal word (loaded one block ahead), the block's removed word arrives through LDS,
//             and a 64-step loop on lane reads, all in SGPRs and redundantly in every wave, decides keep or
//             drop with no memory access and no barrier.  Then thread t > block ORs the words bits[row][t]
//             of the kept rows into its own word, eight independent loads in flight at a time (a batch
//             short of eight repeats its first row: OR is idempotent).  One barrier and one memory round trip
//             per 64 boxes instead of one per box; the matrix never leaves the device.
// The sweep is sequential over blocks by nature (block b's removed word needs every kept row before it), so
// more workgroups would only add grid-wide synchronisation; its parallelism is across the column words.
#include "common.h"

namespace samq {
namespace {

constexpr int NMS_MAX = 32768;

typedef unsigned long long u64;

__device__ __forceinline__ float lane_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ u64 lane_u64(u64 v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 uniform_u64(u64 v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void nms_bits(const float4_t* __restrict__ boxes, u64* __restrict__ bits, int n,
                                               int ct, float thr) {
  const int cb = blockIdx.x, rb = blockIdx.y, lane = threadIdx.x;
  if (cb < rb) return;
  const int row = rb * 64 + lane, col = cb * 64 + lane;
  const float4_t r = boxes[min(row, n - 1)], c = boxes[min(col, n - 1)];
  const float ra = (r.z - r.x) * (r.w - r.y), ca = (c.z - c.x) * (c.w - c.y);
  u64 word = 0;
#pragma unroll 8
  for (int j = 0; j < 64; ++j) {
    const float cx1 = lane_f(c.x, j), cy1 = lane_f(c.y, j), cx2 = lane_f(c.z, j), cy2 = lane_f(c.w, j);
    const float w = fmaxf(fminf(r.z, cx2) - fmaxf(r.x, cx1), 0.f);
    const float h = fmaxf(fminf(r.w, cy2) - fmaxf(r.y, cy1), 0.f);
    const float inter = w * h;
    const float iou = inter / (ra + lane_f(ca, j) - inter);
    word |= (u64)(iou > thr) << j;
  }
  const int ncol = min(64, n - cb * 64);
  u64 live = ncol == 64 ? ~0ull : (1ull << ncol) - 1;
  if (cb == rb) live &= ~((2ull << lane) - 1);      // strictly right of the diagonal
  if (row < n) bits[(size_t)row * ct + cb] = word & live;
}

__global__ __launch_bounds__(512) void nms_sweep(const u64* __restrict__ bits, const int* __restrict__ order,
                                                 int* __restrict__ keep, int* __restrict__ n_keep, int n, int ct) {
  __shared__ u64 cur[2];
  const int t = threadIdx.x, lane = t & 63;
  u64 mine = 0;      // removed word of columns 64 t ..
  int kept = 0;
  u64 d = lane < n ? bits[(size_t)lane * ct] : 0;     // block 0's diagonal words
  for (int rb = 0; rb < ct; ++rb) {
    if (t == rb) cur[rb & 1] = mine;
    u64 dn = 0;
    const int nrow = (rb + 1) * 64 + lane;
    if (rb + 1 < ct && nrow < n) dn = bits[(size_t)nrow * ct + rb + 1];
    __syncthreads();
    u64 R = uniform_u64(cur[rb & 1]);
    const int valid = min(64, n - rb * 64);
    if (valid < 64) R |= ~0ull << valid;
    u64 km = 0;
#pragma unroll
    for (int r = 0; r < 64; ++r) {
      if (!((R >> r) & 1)) {
        km |= 1ull << r;
        R |= lane_u64(d, r);
      }
    }
    if (t < 64 && ((km >> lane) & 1)) keep[kept + __popcll(km & ((1ull << lane) - 1))] = order[rb * 64 + lane];
    kept += __popcll(km);
    if (t > rb && t < ct) {
      const u64* rowp = bits + (size_t)rb * 64 * ct + t;
      u64 left = km;
      while (left) {
        const int r0 = __builtin_ctzll(left);
        int rr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          rr[u] = left ? __builtin_ctzll(left) : r0;
          left &= left - 1;
        }
        u64 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = rowp[(size_t)rr[u] * ct];
#pragma unroll
        for (int u = 0; u < 8; ++u) mine |= v[u];
      }
    }
    d = dn;
  }
  if (t == 0) *n_keep = kept;
}

size_t words(int n) { return (size_t)n * ((n + 63) / 64); }

}  // namespace
}  // namespace samq

using namespace samq;

extern "C" size_t samq_box_nms_workspace(int n) {
  return n <= 0 || n > NMS_MAX ? 0 : words(n) * sizeof(u64);
}

extern "C" int samq_box_nms(const float* boxes, const int32_t* order, int n, float thr, int32_t* keep,
                            int32_t* n_keep, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (n == 0) return SAMQ_OK;
  SAMQ_REQUIRE(n > 0, SAMQ_ERR_INVALID, "box_nms: n must be >= 0");
  SAMQ_REQUIRE(n <= NMS_MAX, SAMQ_ERR_UNSUPPORTED, "box_nms: more than 32768 boxes");
  SAMQ_REQUIRE(boxes && order && keep && n_keep && workspace, SAMQ_ERR_INVALID, "box_nms: null pointer");
  SAMQ_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)workspace & 7) == 0 &&
                   (((uintptr_t)order | (uintptr_t)keep | (uintptr_t)n_keep) & 3) == 0,
               SAMQ_ERR_INVALID, "box_nms: misaligned pointer");
  SAMQ_REQUIRE(workspace_bytes >= words(n) * sizeof(u64), SAMQ_ERR_INVALID, "box_nms: workspace too small");
  const int ct = (n + 63) / 64;
  u64* bits = (u64*)workspace;
  hipLaunchKernelGGL(nms_bits, dim3((unsigned)ct, (unsigned)ct), dim3(64), 0, stream, (const float4_t*)boxes, bits, n,
                     ct, thr);
  hipLaunchKernelGGL(nms_sweep, dim3(1), dim3((unsigned)(64 * ((ct + 63) / 64))), 0, stream, (const u64*)bits, order,
                     keep, n_keep, n, ct);
  SAMQ_LAUNCH_CHECK("box_nms launch");
  return SAMQ_OK;
}
