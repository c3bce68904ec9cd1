// Attention kernels: the pieces the three kernel families share -- the launch parameters, the
// fp16 / int8-code output store, counted vmcnt waits, the asm form of ds_read_b64_tr_b16 and the
// MFMA / max helpers.  Included by attention.hip only (through the kernel headers).
#pragma once

#include "common.h"

namespace samq {

constexpr float LOG2E = 1.4426950408889634f;

__device__ __attribute__((aligned(16))) _Float16 g_zero16[8];   // zero source for pad slots

struct AttnParams {
  const _Float16* qkv;      // token stride tok_stride (elements); q at h*D, k at C+h*D, v at 2C+h*D
  const _Float16* qkv_bias; // [3C] or null
  const _Float16* relh;     // table [2S-1][D] f16  | precomputed [B'*heads][S][S][S] f16
  const _Float16* relw;
  _Float16* out;            // token stride C
  int64_t tok_stride;
  int C, heads;
  int S;                    // window side (windowed) or grid side (global)
  int H, W;                 // image token grid
  int nwx, upi;             // windows per row, windows per image
  float scale;              // sm_scale
  int nqb, units;           // streaming path with a 1-D XCD-ordered grid: query blocks, units
  float out_scale, out_inv; // > 0: out holds int8 codes q8(fp16(o), out_scale) (W4A8 proj QAct)
};

// Store 4 output channels at element offset off of the [B, H, W, C] output: fp16, or (W4A8) the
// int8 codes of the proj input QAct applied to the f32 attention output itself (round 4: no fp16
// rounding in between -- the W4A8 oracle quantises its f32 attention; the fp16 round trip moved
// ~127 * 2^-11 code units at the top of the range, the dominant share of the stage's one-code
// flips).
__device__ __forceinline__ void attn_store4(const AttnParams& p, int64_t off, float4_t o) {
  if (p.out_scale > 0.f) {
    const float lim = 130.0f * p.out_scale;
    const float2_t c01 = q8_exact2(float2_t{o[0], o[1]}, p.out_scale, p.out_inv, lim);
    const float2_t c23 = q8_exact2(float2_t{o[2], o[3]}, p.out_scale, p.out_inv, lim);
    *(uint32_t*)((int8_t*)p.out + off) = q8_pack4(c01.x, c01.y, c23.x, c23.y);
  } else {
    *(half4_t*)(p.out + off) = half4_t{(_Float16)o[0], (_Float16)o[1], (_Float16)o[2], (_Float16)o[3]};
  }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 15, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ds_read_b64_tr_b16 through inline asm: the intrinsic form carries no alias information, so the
// compiler treats it as possibly reading the in-flight LDS-DMA ring and drains vmcnt(0) before it
// (killing the K/V prefetch).  The asm form is invisible to that analysis; the caller waits
// lgkmcnt itself in an asm that takes the fragments as "+v" operands (which also orders the MFMAs
// after the wait).  OFF is the instruction's 16-bit immediate offset (no VGPR per address).
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)((const SAMQ_LDS char*)p);
}
template <int OFF>
__device__ __forceinline__ half4_t ds_read_tr16_off(uint32_t addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset");
  half4_t r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}

__device__ __forceinline__ float max3f(float a, float b, float c) {
  // NOT inline asm: the hazard recognizer does not pad an asm VALU read of a fresh MFMA result,
  // which then reads stale accumulator lanes at random (nondeterministic scores).
  return fmaxf(fmaxf(a, b), c);
}

__device__ __forceinline__ float16_t mfma32(half8_t a, half8_t b, float16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

}  // namespace samq
