// Windowed / global multi-head attention with in-kernel decomposed relative-position bias.
//
// Replaces QuantAttention's attention part (gptq_triton/fused_attention.py:107-149): the two
// torch.matmul rel-pos products (add_decomposed_rel_pos :46-80), the `torch.full(+inf)` output
// init and the Triton flash kernel `_fwd_kernel1` (:159-309) -- and, in the windowed blocks,
// the window_partition / window_unpartition copies (image_encoder.py:195-202, 282-333): tokens
// are read from / written to the natural [B, H, W, C] layout, padded window tokens are
// synthesised in-kernel (their q/k/v equal the qkv bias).
//
// Three kernels, one header each: the window kernel for SAM's 14 x 14 windows (attention_win.h),
// the 32x32-MFMA kernel for the ViT-H global blocks (attention_glob80.h) and the general kernel
// for every other geometry and for precomputed bias tensors (attention_rel.h).  This file holds
// the launchers, the dispatcher and the C entry points.
#include "attention_glob80.h"
#include "attention_rel.h"
#include "attention_win.h"

namespace samq {

static int launch_glob80(const AttnParams& p, int units, hipStream_t stream) {
  AttnParams q = p;
  q.nqb = 16;
  q.units = units;
  hipLaunchKernelGGL(glob80_attention_kernel, dim3(16 * p.heads * units), dim3(512), 0, stream, q);
  SAMQ_LAUNCH_CHECK("glob80_attention launch");
  return SAMQ_OK;
}

template <int D>
static int launch_win(const AttnParams& p, int units, hipStream_t stream) {
  const int items = units * p.heads;
  // The W4A8 int8-code store (round 5): P as fp16 hi + lo (PHL), the output at
  // fp32-level error before the proj QAct's quantiser -- window-stage codes off by one 1.21-1.33e-3
  // instead of 2.05-2.24e-3, for two MFMAs per P.V step (int8-store launch 45.4 vs 35.5 us, W4A8
  // step -1.4 %, profiles/r5_w4a8_window_phl.log)
  if (p.out_scale > 0.f)
    hipLaunchKernelGGL((win_attention_kernel<D, true>), dim3(items), dim3(256), 0, stream, p, items);
  else
    hipLaunchKernelGGL((win_attention_kernel<D>), dim3(items), dim3(256), 0, stream, p, items);
  SAMQ_LAUNCH_CHECK("win_attention launch");
  return SAMQ_OK;
}

template <int D, int SP, int NW, bool RES, bool PRE, int RS = 16, int SC = 0>
static int launch_attn(const AttnParams& p, int units, hipStream_t stream) {
  const int tiles = p.S * (SP / 16);
  const int qblocks = (tiles + NW * REL_QT - 1) / (NW * REL_QT);
  if (!RES && (p.heads * units) % 8 == 0) {   // 1-D grid, XCD-aware (see the kernel)
    AttnParams q = p;
    q.nqb = qblocks;
    q.units = units;
    hipLaunchKernelGGL((rel_attention_kernel<D, SP, NW, RES, PRE, RS, SC>), dim3(qblocks * p.heads * units),
                       dim3(64 * NW), 0, stream, q);
  } else {
    hipLaunchKernelGGL((rel_attention_kernel<D, SP, NW, RES, PRE, RS, SC>), dim3(qblocks, p.heads, units),
                       dim3(64 * NW), 0, stream, p);
  }
  SAMQ_LAUNCH_CHECK("rel_attention launch");
  return SAMQ_OK;
}

template <bool PRE>
static int dispatch_attn(const AttnParams& p, int hd, int units, hipStream_t stream) {
  const int S = p.S;
  if (!PRE && S == 14)   // SAM's window size: two-workgroups-per-CU window kernel
    return hd == 80 ? launch_win<80>(p, units, stream) : launch_win<64>(p, units, stream);
  // ViT-H global blocks: the 32x32-MFMA kernel (needs heads * units % 8 == 0 for its XCD order)
  if (!PRE && S == 64 && hd == 80 && (p.heads * units) % 8 == 0 && p.H == 64 && p.W == 64)
    return launch_glob80(p, units, stream);
  if (S <= 16) {  // whole window / small grid resident in LDS; one query tile per grid row
    if constexpr (PRE) {   // !PRE && S == 14 is the window kernel's (above)
      if (S == 14)
        return hd == 80 ? launch_attn<80, 16, 7, true, PRE, 14, 14>(p, units, stream)
                        : launch_attn<64, 16, 7, true, PRE, 14, 14>(p, units, stream);
    }
    return hd == 80 ? launch_attn<80, 16, 8, true, PRE>(p, units, stream)
                    : launch_attn<64, 16, 8, true, PRE>(p, units, stream);
  } else if (S == 32) {
    return hd == 80 ? launch_attn<80, 32, 8, false, PRE, 16, 32>(p, units, stream)
                    : launch_attn<64, 32, 8, false, PRE, 16, 32>(p, units, stream);
  } else {
    return hd == 80 ? launch_attn<80, 64, 8, false, PRE, 16, 64>(p, units, stream)
                    : launch_attn<64, 64, 8, false, PRE, 16, 64>(p, units, stream);
  }
}

}  // namespace samq

using namespace samq;

static int rel_attention_impl(const void* qkv, const void* qkv_bias, const void* rel_pos_h, const void* rel_pos_w,
                              void* out, int B, int H, int W, int heads, int hd, int window, float sm_scale,
                              float out_scale, hipStream_t stream) {
  if (B == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(qkv && rel_pos_h && rel_pos_w && out, SAMQ_ERR_INVALID, "rel_attention: null pointer");
  SAMQ_REQUIRE(hd == 64 || hd == 80, SAMQ_ERR_UNSUPPORTED, "rel_attention: head_dim must be 64 or 80");
  SAMQ_REQUIRE(B > 0 && H > 0 && W > 0 && heads > 0, SAMQ_ERR_INVALID, "rel_attention: bad shape");
  AttnParams p{};
  p.qkv = (const _Float16*)qkv;
  p.qkv_bias = (const _Float16*)qkv_bias;
  p.relh = (const _Float16*)rel_pos_h;
  p.relw = (const _Float16*)rel_pos_w;
  p.out = (_Float16*)out;
  p.C = heads * hd;
  p.tok_stride = 3 * (int64_t)p.C;
  p.heads = heads;
  p.H = H;
  p.W = W;
  p.scale = sm_scale;
  p.out_scale = out_scale;
  p.out_inv = out_scale > 0.f ? 1.0f / out_scale : 0.f;
  int units;
  if (window > 0) {
    SAMQ_REQUIRE(window <= 16, SAMQ_ERR_UNSUPPORTED, "rel_attention: window must be <= 16");
    p.S = window;
    const int nwy = (H + window - 1) / window, nwx = (W + window - 1) / window;
    p.nwx = nwx;
    p.upi = nwy * nwx;
    units = B * p.upi;
  } else {
    SAMQ_REQUIRE(H == W, SAMQ_ERR_UNSUPPORTED, "rel_attention: global attention needs H == W");
    SAMQ_REQUIRE(H <= 16 || H == 32 || H == 64, SAMQ_ERR_UNSUPPORTED,
                 "rel_attention: global grid side must be <= 16, 32 or 64");
    p.S = H;
    p.nwx = 1;
    p.upi = 1;
    units = B;
  }
  SAMQ_REQUIRE(units <= 65535, SAMQ_ERR_INVALID, "rel_attention: too many windows*batch");
  return dispatch_attn<false>(p, hd, units, stream);
}

extern "C" int samq_rel_attention(const void* qkv, const void* qkv_bias, const void* rel_pos_h, const void* rel_pos_w,
                                  void* out, int B, int H, int W, int heads, int hd, int window, float sm_scale,
                                  hipStream_t stream) {
  return rel_attention_impl(qkv, qkv_bias, rel_pos_h, rel_pos_w, out, B, H, W, heads, hd, window, sm_scale, 0.f,
                            stream);
}

extern "C" int samq_rel_attention_q(const void* qkv, const void* qkv_bias, const void* rel_pos_h,
                                    const void* rel_pos_w, int8_t* out, int B, int H, int W, int heads, int hd,
                                    int window, float sm_scale, float out_scale, hipStream_t stream) {
  SAMQ_REQUIRE(out_scale > 0.f, SAMQ_ERR_INVALID, "rel_attention_q: out_scale must be > 0");
  SAMQ_REQUIRE(((uintptr_t)out & 3) == 0, SAMQ_ERR_INVALID, "rel_attention_q: out must be 4-byte aligned");
  return rel_attention_impl(qkv, qkv_bias, rel_pos_h, rel_pos_w, out, B, H, W, heads, hd, window, sm_scale,
                            out_scale, stream);
}

extern "C" int samq_attention_relbias(const void* inp, const void* rel_h, const void* rel_w, void* out, int B, int S,
                                      int heads, int hd, float sm_scale, hipStream_t stream) {
  SAMQ_REQUIRE(inp && rel_h && rel_w && out, SAMQ_ERR_INVALID, "attention_relbias: null pointer");
  SAMQ_REQUIRE(hd == 64 || hd == 80, SAMQ_ERR_UNSUPPORTED, "attention_relbias: head_dim must be 64 or 80");
  SAMQ_REQUIRE(B > 0 && B <= 65535 && heads > 0, SAMQ_ERR_INVALID, "attention_relbias: bad shape");
  SAMQ_REQUIRE(S <= 16 || S == 32 || S == 64, SAMQ_ERR_UNSUPPORTED,
               "attention_relbias: grid side must be <= 16, 32 or 64");
  AttnParams p{};
  p.qkv = (const _Float16*)inp;
  p.qkv_bias = nullptr;
  p.relh = (const _Float16*)rel_h;
  p.relw = (const _Float16*)rel_w;
  p.out = (_Float16*)out;
  p.C = heads * hd;
  p.tok_stride = 3 * (int64_t)p.C;
  p.heads = heads;
  p.S = S;
  p.H = S;
  p.W = S;
  p.nwx = 1;
  p.upi = 1;
  p.scale = sm_scale;
  return dispatch_attn<true>(p, hd, B, stream);
}
