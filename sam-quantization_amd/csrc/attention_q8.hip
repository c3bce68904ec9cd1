// W8A8 (fq_vit) attention with decomposed relative position on int8 q/k/v codes, gfx950.
//
// Replaces fq_vit's quant-mode Attention.forward (fq_vit/models/sam/image_encoder.py:437-478):
//   qkv   = qact1(qkv(x))                       -> int8 codes, per-tensor scale s_qkv (input)
//   attn  = qact_attn1((q * scale) @ k^T)       -> quantised with s_a1
//   attn  = use_rel_pos_qact(attn + rel_h + rel_w)   (add_decomposed_rel_pos, quirk-1 rel_w
//           indexed by the query ROW, image_encoder.py:402)          -> quantised with s_a2
//   attn  = softmax(attn)                       (QIntSoftmax = F.softmax, layers.py:379)
//   o     = qact2(attn @ v)                     -> int8 codes with s_out (output, proj input)
// together with window_partition / window_unpartition (padded tokens are keys/values whose qkv is
// the fake-quantised qkv bias, exactly as the reference's zero-padded LayerNorm output projects).
//
// Arithmetic (all exact or fp32, SURVEY.md §8c Oracle F):
//   * q.k on v_mfma_i32_16x16x64_i8: exact int32; value = int * (s_qkv * scale * s_qkv);
//   * rel_h / rel_w: fp32 dot products of the fake-quant q (code * s_qkv) with the f32 tables;
//   * the two score quantisers multiply by the hoisted reciprocal of the scale, round with rintf
//     (round-half-to-even, as torch.round in uniform.py:31-36) and clamp to [-128, 127];
//   * softmax in fp32 (online, exp of x - max as the reference), P.V on fp16 MFMA with P split
//     hi + lo (both fp16; |P - hi - lo| ~ 2^-22 |P|) and the exact int8 V codes as fp16.
//
// Kernels, each templated on the head dim D = 64 / 80 (shared pieces: attention_q8_util.h):
//   attention_q8_win.h      14 x 14 windows, half a window's query rows per workgroup;
//   attention_q8_generic.h  other windows <= 16 (resident keys, 13 or 16 waves) and global grids
//                           below 64 x 64 (64-key chunks streamed through LDS);
//   attention_q8_row64.h    the global 64 x 64 grid, int8 V or the producer's fp16 copy of V.
#include "attention_q8_generic.h"
#include "attention_q8_row64.h"
#include "attention_q8_win.h"

using namespace samq;

// f(integral_constant<int, hd>) for the two head dims the kernels are built for
template <typename F>
static void with_head_dim(int hd, F&& f) {
  if (hd == 64) f(std::integral_constant<int, 64>{});
  else f(std::integral_constant<int, 80>{});
}

extern "C" int samq_rel_attention_q8_rows(const int8_t* qkv, const float* qkv_bias, const float* rel_pos_h,
                                          const float* rel_pos_w, int8_t* out, int B, int H, int W, int heads,
                                          int hd, int window, float sm_scale, float s_qkv, float s_a1, float s_a2,
                                          float s_out, int row0, int rows, const void* v16, hipStream_t stream) {
  if (B == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(qkv && rel_pos_h && rel_pos_w && out, SAMQ_ERR_INVALID, "rel_attention_q8: null pointer");
  SAMQ_REQUIRE(hd == 64 || hd == 80, SAMQ_ERR_UNSUPPORTED, "rel_attention_q8: head_dim must be 64 or 80");
  SAMQ_REQUIRE(B > 0 && H > 0 && W > 0 && heads > 0, SAMQ_ERR_INVALID, "rel_attention_q8: bad shape");
  SAMQ_REQUIRE(s_qkv > 0.f && s_a1 > 0.f && s_a2 > 0.f && s_out > 0.f, SAMQ_ERR_INVALID,
               "rel_attention_q8: scales must be > 0");
  SAMQ_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 3) == 0, SAMQ_ERR_INVALID,
               "rel_attention_q8: qkv must be 16-byte aligned");
  if (rows < 0) { row0 = 0; rows = H; }   // the whole grid
  SAMQ_REQUIRE(row0 >= 0 && rows > 0 && row0 + rows <= H, SAMQ_ERR_INVALID, "rel_attention_q8: bad row range");
  SAMQ_REQUIRE(window > 0 ? (row0 % window == 0 && (rows % window == 0 || row0 + rows == H))
                          : (rows == H || H == 64), SAMQ_ERR_UNSUPPORTED,
               "rel_attention_q8: a row range must cover whole windows (global: the 64 x 64 grid only)");
  SAMQ_REQUIRE(((uintptr_t)v16 & 15) == 0, SAMQ_ERR_INVALID, "rel_attention_q8: v16 must be 16-byte aligned");
  AttnQ8Params p{};
  p.qkv = qkv; p.qkv_bias = qkv_bias; p.relh = rel_pos_h; p.relw = rel_pos_w; p.out = out;
  p.v16 = (const _Float16*)v16;
  p.B = B; p.H = H; p.W = W; p.heads = heads; p.C = heads * hd;
  // (q * scale) . k with q = c_q * s_qkv, k = c_k * s_qkv  (fq_vit image_encoder.py:455)
  p.qk_scale = (s_qkv * sm_scale) * s_qkv;
  p.s_qkv = s_qkv; p.s_a1 = s_a1; p.s_a2 = s_a2; p.s_out = s_out;
  p.inv_a1 = 1.0f / s_a1; p.inv_a2 = 1.0f / s_a2; p.k2 = s_a2 * 1.4426950408889634f;
  if (window > 0) {
    SAMQ_REQUIRE(window <= 16, SAMQ_ERR_UNSUPPORTED, "rel_attention_q8: window must be <= 16");
    p.S = window; p.window = window;
    p.nwh = (rows + window - 1) / window; p.nww = (W + window - 1) / window;
    p.row0 = row0 / window;
    p.L = window * window;
  } else {
    SAMQ_REQUIRE(H == W && H <= 64, SAMQ_ERR_UNSUPPORTED, "rel_attention_q8: global attention needs H == W <= 64");
    p.S = H; p.window = 0; p.nwh = p.nww = 1; p.L = H * W;
    p.row0 = row0;
  }
  with_head_dim(hd, [&](auto hdc) {
    constexpr int D = decltype(hdc)::value;
    constexpr int NWQ = 4;   // global: waves of 16 queries per workgroup
    const unsigned items = B * p.nwh * p.nww;
    if (window == 14)        // SAM's 14 x 14 windows: key and query rows of 16 slots, half a window per workgroup
      hipLaunchKernelGGL((rel_attention_q8_win_kernel<D, 14, 7>), dim3(items, heads, 2), dim3(64 * 7), 0, stream, p);
    else if (window > 0 && p.L <= 13 * 16)
      hipLaunchKernelGGL((rel_attention_q8_kernel<D, true, 13, 256, 16>), dim3(items, heads, 1), dim3(64 * 13), 0,
                         stream, p);
    else if (window > 0)
      hipLaunchKernelGGL((rel_attention_q8_kernel<D, true, 16, 256, 16>), dim3(items, heads, 1), dim3(64 * 16), 0,
                         stream, p);
    else if (H != 64)
      hipLaunchKernelGGL((rel_attention_q8_kernel<D, false, NWQ, 64, 64>),
                         dim3(B, heads, (p.L + 16 * NWQ - 1) / (16 * NWQ)), dim3(64 * NWQ), 0, stream, p);
    else if (v16)            // 64 x 64: one grid row of queries per workgroup (16 * NWQ == 64)
      hipLaunchKernelGGL((rel_attention_q8_row64_kernel<D, NWQ, true>), dim3(B, heads, rows), dim3(64 * NWQ), 0,
                         stream, p);
    else
      hipLaunchKernelGGL((rel_attention_q8_row64_kernel<D, NWQ>), dim3(B, heads, rows), dim3(64 * NWQ), 0, stream, p);
  });
  SAMQ_LAUNCH_CHECK("rel_attention_q8 launch");
  return SAMQ_OK;
}

// The same on codes with zero points (AttnQ8ParamsZp, attention_q8_util.h): the ZP instantiation of
// every kernel above.  No fp16 V copy: the row64 kernel runs its int8-V form.
extern "C" int samq_rel_attention_q8_zp(const int8_t* qkv, const float* qkv_bias, const float* rel_pos_h,
                                        const float* rel_pos_w, int8_t* out, int B, int H, int W, int heads, int hd,
                                        int window, float sm_scale, float s_qkv, float s_a1, float s_a2, float s_out,
                                        int row0, int rows, const void* v16, int zp_qkv, int zp_a1, int zp_a2,
                                        int zp_out, hipStream_t stream) {
  if (B == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(qkv && rel_pos_h && rel_pos_w && out, SAMQ_ERR_INVALID, "rel_attention_q8_zp: null pointer");
  SAMQ_REQUIRE(hd == 64 || hd == 80, SAMQ_ERR_UNSUPPORTED, "rel_attention_q8_zp: head_dim must be 64 or 80");
  SAMQ_REQUIRE(!v16, SAMQ_ERR_UNSUPPORTED, "rel_attention_q8_zp: no fp16 V copy under zero points (pass null)");
  SAMQ_REQUIRE(B > 0 && H > 0 && W > 0 && heads > 0, SAMQ_ERR_INVALID, "rel_attention_q8_zp: bad shape");
  SAMQ_REQUIRE(s_qkv > 0.f && s_a1 > 0.f && s_a2 > 0.f && s_out > 0.f, SAMQ_ERR_INVALID,
               "rel_attention_q8_zp: scales must be > 0");
  auto zok = [](int z) { return z >= -128 && z <= 127; };
  SAMQ_REQUIRE(zok(zp_qkv) && zok(zp_a1) && zok(zp_a2) && zok(zp_out), SAMQ_ERR_INVALID,
               "rel_attention_q8_zp: zero points must be in [-128, 127]");
  SAMQ_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 3) == 0, SAMQ_ERR_INVALID,
               "rel_attention_q8_zp: qkv must be 16-byte aligned");
  if (rows < 0) { row0 = 0; rows = H; }   // the whole grid
  SAMQ_REQUIRE(row0 >= 0 && rows > 0 && row0 + rows <= H, SAMQ_ERR_INVALID, "rel_attention_q8_zp: bad row range");
  SAMQ_REQUIRE(window > 0 ? (row0 % window == 0 && (rows % window == 0 || row0 + rows == H))
                          : (rows == H || H == 64), SAMQ_ERR_UNSUPPORTED,
               "rel_attention_q8_zp: a row range must cover whole windows (global: the 64 x 64 grid only)");
  AttnQ8ParamsZp p{};
  p.qkv = qkv; p.qkv_bias = qkv_bias; p.relh = rel_pos_h; p.relw = rel_pos_w; p.out = out;
  p.v16 = nullptr;
  p.B = B; p.H = H; p.W = W; p.heads = heads; p.C = heads * hd;
  p.qk_scale = (s_qkv * sm_scale) * s_qkv;
  p.s_qkv = s_qkv; p.s_a1 = s_a1; p.s_a2 = s_a2; p.s_out = s_out;
  p.inv_a1 = 1.0f / s_a1; p.inv_a2 = 1.0f / s_a2; p.k2 = s_a2 * 1.4426950408889634f;
  p.z_qkv = (float)zp_qkv; p.z_a1 = (float)zp_a1; p.z_a2 = (float)zp_a2; p.z_out = (float)zp_out;
  p.zfold = (float)zp_a2 - (float)zp_a1 * (s_a1 * p.inv_a2);
  p.zi_qkv = zp_qkv; p.dz2 = hd * zp_qkv * zp_qkv;
  p.zc_twice = zp_qkv == -128;
  p.zc = (int)(0x01010101u * (uint32_t)((p.zc_twice ? 64 : -zp_qkv) & 0xFF));
  if (window > 0) {
    SAMQ_REQUIRE(window <= 16, SAMQ_ERR_UNSUPPORTED, "rel_attention_q8_zp: window must be <= 16");
    p.S = window; p.window = window;
    p.nwh = (rows + window - 1) / window; p.nww = (W + window - 1) / window;
    p.row0 = row0 / window;
    p.L = window * window;
  } else {
    SAMQ_REQUIRE(H == W && H <= 64, SAMQ_ERR_UNSUPPORTED, "rel_attention_q8_zp: global attention needs H == W <= 64");
    p.S = H; p.window = 0; p.nwh = p.nww = 1; p.L = H * W;
    p.row0 = row0;
  }
  with_head_dim(hd, [&](auto hdc) {
    constexpr int D = decltype(hdc)::value;
    constexpr int NWQ = 4;
    const unsigned items = B * p.nwh * p.nww;
    if (window == 14)
      hipLaunchKernelGGL((rel_attention_q8_win_kernel<D, 14, 7, true>), dim3(items, heads, 2), dim3(64 * 7), 0, stream, p);
    else if (window > 0 && p.L <= 13 * 16)
      hipLaunchKernelGGL((rel_attention_q8_kernel<D, true, 13, 256, 16, true>), dim3(items, heads, 1), dim3(64 * 13), 0,
                         stream, p);
    else if (window > 0)
      hipLaunchKernelGGL((rel_attention_q8_kernel<D, true, 16, 256, 16, true>), dim3(items, heads, 1), dim3(64 * 16), 0,
                         stream, p);
    else if (H != 64)
      hipLaunchKernelGGL((rel_attention_q8_kernel<D, false, NWQ, 64, 64, true>),
                         dim3(B, heads, (p.L + 16 * NWQ - 1) / (16 * NWQ)), dim3(64 * NWQ), 0, stream, p);
    else
      hipLaunchKernelGGL((rel_attention_q8_row64_kernel<D, NWQ, false, true>), dim3(B, heads, rows), dim3(64 * NWQ), 0,
                         stream, p);
  });
  SAMQ_LAUNCH_CHECK("rel_attention_q8_zp launch");
  return SAMQ_OK;
}

extern "C" int samq_rel_attention_q8(const int8_t* qkv, const float* qkv_bias, const float* rel_pos_h,
                                     const float* rel_pos_w, int8_t* out, int B, int H, int W, int heads, int hd,
                                     int window, float sm_scale, float s_qkv, float s_a1, float s_a2, float s_out,
                                     hipStream_t stream) {
  return samq_rel_attention_q8_rows(qkv, qkv_bias, rel_pos_h, rel_pos_w, out, B, H, W, heads, hd, window, sm_scale,
                                    s_qkv, s_a1, s_a2, s_out, 0, -1, nullptr, stream);
}
