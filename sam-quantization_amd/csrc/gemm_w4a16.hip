// W4A16 GEMM for GPTQ-packed int4 weights on gfx950 fp16 MFMA.
//
// Replaces the reference's Triton `matmul4_kernel` + `triton_matmul4`
// (gptq_triton/quant_linear.py:231-352, 355-437):  C[M,N] = A[M,K] . W[K,N] (+bias, ...)
// with W[k,n] = s[g,n] * (q[k,n] - zp[g,n]),  q = (qweight[k/8,n] >> 4(k%8)) & 15,
// zp = ((qzeros[g,n/8] >> 4(n%8)) & 15) + 1.
//
// Numerics (deliberately NOT the reference's fp16 dequant `fp16(q*s) - fp16(zp*s)`, which
// is the dominant error of the reference path): the MFMA multiplies
// fp16 activations by the EXACT small integers (q - zp) in [-16, 15], accumulates in fp32,
// and applies the per-channel scale in the fp32 epilogue (groupsize == K).  With groups
// (groupsize < K) the integer is scaled once, in fp16, per group: fp16((q - zp) * s).
//
// Design (MI355X-first, not a translation of the Triton tiling):
//  * weights are repacked once at load (samq_w4_repack) into MFMA-fragment order: one
//    dwordx4 per lane holds the 4 k16-steps of its B column for a 64-deep K tile, with the
//    nibbles interleaved so that ((w >> 4i) & 0x000F000F) | 0x64006400 is directly the fp16
//    pair (1024+q[2i], 1024+q[2i+1]) -> 7 VALU ops unpack 8 weights, 4 v_pk_add_f16 remove
//    the zero point.  B never touches LDS: each wave streams its own fragments from L2.
//  * A is staged global->LDS with global_load_lds_dwordx4 (no VGPR round trip), double
//    buffered, XOR-swizzled on the SOURCE address (LDS image lane-linear) so the
//    ds_read_b128 fragment reads of v_mfma_f32_32x32x16_f16 are bank-conflict free.
//  * wave tiles are >=128 rows (except small fallback configs) so the in-register unpack of
//    each B word is amortised over >=4 MFMAs (VALU:MFMA issue ~1:3).
//  * fused epilogues: +bias, +bias+GELU(erf), and fp32 residual accumulate (x += y) so the
//    residual stream never takes an extra HBM round trip.
//  * XCD-aware bijective blockIdx remap: consecutive tiles (same A rows) share an L2.
//
// This file holds the repack kernel, the tile-config table, the launchers and the C ABI; the GEMM
// kernels live in gemm_w4a16_ring.h (v1, v3) and gemm_w4a16_pp.h (ping-pong), their shared
// helpers in gemm_w4a16_util.h.
#include "common.h"
#include "gemm_w4a16_pp.h"
#include "gemm_w4a16_ring.h"

// packed-weight layout produced by samq_w4_repack (and expected by samq_w4a16_gemm)
#ifndef SAMQ_W4_LAYOUT
#define SAMQ_W4_LAYOUT 1
#endif

namespace samq {

// ------------------------------------------------------------------ repack
// packed word index ((nt * (K/64) + kb) * 64 + lane) * 4 + s   holds column n = nt*32 + (lane&31),
// k = kb*64 + 16*s + 8*(lane>>5) + {0..7}, nibble order [k0,k2,k4,k6 | k1,k3,k5,k7].
// LAYOUT 3 (int8 MFMA fragments of v_mfma_i32_32x32x32_i8, used by the W4A8 GEMM in gemm_i8.hip):
// 2-KiB blocks (nt, kb) over 128-deep K tiles, two 1-KiB pieces p; word w of lane l in piece p
// holds column nt*32 + (l&31), k = kb*128 + 32*(2p + (w>>1)) + 16*(l>>5) + 8*(w&1) + {0..7} with
// nibble order [k0,k4,k1,k5,k2,k6,k3,k7], so (w & 0x0F0F0F0F) are the bytes k0..k3 and
// ((w >> 4) & 0x0F0F0F0F) the bytes k4..k7.
template <int LAYOUT>
__global__ void w4_repack_kernel(const uint32_t* __restrict__ qweight, uint32_t* __restrict__ out,
                                 int K, int N) {
  const int64_t total = (int64_t)K * N / 8;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int s = idx & 3;
    const int lane = (idx >> 2) & 63;
    if (LAYOUT == 3) {
      const int p = (idx >> 8) & 1;
      const int64_t blk = idx >> 9;            // nt * (K/128) + kb
      const int kbs = K / 128;
      const int kb = (int)(blk % kbs);
      const int nt = (int)(blk / kbs);
      const int n = nt * 32 + (lane & 31);
      const int k0 = kb * 128 + 32 * (2 * p + (s >> 1)) + 16 * (lane >> 5) + 8 * (s & 1);
      const uint32_t w = qweight[(int64_t)(k0 >> 3) * N + n];
      uint32_t o = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o |= ((w >> (4 * i)) & 0xFu) << (8 * i);            // q[i]   -> byte i, low nibble
        o |= ((w >> (4 * i + 16)) & 0xFu) << (8 * i + 4);   // q[i+4] -> byte i, high nibble
      }
      out[idx] = o;
      continue;
    }
    const int64_t blk = idx >> 8;             // nt * (K/64) + kb
    const int kbs = K / 64;
    const int kb = (int)(blk % kbs);
    const int nt = (int)(blk / kbs);
    const int n = nt * 32 + (lane & 31);
    const int k0 = kb * 64 + 16 * s + 8 * (lane >> 5);
    const uint32_t w = qweight[(int64_t)(k0 >> 3) * N + n];
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o |= ((w >> (8 * i)) & 0xFu) << (4 * i);             // q[2i]   -> bits 4i
      o |= ((w >> (8 * i + 4)) & 0xFu) << (16 + 4 * i);    // q[2i+1] -> bits 16+4i
    }
    out[idx] = o;
  }
}

// ------------------------------------------------------------------ dispatch
struct GemmArgs {
  const _Float16* A; int64_t lda; const u32x4* Wp; const _Float16* scales; const uint32_t* qzeros;
  const _Float16* bias; void* C; int64_t ldc; int M, N, K, groupsize;
  LnfArgs lnf;
};

// CU count of the CURRENT device, cached per device id (a process may drive several GPUs)
static int cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  if (cached[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

// ---- tile descriptions.  A row of the config table (with_cfg) is one of these types: BN is the tile
// width N must divide by, VEC says the kernel stores 16-byte row vectors (C 16-byte aligned,
// ldc % 8 == 0), LNF that the LayerNorm-fold epilogues may run on it, launch<EPI, GR> starts it.

// v1 (register-staged B): BM x BN tile of WMW x WNW waves, scalar stores -- any C alignment
template <int BM, int BN_, int WMW, int WNW>
struct V1Tile {
  static constexpr int BN = BN_;
  static constexpr bool VEC = false, LNF = false;
  template <int EPI, bool GR>
  static int launch(const GemmArgs& a, hipStream_t st) {
    const int nwg = ((a.M + BM - 1) / BM) * (a.N / BN);
    hipLaunchKernelGGL((w4a16_gemm_kernel<BM, BN, WMW, WNW, EPI, GR>), dim3(nwg), dim3(64 * WMW * WNW), 0, st,
                       a.A, a.lda, a.Wp, a.scales, a.qzeros, a.bias, a.C, a.ldc, a.M, a.N, a.K, a.groupsize);
    SAMQ_LAUNCH_CHECK("w4a16_gemm launch");
    return SAMQ_OK;
  }
};

// v3 (3-stage LDS-DMA ring): BM x BN tile of WMW x WNW waves
template <int BM, int BN_, int WMW, int WNW>
struct V3Tile {
  static constexpr int BN = BN_;
  static constexpr bool VEC = true, LNF = false;
  template <int EPI, bool GR>
  static int launch(const GemmArgs& a, hipStream_t st) {
    const int nwg = ((a.M + BM - 1) / BM) * (a.N / BN);
    hipLaunchKernelGGL((w4a16_gemm_v3<BM, BN, WMW, WNW, EPI, GR>), dim3(nwg), dim3(64 * WMW * WNW), 0, st,
                       a.A, a.lda, a.Wp, a.scales, a.qzeros, a.bias, a.C, a.ldc, a.M, a.N, a.K, a.groupsize);
    SAMQ_LAUNCH_CHECK("w4a16_gemm_v3 launch");
    return SAMQ_OK;
  }
};

// One instantiation of the ping-pong kernel: WMW x (8 / WMW) waves of TM x TN 32x32 tiles each, NPH
// k-phases per K tile, a ring of STAGES slots with lookahead LA, and the PP_* flags
template <int WMW, int TM, int TN, int NPH, int STAGES, int LA, int FLAGS = 0>
struct PpShape {
  static constexpr int BM = WMW * TM * 32, BN = (8 / WMW) * TN * 32;
  template <int MORE>
  using With = PpShape<WMW, TM, TN, NPH, STAGES, LA, FLAGS | MORE>;
  template <int EPI>
  static int launch(const GemmArgs& a, hipStream_t st) {
    constexpr bool F16_OUT = EPI == SAMQ_EPI_BIAS || EPI == SAMQ_EPI_BIAS_GELU;
    if constexpr ((FLAGS & PP_TE_STAGED) != 0 && !F16_OUT) {
      return fail(SAMQ_ERR_UNSUPPORTED, "w4a16_gemm: cfg 104 has f16 epilogues (BIAS / BIAS_GELU) only");
    } else {
      // PP_F16T stages f16 outputs; the f32 epilogues of such a config run the plain shape
      constexpr int VAR = F16_OUT ? FLAGS : FLAGS & ~PP_F16T;
      if (lnf_consumer(EPI)) {
        // the consumer's row partials must fit the LDS the ring frees (a grouped cfg 57 ring leaves
        // room for K <= 1728 only)
        constexpr int kmax = Pp2Lds<WMW, TM, TN, STAGES, EPI, VAR>::LNF_KMAX;
        if (a.K > kmax) return fail(SAMQ_ERR_UNSUPPORTED, "w4a16_gemm_lnf: consumer K exceeds this config's LDS row-partial budget");
      }
      int nwg = ((a.M + BM - 1) / BM) * (a.N / BN);
      if ((VAR & PP_PERSISTENT) != 0 && nwg > cu_count()) {   // <= 1 workgroup per CU, whole XCD rounds
        const int cus = cu_count() & ~7;
        nwg = cus >= 8 ? cus : cu_count();
      }
      hipLaunchKernelGGL((w4a16_gemm_pp2<WMW, TM, TN, NPH, STAGES, LA, EPI, VAR>), dim3(nwg), dim3(512), 0, st,
                         a.A, a.lda, a.Wp, a.scales, a.qzeros, a.bias, a.C, a.ldc, a.M, a.N, a.K, a.groupsize / 64, a.lnf);
      SAMQ_LAUNCH_CHECK("w4a16_gemm_pp2 launch");
      return SAMQ_OK;
    }
  }
};
struct NoGrouped {};   // a ping-pong config without a form for grouped weights

// ping-pong: the shape for per-channel weights (groupsize == K) and the one for grouped weights
template <class PerChannel, class Grouped = NoGrouped, bool LNF_ = false>
struct PpTile {
  static constexpr int BN = PerChannel::BN;
  static constexpr bool VEC = true, LNF = LNF_;
  template <int EPI, bool GR>
  static int launch(const GemmArgs& a, hipStream_t st) {
    using Shape = std::conditional_t<GR, Grouped, PerChannel>;
    if constexpr (std::is_same_v<Shape, NoGrouped>)
      return fail(SAMQ_ERR_INVALID, "w4a16_gemm: grouped weights take ping-pong configs 57 / 64 only");
    else
      return Shape::template launch<EPI>(a, st);
  }
};

struct NoTile {   // an id the table does not have
  static constexpr int BN = 0;
  static constexpr bool VEC = false, LNF = false;
  template <int EPI, bool GR>
  static int launch(const GemmArgs&, hipStream_t) { return fail(SAMQ_ERR_INVALID, "w4a16_gemm: unknown tile config"); }
};

// The product ping-pong shapes.  256x256 tiles, 2x4 waves of 128x64, 2 k-phases; per-channel: 4
// ring slots, lookahead 3.  Grouped with the group row in the ring: 3 slots, lookahead 2 (four
// 40 KiB stages fill the 160 KiB LDS, the group row needs 640 B more); with the group rows in
// registers (PP_GROUP_REGS) the ring is the per-channel one again.
using PpRing43 = PpShape<2, 4, 2, 2, 4, 3>;
using PpRing32 = PpShape<2, 4, 2, 2, 3, 2>;
using Pp57 = PpRing43::With<PP_WAVE_SGPR>;   // -3..-6 % isolated vs the VGPR wave index at M = 8192
using Pp64 = Pp57::With<PP_MFMA16>;          // cfg 57 on 16x16x32 MFMA
using Pp57g = PpRing32::With<PP_GROUPED>;
using Pp64g = Pp57g::With<PP_MFMA16>;        // (slower than 57g on every shape)
using Pp57gr = Pp57::With<PP_GROUPED | PP_GROUP_REGS>;
using Pp64gr = Pp64::With<PP_GROUPED | PP_GROUP_REGS>;

// ---- the config table: f(row) for the row of tile config id cfg (f(NoTile) for any other id).
// A new config is one new case here.
template <class F>
static int with_cfg(int cfg, F&& f) {
  switch (cfg) {
    case 1: return f(V1Tile<256, 256, 2, 4>{});
    case 2: return f(V1Tile<256, 128, 2, 2>{});
    case 3: return f(V1Tile<128, 128, 2, 2>{});
    case 4: return f(V1Tile<64, 64, 2, 2>{});
    case 5: return f(V1Tile<64, 32, 2, 1>{});
    case 6: return f(V1Tile<128, 256, 1, 4>{});
    case 7: return f(V1Tile<256, 256, 1, 8>{});
    case 9: return f(V1Tile<128, 256, 2, 4>{});
    case 21: return f(V3Tile<256, 256, 2, 4>{});
    case 22: return f(V3Tile<128, 256, 2, 4>{});
    case 23: return f(V3Tile<128, 128, 2, 2>{});
    case 24: return f(V3Tile<256, 128, 2, 2>{});
    case 25: return f(V3Tile<128, 256, 1, 4>{});
    case 26: return f(V3Tile<64, 64, 2, 2>{});
    // 320-column tiles: ViT-H N in {1280, 3840, 5120} and M = 128*B give whole waves of tiles
    case 29: return f(V3Tile<128, 320, 2, 5>{});
    case 30: return f(V3Tile<256, 320, 2, 5>{});
    case 31: return f(V3Tile<128, 320, 1, 5>{});
    case 55: return f(PpTile<PpRing32>{});                        // 3 slots, lookahead 2
    case 56: return f(PpTile<PpShape<2, 4, 2, 2, 4, 2>>{});       // 4 slots, lookahead 2 (DMA in both phases)
    case 57: return f(PpTile<Pp57, Pp57g, true>{});
    case 58: return f(PpTile<PpShape<2, 4, 2, 1, 4, 2>>{});       // 1 phase / K tile, 4 slots, lookahead 2
    case 62: return f(PpTile<PpShape<4, 2, 4, 2, 4, 3>>{});       // 4x2 waves (64x128 each): A read 2x, B 4x
    case 64: return f(PpTile<Pp64, Pp64g, true>{});
    case 65: return f(PpTile<PpShape<2, 4, 2, 2, 4, 2, PP_MFMA16>>{});   // cfg 56 on 16x16x32 MFMA
    case 100: return f(PpTile<Pp57::With<PP_DMA_SPREAD>>{});      // cfg 57 / 64, LDS-DMA spread through the MFMA burst
    case 101: return f(PpTile<Pp64::With<PP_DMA_SPREAD>>{});
    case 104: return f(PpTile<Pp57::With<PP_TE_STAGED>>{});       // cfg 57, transposed accumulators, f16 outputs only
    case 107: return f(PpTile<Pp57::With<PP_PERSISTENT>>{});      // cfg 57 / 64 persistent: stores drain under the
    case 108: return f(PpTile<Pp64::With<PP_PERSISTENT>>{});      //   next tile's prologue
    case 109: return f(PpTile<Pp57::With<PP_EARLY_EP>>{});        // cfg 57 / 64, scale / bias loaded before the prologue
    case 110: return f(PpTile<Pp64::With<PP_EARLY_EP>>{});
    case 111: return f(PpTile<Pp57::With<PP_F16T>>{});            // cfg 57, f16 outputs staged transposed
    // grouped weights with the group's scale / zero words prefetched into VGPRs.  Selectable, not the
    // default: measured neutral (155.6 vs 155.3 img/s), and its inline-asm loads leave the compiler
    // free to move the not-yet-filled registers before their counted wait.  Per-channel: 57 / 64
    case 112: return f(PpTile<Pp57, Pp57gr>{});
    case 113: return f(PpTile<Pp64, Pp64gr>{});
    case 114: return f(PpTile<Pp57, Pp57g>{});                    // the grouped cfg 57 under its own id
#ifdef SAMQ_TUNING
    // tuning build only (make tuning): TIMING-ONLY variants of cfg 57 / 64 that compute wrong results
    // on purpose -- never reachable through the product library
    case 70: return f(PpTile<PpRing43::With<PP_T_NO_RESTAGE>>{});
    case 71: return f(PpTile<PpRing43::With<PP_T_NO_MFMA>>{});
    case 72: return f(PpTile<PpRing43::With<PP_T_NO_RESTAGE | PP_T_NO_MFMA>>{});
    case 102: return f(PpTile<Pp57::With<PP_T_NO_EPILOGUE>>{});
    case 103: return f(PpTile<Pp64::With<PP_T_NO_EPILOGUE>>{});
#endif
    default: return f(NoTile{});
  }
}

template <int EPI, bool GR>
static int launch_epi(const GemmArgs& a, int cfg, hipStream_t st) {
  return with_cfg(cfg, [&](auto row) { return decltype(row)::template launch<EPI, GR>(a, st); });
}

// LayerNorm-fold epilogues: the product ping-pong configs only
template <int EPI, bool GR>
static int launch_lnf(const GemmArgs& a, int cfg, hipStream_t st) {
  return with_cfg(cfg, [&](auto row) {
    if constexpr (decltype(row)::LNF) return decltype(row)::template launch<EPI, GR>(a, st);
    else return fail(SAMQ_ERR_UNSUPPORTED, "w4a16_gemm_lnf: the LayerNorm fold needs ping-pong config 57 or 64");
  });
}

// gated-MLP epilogue: the 32x32x16 ping-pong config (57) only
template <bool GR>
static int launch_silu(const GemmArgs& a, hipStream_t st) {
  return PpTile<Pp57, Pp57g>::launch<SAMQ_EPI_SILU_MUL, GR>(a, st);
}

// Measured on MI355X (tools/bench_gemm.py, ViT-H shapes at M = 16384): the 3-stage LDS-DMA
// kernel with 128x256 tiles / 64x64 wave tiles (cfg 22, 2 workgroups per CU) is the fastest or
// within 2 % of it on every projection shape and beats dense fp16 hipBLASLt on 3 of 4.
// The ping-pong v6 (cfg 57: 256x256 tiles, 4-slot ring, lookahead 3) is 5-7 % faster on the wide
// projections (qkv N=3840, lin1 N=5120 at M=16384: 1090 / 970 TF/s vs 1016 / 925); with N=1280 its
// 320 tiles leave a 25 % second round on 256 CUs, where v3's 2-workgroup/CU 128x256 stays ahead.
// 128x320 tiles (cfg 29) make exactly one round on the chip for the N=1280 projections of one
// 2-image lane (M = 8192: isolated proj 38 vs 42 us, lin2 105 vs 124 us against cfg 22,
// profiles/r1_v12_gemm_scan_m8192.log) but are the slowest per CU in steady state; see pick_cfg.
static int pick_cfg(int M, int N, bool grouped) {
  // v6 from two images up: at M = 4096 (one image) lin1 runs 63.5 us on cfg 22 vs 77.9 on v6 and
  // qkv is a tie (profiles/r1_v20_gemm_scan_m4096.log).  The N = 1280 projections (proj, lin2)
  // take v6 on 16x16x32 MFMA (cfg 64): in steady state (M = 65536, no tile-round tail) lin2 runs
  // 1161 TF/s there vs 969 on the one-round 128x320 tiles (cfg 29) that win an isolated M = 8192
  // launch, and inside the 2-lane graph -- where the other lane fills any tail -- the step drops
  // 25.66 -> 24.35 ms with bit-identical output (profiles/r2_cfg_ab.log)
  // grouped weights: the 32x32x16 ping-pong with the group rows in the ring (PP_GROUPED) for every
  // N (its 16x16x32 twin is 6-13 % slower on all four shapes, profiles/r3_gemm_grouped.log)
  if (N % 256 == 0 && M >= 8192) return grouped || N >= 2048 ? 57 : 64;
  if (N % 256 == 0 && M >= 1024) return 22;
  if (N % 128 == 0 && M >= 512) return 23;
  if (N % 64 == 0) return 26;
  return 5;
}

static int cfg_bn(int cfg) { return with_cfg(cfg, [](auto row) { return decltype(row)::BN; }); }
static bool cfg_vec(int cfg) { return with_cfg(cfg, [](auto row) { return (int)decltype(row)::VEC; }) != 0; }

}  // namespace samq

using namespace samq;

extern "C" size_t samq_w4_packed_words(int K, int N) { return (size_t)K * (size_t)N / 8; }

extern "C" int samq_w4_repack_layout(const int32_t* qweight, int32_t* packed, int K, int N, int layout,
                                     hipStream_t stream) {
  SAMQ_REQUIRE(qweight && packed, SAMQ_ERR_INVALID, "w4_repack: null pointer");
  SAMQ_REQUIRE(K > 0 && N > 0 && K % 64 == 0, SAMQ_ERR_INVALID, "w4_repack: K must be a positive multiple of 64");
  SAMQ_REQUIRE(N % 32 == 0, SAMQ_ERR_INVALID, "w4_repack: N must be a multiple of 32");
  SAMQ_REQUIRE(layout == 1 || layout == 3, SAMQ_ERR_INVALID, "w4_repack: layout must be 1 or 3");
  SAMQ_REQUIRE(layout != 3 || K % 128 == 0, SAMQ_ERR_INVALID, "w4_repack: layout 3 needs K % 128 == 0");
  const int64_t total = (int64_t)K * N / 8;
  const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  if (layout == 3)
    hipLaunchKernelGGL(w4_repack_kernel<3>, dim3(blocks), dim3(256), 0, stream, (const uint32_t*)qweight,
                       (uint32_t*)packed, K, N);
  else
    hipLaunchKernelGGL(w4_repack_kernel<1>, dim3(blocks), dim3(256), 0, stream, (const uint32_t*)qweight,
                       (uint32_t*)packed, K, N);
  SAMQ_LAUNCH_CHECK("w4_repack launch");
  return SAMQ_OK;
}

extern "C" int samq_w4_repack(const int32_t* qweight, int32_t* packed, int K, int N, hipStream_t stream) {
  return samq_w4_repack_layout(qweight, packed, K, N, SAMQ_W4_LAYOUT, stream);
}

extern "C" int samq_w4a16_gemm_cfg(const void* A, int64_t lda, const int32_t* wpacked, const void* scales,
                                   const int32_t* qzeros, const void* bias, void* C, int64_t ldc, int M, int N,
                                   int K, int groupsize, int epilogue, int cfg, hipStream_t stream) {
  if (M == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(A && wpacked && scales && qzeros && C, SAMQ_ERR_INVALID, "w4a16_gemm: null pointer");
  SAMQ_REQUIRE(M >= 0 && N > 0 && K > 0, SAMQ_ERR_INVALID, "w4a16_gemm: bad shape");
  SAMQ_REQUIRE(K % 64 == 0, SAMQ_ERR_INVALID, "w4a16_gemm: K must be a multiple of 64");
  SAMQ_REQUIRE(N % 32 == 0, SAMQ_ERR_INVALID, "w4a16_gemm: N must be a multiple of 32");
  SAMQ_REQUIRE(lda >= K && lda % 8 == 0 && ((uintptr_t)A & 15) == 0, SAMQ_ERR_INVALID,
               "w4a16_gemm: A must be 16-byte aligned with lda >= K, lda % 8 == 0");
  SAMQ_REQUIRE(ldc >= N, SAMQ_ERR_INVALID, "w4a16_gemm: ldc < N");
  if (groupsize == -1) groupsize = K;
  SAMQ_REQUIRE(groupsize > 0 && (groupsize == K || groupsize % 64 == 0), SAMQ_ERR_INVALID,
               "w4a16_gemm: groupsize must be -1, K, or a multiple of 64");
  if (M == 0) return SAMQ_OK;
  // the v3 and ping-pong kernels store 16-byte row vectors: C 16-byte aligned, ldc % 8 == 0
  const bool vec_ok = ((uintptr_t)C & 15) == 0 && ldc % 8 == 0;
  if (cfg <= 0) {
    cfg = pick_cfg(M, N, groupsize != -1 && groupsize != K);
    if (!vec_ok && cfg_vec(cfg)) cfg = N % 128 == 0 ? 3 : (N % 64 == 0 ? 4 : 5);
  }
  SAMQ_REQUIRE(cfg_bn(cfg) > 0, SAMQ_ERR_INVALID, "w4a16_gemm: unknown tile config");
  SAMQ_REQUIRE(N % cfg_bn(cfg) == 0, SAMQ_ERR_INVALID, "w4a16_gemm: N not divisible by tile");
  SAMQ_REQUIRE(vec_ok || !cfg_vec(cfg), SAMQ_ERR_INVALID,
               "w4a16_gemm: this tile config needs a 16-byte aligned C with ldc % 8 == 0");
  GemmArgs a{(const _Float16*)A, lda, (const u32x4*)wpacked, (const _Float16*)scales, (const uint32_t*)qzeros,
             (const _Float16*)bias, C, ldc, M, N, K, groupsize};
  const bool gr = groupsize != K;
  switch (epilogue) {
    case SAMQ_EPI_BIAS: return gr ? launch_epi<SAMQ_EPI_BIAS, true>(a, cfg, stream) : launch_epi<SAMQ_EPI_BIAS, false>(a, cfg, stream);
    case SAMQ_EPI_BIAS_GELU: return gr ? launch_epi<SAMQ_EPI_BIAS_GELU, true>(a, cfg, stream) : launch_epi<SAMQ_EPI_BIAS_GELU, false>(a, cfg, stream);
    case SAMQ_EPI_RESADD_F32: return gr ? launch_epi<SAMQ_EPI_RESADD_F32, true>(a, cfg, stream) : launch_epi<SAMQ_EPI_RESADD_F32, false>(a, cfg, stream);
    case SAMQ_EPI_F32: return gr ? launch_epi<SAMQ_EPI_F32, true>(a, cfg, stream) : launch_epi<SAMQ_EPI_F32, false>(a, cfg, stream);
    default: return fail(SAMQ_ERR_INVALID, "w4a16_gemm: unknown epilogue");
  }
}

extern "C" int samq_w4a16_gated_mlp(const void* A, int64_t lda, const int32_t* wpacked, const void* scales,
                                    const int32_t* qzeros, void* C, int64_t ldc, int M, int N2, int K, int groupsize,
                                    hipStream_t stream) {
  if (M == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(A && wpacked && scales && qzeros && C, SAMQ_ERR_INVALID, "w4a16_gated_mlp: null pointer");
  SAMQ_REQUIRE(M >= 0 && N2 > 0 && K > 0 && K % 64 == 0, SAMQ_ERR_INVALID,
               "w4a16_gated_mlp: K must be a positive multiple of 64");
  SAMQ_REQUIRE(N2 % 256 == 0, SAMQ_ERR_INVALID, "w4a16_gated_mlp: 2N must be a multiple of 256");
  SAMQ_REQUIRE(lda >= K && lda % 8 == 0 && ((uintptr_t)A & 15) == 0 && ldc >= N2 / 2 && ldc % 8 == 0 &&
               ((uintptr_t)C & 15) == 0, SAMQ_ERR_INVALID, "w4a16_gated_mlp: 16-byte aligned A / C rows required");
  if (groupsize == -1) groupsize = K;
  SAMQ_REQUIRE(groupsize > 0 && (groupsize == K || groupsize % 64 == 0), SAMQ_ERR_INVALID,
               "w4a16_gated_mlp: groupsize must be -1, K, or a multiple of 64");
  if (M == 0) return SAMQ_OK;
  GemmArgs a{(const _Float16*)A, lda, (const u32x4*)wpacked, (const _Float16*)scales, (const uint32_t*)qzeros,
             nullptr, C, ldc, M, N2, K, groupsize};
  return groupsize != K ? launch_silu<true>(a, stream) : launch_silu<false>(a, stream);
}

extern "C" int samq_w4a16_gemm_lnf(const void* A, int64_t lda, const int32_t* wpacked, const void* scales,
                                   const int32_t* qzeros, const void* bias, void* C, int64_t ldc, int M, int N,
                                   int K, int groupsize, int epilogue, int cfg, const float* gamma, const float* gw,
                                   const float* bw, float* stats, float* mu, void* aout, float eps,
                                   hipStream_t stream) {
  if (M == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(A && wpacked && scales && qzeros && C && stats && mu, SAMQ_ERR_INVALID, "w4a16_gemm_lnf: null pointer");
  SAMQ_REQUIRE(M >= 0 && N > 0 && K > 0 && K % 64 == 0 && N % 256 == 0, SAMQ_ERR_INVALID,
               "w4a16_gemm_lnf: K % 64 == 0 and N % 256 == 0 required");
  SAMQ_REQUIRE(lda >= K && lda % 8 == 0 && ((uintptr_t)A & 15) == 0 && ldc >= N && ldc % 8 == 0 &&
               ((uintptr_t)C & 15) == 0, SAMQ_ERR_INVALID, "w4a16_gemm_lnf: 16-byte aligned A / C rows required");
  if (groupsize == -1) groupsize = K;
  SAMQ_REQUIRE(groupsize > 0 && (groupsize == K || groupsize % 64 == 0), SAMQ_ERR_INVALID,
               "w4a16_gemm_lnf: groupsize must be -1, K, or a multiple of 64");
  const bool gr = groupsize != K;
  if (cfg <= 0) cfg = pick_cfg(M, N, gr);
  LnfArgs L{gamma, gw, bw, stats, mu, (_Float16*)aout, eps, K / 64, nullptr};
  if (epilogue == SAMQ_EPI_RESADD_LNF) {
    SAMQ_REQUIRE(gamma && aout, SAMQ_ERR_INVALID, "w4a16_gemm_lnf: the producer needs gamma and aout");
  } else if (epilogue == SAMQ_EPI_BIAS_LNF || epilogue == SAMQ_EPI_GELU_LNF) {
    SAMQ_REQUIRE(gw && bw, SAMQ_ERR_INVALID, "w4a16_gemm_lnf: the consumer needs gw and bw");
    // the workgroup's row partial sums (256 rows x K/64 pairs) are staged in the LDS the ring
    // leaves free in the epilogue: Pp2Lds::LNF_KMAX per config (PpShape::launch checks it -- K <= 3008
    // for cfg 57, 3968 for cfg 64 per-channel; 1728 / 2688 for grouped weights' 3-slot rings)
  } else {
    return fail(SAMQ_ERR_INVALID, "w4a16_gemm_lnf: epilogue must be RESADD_LNF, BIAS_LNF or GELU_LNF");
  }
  if (M == 0) return SAMQ_OK;
  GemmArgs a{(const _Float16*)A, lda, (const u32x4*)wpacked, (const _Float16*)scales, (const uint32_t*)qzeros,
             (const _Float16*)bias, C, ldc, M, N, K, groupsize, L};
  switch (epilogue) {
    case SAMQ_EPI_RESADD_LNF: return gr ? launch_lnf<SAMQ_EPI_RESADD_LNF, true>(a, cfg, stream)
                                        : launch_lnf<SAMQ_EPI_RESADD_LNF, false>(a, cfg, stream);
    case SAMQ_EPI_BIAS_LNF: return gr ? launch_lnf<SAMQ_EPI_BIAS_LNF, true>(a, cfg, stream)
                                      : launch_lnf<SAMQ_EPI_BIAS_LNF, false>(a, cfg, stream);
    default: return gr ? launch_lnf<SAMQ_EPI_GELU_LNF, true>(a, cfg, stream)
                       : launch_lnf<SAMQ_EPI_GELU_LNF, false>(a, cfg, stream);
  }
}

extern "C" int samq_w4a16_gemm(const void* A, int64_t lda, const int32_t* wpacked, const void* scales,
                               const int32_t* qzeros, const void* bias, void* C, int64_t ldc, int M, int N, int K,
                               int groupsize, int epilogue, hipStream_t stream) {
  return samq_w4a16_gemm_cfg(A, lda, wpacked, scales, qzeros, bias, C, ldc, M, N, K, groupsize, epilogue, 0, stream);
}
