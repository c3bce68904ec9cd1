// Int8-activation GEMMs on gfx950 int8 MFMA (v_mfma_i32_32x32x32_i8):
//   W8A8: int8 per-output-channel symmetric weights x int8 per-tensor activations -- the fq_vit
//         QLinear / QConv2d compute (fq_vit/models/ptq/layers.py:160-200, 11-74) whose inputs are
//         the int8 codes of the preceding QAct (layers.py:203-242, quantizer/uniform.py:23-45);
//   W4A8: GPTQ int4 weights (gptq_triton/quant_linear.py:66-116 buffers) x int8 activations --
//         the composition "QuantLinear + fq_vit QAct on its input" (SURVEY.md §8c Oracle W4A8).
//
// C[m,n] = epilogue( float(sum_k a[m,k] * w[k,n]) * (a_scale * w_scale[n]) + bias[n] ), with the
// integer sum EXACT in int32 (the reference sums the dequantised fp32 products; both agree up to
// fp32 rounding of the final value).  W4: w = q - zp, either converted to int8 in registers
//   (bytes(q) | 0x80 minus zp per byte never borrows: q in [0,15], zp in [1,16]; ^0x80 -> int8)
// or, in the ping-pong kernel's row-sum form (cfg 86), as sum a * q - zp * sum a.
//
// Quantising epilogues (int8 output codes, fq_vit fake quant with a TRUE division and
// round-half-to-even, clamp [-128, 127]):
//   Q8      out = q(y, out_scale)                                  (Linear -> QAct)
//   Q8_GELU out = q(GELU(y), out_scale)                            (lin1 -> GELU -> mlp.qact1)
//   Q8_RES  out = q(R * res_scale + fq(y, mid_scale), out_scale)   (proj -> qact3 -> +x -> qact2)
//           (mid_scale <= 0: no intermediate quantiser); R int8 codes, may alias C.
//
// Activations with zero points (samq_i8_gemm_zp, samq_w8a8_conv_gemm_zp; W8, the three quantising
// epilogues): the ring kernels instantiated on I8EpiZp (gemm_i8_epilogue.h) -- an int32 col_offset[n]
// = -zp_a * sum_k W[n, k] joins the sum before the scaling, the quantisers and the residual carry
// their zero points.  The symmetric instantiations are untouched.
//
// Power-of-Two Factor activations (samq_i8_gemm_ptf, samq_w8a8_conv_gemm_ptf): the same kernels on
// I8EpiPtf -- per-column exponents of the output quantiser and of the residual, and an input with
// per-k exponents by masked-pass replay (gemm_i8_ring.h).  The I8EpiZp instantiations are untouched.
//
// The kernels: gemm_i8_ring.h (2- / 3-slot LDS ring, every weight format), gemm_i8_pp.h (W4
// ping-pong), gemm_i8_epilogue.h (their shared epilogue).  Here: the W8 repack, the launchers, the
// tile-config table and the C entry points.
#include "gemm_i8_pp.h"
#include "gemm_i8_ring.h"

namespace samq {

// ------------------------------------------------------------------ W8 repack
// packed byte (((nt * (K/128) + kb) * 4 + s) * 64 + lane) * 16 + j  =  W[n][k] with
// n = nt*32 + (lane&31), k = kb*128 + 32*s + 16*(lane>>5) + j   (W row-major [N][K], i.e. the
// nn.Linear / flattened Conv2d weight layout).
__global__ void w8_repack_kernel(const int8_t* __restrict__ w, int8_t* __restrict__ out, int K, int N) {
  const int64_t units = (int64_t)K * N / 16;
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    const int lane = u & 63;
    const int s = (u >> 6) & 3;
    const int64_t blk = u >> 8;
    const int kbs = K / 128;
    const int kb = (int)(blk % kbs), nt = (int)(blk / kbs);
    const int n = nt * 32 + (lane & 31);
    const int k = kb * 128 + 32 * s + 16 * (lane >> 5);
    *(u32x4*)(out + u * 16) = *(const u32x4*)(w + (int64_t)n * K + k);
  }
}

// ------------------------------------------------------------------ launchers
struct I8Args {
  const int8_t* A; int64_t lda; const char* Wp; const float* wscale; const uint32_t* qzeros;
  const float* bias; void* C; int64_t ldc; int M, N, K; I8Epi ep; I8Gather ga;
  // the _zp entries only (launch_i8<..., ZP = true>): the I8EpiZp fields beyond ep
  const int* col_offset = nullptr; float mid_zp = 0.f, res_zp = 0.f, out_zp = 0.f; const int8_t* pad16 = nullptr;
  // the _ptf entries only (launch_i8_ptf): the I8EpiPtf fields beyond those
  const uint8_t* out_exp = nullptr; const uint8_t* res_exp = nullptr; int k_tiles_a = 0; int k_shift[3] = {0, 0, 0};
};

template <int BM, int BN, int WMW, int WNW, int EPI, int BF, int ST, int AG = AG_ROWS, bool GRP = false, bool ZP = false>
static int launch_i8(const I8Args& a, hipStream_t st) {
  const int nwg = ((a.M + BM - 1) / BM) * (a.N / BN);
  if constexpr (ZP) {
    I8EpiZp ez;
    static_cast<I8Epi&>(ez) = a.ep;
    ez.col_offset = a.col_offset;
    ez.mid_zp = a.mid_zp;
    ez.res_zp = a.res_zp;
    ez.out_zp = a.out_zp;
    ez.pad16 = a.pad16;
    hipLaunchKernelGGL((i8_gemm_kernel<BM, BN, WMW, WNW, EPI, BF, ST, AG, GRP, I8EpiZp>), dim3(nwg),
                       dim3(64 * WMW * WNW), 0, st, a.A, a.lda, a.Wp, a.wscale, a.qzeros, a.bias, a.C, a.ldc, a.M, a.N,
                       a.K, ez, a.ga);
  } else {
    hipLaunchKernelGGL((i8_gemm_kernel<BM, BN, WMW, WNW, EPI, BF, ST, AG, GRP>), dim3(nwg), dim3(64 * WMW * WNW), 0, st,
                       a.A, a.lda, a.Wp, a.wscale, a.qzeros, a.bias, a.C, a.ldc, a.M, a.N, a.K, a.ep, a.ga);
  }
  SAMQ_LAUNCH_CHECK("i8_gemm launch");
  return SAMQ_OK;
}

// W8 on Power-of-Two Factor activations (samq_i8_gemm_ptf / samq_w8a8_conv_gemm_ptf): the ring kernel on I8EpiPtf
template <int BM, int BN, int WMW, int WNW, int EPI, int ST, int AG = AG_ROWS>
static int launch_i8_ptf(const I8Args& a, hipStream_t st) {
  const int nwg = ((a.M + BM - 1) / BM) * (a.N / BN);
  I8EpiPtf ez;
  static_cast<I8Epi&>(ez) = a.ep;
  ez.col_offset = a.col_offset;
  ez.mid_zp = a.mid_zp;
  ez.res_zp = a.res_zp;
  ez.out_zp = a.out_zp;
  ez.pad16 = a.pad16;
  ez.out_exp = a.out_exp;
  ez.res_exp = a.res_exp;
  ez.k_tiles_a = a.k_tiles_a;
  for (int p = 0; p < 3; ++p) ez.k_shift[p] = a.k_shift[p];
  hipLaunchKernelGGL((i8_gemm_kernel<BM, BN, WMW, WNW, EPI, BF_W8, ST, AG, false, I8EpiPtf>), dim3(nwg),
                     dim3(64 * WMW * WNW), 0, st, a.A, a.lda, a.Wp, a.wscale, a.qzeros, a.bias, a.C, a.ldc, a.M, a.N,
                     a.K, ez, a.ga);
  SAMQ_LAUNCH_CHECK("i8_gemm_ptf launch");
  return SAMQ_OK;
}

template <int EPI, int FLAGS>
static int launch_i8_pp2(const I8Args& a, hipStream_t st) {
  if constexpr ((FLAGS & I8PP_ROW_SUMS) != 0)   // row sums on the 24-bit multiply (i8_epilogue_slice ZPS)
    SAMQ_REQUIRE(a.K < 65536, SAMQ_ERR_UNSUPPORTED, "w4a8_gemm: the row-sum zero-point path needs K < 65536");
  const int nwg = ((a.M + 255) / 256) * (a.N / 256);
  hipLaunchKernelGGL((i8_gemm_pp2<EPI, FLAGS>), dim3(nwg), dim3(512), 0, st, a.A, a.lda, a.Wp, a.wscale, a.qzeros,
                     a.bias, a.C, a.ldc, a.M, a.N, a.K, a.ep);
  SAMQ_LAUNCH_CHECK("i8_gemm_pp2 launch");
  return SAMQ_OK;
}

// ---- tile descriptions.  A row of the config table (with_i8_cfg) is one of these types: BN is the
// tile width N must divide by, launch<EPI, BF> starts it on per-channel weights of format BF and
// launch_grouped<EPI> on grouped W4 weights.

// 3-slot-ring kernel: BM x BN tile of WMW x WNW waves on ST4 ring slots for W4 weights and ST8 for
// W8.  GROUPED_: grouped W4 weights may run on it (f32 group accumulators beside the int32 ones:
// wave tiles of at most 64x64, so that the pair of accumulator sets fits the registers)
template <int BM, int BN_, int WMW, int WNW, int ST4, int ST8 = ST4, bool GROUPED_ = false>
struct I8Ring {
  static constexpr int BN = BN_;
  static constexpr bool GROUPED = GROUPED_;
  template <int EPI, int BF>
  static int launch(const I8Args& a, hipStream_t st) {
    return launch_i8<BM, BN, WMW, WNW, EPI, BF, BF == BF_W4 ? ST4 : ST8>(a, st);
  }
  template <int EPI>
  static int launch_grouped(const I8Args& a, hipStream_t st) {
    return launch_i8<BM, BN, WMW, WNW, EPI, BF_W4, ST4, AG_ROWS, true>(a, st);
  }
  template <int EPI>
  static int launch_zp(const I8Args& a, hipStream_t st) {   // W8, activations with zero points
    return launch_i8<BM, BN, WMW, WNW, EPI, BF_W8, ST8, AG_ROWS, false, true>(a, st);
  }
  // W8, Power-of-Two Factor activations: instantiated for the tiles the automatic pick can return for
  // W8 weights (cfg 89 / 84: 64x64, 90 / 88: 64x128, 82: 128x256, 83: 128x128 on three slots)
  static constexpr bool PTF = (BM == 64 && BN == 64) || (BM == 64 && BN == 128) ||
                              (BM == 128 && BN == 256 && WMW == 2 && WNW == 4) ||
                              (BM == 128 && BN == 128 && WMW == 2 && WNW == 2 && ST8 == 3);
  template <int EPI>
  static int launch_ptf(const I8Args& a, hipStream_t st) {
    if constexpr (PTF) return launch_i8_ptf<BM, BN, WMW, WNW, EPI, ST8>(a, st);
    else return fail(SAMQ_ERR_UNSUPPORTED, "i8_gemm_ptf: this tile config is not built for PTF activations "
                                           "(cfg 0, 82, 83, 84, 88, 89, 90 are)");
  }
};
template <int BM, int BN, int WMW, int WNW, int ST>
using I8RingG = I8Ring<BM, BN, WMW, WNW, ST, ST, true>;

// W4 ping-pong kernel (256x256) under tile config id ID.  The row-sum product form
// (FLAGS == I8PP_ROW_SUMS) takes the row sums of A from their producer where the caller has them
template <int ID, int FLAGS>
struct I8Pp {
  static constexpr int BN = 256;
  static constexpr bool GROUPED = false;
  template <int EPI, int BF>
  static int launch(const I8Args& a, hipStream_t st) {
    if constexpr (BF != BF_W4)
      return fail(SAMQ_ERR_INVALID, "i8_gemm: cfg " + std::to_string(ID) + " is the W4 ping-pong kernel");
    else if (FLAGS == I8PP_ROW_SUMS && a.ep.rs_in) return launch_i8_pp2<EPI, I8PP_ROW_SUMS | I8PP_RS_IN>(a, st);
    else return launch_i8_pp2<EPI, FLAGS>(a, st);
  }
  template <int EPI>
  static int launch_zp(const I8Args&, hipStream_t) {
    return fail(SAMQ_ERR_INVALID, "i8_gemm_zp: cfg " + std::to_string(ID) + " is the W4 ping-pong kernel");
  }
  template <int EPI>
  static int launch_ptf(const I8Args&, hipStream_t) {
    return fail(SAMQ_ERR_INVALID, "i8_gemm_ptf: cfg " + std::to_string(ID) + " is the W4 ping-pong kernel");
  }
};

struct I8NoTile {   // an id the table does not have
  static constexpr int BN = 0;
  static constexpr bool GROUPED = false;
  template <int EPI, int BF>
  static int launch(const I8Args&, hipStream_t) { return fail(SAMQ_ERR_INVALID, "i8_gemm: unknown tile config"); }
  template <int EPI>
  static int launch_zp(const I8Args&, hipStream_t) { return fail(SAMQ_ERR_INVALID, "i8_gemm_zp: unknown tile config"); }
  template <int EPI>
  static int launch_ptf(const I8Args&, hipStream_t) { return fail(SAMQ_ERR_INVALID, "i8_gemm_ptf: unknown tile config"); }
};

// ---- the config table: f(row) for the row of tile config id cfg (f(I8NoTile) for any other id).
// A new config is one new case here.
template <class F>
static int with_i8_cfg(int cfg, F&& f) {
  switch (cfg) {
    case 81: return f(I8Ring<256, 256, 2, 4, 3, 2>{});   // W4: 3 ring slots, W8: 2
    case 82: return f(I8Ring<128, 256, 2, 4, 3>{});
    case 83: return f(I8RingG<128, 128, 2, 2, 3>{});
    case 84: return f(I8RingG<64, 64, 2, 2, 3>{});
    case 85: return f(I8Pp<85, 0>{});               // zero point per weight in the unpack
    case 86: return f(I8Pp<86, I8PP_ROW_SUMS>{});   // zero point through the row sums of A
    case 87: return f(I8RingG<128, 64, 2, 2, 3>{});
    case 88: return f(I8RingG<64, 128, 2, 2, 3>{});
    case 89: return f(I8Ring<64, 64, 2, 2, 2>{});
    case 90: return f(I8Ring<64, 128, 2, 2, 2>{});
    case 91: return f(I8Ring<32, 64, 1, 2, 2>{});
    case 92: return f(I8Ring<64, 32, 2, 1, 2>{});
    // bigger tiles on a 2-slot ring for the L2-bound vit_b B = 1 shapes (each 64x64 tile re-reads
    // its A and B panels from L2: 128x128 halves those bytes per output)
    case 180: return f(I8Ring<128, 128, 2, 2, 2>{});   // 64 KiB: two workgroups per CU
    case 181: return f(I8Ring<128, 64, 2, 2, 2>{});    // 48 KiB
    case 182: return f(I8Ring<128, 128, 2, 4, 2>{});   // 8 waves of 64x32
#ifdef SAMQ_TUNING
    // tuning build only (make tuning): TIMING-ONLY variants of cfg 86 that compute wrong results or
    // write nothing -- never reachable through the product library
    case 94: return f(I8Pp<94, I8PP_ROW_SUMS | I8PP_T_NO_EPILOGUE>{});
    case 96: return f(I8Pp<96, I8PP_ROW_SUMS | I8PP_T_NO_MFMA>{});
    case 97: return f(I8Pp<97, I8PP_ROW_SUMS | I8PP_T_NO_RESTAGE>{});
#endif
    default: return f(I8NoTile{});
  }
}

static int i8_cfg_bn(int cfg) { return with_i8_cfg(cfg, [](auto row) { return decltype(row)::BN; }); }

template <int EPI, int BF>
static int launch_i8_cfg(const I8Args& a, int cfg, hipStream_t st) {
  return with_i8_cfg(cfg, [&](auto row) { return decltype(row)::template launch<EPI, BF>(a, st); });
}

// W8 on activations with zero points (samq_i8_gemm_zp)
template <int EPI>
static int launch_i8_cfg_zp(const I8Args& a, int cfg, hipStream_t st) {
  return with_i8_cfg(cfg, [&](auto row) { return decltype(row)::template launch_zp<EPI>(a, st); });
}

// W8 on Power-of-Two Factor activations (samq_i8_gemm_ptf)
template <int EPI>
static int launch_i8_cfg_ptf(const I8Args& a, int cfg, hipStream_t st) {
  return with_i8_cfg(cfg, [&](auto row) { return decltype(row)::template launch_ptf<EPI>(a, st); });
}

// grouped W4 (ep.kpg K tiles per group)
template <int EPI>
static int launch_i8_grouped(const I8Args& a, int cfg, hipStream_t st) {
  return with_i8_cfg(cfg, [&](auto row) {
    if constexpr (decltype(row)::GROUPED) return decltype(row)::template launch_grouped<EPI>(a, st);
    else return fail(SAMQ_ERR_INVALID, "w4a8_gemm: grouped weights take tile configs 83 / 84 / 87 / 88");
  });
}

// The automatic pick, each rule with its measurement on MI355X (all pairs bit-identical):
//  - W4 from two images up (M >= 8192), N % 256 == 0: the ping-pong kernel (86).  In the 2-lane
//    W4A8 graph (interleaved A/B, tools/bench_cfg_ab_w4a8.py) 37.64 ms per step vs 38.33 on the
//    3-slot 256x256 tiles (81) and 38.34 on its plain-unpack form (85).  256x256 tiles as such: in steady state (tools/bench_i8.py
//    --m 65536: no tile-round tail) the fastest per CU on every ViT-H shape (lin2 1717 TOPS vs 1602
//    on 128x128, proj 857 vs 833), and with proj / lin2 on them the graph step went 40.06 ->
//    38.29 ms (profiles/r2_cfg_ab_w4a8.log) although 128x128 wins an isolated M = 16384 launch
//    (profiles/r1_v11_i8_scan.log): the graph's other lane fills the tile-round tail.
//    Other N % 128 == 0 there: 128x128 (83).
//  - W8 below two rounds of 128x256 tiles (fq_vit vit_b at B = 1, M = 4096): small tiles on a
//    2-slot ring (32 KiB LDS, five workgroups per CU instead of three) fill the chip.  64x64 (89)
//    vs 128x256: 77 vs 88-90 us per block (tools/bench_i8.py --w8-vitb,
//    profiles/r1_v17_w8_scan.log); 2 slots vs 3: 1.8325 vs 1.8610 ms per image in the W8A8 graph
//    (tools/bench_cfg_ab_w8a8.py, profiles/r3_w8_cfg_ab.log).  The wide outputs (qkv N = 2304,
//    lin1 N = 3072) on 64x128 (90): 1.7067 vs 1.7568 ms per image; proj / lin2 (N = 768) stay on
//    64x64 (all four on 64x128: 1.7335; profiles/r5_w8_cfg_ab_64x128.log).
//  - otherwise the 3-slot ring on the largest tile that N divides by and M fills.
static int i8_pick_cfg(int M, int N, int bfmt) {
  if (bfmt == BF_W4 && M >= 8192) {
    if (N % 256 == 0) return 86;
    if (N % 128 == 0) return 83;
  }
  const int64_t t256 = (int64_t)((M + 127) / 128) * (N / 256);
  if (bfmt == BF_W8 && t256 < 512 && N % 128 == 0 && N > 1024) return 90;
  if (bfmt == BF_W8 && t256 < 512 && N % 64 == 0) return 89;
  if (N % 256 == 0 && t256 >= 512) return 82;
  if (N % 128 == 0 && M >= 256) return 83;
  return 84;
}

static int i8_dispatch_grouped(const I8Args& a, int epi, int cfg, hipStream_t st) {
  switch (epi) {
    case SAMQ_EPI_BIAS: return launch_i8_grouped<SAMQ_EPI_BIAS>(a, cfg, st);
    case SAMQ_EPI_BIAS_GELU: return launch_i8_grouped<SAMQ_EPI_BIAS_GELU>(a, cfg, st);
    case SAMQ_EPI_RESADD_F32: return launch_i8_grouped<SAMQ_EPI_RESADD_F32>(a, cfg, st);
    case SAMQ_EPI_F32: return launch_i8_grouped<SAMQ_EPI_F32>(a, cfg, st);
    case SAMQ_EPI_Q8: return launch_i8_grouped<SAMQ_EPI_Q8>(a, cfg, st);
    case SAMQ_EPI_Q8_GELU: return launch_i8_grouped<SAMQ_EPI_Q8_GELU>(a, cfg, st);
    default: return fail(SAMQ_ERR_INVALID, "w4a8_gemm: unknown epilogue for grouped weights");
  }
}

static int i8_dispatch(const I8Args& a, int bfmt, int epi, int cfg, hipStream_t st) {
#define I8_EPI(E) \
  case E: return bfmt == BF_W8 ? launch_i8_cfg<E, BF_W8>(a, cfg, st) : launch_i8_cfg<E, BF_W4>(a, cfg, st)
  switch (epi) {
    I8_EPI(SAMQ_EPI_BIAS);
    I8_EPI(SAMQ_EPI_BIAS_GELU);
    I8_EPI(SAMQ_EPI_RESADD_F32);
    I8_EPI(SAMQ_EPI_F32);
    I8_EPI(SAMQ_EPI_Q8);
    I8_EPI(SAMQ_EPI_Q8_GELU);
    I8_EPI(SAMQ_EPI_Q8_RES);
    default: return fail(SAMQ_ERR_INVALID, "i8_gemm: unknown epilogue");
  }
#undef I8_EPI
}

}  // namespace samq

using namespace samq;

extern "C" int samq_w8_repack(const int8_t* w, int8_t* packed, int K, int N, hipStream_t stream) {
  SAMQ_REQUIRE(w && packed, SAMQ_ERR_INVALID, "w8_repack: null pointer");
  SAMQ_REQUIRE(K > 0 && K % 128 == 0, SAMQ_ERR_INVALID, "w8_repack: K must be a positive multiple of 128");
  SAMQ_REQUIRE(N > 0 && N % 32 == 0, SAMQ_ERR_INVALID, "w8_repack: N must be a multiple of 32");
  SAMQ_REQUIRE(((uintptr_t)w & 15) == 0 && ((uintptr_t)packed & 15) == 0, SAMQ_ERR_INVALID,
               "w8_repack: pointers must be 16-byte aligned");
  const int64_t units = (int64_t)K * N / 16;
  const int blocks = (int)((units + 255) / 256 < 8192 ? (units + 255) / 256 : 8192);
  hipLaunchKernelGGL(w8_repack_kernel, dim3(blocks), dim3(256), 0, stream, w, packed, K, N);
  SAMQ_LAUNCH_CHECK("w8_repack launch");
  return SAMQ_OK;
}

extern "C" int samq_i8_gemm_cfg(const int8_t* A, int64_t lda, int bfmt, const void* wpacked, const float* wscale,
                                const int32_t* qzeros, const float* bias, void* C, int64_t ldc, const int8_t* R,
                                int64_t ldr, int M, int N, int K, int epilogue, float a_scale, float mid_scale,
                                float res_scale, float out_scale, int cfg, hipStream_t stream) {
  if (M == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(A && wpacked && wscale && C, SAMQ_ERR_INVALID, "i8_gemm: null pointer");
  SAMQ_REQUIRE(bfmt == BF_W8 || bfmt == BF_W4, SAMQ_ERR_INVALID, "i8_gemm: unknown weight format");
  SAMQ_REQUIRE(bfmt == BF_W8 || qzeros, SAMQ_ERR_INVALID, "i8_gemm: W4 needs qzeros");
  SAMQ_REQUIRE(M >= 0 && N > 0 && K > 0 && K % 128 == 0, SAMQ_ERR_INVALID, "i8_gemm: K must be a multiple of 128");
  SAMQ_REQUIRE(N % 64 == 0, SAMQ_ERR_INVALID, "i8_gemm: N must be a multiple of 64");
  SAMQ_REQUIRE(lda >= K && lda % 16 == 0 && ((uintptr_t)A & 15) == 0, SAMQ_ERR_INVALID,
               "i8_gemm: A must be 16-byte aligned with lda >= K, lda % 16 == 0");
  SAMQ_REQUIRE(ldc >= N && ((uintptr_t)C & 15) == 0, SAMQ_ERR_INVALID, "i8_gemm: C must be 16-byte aligned, ldc >= N");
  const bool q8 = epilogue == SAMQ_EPI_Q8 || epilogue == SAMQ_EPI_Q8_GELU || epilogue == SAMQ_EPI_Q8_RES;
  const bool f32 = epilogue == SAMQ_EPI_RESADD_F32 || epilogue == SAMQ_EPI_F32;
  SAMQ_REQUIRE(ldc % (q8 ? 16 : (f32 ? 4 : 8)) == 0, SAMQ_ERR_INVALID, "i8_gemm: ldc breaks 16-byte row alignment");
  SAMQ_REQUIRE(!q8 || out_scale > 0.f, SAMQ_ERR_INVALID, "i8_gemm: quantising epilogue needs out_scale > 0");
  SAMQ_REQUIRE(epilogue != SAMQ_EPI_Q8_RES || (R && ldr % 16 == 0 && ((uintptr_t)R & 15) == 0), SAMQ_ERR_INVALID,
               "i8_gemm: Q8_RES needs a 16-byte aligned residual R with ldr % 16 == 0");
  if (cfg <= 0) cfg = i8_pick_cfg(M, N, bfmt);
  SAMQ_REQUIRE(i8_cfg_bn(cfg) > 0, SAMQ_ERR_INVALID, "i8_gemm: unknown tile config");
  SAMQ_REQUIRE(N % i8_cfg_bn(cfg) == 0, SAMQ_ERR_INVALID, "i8_gemm: N not divisible by tile");
  I8Args a{A, lda, (const char*)wpacked, wscale, (const uint32_t*)qzeros, bias, C, ldc, M, N, K,
           I8Epi{a_scale, mid_scale, res_scale, out_scale, R, ldr, 0}, I8Gather{0, 0, 0}};
  return i8_dispatch(a, bfmt, epilogue, cfg, stream);
}

extern "C" int samq_w8a8_conv_gemm(const int8_t* x, int mode, int B, int Cin, int side, const int8_t* wpacked,
                                   const float* wscale, const float* bias, void* C, const int8_t* R, int rmod,
                                   int N, int epilogue, float a_scale, float mid_scale, float res_scale,
                                   float out_scale, hipStream_t stream) {
  if (B == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(x && wpacked && wscale && C, SAMQ_ERR_INVALID, "w8a8_conv_gemm: null pointer");
  SAMQ_REQUIRE(mode == AG_PATCH || mode == AG_3X3, SAMQ_ERR_INVALID, "w8a8_conv_gemm: mode must be 1 (patch) or 2 (3x3)");
  SAMQ_REQUIRE(epilogue == SAMQ_EPI_Q8 || epilogue == SAMQ_EPI_Q8_RES, SAMQ_ERR_UNSUPPORTED,
               "w8a8_conv_gemm: epilogue must be Q8 or Q8_RES");
  SAMQ_REQUIRE(B > 0 && Cin > 0 && side > 0 && N > 0 && N % 64 == 0, SAMQ_ERR_INVALID, "w8a8_conv_gemm: bad shape");
  SAMQ_REQUIRE(out_scale > 0.f, SAMQ_ERR_INVALID, "w8a8_conv_gemm: needs out_scale > 0");
  SAMQ_REQUIRE(epilogue != SAMQ_EPI_Q8_RES || (R && ((uintptr_t)R & 15) == 0), SAMQ_ERR_INVALID,
               "w8a8_conv_gemm: Q8_RES needs a 16-byte aligned residual");
  SAMQ_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)C & 15) == 0, SAMQ_ERR_INVALID,
               "w8a8_conv_gemm: operands must be 16-byte aligned");
  int G, K;
  if (mode == AG_PATCH) {
    SAMQ_REQUIRE(side % 16 == 0 && (Cin * 256) % 128 == 0, SAMQ_ERR_UNSUPPORTED,
                 "w8a8_conv_gemm: patch mode is the 16x16 / stride 16 PatchEmbed");
    G = side / 16;
    K = Cin * 256;
  } else {
    SAMQ_REQUIRE(Cin % 128 == 0, SAMQ_ERR_UNSUPPORTED, "w8a8_conv_gemm: 3x3 mode needs Cin % 128 == 0");
    G = side;
    K = 9 * Cin;
  }
  const int M = B * G * G;
  I8Args a{x, K, (const char*)wpacked, wscale, nullptr, bias, C, N, M, N, K,
           I8Epi{a_scale, mid_scale, res_scale, out_scale, R, N, rmod}, I8Gather{side, G, Cin}};
  if (epilogue == SAMQ_EPI_Q8)
    return mode == AG_PATCH ? launch_i8<64, 64, 2, 2, SAMQ_EPI_Q8, BF_W8, 3, AG_PATCH>(a, stream)
                            : launch_i8<64, 64, 2, 2, SAMQ_EPI_Q8, BF_W8, 3, AG_3X3>(a, stream);
  return mode == AG_PATCH ? launch_i8<64, 64, 2, 2, SAMQ_EPI_Q8_RES, BF_W8, 3, AG_PATCH>(a, stream)
                          : launch_i8<64, 64, 2, 2, SAMQ_EPI_Q8_RES, BF_W8, 3, AG_3X3>(a, stream);
}

// The zero-point arguments shared by samq_i8_gemm_zp and samq_w8a8_conv_gemm_zp
static int i8_zp_args(I8Args& a, const int32_t* col_offset, int mid_zp, int res_zp, int out_zp, const char* who) {
  auto ok = [](int z) { return z >= -128 && z <= 127; };
  SAMQ_REQUIRE(ok(mid_zp) && ok(res_zp) && ok(out_zp), SAMQ_ERR_INVALID,
               std::string(who) + ": zero points must be in [-128, 127]");
  SAMQ_REQUIRE(((uintptr_t)col_offset & 3) == 0, SAMQ_ERR_INVALID, std::string(who) + ": col_offset must be 4-byte aligned");
  a.col_offset = col_offset;
  a.mid_zp = (float)mid_zp;
  a.res_zp = (float)res_zp;
  a.out_zp = (float)out_zp;
  return SAMQ_OK;
}

extern "C" int samq_i8_gemm_zp(const int8_t* A, int64_t lda, const int8_t* wpacked, const float* wscale,
                               const float* bias, void* C, int64_t ldc, const int8_t* R, int64_t ldr, int M, int N,
                               int K, int epilogue, float a_scale, float mid_scale, float res_scale, float out_scale,
                               int cfg, const int32_t* col_offset, int mid_zp, int res_zp, int out_zp, int rmod,
                               hipStream_t stream) {
  if (M == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(epilogue == SAMQ_EPI_Q8 || epilogue == SAMQ_EPI_Q8_GELU || epilogue == SAMQ_EPI_Q8_RES,
               SAMQ_ERR_UNSUPPORTED, "i8_gemm_zp: epilogue must be Q8, Q8_GELU or Q8_RES");
  SAMQ_REQUIRE(A && wpacked && wscale && C, SAMQ_ERR_INVALID, "i8_gemm_zp: null pointer");
  SAMQ_REQUIRE(M >= 0 && N > 0 && K > 0 && K % 128 == 0, SAMQ_ERR_INVALID, "i8_gemm_zp: K must be a multiple of 128");
  SAMQ_REQUIRE(N % 64 == 0, SAMQ_ERR_INVALID, "i8_gemm_zp: N must be a multiple of 64");
  SAMQ_REQUIRE(lda >= K && lda % 16 == 0 && ((uintptr_t)A & 15) == 0, SAMQ_ERR_INVALID,
               "i8_gemm_zp: A must be 16-byte aligned with lda >= K, lda % 16 == 0");
  SAMQ_REQUIRE(ldc >= N && ldc % 16 == 0 && ((uintptr_t)C & 15) == 0, SAMQ_ERR_INVALID,
               "i8_gemm_zp: C must be 16-byte aligned rows, ldc >= N");
  SAMQ_REQUIRE(out_scale > 0.f, SAMQ_ERR_INVALID, "i8_gemm_zp: needs out_scale > 0");
  SAMQ_REQUIRE(epilogue != SAMQ_EPI_Q8_RES || (R && ldr >= N && ldr % 16 == 0 && ((uintptr_t)R & 15) == 0),
               SAMQ_ERR_INVALID, "i8_gemm_zp: Q8_RES needs a 16-byte aligned residual R with ldr >= N, ldr % 16 == 0");
  SAMQ_REQUIRE(rmod >= 0, SAMQ_ERR_INVALID, "i8_gemm_zp: rmod must be >= 0");
  if (cfg <= 0) cfg = i8_pick_cfg(M, N, BF_W8);
  SAMQ_REQUIRE(i8_cfg_bn(cfg) > 0, SAMQ_ERR_INVALID, "i8_gemm_zp: unknown tile config");
  SAMQ_REQUIRE(N % i8_cfg_bn(cfg) == 0, SAMQ_ERR_INVALID, "i8_gemm_zp: N not divisible by tile");
  I8Args a{A, lda, (const char*)wpacked, wscale, nullptr, bias, C, ldc, M, N, K,
           I8Epi{a_scale, mid_scale, res_scale, out_scale, R, ldr, rmod}, I8Gather{0, 0, 0}};
  if (const int e = i8_zp_args(a, col_offset, mid_zp, res_zp, out_zp, "i8_gemm_zp")) return e;
  switch (epilogue) {
    case SAMQ_EPI_Q8: return launch_i8_cfg_zp<SAMQ_EPI_Q8>(a, cfg, stream);
    case SAMQ_EPI_Q8_GELU: return launch_i8_cfg_zp<SAMQ_EPI_Q8_GELU>(a, cfg, stream);
    default: return launch_i8_cfg_zp<SAMQ_EPI_Q8_RES>(a, cfg, stream);
  }
}

extern "C" int samq_w8a8_conv_gemm_zp(const int8_t* x, int mode, int B, int Cin, int side, const int8_t* wpacked,
                                      const float* wscale, const float* bias, void* C, const int8_t* R, int rmod,
                                      int N, int epilogue, float a_scale, float mid_scale, float res_scale,
                                      float out_scale, const int32_t* col_offset, int mid_zp, int res_zp, int out_zp,
                                      const int8_t* pad16, hipStream_t stream) {
  if (B == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(x && wpacked && wscale && C, SAMQ_ERR_INVALID, "w8a8_conv_gemm_zp: null pointer");
  SAMQ_REQUIRE(mode == AG_PATCH || mode == AG_3X3, SAMQ_ERR_INVALID,
               "w8a8_conv_gemm_zp: mode must be 1 (patch) or 2 (3x3)");
  SAMQ_REQUIRE(epilogue == SAMQ_EPI_Q8 || epilogue == SAMQ_EPI_Q8_RES, SAMQ_ERR_UNSUPPORTED,
               "w8a8_conv_gemm_zp: epilogue must be Q8 or Q8_RES");
  SAMQ_REQUIRE(B > 0 && Cin > 0 && side > 0 && N > 0 && N % 64 == 0, SAMQ_ERR_INVALID, "w8a8_conv_gemm_zp: bad shape");
  SAMQ_REQUIRE(out_scale > 0.f, SAMQ_ERR_INVALID, "w8a8_conv_gemm_zp: needs out_scale > 0");
  SAMQ_REQUIRE(epilogue != SAMQ_EPI_Q8_RES || (R && ((uintptr_t)R & 15) == 0), SAMQ_ERR_INVALID,
               "w8a8_conv_gemm_zp: Q8_RES needs a 16-byte aligned residual");
  SAMQ_REQUIRE(rmod >= 0, SAMQ_ERR_INVALID, "w8a8_conv_gemm_zp: rmod must be >= 0");
  SAMQ_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)C & 15) == 0, SAMQ_ERR_INVALID,
               "w8a8_conv_gemm_zp: operands must be 16-byte aligned");
  SAMQ_REQUIRE(mode != AG_3X3 || (pad16 && ((uintptr_t)pad16 & 15) == 0), SAMQ_ERR_INVALID,
               "w8a8_conv_gemm_zp: 3x3 mode needs pad16, 16 bytes of the input's zero-point code, 16-byte aligned");
  int G, K;
  if (mode == AG_PATCH) {
    SAMQ_REQUIRE(side % 16 == 0 && (Cin * 256) % 128 == 0, SAMQ_ERR_UNSUPPORTED,
                 "w8a8_conv_gemm_zp: patch mode is the 16x16 / stride 16 PatchEmbed");
    G = side / 16;
    K = Cin * 256;
  } else {
    SAMQ_REQUIRE(Cin % 128 == 0, SAMQ_ERR_UNSUPPORTED, "w8a8_conv_gemm_zp: 3x3 mode needs Cin % 128 == 0");
    G = side;
    K = 9 * Cin;
  }
  const int M = B * G * G;
  I8Args a{x, K, (const char*)wpacked, wscale, nullptr, bias, C, N, M, N, K,
           I8Epi{a_scale, mid_scale, res_scale, out_scale, R, N, rmod}, I8Gather{side, G, Cin}};
  if (const int e = i8_zp_args(a, col_offset, mid_zp, res_zp, out_zp, "w8a8_conv_gemm_zp")) return e;
  a.pad16 = pad16;
  if (epilogue == SAMQ_EPI_Q8)
    return mode == AG_PATCH ? launch_i8<64, 64, 2, 2, SAMQ_EPI_Q8, BF_W8, 3, AG_PATCH, false, true>(a, stream)
                            : launch_i8<64, 64, 2, 2, SAMQ_EPI_Q8, BF_W8, 3, AG_3X3, false, true>(a, stream);
  return mode == AG_PATCH ? launch_i8<64, 64, 2, 2, SAMQ_EPI_Q8_RES, BF_W8, 3, AG_PATCH, false, true>(a, stream)
                          : launch_i8<64, 64, 2, 2, SAMQ_EPI_Q8_RES, BF_W8, 3, AG_3X3, false, true>(a, stream);
}

// samq_i8_gemm_zp on Power-of-Two Factor activations.  K is the kernel's K = P * k_tiles_a * 128 (the
// stacked masked weight copies, P <= 4); A has k_tiles_a * 128 columns.
extern "C" int samq_i8_gemm_ptf(const int8_t* A, int64_t lda, const int8_t* wpacked, const float* wscale,
                                const float* bias, void* C, int64_t ldc, const int8_t* R, int64_t ldr, int M, int N,
                                int K, int epilogue, float a_scale, float mid_scale, float res_scale, float out_scale,
                                int cfg, const int32_t* col_offset, int mid_zp, int res_zp, int out_zp, int rmod,
                                const uint8_t* out_exp, const uint8_t* res_exp, int k_tiles_a, int k_shift0,
                                int k_shift1, int k_shift2, hipStream_t stream) {
  if (M == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(epilogue == SAMQ_EPI_Q8 || epilogue == SAMQ_EPI_Q8_GELU || epilogue == SAMQ_EPI_Q8_RES,
               SAMQ_ERR_UNSUPPORTED, "i8_gemm_ptf: epilogue must be Q8, Q8_GELU or Q8_RES");
  SAMQ_REQUIRE(A && wpacked && wscale && C, SAMQ_ERR_INVALID, "i8_gemm_ptf: null pointer");
  SAMQ_REQUIRE(M >= 0 && N > 0 && K > 0 && K % 128 == 0, SAMQ_ERR_INVALID, "i8_gemm_ptf: K must be a multiple of 128");
  SAMQ_REQUIRE(N % 64 == 0, SAMQ_ERR_INVALID, "i8_gemm_ptf: N must be a multiple of 64");
  SAMQ_REQUIRE(k_tiles_a >= 1 && (K / 128) % k_tiles_a == 0 && K / 128 / k_tiles_a <= 4, SAMQ_ERR_INVALID,
               "i8_gemm_ptf: K must be 1 to 4 passes over k_tiles_a tiles of 128");
  const int passes = K / 128 / k_tiles_a;
  const int64_t ka = (int64_t)k_tiles_a * 128;
  const int shifts[3] = {k_shift0, k_shift1, k_shift2};
  int total = 0;
  for (int p = 0; p < 3; ++p) {
    if (p < passes - 1) {
      SAMQ_REQUIRE(shifts[p] >= 1 && shifts[p] <= 3, SAMQ_ERR_INVALID, "i8_gemm_ptf: k_shift of a pass must be in 1..3");
      total += shifts[p];
    } else {
      SAMQ_REQUIRE(shifts[p] == 0, SAMQ_ERR_INVALID, "i8_gemm_ptf: k_shift beyond the passes must be 0");
    }
  }
  SAMQ_REQUIRE(total <= 3, SAMQ_ERR_INVALID, "i8_gemm_ptf: the input exponents (the k_shift sum) must stay within 0..3");
  SAMQ_REQUIRE(passes == 1 || epilogue == SAMQ_EPI_Q8, SAMQ_ERR_UNSUPPORTED,
               "i8_gemm_ptf: input exponents (more than one pass) with the Q8 epilogue only");
  SAMQ_REQUIRE(passes == 1 || ((int64_t)255 * 128 << total) * ka < ((int64_t)1 << 31), SAMQ_ERR_UNSUPPORTED,
               "i8_gemm_ptf: 255 * 128 * 2^max_exp * K_A must stay below 2^31");
  SAMQ_REQUIRE(lda >= ka && lda % 16 == 0 && ((uintptr_t)A & 15) == 0, SAMQ_ERR_INVALID,
               "i8_gemm_ptf: A must be 16-byte aligned with lda >= k_tiles_a * 128, lda % 16 == 0");
  SAMQ_REQUIRE(ldc >= N && ldc % 16 == 0 && ((uintptr_t)C & 15) == 0, SAMQ_ERR_INVALID,
               "i8_gemm_ptf: C must be 16-byte aligned rows, ldc >= N");
  SAMQ_REQUIRE(out_scale > 0.f, SAMQ_ERR_INVALID, "i8_gemm_ptf: needs out_scale > 0");
  SAMQ_REQUIRE(epilogue != SAMQ_EPI_Q8_RES || (R && ldr >= N && ldr % 16 == 0 && ((uintptr_t)R & 15) == 0),
               SAMQ_ERR_INVALID, "i8_gemm_ptf: Q8_RES needs a 16-byte aligned residual R with ldr >= N, ldr % 16 == 0");
  SAMQ_REQUIRE(rmod >= 0, SAMQ_ERR_INVALID, "i8_gemm_ptf: rmod must be >= 0");
  SAMQ_REQUIRE(((uintptr_t)out_exp & 15) == 0 && ((uintptr_t)res_exp & 15) == 0, SAMQ_ERR_INVALID,
               "i8_gemm_ptf: out_exp / res_exp must be 16-byte aligned");
  SAMQ_REQUIRE(!res_exp || epilogue == SAMQ_EPI_Q8_RES, SAMQ_ERR_INVALID, "i8_gemm_ptf: res_exp needs the Q8_RES epilogue");
  if (cfg <= 0) cfg = i8_pick_cfg(M, N, BF_W8);
  SAMQ_REQUIRE(i8_cfg_bn(cfg) > 0, SAMQ_ERR_INVALID, "i8_gemm_ptf: unknown tile config");
  SAMQ_REQUIRE(N % i8_cfg_bn(cfg) == 0, SAMQ_ERR_INVALID, "i8_gemm_ptf: N not divisible by tile");
  I8Args a{A, lda, (const char*)wpacked, wscale, nullptr, bias, C, ldc, M, N, K,
           I8Epi{a_scale, mid_scale, res_scale, out_scale, R, ldr, rmod}, I8Gather{0, 0, 0}};
  if (const int e = i8_zp_args(a, col_offset, mid_zp, res_zp, out_zp, "i8_gemm_ptf")) return e;
  a.out_exp = out_exp;
  a.res_exp = res_exp;
  a.k_tiles_a = k_tiles_a;
  for (int p = 0; p < 3; ++p) a.k_shift[p] = shifts[p];
  switch (epilogue) {
    case SAMQ_EPI_Q8: return launch_i8_cfg_ptf<SAMQ_EPI_Q8>(a, cfg, stream);
    case SAMQ_EPI_Q8_GELU: return launch_i8_cfg_ptf<SAMQ_EPI_Q8_GELU>(a, cfg, stream);
    default: return launch_i8_cfg_ptf<SAMQ_EPI_Q8_RES>(a, cfg, stream);
  }
}

// samq_w8a8_conv_gemm_zp with the output quantiser's exponents (out_exp, uint8 [N], null = 0)
extern "C" int samq_w8a8_conv_gemm_ptf(const int8_t* x, int mode, int B, int Cin, int side, const int8_t* wpacked,
                                       const float* wscale, const float* bias, void* C, const int8_t* R, int rmod,
                                       int N, int epilogue, float a_scale, float mid_scale, float res_scale,
                                       float out_scale, const int32_t* col_offset, int mid_zp, int res_zp, int out_zp,
                                       const int8_t* pad16, const uint8_t* out_exp, hipStream_t stream) {
  if (B == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(x && wpacked && wscale && C, SAMQ_ERR_INVALID, "w8a8_conv_gemm_ptf: null pointer");
  SAMQ_REQUIRE(mode == AG_PATCH || mode == AG_3X3, SAMQ_ERR_INVALID,
               "w8a8_conv_gemm_ptf: mode must be 1 (patch) or 2 (3x3)");
  SAMQ_REQUIRE(epilogue == SAMQ_EPI_Q8 || epilogue == SAMQ_EPI_Q8_RES, SAMQ_ERR_UNSUPPORTED,
               "w8a8_conv_gemm_ptf: epilogue must be Q8 or Q8_RES");
  SAMQ_REQUIRE(B > 0 && Cin > 0 && side > 0 && N > 0 && N % 64 == 0, SAMQ_ERR_INVALID, "w8a8_conv_gemm_ptf: bad shape");
  SAMQ_REQUIRE(out_scale > 0.f, SAMQ_ERR_INVALID, "w8a8_conv_gemm_ptf: needs out_scale > 0");
  SAMQ_REQUIRE(epilogue != SAMQ_EPI_Q8_RES || (R && ((uintptr_t)R & 15) == 0), SAMQ_ERR_INVALID,
               "w8a8_conv_gemm_ptf: Q8_RES needs a 16-byte aligned residual");
  SAMQ_REQUIRE(rmod >= 0, SAMQ_ERR_INVALID, "w8a8_conv_gemm_ptf: rmod must be >= 0");
  SAMQ_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)C & 15) == 0 && ((uintptr_t)out_exp & 15) == 0, SAMQ_ERR_INVALID,
               "w8a8_conv_gemm_ptf: operands and out_exp must be 16-byte aligned");
  SAMQ_REQUIRE(mode != AG_3X3 || (pad16 && ((uintptr_t)pad16 & 15) == 0), SAMQ_ERR_INVALID,
               "w8a8_conv_gemm_ptf: 3x3 mode needs pad16, 16 bytes of the input's zero-point code, 16-byte aligned");
  int G, K;
  if (mode == AG_PATCH) {
    SAMQ_REQUIRE(side % 16 == 0 && (Cin * 256) % 128 == 0, SAMQ_ERR_UNSUPPORTED,
                 "w8a8_conv_gemm_ptf: patch mode is the 16x16 / stride 16 PatchEmbed");
    G = side / 16;
    K = Cin * 256;
  } else {
    SAMQ_REQUIRE(Cin % 128 == 0, SAMQ_ERR_UNSUPPORTED, "w8a8_conv_gemm_ptf: 3x3 mode needs Cin % 128 == 0");
    G = side;
    K = 9 * Cin;
  }
  const int M = B * G * G;
  I8Args a{x, K, (const char*)wpacked, wscale, nullptr, bias, C, N, M, N, K,
           I8Epi{a_scale, mid_scale, res_scale, out_scale, R, N, rmod}, I8Gather{side, G, Cin}};
  if (const int e = i8_zp_args(a, col_offset, mid_zp, res_zp, out_zp, "w8a8_conv_gemm_ptf")) return e;
  a.pad16 = pad16;
  a.out_exp = out_exp;
  a.k_tiles_a = K / 128;
  if (epilogue == SAMQ_EPI_Q8)
    return mode == AG_PATCH ? launch_i8_ptf<64, 64, 2, 2, SAMQ_EPI_Q8, 3, AG_PATCH>(a, stream)
                            : launch_i8_ptf<64, 64, 2, 2, SAMQ_EPI_Q8, 3, AG_3X3>(a, stream);
  return mode == AG_PATCH ? launch_i8_ptf<64, 64, 2, 2, SAMQ_EPI_Q8_RES, 3, AG_PATCH>(a, stream)
                          : launch_i8_ptf<64, 64, 2, 2, SAMQ_EPI_Q8_RES, 3, AG_3X3>(a, stream);
}

extern "C" int samq_w8a8_gemm(const int8_t* A, int64_t lda, const int8_t* wpacked, const float* wscale,
                              const float* bias, void* C, int64_t ldc, const int8_t* R, int64_t ldr, int M, int N,
                              int K, int epilogue, float a_scale, float mid_scale, float res_scale, float out_scale,
                              hipStream_t stream) {
  return samq_i8_gemm_cfg(A, lda, BF_W8, wpacked, wscale, nullptr, bias, C, ldc, R, ldr, M, N, K, epilogue, a_scale,
                          mid_scale, res_scale, out_scale, 0, stream);
}

extern "C" int samq_w4a8_gemm_cfg(const int8_t* A, int64_t lda, const int32_t* wpacked, const float* wscale,
                                  const int32_t* qzeros, const float* bias, void* C, int64_t ldc, int M, int N,
                                  int K, int groupsize, int epilogue, float a_scale, float out_scale, int cfg,
                                  hipStream_t stream) {
  SAMQ_REQUIRE(epilogue != SAMQ_EPI_Q8_RES, SAMQ_ERR_INVALID, "w4a8_gemm: Q8_RES is a W8A8 epilogue");
  if (groupsize == -1 || groupsize == K)
    return samq_i8_gemm_cfg(A, lda, BF_W4, wpacked, wscale, qzeros, bias, C, ldc, nullptr, 0, M, N, K, epilogue,
                            a_scale, 0.f, 0.f, out_scale, cfg, stream);
  // grouped weights (gptq_triton/quant_linear.py:324-335: per-group scale / zero rows)
  if (M == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(A && wpacked && wscale && qzeros && C, SAMQ_ERR_INVALID, "w4a8_gemm: null pointer");
  SAMQ_REQUIRE(M >= 0 && N > 0 && K > 0 && K % 128 == 0 && N % 64 == 0, SAMQ_ERR_INVALID,
               "w4a8_gemm: K % 128 == 0 and N % 64 == 0 required");
  SAMQ_REQUIRE(groupsize > 0 && groupsize % 128 == 0, SAMQ_ERR_UNSUPPORTED,
               "w4a8_gemm: grouped weights need a groupsize that is a multiple of 128 (the int8 K tile)");
  SAMQ_REQUIRE(lda >= K && lda % 16 == 0 && ((uintptr_t)A & 15) == 0, SAMQ_ERR_INVALID,
               "w4a8_gemm: A must be 16-byte aligned with lda >= K, lda % 16 == 0");
  const bool q8 = epilogue == SAMQ_EPI_Q8 || epilogue == SAMQ_EPI_Q8_GELU;
  const bool f32 = epilogue == SAMQ_EPI_RESADD_F32 || epilogue == SAMQ_EPI_F32;
  SAMQ_REQUIRE(ldc >= N && ((uintptr_t)C & 15) == 0 && ldc % (q8 ? 16 : (f32 ? 4 : 8)) == 0, SAMQ_ERR_INVALID,
               "w4a8_gemm: C must be 16-byte aligned rows, ldc >= N");
  SAMQ_REQUIRE(!q8 || out_scale > 0.f, SAMQ_ERR_INVALID, "w4a8_gemm: quantising epilogue needs out_scale > 0");
  if (cfg <= 0) cfg = N % 128 == 0 && M >= 1024 ? 83 : 84;
  SAMQ_REQUIRE(i8_cfg_bn(cfg) > 0, SAMQ_ERR_INVALID, "w4a8_gemm: unknown tile config");
  SAMQ_REQUIRE(N % i8_cfg_bn(cfg) == 0, SAMQ_ERR_INVALID, "w4a8_gemm: N not divisible by tile");
  I8Args a{A, lda, (const char*)wpacked, wscale, (const uint32_t*)qzeros, bias, C, ldc, M, N, K,
           I8Epi{a_scale, 0.f, 0.f, out_scale, nullptr, 0, 0, groupsize / 128}, I8Gather{0, 0, 0}};
  return i8_dispatch_grouped(a, epilogue, cfg, stream);
}

extern "C" int samq_w8a8_gemm_v16(const int8_t* A, int64_t lda, const int8_t* wpacked, const float* wscale,
                                  const float* bias, int8_t* C, int64_t ldc, int M, int N, int K, float a_scale,
                                  float out_scale, void* v16, int v_col0, int64_t ldv, int cfg, hipStream_t stream) {
  if (M == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(A && wpacked && wscale && C && v16, SAMQ_ERR_INVALID, "w8a8_gemm_v16: null pointer");
  SAMQ_REQUIRE(M > 0 && N > 0 && K > 0 && K % 128 == 0 && N % 64 == 0, SAMQ_ERR_INVALID,
               "w8a8_gemm_v16: K % 128 == 0 and N % 64 == 0 required");
  SAMQ_REQUIRE(lda >= K && lda % 16 == 0 && ((uintptr_t)A & 15) == 0 && ldc >= N && ldc % 16 == 0 &&
               ((uintptr_t)C & 15) == 0, SAMQ_ERR_INVALID, "w8a8_gemm_v16: 16-byte aligned rows required");
  SAMQ_REQUIRE(out_scale > 0.f, SAMQ_ERR_INVALID, "w8a8_gemm_v16: needs out_scale > 0");
  if (cfg <= 0) cfg = i8_pick_cfg(M, N, BF_W8);
  SAMQ_REQUIRE(i8_cfg_bn(cfg) > 0, SAMQ_ERR_INVALID, "w8a8_gemm_v16: unknown tile config");
  SAMQ_REQUIRE(N % i8_cfg_bn(cfg) == 0, SAMQ_ERR_INVALID, "w8a8_gemm_v16: N not divisible by tile");
  SAMQ_REQUIRE(v_col0 >= 0 && v_col0 < N && v_col0 % 64 == 0 && ldv >= N - v_col0 && ldv % 8 == 0 &&
               ((uintptr_t)v16 & 15) == 0, SAMQ_ERR_INVALID,
               "w8a8_gemm_v16: v_col0 must be a multiple of 64 inside N; v16 rows 16-byte aligned, ldv >= N - v_col0");
  I8Args a{A, lda, (const char*)wpacked, wscale, nullptr, bias, C, ldc, M, N, K,
           I8Epi{a_scale, 0.f, 0.f, out_scale, nullptr, 0, 0, 0, nullptr, nullptr, (_Float16*)v16, v_col0, ldv},
           I8Gather{0, 0, 0}};
  return launch_i8_cfg<SAMQ_EPI_Q8, BF_W8>(a, cfg, stream);
}

extern "C" int samq_w4a8_gemm_rs(const int8_t* A, int64_t lda, const int32_t* wpacked, const float* wscale,
                                 const int32_t* qzeros, const float* bias, void* C, int64_t ldc, int M, int N, int K,
                                 int epilogue, float a_scale, float out_scale, const int32_t* rowsum_in,
                                 int32_t* rowsum_out, int cfg, hipStream_t stream) {
  if (M == 0) return SAMQ_OK;   // empty batch: no work, data pointers may be null
  SAMQ_REQUIRE(epilogue != SAMQ_EPI_Q8_RES, SAMQ_ERR_INVALID, "w4a8_gemm_rs: Q8_RES is a W8A8 epilogue");
  SAMQ_REQUIRE(!rowsum_out || epilogue == SAMQ_EPI_Q8 || epilogue == SAMQ_EPI_Q8_GELU, SAMQ_ERR_INVALID,
               "w4a8_gemm_rs: rowsum_out needs an int8-code epilogue (Q8 / Q8_GELU)");
  SAMQ_REQUIRE(M < (1 << 30) && (!rowsum_in || K < 65536), SAMQ_ERR_UNSUPPORTED,
               "w4a8_gemm_rs: row sums need K < 65536");
  SAMQ_REQUIRE(A && wpacked && wscale && qzeros && C, SAMQ_ERR_INVALID, "w4a8_gemm_rs: null pointer");
  SAMQ_REQUIRE(lda >= K && lda % 16 == 0 && ((uintptr_t)A & 15) == 0, SAMQ_ERR_INVALID,
               "w4a8_gemm_rs: A must be 16-byte aligned with lda >= K, lda % 16 == 0");
  SAMQ_REQUIRE(M > 0 && N > 0 && K > 0 && K % 128 == 0 && N % 64 == 0, SAMQ_ERR_INVALID,
               "w4a8_gemm_rs: K % 128 == 0 and N % 64 == 0 required");
  const bool q8 = epilogue == SAMQ_EPI_Q8 || epilogue == SAMQ_EPI_Q8_GELU;
  const bool f32 = epilogue == SAMQ_EPI_RESADD_F32 || epilogue == SAMQ_EPI_F32;
  SAMQ_REQUIRE(ldc >= N && ((uintptr_t)C & 15) == 0 && ldc % (q8 ? 16 : (f32 ? 4 : 8)) == 0, SAMQ_ERR_INVALID,
               "w4a8_gemm_rs: C must be 16-byte aligned rows, ldc >= N");
  SAMQ_REQUIRE(!q8 || out_scale > 0.f, SAMQ_ERR_INVALID, "w4a8_gemm_rs: quantising epilogue needs out_scale > 0");
  if (cfg <= 0) cfg = i8_pick_cfg(M, N, BF_W4);
  SAMQ_REQUIRE(i8_cfg_bn(cfg) > 0, SAMQ_ERR_INVALID, "w4a8_gemm_rs: unknown tile config");
  SAMQ_REQUIRE(N % i8_cfg_bn(cfg) == 0, SAMQ_ERR_INVALID, "w4a8_gemm_rs: N not divisible by tile");
  I8Args a{A, lda, (const char*)wpacked, wscale, (const uint32_t*)qzeros, bias, C, ldc, M, N, K,
           I8Epi{a_scale, 0.f, 0.f, out_scale, nullptr, 0, 0, 0, rowsum_in, rowsum_out}, I8Gather{0, 0, 0}};
  return i8_dispatch(a, BF_W4, epilogue, cfg, stream);
}

extern "C" int samq_w4a8_gemm(const int8_t* A, int64_t lda, const int32_t* wpacked, const float* wscale,
                              const int32_t* qzeros, const float* bias, void* C, int64_t ldc, int M, int N, int K,
                              int groupsize, int epilogue, float a_scale, float out_scale, hipStream_t stream) {
  return samq_w4a8_gemm_cfg(A, lda, wpacked, wscale, qzeros, bias, C, ldc, M, N, K, groupsize, epilogue, a_scale,
                            out_scale, 0, stream);
}
