// fpq_gemm.hip - the consumers on the far side of the quantizers and of the KV path:
// FP4 / FP6 / FP8 matrix-core GEMMs on quantizer codes, attention over the cache, the gated residual tail.
// One translation unit of libfpq_hip.so; the quantizers and the code-emitting kernels that feed these consumers are compiled in
// fpq_kernels.hip, fpq_rotate.hip and fpq_adaln.hip.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_gemm_fp4.h"
#include "fpq_gemm_fp8.h"
#include "fpq_gemm_fp6.h"
#include "fpq_attention.h"

// Per-group scales [rows, groups] (fp16 or fp32) -> the fp32 k-major scale image [groups][image_rows] of the FP4 GEMM (include/fpq.h):
// image_rows = rows rounded up to 4 (activation side) or to 64 (weight side; natural row order), padding = 0.
template <typename Ts>
__global__ __launch_bounds__(256) void scales_to_kmajor_kernel(const Ts* __restrict__ scales, float* __restrict__ image, int64_t rows,
                                                               int64_t image_rows, int groups) {
  const int64_t n = (int64_t)groups * image_rows;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t g = i / image_rows, r = i - g * image_rows;
    image[i] = r < rows ? (float)scales[r * groups + g] : 0.0f;
  }
}

// ---- what the GEMM entry points below share (fpq_gemm_launch.h: the epilogue, split-output and q / k norm descriptors, the tile
// choice, the launch) ----------
#include "fpq_gemm_launch.h"

constexpr int kTileDoesNotFit = 1;   // (not an FPQ_* code) the tiling's LDS image is too large at this K: the caller tries the next one

// the FP4 LDS-DMA kernel with 32 MT x 128 tiles and epilogue XE; lds: GemmGldsCfg's figure for that epilogue
template <int MT, typename XE>
int launch_fp4_glds(const GemmCall& c, int w_scale_dtype, size_t lds, XE xe) {
  if (lds > 160 * 1024) return kTileDoesNotFit;
  return with_dtype(w_scale_dtype, [&](auto tw) {
    return gemm_launch(gemm_fp4_glds_kernel<decltype(tw), MT, 4, XE>, GemmGldsCfg<MT, 4>::BM, GemmGldsCfg<MT, 4>::BN, 256, lds, c, xe);
  });
}
// the FP4 deep-ring kernel (64 x 128 tiles, FPQ_GEMM_CFG 40) with epilogue XE; lds: GemmRingCfg's figure for that epilogue
template <typename XE>
int launch_fp4_ring(const GemmCall& c, int w_scale_dtype, size_t lds, XE xe) {
  if (lds > 160 * 1024) return kTileDoesNotFit;
  return with_dtype(w_scale_dtype, [&](auto tw) {
    return gemm_launch(gemm_fp4_ring_kernel<decltype(tw), XE>, GemmRingCfg::BM, GemmRingCfg::BN, 256, lds, c, xe);
  });
}
// THE tiling of an FP4 LDS-DMA call - the Linear (fc1_shift < 0; plain, split or q / k norm) or the fc1 form (fc1_shift = the dual
// quantizer's table shift: its bucket table lies behind the scale tiles) - for the launch and for fpq_gemm_fp4_tiling alike:
// gemm_glds_tiling's choice, then the fall-through where that tiling's LDS image does not fit a CU's 160 KiB at this K (the ring
// to the 64 x 128 tile, that and the 256 x 128 one to 128 x 128).  -> 10 / 20 / 30 / 40, or kTileDoesNotFit when nothing fits.
int gemm_fp4_plan(int64_t tokens, int64_t outs, int G, int fc1_shift) {
  const size_t table = fc1_shift < 0 ? 0 : (size_t)2 << (16 - fc1_shift), cap = 160 * 1024;
  int cfg = gemm_glds_tiling(tokens, outs, true, 2 * (GemmGldsCfg<8, 4>::lds(G) + table) <= cap, true);
  if (cfg == 40 && GemmRingCfg::lds(G) + table > cap) cfg = 30;
  if (cfg == 30 && GemmGldsCfg<2, 4>::lds(G) + table > cap) cfg = 20;
  if (cfg == 10 && GemmGldsCfg<8, 4>::lds(G) + table > cap) cfg = 20;
  if (cfg == 20 && GemmGldsCfg<4, 4>::lds(G) + table > cap) return kTileDoesNotFit;
  return cfg;
}
// the register-staged FP4 kernel
template <int MT, int NT, int WR, int WC>
int launch_fp4_staged(const GemmCall& c, int w_scale_dtype) {
  using Cfg = GemmCfg<MT, NT, WR, WC>;
  return with_dtype(w_scale_dtype, [&](auto tw) {
    return gemm_launch(gemm_fp4_kernel<decltype(tw), MT, NT, WR, WC>, Cfg::BM, Cfg::BN, Cfg::NTHR, Cfg::lds((int)(c.k / 128)), c);
  });
}
// the row-scaled FP6 kernel for one epilogue and one format pair (FA, FB: cbsz of the activations, blgp of the weights; 2 = E2M3,
// 3 = E3M2).  A pair with an E3M2 side is compiled for fp16 activation scales only - what the quantizers of activations produce;
// all four dtype pairs for all four format pairs would double this unit's compile time (60 instantiations instead of 96) - and
// gemm_fp6_rows_impl refuses the other combinations before it gets here.
template <typename Tsa, typename Tsw, int MT, int FA, int FB, typename XE>
int launch_fp6(const GemmCall& c, XE xe) {
  using Cfg = GemmFp6Cfg<MT, 4>;
  if constexpr (__is_same(XE, GemmSqErr)) {   // the squared-error tail: one name for all four pairs, the same scale dtypes per pair
    if constexpr ((FA == 2 && FB == 2) || __is_same(Tsa, _Float16))
      return gemm_launch(gemm_f6_rows_sqerr_kernel<Tsa, Tsw, MT, 4, XE, FA, FB>, Cfg::BM, Cfg::BN, 256, Cfg::lds(), c, xe);
    else
      return FPQ_ERR_DTYPE;
  } else if constexpr (FA == 2 && FB == 2)
    return gemm_launch(gemm_fp6_rows_kernel<Tsa, Tsw, MT, 4, XE>, Cfg::BM, Cfg::BN, 256, Cfg::lds(), c, xe);
  else if constexpr (__is_same(Tsa, _Float16))
    return gemm_launch(gemm_fp6_rows_bf6_kernel<Tsa, Tsw, MT, 4, XE, FA, FB>, Cfg::BM, Cfg::BN, 256, Cfg::lds(), c, xe);
  else
    return FPQ_ERR_DTYPE;
}
// ... from the runtime scale dtypes, operand formats (FPQ_E2M3 / FPQ_E3M2 per side) and epilogue of a call
template <int MT>
int dispatch_fp6(const GemmCall& c, int a_scale_dtype, int w_scale_dtype, int a_table, int w_table, bool split, const GemmQkNorm* qkn,
                 const GemmSqErr* sqx = nullptr) {
  return with_dtype(a_scale_dtype, [&](auto ta) {
    return with_dtype(w_scale_dtype, [&](auto tw) {
      auto formats = [&](auto fa, auto fb) {
        using Ta = decltype(ta);
        using Tw = decltype(tw);
        constexpr int FA = decltype(fa)::value, FB = decltype(fb)::value;
        if (sqx) return launch_fp6<Ta, Tw, MT, FA, FB>(c, *sqx);
        if (qkn) return launch_fp6<Ta, Tw, MT, FA, FB>(c, *qkn);
        if (split) return launch_fp6<Ta, Tw, MT, FA, FB>(c, GemmSplit{});
        return launch_fp6<Ta, Tw, MT, FA, FB>(c, GemmNoFc1{});
      };
      if (a_table == FPQ_E3M2) return w_table == FPQ_E3M2 ? formats(Int<3>{}, Int<3>{}) : formats(Int<3>{}, Int<2>{});
      return w_table == FPQ_E3M2 ? formats(Int<2>{}, Int<3>{}) : formats(Int<2>{}, Int<2>{});
    });
  });
}
template <int MT>
int dispatch_fp8(const GemmCall& c, int a_scale_dtype, int w_scale_dtype) {
  using Cfg = GemmFp8Cfg<MT, 4>;
  return with_dtype(a_scale_dtype, [&](auto ta) {
    return with_dtype(w_scale_dtype, [&](auto tw) {
      return gemm_launch(gemm_fp8_rows_kernel<decltype(ta), decltype(tw), MT, 4>, Cfg::BM, Cfg::BN, 256, Cfg::lds(), c);
    });
  });
}
}  // namespace

extern "C" {

int fpq_attention_blhc(const void* q, const void* k, const void* v, void* out, int64_t batch, int64_t lq, int64_t lkv,
                       int64_t heads, int64_t head_dim, int64_t q_batch_pitch, int64_t q_token_pitch,
                       int64_t kv_batch_pitch, int64_t kv_token_pitch, float scale, fpq_stream_t stream) {
  if (batch < 0 || lq < 0 || lkv < 0 || heads <= 0) return FPQ_ERR_ARG;
  if (head_dim != 64) return FPQ_ERR_SHAPE;
  if (batch == 0 || lq == 0) return FPQ_OK;
  if (lkv == 0 || !(scale > 0.0f)) return FPQ_ERR_ARG;            // softmax over nothing
  if (!q || !k || !v || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) != 0) return FPQ_ERR_ARG;
  if (q_batch_pitch % 8 != 0 || q_token_pitch % 8 != 0 || kv_batch_pitch % 8 != 0 || kv_token_pitch % 8 != 0)
    return FPQ_ERR_SHAPE;
  if (lq > 0x7FFFFFFF || lkv > 0x7FFFFFFF || batch * heads > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  AttnArgs a;
  a.q = (const uint16_t*)q;
  a.k = (const uint16_t*)k;
  a.v = (const uint16_t*)v;
  a.out = (uint16_t*)out;
  a.q_batch = q_batch_pitch;
  a.q_token = q_token_pitch;
  a.kv_batch = kv_batch_pitch;
  a.kv_token = kv_token_pitch;
  a.batch = (int)batch;
  a.heads = (int)heads;
  a.lq = (int)lq;
  a.lkv = (int)lkv;
  a.q_tiles = (int)((lq + 127) / 128);
  a.scale_log2e = scale * 1.4426950408889634f;
  const int64_t groups = (batch * heads + 7) / 8;
  const int64_t n_wg = groups * a.q_tiles * 8;
  if (n_wg > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  hipLaunchKernelGGL(attn_fwd64_kernel<AttnFp16Src>, dim3((unsigned)n_wg), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch();
}

int fpq_attention_blhc_kvcodes(const void* q, const uint8_t* codes, const void* scales, int kv_bit, int64_t max_len, int64_t n_packed,
                               const void* new_k, const void* new_v, int64_t new_batch_pitch, int64_t new_token_pitch, int64_t n_new,
                               void* out, int64_t batch, int64_t lq, int64_t heads, int64_t head_dim, int64_t q_batch_pitch,
                               int64_t q_token_pitch, float scale, fpq_stream_t stream) {
  if (batch < 0 || lq < 0 || heads <= 0 || max_len < 0 || n_packed < 0 || n_new < 0 || head_dim != 64) return FPQ_ERR_ARG;
  if ((kv_bit != 6 && kv_bit != 4) || (kv_bit == 4 && heads % 2 != 0) || n_packed > max_len) return FPQ_ERR_ARG;
  if (batch == 0 || lq == 0) return FPQ_OK;
  const int64_t lkv = n_packed + n_new;
  if (lkv == 0 || !(scale > 0.0f) || !q || !out) return FPQ_ERR_ARG;
  if (n_packed > 0 && (!codes || !scales)) return FPQ_ERR_ARG;
  if (n_new > 0 && (!new_k || !new_v)) return FPQ_ERR_ARG;
  if ((((uintptr_t)q | (uintptr_t)out | (uintptr_t)new_k | (uintptr_t)new_v | (uintptr_t)codes | (uintptr_t)scales) & 15) != 0)
    return FPQ_ERR_ARG;
  if (q_batch_pitch % 8 != 0 || q_token_pitch % 8 != 0 || new_batch_pitch % 8 != 0 || new_token_pitch % 8 != 0 ||
      q_batch_pitch < 0 || q_token_pitch < 0 || new_batch_pitch < 0 || new_token_pitch < 0)
    return FPQ_ERR_ARG;
  if (lq > 0x7FFFFFFF || lkv > 0x7FFFFFFF || batch * heads > 0x7FFFFFFF) return FPQ_ERR_ARG;
  AttnCodesArgs a;
  a.q = (const uint16_t*)q;
  a.k = (const uint16_t*)new_k;
  a.v = (const uint16_t*)new_v;
  a.out = (uint16_t*)out;
  a.q_batch = q_batch_pitch;
  a.q_token = q_token_pitch;
  a.kv_batch = new_batch_pitch;
  a.kv_token = new_token_pitch;
  a.batch = (int)batch;
  a.heads = (int)heads;
  a.lq = (int)lq;
  a.lkv = (int)lkv;
  a.q_tiles = (int)((lq + 127) / 128);
  a.scale_log2e = scale * 1.4426950408889634f;
  a.codes = codes;
  a.scales = (const uint16_t*)scales;
  a.codes_slab = batch * max_len * heads * (kv_bit == 6 ? 48 : 32);
  a.scales_slab = batch * max_len * (kv_bit == 6 ? heads : heads / 2);
  a.max_len = max_len;
  a.n_packed = (int)n_packed;
  const int64_t groups = (batch * heads + 7) / 8;
  const int64_t n_wg = groups * a.q_tiles * 8;
  if (n_wg > 0x7FFFFFFF) return FPQ_ERR_ARG;
  if (kv_bit == 6)
    hipLaunchKernelGGL(attn_fwd64_kernel<AttnCodesSrc<6>>, dim3((unsigned)n_wg), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(attn_fwd64_kernel<AttnCodesSrc<4>>, dim3((unsigned)n_wg), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch();
}

int fpq_gemm_fp4_mx(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales,
                    int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                    fpq_stream_t stream) {
  return fpq_gemm_fp4_mx_ex(a_codes, a_scales, w_codes, w_scales, w_scale_dtype, bias, out, tokens, outs, k, nullptr, stream);
}

int fpq_gemm_fp6_rows(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                      const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs,
                      int64_t k, fpq_stream_t stream) {
  return fpq_gemm_fp6_rows_ex(a_codes, a_scales, a_scale_dtype, w_codes, w_scales, w_scale_dtype, bias, out, tokens, outs, k,
                              nullptr, stream);
}

int fpq_gemm_fp8_rows(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                      const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs,
                      int64_t k, fpq_stream_t stream) {
  return fpq_gemm_fp8_rows_ex(a_codes, a_scales, a_scale_dtype, w_codes, w_scales, w_scale_dtype, bias, out, tokens, outs, k,
                              nullptr, stream);
}

// out = resid + y * gate[row / rows_per_gate, :], fp16 with one rounding per operation (the GEMM epilogues' tail as a
// kernel of its own, for Linears that run elsewhere - e.g. fc2's fp16 GEMM)
__global__ __launch_bounds__(kBlock) void gate_residual_kernel(const u32x4* y, const u32x4* __restrict__ gate,
                                                              const u32x4* resid, u32x4* out, int64_t n_vec, int row_vec,
                                                              int rows_per_gate) {
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n_vec; v += (int64_t)gridDim.x * kBlock) {
    const int64_t row = v / row_vec;
    const int c = (int)(v - row * row_vec);
    u32x4 a = __builtin_nontemporal_load(y + v);
    const u32x4 g = gate[(row / rows_per_gate) * row_vec + c];
    const u32x4 r = resid[v];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const fpq_h2_t p = __builtin_bit_cast(fpq_h2_t, (uint32_t)a[i]) * __builtin_bit_cast(fpq_h2_t, (uint32_t)g[i]);
      a[i] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(fpq_h2_t, (uint32_t)r[i]) + p);
    }
    out[v] = a;
  }
}

int fpq_gate_residual(const void* y, const void* gate, const void* residual, void* out, int64_t rows, int64_t cols,
                      int64_t rows_per_gate, fpq_stream_t stream) {
  if (rows < 0 || cols < 0 || rows_per_gate < 1 || rows_per_gate > 0x7FFFFFFF) return FPQ_ERR_ARG;
  if (cols % 8 != 0 || cols / 8 > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!y || !gate || !residual || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)y | (uintptr_t)gate | (uintptr_t)residual | (uintptr_t)out) & 15) != 0) return FPQ_ERR_ARG;
  const int64_t n_vec = rows * (cols / 8);
  const int64_t wgs = (n_vec + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(gate_residual_kernel, dim3(grid_for(wgs, 1 << 20)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const u32x4*)y, (const u32x4*)gate, (const u32x4*)residual, (u32x4*)out, n_vec, (int)(cols / 8),
                     (int)rows_per_gate);
  return check_launch();
}

// km: both operands are k-major images (include/fpq.h); only the LDS-DMA kernels read them
static int gemm_fp4_mx_impl(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales,
                            int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                            const fpq_gemm_epilogue_t* epilogue, bool km, fpq_stream_t stream, const fpq_gemm_split_t* split = nullptr,
                            const GemmQkNorm* qkn = nullptr, const GemmSqErrCall* sq = nullptr) {
  // sq: the squared-error form (include/fpq.h, fpq_gemm_fp4_sqerr; row-major, no epilogue, no split): `out` is not looked at, the
  // form's own checks follow the family's, the LDS-DMA kernels only (as km / split), then the finish launch
  if (tokens < 0 || outs < 0 || k < 0) return FPQ_ERR_ARG;
  GemmEpi epi;
  if (int rc = gemm_epilogue(epilogue, &epi)) return rc;
  if (split) {   // the LDS-DMA kernels' plain epilogue only
    if (int rc = gemm_split(split, epilogue, tokens, outs, false, &epi)) return rc;
    // (never written through: every tile belongs to a part.)  Part 0 thereby meets the 16-byte test of `out` below, which is
    // stricter than the header's 8 bytes; the FP6 family exempts it.
    if (!out) out = split->out[0];
  }
  if (km) {   // scales come as fp32 k-major images too (include/fpq.h); their lane offsets are 32-bit: 3 planes of rows * 4 bytes
    if (w_scale_dtype != FPQ_F32) return FPQ_ERR_DTYPE;
    if (tokens >= (1ll << 28) || outs >= (1ll << 28)) return FPQ_ERR_SHAPE;
    if ((((uintptr_t)a_scales | (uintptr_t)w_scales) & 15) != 0) return FPQ_ERR_ARG;
    epi.km_w_rows = (int)((outs + 63) / 64 * 64);
  }
  if (w_scale_dtype != FPQ_F16 && w_scale_dtype != FPQ_F32) return FPQ_ERR_DTYPE;
  if (k % 128 != 0 || k > 128 * 64 || outs % 8 != 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  GemmSqErr sqx{};
  if (tokens == 0 || outs == 0) {
    if (!sq) return FPQ_OK;
    if (int rc = gemm_sqerr_args(*sq, true, &sqx)) return rc;
    return gemm_sqerr_finish(*sq, 0, 0, 64, stream);
  }
  if (k == 0 || !a_codes || !a_scales || !w_codes || !w_scales || (!sq && !out)) return FPQ_ERR_ARG;
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (sq ? 0 : (uintptr_t)out)) & 15) != 0) return FPQ_ERR_ARG;
  const int G = (int)(k / 128);
  // The LDS-DMA kernel in the tiling gemm_fp4_plan chooses; the register-staged kernel when no LDS image fits (very long K),
  // when the bias is not 8-byte aligned (the LDS-DMA kernels read it four outputs at a time), or when FPQ_GEMM_CFG names
  // anything but an LDS-DMA tiling (0..2 are the register-staged kernel's own; experiments, tests) - but it reads row-major codes
  // and writes one tensor.
  int cfg = gemm_fp4_plan(tokens, outs, G, -1);
  if (cfg == kTileDoesNotFit) cfg = 0;
  if (cfg == 40 && sq) cfg = 30;   // the ring has no squared-error form: its tile behind the two-stage ring (the same bits)
  if (km || split || sq) {
    if (((uintptr_t)bias & 7) != 0 || outs + 63 > 0x7FFFFFFF) return FPQ_ERR_ARG;
  } else if (((uintptr_t)bias & 7) != 0) {
    cfg = 0;
  } else if (fpq_opt_set(OPT_FPQ_GEMM_CFG)) {
    const int want = fpq_opt(OPT_FPQ_GEMM_CFG, 0);
    if (want != 10 && want != 20 && want != 30 && want != 40) cfg = want;   // (a forced LDS-DMA tiling is in the plan already)
  }
  if (sq)
    if (int rc = gemm_sqerr_args(*sq, false, &sqx)) return rc;
  const GemmCall c{a_codes, a_scales, w_codes, w_scales, bias, out, tokens, outs, k, epi, (hipStream_t)stream};
  auto glds = [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    const size_t lds = GemmGldsCfg<MT, 4>::lds(G);
    if (sq) {
      if (int rc = launch_fp4_glds<MT>(c, w_scale_dtype, lds, sqx)) return rc;   // (kTileDoesNotFit: gemm_fp4_plan has ruled it out)
      return gemm_sqerr_finish(*sq, tokens, outs, GemmGldsCfg<MT, 4>::BM, stream);
    }
    return qkn ? launch_fp4_glds<MT>(c, w_scale_dtype, lds, *qkn) : launch_fp4_glds<MT>(c, w_scale_dtype, lds, GemmNoFc1{});
  };
  if (cfg == 40) return qkn ? launch_fp4_ring(c, w_scale_dtype, GemmRingCfg::lds(G), *qkn) : launch_fp4_ring(c, w_scale_dtype, GemmRingCfg::lds(G), GemmNoFc1{});
  if (cfg == 30) return glds(Int<2>{});   // 64 x 128 tiles
  if (cfg == 10) return glds(Int<8>{});
  if (cfg == 20) return glds(Int<4>{});
  if (km || split || sq) return FPQ_ERR_SHAPE;   // K too long for the LDS-DMA kernel's scale tiles
  if (cfg == 1) return launch_fp4_staged<2, 4, 4, 2>(c, w_scale_dtype);
  if (cfg == 2) return launch_fp4_staged<4, 4, 2, 4>(c, w_scale_dtype);
  return launch_fp4_staged<4, 4, 2, 2>(c, w_scale_dtype);
}

int fpq_gemm_fp4_mx_ex(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales,
                       int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                       const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  return gemm_fp4_mx_impl(a_codes, a_scales, w_codes, w_scales, w_scale_dtype, bias, out, tokens, outs, k, epilogue, false, stream);
}
int fpq_gemm_fp4_mx_split(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales, int w_scale_dtype,
                          const void* bias, int64_t tokens, int64_t outs, int64_t k, const fpq_gemm_split_t* split, int kmajor,
                          fpq_stream_t stream) {
  if (!split) return FPQ_ERR_ARG;
  return gemm_fp4_mx_impl(a_codes, a_scales, w_codes, w_scales, w_scale_dtype, bias, nullptr, tokens, outs, k, nullptr, kmajor != 0, stream, split);
}
int fpq_gemm_fp4_mx_split_qknorm(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales,
                                 int w_scale_dtype, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                 const fpq_gemm_split_t* split, const float* q_head_scale, int kmajor, fpq_stream_t stream) {
  GemmQkNorm qkn;
  if (int rc = gemm_qknorm(split, bias, q_head_scale, &qkn)) return rc;
  return gemm_fp4_mx_impl(a_codes, a_scales, w_codes, w_scales, w_scale_dtype, nullptr, nullptr, tokens, outs, k, nullptr, kmajor != 0, stream,
                          split, &qkn);
}
int64_t fpq_gemm_sqerr_workspace_bytes(int64_t tokens, int64_t outs) {
  if (tokens < 0 || outs < 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF) return FPQ_ERR_ARG;
  return gemm_sqerr_workspace_bytes(tokens, outs);
}
int fpq_gemm_fp4_sqerr(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales, int w_scale_dtype,
                       const void* bias, const void* ref, int ref_dtype, const float* row_weight, float* loss_out, void* workspace,
                       int64_t tokens, int64_t outs, int64_t k, fpq_stream_t stream) {
  const GemmSqErrCall sq{ref, ref_dtype, row_weight, loss_out, workspace};
  return gemm_fp4_mx_impl(a_codes, a_scales, w_codes, w_scales, w_scale_dtype, bias, nullptr, tokens, outs, k, nullptr, false, stream,
                          nullptr, nullptr, &sq);
}
int fpq_gemm_fp4_mx_km(const uint8_t* a_image, const void* a_scales, const uint8_t* w_image, const void* w_scales,
                       int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                       const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  return gemm_fp4_mx_impl(a_image, a_scales, w_image, w_scales, w_scale_dtype, bias, out, tokens, outs, k, epilogue, true, stream);
}

#ifdef FPQ_GEMM6_STAMPS
// diagnostic builds only: where the FP6 GEMM's wavefronts put their per-phase stamp sums ([wavefronts][8] uint64, zeroed by the caller)
int fpq_debug_gemm6_stamp_buffer(void* device_buffer) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_gemm6_stamps), &device_buffer, sizeof(void*)) == hipSuccess ? FPQ_OK : FPQ_ERR_LAUNCH;
}
#endif

// fc1 with GELU and fc2's dual-format input quantizer in the GEMM's epilogue (fpq_gemm_fp4.h, GemmFc1)
static int gemm_fp4_gelu_dual_impl(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales,
                                   int w_scale_dtype, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                                   int64_t k, void* nan_flag, bool km, fpq_stream_t stream) {
  if (tokens < 0 || outs < 0 || k < 0) return FPQ_ERR_ARG;
  if (w_scale_dtype != FPQ_F16 && w_scale_dtype != FPQ_F32) return FPQ_ERR_DTYPE;
  // outs % 128: an output tile is one quantization group wide
  if (k % 128 != 0 || k > 128 * 64 || outs % 128 != 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  if (tokens == 0 || outs == 0) return FPQ_OK;
  if (k == 0 || !a_codes || !a_scales || !w_codes || !w_scales || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (uintptr_t)out | (uintptr_t)gelu_out) & 15) != 0 || ((uintptr_t)bias & 7) != 0 ||
      ((uintptr_t)nan_flag & 7) != 0)
    return FPQ_ERR_ARG;
  // the dual quantizer's table and arguments (fpq_fast16.h, lut16_host: built once, immutable afterwards)
  const Lut16Host& dual = lut16_host(FPQ_E1M2_NEG, FPQ_E2M1_POS);
  if (!dual.tab_valid) return FPQ_ERR_TABLE;
  GemmFc1 xe;
  xe.a = dual.args;
  xe.tab = dual.tab;
  xe.h_out = (_Float16*)gelu_out;
  xe.nan_flag = (uint32_t*)nan_flag;
  const int G = (int)(k / 128);
  GemmEpi epi{nullptr, nullptr, 1, km ? (int)outs : 0};   // (outs % 128 == 0: the weight image has exactly outs rows)
  if (km && (w_scale_dtype != FPQ_F32 || tokens >= (1ll << 28) || (((uintptr_t)a_scales | (uintptr_t)w_scales) & 15) != 0)) return FPQ_ERR_ARG;
  const int cfg = gemm_fp4_plan(tokens, outs, G, xe.a.shift);
  const GemmCall c{a_codes, a_scales, w_codes, w_scales, bias, out, tokens, outs, k, epi, (hipStream_t)stream};
  auto glds = [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    return launch_fp4_glds<MT>(c, w_scale_dtype, GemmGldsCfg<MT, 4>::lds_fc1(G, xe.a.shift), xe);
  };
  int rc = kTileDoesNotFit;
  if (cfg == 40) rc = launch_fp4_ring(c, w_scale_dtype, GemmRingCfg::lds_fc1(G, xe.a.shift), xe);
  if (cfg == 30) rc = glds(Int<2>{});
  if (cfg == 10) rc = glds(Int<8>{});
  if (cfg == 20) rc = glds(Int<4>{});
  if (rc == kTileDoesNotFit) return FPQ_ERR_SHAPE;   // K too long for the LDS-DMA kernel's scale tiles
  if (rc) return rc;
  return nan_flag ? fpq_internal_zero_if_flag(out, tokens * outs * 2, nan_flag, stream) : FPQ_OK;
}
int fpq_gemm_fp4_gelu_dual(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales,
                           int w_scale_dtype, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                           int64_t k, void* nan_flag, fpq_stream_t stream) {
  return gemm_fp4_gelu_dual_impl(a_codes, a_scales, w_codes, w_scales, w_scale_dtype, bias, out, gelu_out, tokens, outs, k, nan_flag, false, stream);
}
// which tiling a call would run (include/fpq.h): the entry points' shape checks, then gemm_fp4_plan - host arithmetic only
int fpq_gemm_fp4_tiling(int64_t tokens, int64_t outs, int64_t k, int form) {
  if (tokens < 0 || outs < 0 || k < 0 || (form != 0 && form != 1)) return FPQ_ERR_ARG;
  if (k % 128 != 0 || k > 128 * 64 || outs % (form == 1 ? 128 : 8) != 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  if (tokens == 0 || outs == 0) return FPQ_OK;   // nothing is launched
  if (k == 0) return FPQ_ERR_ARG;
  int shift = -1;
  if (form == 1) {
    const Lut16Host& dual = lut16_host(FPQ_E1M2_NEG, FPQ_E2M1_POS);
    if (!dual.tab_valid) return FPQ_ERR_TABLE;
    shift = dual.args.shift;
  }
  const int cfg = gemm_fp4_plan(tokens, outs, (int)(k / 128), shift);
  return cfg == kTileDoesNotFit ? FPQ_ERR_SHAPE : cfg;
}
int fpq_gemm_fp4_gelu_dual_km(const uint8_t* a_image, const void* a_scales, const uint8_t* w_image, const void* w_scales,
                              int w_scale_dtype, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                              int64_t k, void* nan_flag, fpq_stream_t stream) {
  return gemm_fp4_gelu_dual_impl(a_image, a_scales, w_image, w_scales, w_scale_dtype, bias, out, gelu_out, tokens, outs, k, nan_flag, true, stream);
}

static int gemm_fp6_rows_impl(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                              const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens,
                              int64_t outs, int64_t k, const fpq_gemm_epilogue_t* epilogue, bool km, fpq_stream_t stream,
                              const fpq_gemm_split_t* split = nullptr, const GemmQkNorm* qkn = nullptr,
                              int a_table = FPQ_E2M3, int w_table = FPQ_E2M3, const GemmSqErrCall* sq = nullptr) {
  // sq: the squared-error form (include/fpq.h, fpq_gemm_f6_rows_sqerr; row-major, no epilogue, no split): `out` is not looked at,
  // the form's own checks follow the family's, then the finish launch
  // a_table / w_table: FPQ_E2M3 or FPQ_E3M2 (checked by the fpq_gemm_f6_* entry points)
  if (tokens < 0 || outs < 0 || k < 0) return FPQ_ERR_ARG;
  GemmEpi epi;
  if (int rc = gemm_epilogue(epilogue, &epi)) return rc;
  if (split) {   // every part is held to the header's 8-byte alignment; whole batch entries only (the FP4 family does not ask for that)
    if (int rc = gemm_split(split, epilogue, tokens, outs, true, &epi)) return rc;
    out = split->out[0];   // (not written through: every tile belongs to a part)
  }
  if (km) {
    if (outs + 63 > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
    epi.km_w_rows = (int)((outs + 63) / 64 * 64);
  }
  if (k % 128 != 0 || outs % 8 != 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF || k > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  if ((a_scale_dtype != FPQ_F16 && a_scale_dtype != FPQ_F32) || (w_scale_dtype != FPQ_F16 && w_scale_dtype != FPQ_F32))
    return FPQ_ERR_DTYPE;
  // a pair with an E3M2 side exists for fp16 activation scales only (fp16 or fp32 weight scales; launch_fp6)
  if ((a_table == FPQ_E3M2 || w_table == FPQ_E3M2) && a_scale_dtype != FPQ_F16) return FPQ_ERR_DTYPE;
  GemmSqErr sqx{};
  if (tokens == 0 || outs == 0) {
    if (!sq) return FPQ_OK;
    if (int rc = gemm_sqerr_args(*sq, true, &sqx)) return rc;
    return gemm_sqerr_finish(*sq, 0, 0, 128, stream);
  }
  if (k == 0 || !a_codes || !a_scales || !w_codes || !w_scales || (!sq && !out)) return FPQ_ERR_ARG;
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (split || sq ? 0 : (uintptr_t)out)) & 15) != 0) return FPQ_ERR_ARG;
  // the LDS-DMA pieces address a tile by a 32-bit lane offset (row inside the tile x row bytes + chunk): the 256-row tile's
  // last row must stay below 2^32 (k above ~22 M would wrap and read wrong rows silently)
  if (255 * (k * 3 / 4) + 128 >= (1ll << 32)) return FPQ_ERR_SHAPE;
  // FPQ_GEMM6_CFG 0: 128 x 128 tiles, 1: 256 x 128 (default for tall problems)
  // 256 x 128 tiles from 4096 tokens on for the wide Linears, from 32768 on for outs < 4096 (tools/gemm_small_steps.py fp6)
  const int cfg6 = fpq_opt_set(OPT_FPQ_GEMM6_CFG) ? fpq_opt(OPT_FPQ_GEMM6_CFG, 0) : (tokens >= 4096 && (outs >= 4096 || tokens >= 32768) ? 1 : 0);
  const GemmCall c{a_codes, a_scales, w_codes, w_scales, bias, out, tokens, outs, k, epi, (hipStream_t)stream};
  if (sq) {
    if (int rc = gemm_sqerr_args(*sq, false, &sqx)) return rc;
    if (int rc = cfg6 == 1 ? dispatch_fp6<8>(c, a_scale_dtype, w_scale_dtype, a_table, w_table, false, nullptr, &sqx)
                           : dispatch_fp6<4>(c, a_scale_dtype, w_scale_dtype, a_table, w_table, false, nullptr, &sqx))
      return rc;
    return gemm_sqerr_finish(*sq, tokens, outs, cfg6 == 1 ? 256 : 128, stream);
  }
  if (cfg6 == 1) return dispatch_fp6<8>(c, a_scale_dtype, w_scale_dtype, a_table, w_table, split != nullptr, qkn);
  return dispatch_fp6<4>(c, a_scale_dtype, w_scale_dtype, a_table, w_table, split != nullptr, qkn);
}
int fpq_gemm_fp6_rows_ex(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                         const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens,
                         int64_t outs, int64_t k, const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  return gemm_fp6_rows_impl(a_codes, a_scales, a_scale_dtype, w_codes, w_scales, w_scale_dtype, bias, out, tokens, outs, k, epilogue, false, stream);
}
int fpq_gemm_fp6_rows_km(const uint8_t* a_image, const void* a_scales, int a_scale_dtype, const uint8_t* w_image,
                         const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens,
                         int64_t outs, int64_t k, const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  return gemm_fp6_rows_impl(a_image, a_scales, a_scale_dtype, w_image, w_scales, w_scale_dtype, bias, out, tokens, outs, k, epilogue, true, stream);
}

int fpq_gemm_fp6_rows_split(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes, const void* w_scales,
                            int w_scale_dtype, const void* bias, int64_t tokens, int64_t outs, int64_t k, const fpq_gemm_split_t* split,
                            int kmajor, fpq_stream_t stream) {
  if (!split) return FPQ_ERR_ARG;
  return gemm_fp6_rows_impl(a_codes, a_scales, a_scale_dtype, w_codes, w_scales, w_scale_dtype, bias, nullptr, tokens, outs, k, nullptr,
                            kmajor != 0, stream, split);
}
int fpq_gemm_fp6_rows_split_qknorm(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                                   const void* w_scales, int w_scale_dtype, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                   const fpq_gemm_split_t* split, const float* q_head_scale, int kmajor, fpq_stream_t stream) {
  GemmQkNorm qkn;
  if (int rc = gemm_qknorm(split, bias, q_head_scale, &qkn)) return rc;
  return gemm_fp6_rows_impl(a_codes, a_scales, a_scale_dtype, w_codes, w_scales, w_scale_dtype, nullptr, nullptr, tokens, outs, k, nullptr,
                            kmajor != 0, stream, split, &qkn);
}

// The FP6 GEMM with the format of each operand as an argument (include/fpq.h): FPQ_E2M3 or FPQ_E3M2 per side, everything else
// as the fpq_gemm_fp6_rows_* entry point of the same shape - (FPQ_E2M3, FPQ_E2M3) launches the very kernel that one launches.
static bool f6_table(int t) { return t == FPQ_E2M3 || t == FPQ_E3M2; }
int fpq_gemm_f6_rows(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, int a_table, const uint8_t* w_codes,
                     const void* w_scales, int w_scale_dtype, int w_table, const void* bias, void* out, int64_t tokens, int64_t outs,
                     int64_t k, const fpq_gemm_epilogue_t* epilogue, int kmajor, fpq_stream_t stream) {
  if (!f6_table(a_table) || !f6_table(w_table)) return FPQ_ERR_TABLE;
  return gemm_fp6_rows_impl(a_codes, a_scales, a_scale_dtype, w_codes, w_scales, w_scale_dtype, bias, out, tokens, outs, k, epilogue,
                            kmajor != 0, stream, nullptr, nullptr, a_table, w_table);
}
int fpq_gemm_f6_rows_sqerr(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, int a_table, const uint8_t* w_codes,
                           const void* w_scales, int w_scale_dtype, int w_table, const void* bias, const void* ref, int ref_dtype,
                           const float* row_weight, float* loss_out, void* workspace, int64_t tokens, int64_t outs, int64_t k,
                           fpq_stream_t stream) {
  if (!f6_table(a_table) || !f6_table(w_table)) return FPQ_ERR_TABLE;
  const GemmSqErrCall sq{ref, ref_dtype, row_weight, loss_out, workspace};
  return gemm_fp6_rows_impl(a_codes, a_scales, a_scale_dtype, w_codes, w_scales, w_scale_dtype, bias, nullptr, tokens, outs, k, nullptr,
                            false, stream, nullptr, nullptr, a_table, w_table, &sq);
}
int fpq_gemm_f6_rows_split(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, int a_table, const uint8_t* w_codes,
                           const void* w_scales, int w_scale_dtype, int w_table, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                           const fpq_gemm_split_t* split, int kmajor, fpq_stream_t stream) {
  if (!f6_table(a_table) || !f6_table(w_table)) return FPQ_ERR_TABLE;
  if (!split) return FPQ_ERR_ARG;
  return gemm_fp6_rows_impl(a_codes, a_scales, a_scale_dtype, w_codes, w_scales, w_scale_dtype, bias, nullptr, tokens, outs, k, nullptr,
                            kmajor != 0, stream, split, nullptr, a_table, w_table);
}
int fpq_gemm_f6_rows_split_qknorm(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, int a_table, const uint8_t* w_codes,
                                  const void* w_scales, int w_scale_dtype, int w_table, const float* bias, int64_t tokens, int64_t outs,
                                  int64_t k, const fpq_gemm_split_t* split, const float* q_head_scale, int kmajor, fpq_stream_t stream) {
  if (!f6_table(a_table) || !f6_table(w_table)) return FPQ_ERR_TABLE;
  GemmQkNorm qkn;
  if (int rc = gemm_qknorm(split, bias, q_head_scale, &qkn)) return rc;
  return gemm_fp6_rows_impl(a_codes, a_scales, a_scale_dtype, w_codes, w_scales, w_scale_dtype, nullptr, nullptr, tokens, outs, k, nullptr,
                            kmajor != 0, stream, split, &qkn, a_table, w_table);
}

// Row-major codes -> k-major image (include/fpq.h): one thread per 16-byte chunk of the image.  seg = bytes of a row per K step of
// 128 elements (64: FP4 nibbles, 96: dense 6-bit codes); dealt: the weight side's row order, image rows = rows rounded up to 64
// (rows past the tensor's end are zero).
__global__ __launch_bounds__(256) void codes_to_kmajor_kernel(const u32x4* __restrict__ codes, u32x4* __restrict__ image, int64_t rows,
                                                              int64_t image_rows, int steps, int seg, int dealt) {
  const int cps = seg >> 4;   // chunks per segment
  const int64_t n = (int64_t)steps * image_rows * cps;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int pc = (int)(i % cps);
    const int64_t sj = i / cps;
    const int64_t j = sj % image_rows;
    const int s = (int)(sj / image_rows);
    const int c = seg == 64 ? (pc ^ glds_chunk_perm((int)(j & 15))) : (pc - fp6_rot((int)(j & 31)) + 6) % 6;
    const int64_t row = dealt ? km_dealt_row(j) : j;
    u32x4 v = u32x4{0, 0, 0, 0};
    if (row < rows) v = codes[(row * steps + s) * cps + c];
    image[i] = v;
  }
}
int fpq_scales_to_kmajor(const void* scales, int scale_dtype, float* image, int64_t rows, int64_t groups, int weight_side,
                         fpq_stream_t stream) {
  if (rows < 0 || groups < 0 || groups > 0x7FFFFFFF) return FPQ_ERR_ARG;
  if (scale_dtype != FPQ_F16 && scale_dtype != FPQ_F32) return FPQ_ERR_DTYPE;
  if (rows == 0 || groups == 0) return FPQ_OK;
  if (!scales || !image || ((uintptr_t)image & 15) != 0) return FPQ_ERR_ARG;
  const int64_t image_rows = weight_side ? (rows + 63) / 64 * 64 : (rows + 3) / 4 * 4;
  const dim3 grid(grid_for((groups * image_rows + 255) / 256, 1 << 16));
  if (scale_dtype == FPQ_F16)
    hipLaunchKernelGGL(scales_to_kmajor_kernel<_Float16>, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)scales, image, rows,
                       image_rows, (int)groups);
  else
    hipLaunchKernelGGL(scales_to_kmajor_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)scales, image, rows,
                       image_rows, (int)groups);
  return check_launch();
}
int fpq_codes_to_kmajor(const uint8_t* codes, uint8_t* image, int64_t rows, int64_t k, int code_bits, int dealt, fpq_stream_t stream) {
  if (rows < 0 || k < 0 || (code_bits != 4 && code_bits != 6)) return FPQ_ERR_ARG;
  if (k % 128 != 0 || k / 128 > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  if (rows == 0 || k == 0) return FPQ_OK;
  if (!codes || !image || (((uintptr_t)codes | (uintptr_t)image) & 15) != 0) return FPQ_ERR_ARG;
  const int seg = code_bits == 4 ? 64 : 96;
  const int64_t image_rows = dealt ? (rows + 63) / 64 * 64 : rows;
  const int64_t n = (k / 128) * image_rows * (seg / 16);
  hipLaunchKernelGGL(codes_to_kmajor_kernel, dim3(grid_for((n + 255) / 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream,
                     (const u32x4*)codes, (u32x4*)image, rows, image_rows, (int)(k / 128), seg, dealt ? 1 : 0);
  return check_launch();
}

int fpq_gemm_fp8_rows_ex(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                         const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens,
                         int64_t outs, int64_t k, const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  if (tokens < 0 || outs < 0 || k < 0) return FPQ_ERR_ARG;
  GemmEpi epi;
  if (int rc = gemm_epilogue(epilogue, &epi)) return rc;
  if (k % 128 != 0 || outs % 8 != 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF || k > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  if ((a_scale_dtype != FPQ_F16 && a_scale_dtype != FPQ_F32) || (w_scale_dtype != FPQ_F16 && w_scale_dtype != FPQ_F32))
    return FPQ_ERR_DTYPE;
  if (tokens == 0 || outs == 0) return FPQ_OK;
  if (k == 0 || !a_codes || !a_scales || !w_codes || !w_scales || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (uintptr_t)out) & 15) != 0) return FPQ_ERR_ARG;
  if (255 * k + 128 >= (1ll << 32)) return FPQ_ERR_SHAPE;   // 32-bit lane offsets inside a tile, as in fpq_gemm_fp6_rows_ex
  const GemmCall c{a_codes, a_scales, w_codes, w_scales, bias, out, tokens, outs, k, epi, (hipStream_t)stream};
  if (fpq_opt(OPT_FPQ_GEMM8_CFG, 0) == 1) return dispatch_fp8<8>(c, a_scale_dtype, w_scale_dtype);
  return dispatch_fp8<4>(c, a_scale_dtype, w_scale_dtype);
}

}  // extern "C"
