// fpq_gemm_w6.hip - the per-group(128) GEMM with a 6-bit WEIGHT fragment (E1M2 / E3M0 weights against E2M1, E1M2 or E3M0
// activations; include/fpq.h, fpq_gemm_w6.h).  One translation unit of libfpq_hip.so, beside fpq_gemm.hip: 96 kernels (three
// activation formats x two weight formats x two tilings, in four forms: plain, fc1 tail, split output, split output with the q / k
// norm, each on row-major operands and on k-major images) that compile while that unit does - about 26 s (18 s before the k-major
// forms) against fpq_gemm.hip's 55 and fpq_adaln.hip's 85, so they stay one unit.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_gemm_fp4.h"
#include "fpq_gemm_fp8.h"
#include "fpq_gemm_fp6.h"
#include "fpq_gemm_w6.h"
#include "fpq_gemm_launch.h"

// 32 MT x 128 tiles; a_table: FPQ_E2M1 (nibbles, cbsz 4), FPQ_E1M2 (FP6 E2M3 codes, cbsz 2) or FPQ_E3M0 (BF6 E3M2, cbsz 3);
// w_table: FPQ_E1M2 (blgp 2) or FPQ_E3M0 (blgp 3); fp32 weight scales (the entry point has checked all three)
// km: the operands are k-major images (c.epi.km_w_rows set, both scale images fp32)
template <int MT>
int launch_w6(const GemmCall& c, int a_table, int w_table, bool km) {
  using Cfg = GemmW6Cfg<MT, 4>;
  const size_t lds = Cfg::lds((int)(c.k / 128), a_table == FPQ_E2M1);
  if (lds > 160 * 1024) return FPQ_ERR_SHAPE;
  auto formats = [&](auto fa, auto fw) {
    if (km) return gemm_launch(gemm_w6_km_kernel<float, MT, 4, decltype(fa)::value, decltype(fw)::value>, Cfg::BM, Cfg::BN, 256, lds, c);
    return gemm_launch(gemm_w6_kernel<float, MT, 4, decltype(fa)::value, decltype(fw)::value>, Cfg::BM, Cfg::BN, 256, lds, c);
  };
  auto weight = [&](auto fa) { return w_table == FPQ_E1M2 ? formats(fa, Int<2>{}) : formats(fa, Int<3>{}); };
  return a_table == FPQ_E2M1 ? weight(Int<4>{}) : a_table == FPQ_E1M2 ? weight(Int<2>{}) : weight(Int<3>{});
}
// 32 MT x 128 tiles and epilogue XE - GemmFc1: the fc1 tail; GemmSplit: the split output (c.epi's sp_* fields set; the kernel takes
// no further argument); GemmQkNorm: the split output with the q / k norm.  Tables as in launch_w6 (the entry point
// has checked them and the fp32 weight scales); lds: GemmW6Cfg's figure for that epilogue; km as in launch_w6.
template <int MT, typename XE>
int launch_w6_form(const GemmCall& c, int a_table, int w_table, size_t lds, XE xe, bool km) {
  using Cfg = GemmW6Cfg<MT, 4>;
  if (lds > 160 * 1024) return FPQ_ERR_SHAPE;
  auto formats = [&](auto fa, auto fw) {
    constexpr int FA = decltype(fa)::value, FW = decltype(fw)::value;
    if constexpr (__is_same(XE, GemmFc1)) {
      if (km) return gemm_launch(gemm_w6_fc1_km_kernel<float, MT, 4, FA, FW>, Cfg::BM, Cfg::BN, 256, lds, c, xe);
      return gemm_launch(gemm_w6_fc1_kernel<float, MT, 4, FA, FW>, Cfg::BM, Cfg::BN, 256, lds, c, xe);
    } else if constexpr (__is_same(XE, GemmFc1X)) {   // the tail of a dual pair without a global clamp
      const GemmFc1& x1 = xe;
      if (km) return gemm_launch(gemm_w6_fc1x_km_kernel<float, MT, 4, FA, FW>, Cfg::BM, Cfg::BN, 256, lds, c, x1);
      return gemm_launch(gemm_w6_fc1x_kernel<float, MT, 4, FA, FW>, Cfg::BM, Cfg::BN, 256, lds, c, x1);
    } else if constexpr (__is_same(XE, GemmQkNorm)) {
      if (km) return gemm_launch(gemm_w6_qkn_km_kernel<float, MT, 4, FA, FW>, Cfg::BM, Cfg::BN, 256, lds, c, xe);
      return gemm_launch(gemm_w6_qkn_kernel<float, MT, 4, FA, FW>, Cfg::BM, Cfg::BN, 256, lds, c, xe);
    } else {
      if (km) return gemm_launch(gemm_w6_split_km_kernel<float, MT, 4, FA, FW>, Cfg::BM, Cfg::BN, 256, lds, c);
      return gemm_launch(gemm_w6_split_kernel<float, MT, 4, FA, FW>, Cfg::BM, Cfg::BN, 256, lds, c);
    }
  };
  auto weight = [&](auto fa) { return w_table == FPQ_E1M2 ? formats(fa, Int<2>{}) : formats(fa, Int<3>{}); };
  return a_table == FPQ_E2M1 ? weight(Int<4>{}) : a_table == FPQ_E1M2 ? weight(Int<2>{}) : weight(Int<3>{});
}

// The k-major rules every W6 entry point slots into its row-major checks where gemm_a6w4_mx_impl has them (include/fpq.h): behind the
// shape rules, tokens and outs below 2^28 (32-bit lane offsets into three planes of the scale images) ...
bool w6_km_sizes(int64_t tokens, int64_t outs) { return tokens < (1ll << 28) && outs < (1ll << 28); }
// ... and behind the pointer checks the scales' alignment: both fp32 scale images 16 bytes, row-major scales their dtype
bool w6_scales_aligned(const void* a_scales, const void* w_scales, bool km) {
  if (km) return (((uintptr_t)a_scales | (uintptr_t)w_scales) & 15) == 0;
  return ((uintptr_t)a_scales & 1) == 0 && ((uintptr_t)w_scales & 3) == 0;
}
int w6_km_w_rows(int64_t outs) { return (int)((outs + 63) / 64 * 64); }

bool w6_tables(int a_table, int w_table) {
  return (a_table == FPQ_E2M1 || a_table == FPQ_E1M2 || a_table == FPQ_E3M0) && (w_table == FPQ_E1M2 || w_table == FPQ_E3M0);
}

// Two LDS-DMA tilings, chosen as fpq_gemm_a6w4_mx chooses between the same two (FPQ_GEMM_CFG 20 / 30 forces one); the checks in
// that entry point's order.  km: both operands and both scale tensors are k-major images (include/fpq.h; gemm_w6_km_kernel)
int gemm_w6_mx_impl(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                    int w_scale_dtype, int w_table, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                    const fpq_gemm_epilogue_t* epilogue, bool km, fpq_stream_t stream) {
  if (a_table != FPQ_E2M1 && a_table != FPQ_E1M2 && a_table != FPQ_E3M0) return FPQ_ERR_TABLE;
  if (w_table != FPQ_E1M2 && w_table != FPQ_E3M0) return FPQ_ERR_TABLE;
  if (tokens < 0 || outs < 0 || k < 0) return FPQ_ERR_ARG;
  GemmEpi epi;
  if (int rc = gemm_epilogue(epilogue, &epi)) return rc;
  if (w_scale_dtype != FPQ_F32) return FPQ_ERR_DTYPE;   // the kernels exist for fp32 weight scales only (fpq_gemm_w6.h)
  // the LDS image of the 128-row tiling with a 6-bit activation is the largest of the four, so it stands for all (112 KiB at
  // k = 8192: the k limit is the tighter one today)
  if (k % 128 != 0 || k > 128 * 64 || outs % 8 != 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF ||
      GemmW6Cfg<4, 4>::lds((int)(k / 128), false) > 160 * 1024)
    return FPQ_ERR_SHAPE;
  if (km && !w6_km_sizes(tokens, outs)) return FPQ_ERR_SHAPE;
  if (tokens == 0 || outs == 0) return FPQ_OK;
  if (k == 0 || !a_codes || !a_scales || !w_codes || !w_scales || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (uintptr_t)out) & 15) != 0 || ((uintptr_t)bias & 7) != 0) return FPQ_ERR_ARG;
  if (!w6_scales_aligned(a_scales, w_scales, km)) return FPQ_ERR_ARG;
  if (km) epi.km_w_rows = w6_km_w_rows(outs);
  const GemmCall c{a_codes, a_scales, w_codes, w_scales, bias, out, tokens, outs, k, epi, (hipStream_t)stream};
  return gemm_glds_tiling(tokens, outs, false, false) == 30 ? launch_w6<2>(c, a_table, w_table, km) : launch_w6<4>(c, a_table, w_table, km);
}

// fc1 with a 6-bit weight: the fc1 tail of fpq_gemm_fp4_gelu_dual / fpq_gemm_a6w4_gelu_dual in the W6 GEMM's epilogue
// (gemm_w6_fc1_kernel); operands, refusal order and tilings of gemm_w6_mx_impl; tail, gelu_out, nan_flag and fix-up launch of
// fpq_gemm_a6w4_gelu_dual; km as there (outs % 128 == 0: the weight image has exactly outs rows)
int gemm_w6_gelu_dual_impl(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                           int w_scale_dtype, int w_table, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                           int64_t k, void* nan_flag, bool km, fpq_stream_t stream, int neg_table = FPQ_E1M2_NEG,
                           int pos_table = FPQ_E2M1_POS) {
  if (!w6_tables(a_table, w_table)) return FPQ_ERR_TABLE;
  // the tail's dual pair (fpq_gemm_w6_gelu_dual_pair): fc2's 4-bit format with the reference's global clamp (the NaN flag), or its
  // 6-bit one, which has no clamp - the flag is not raised and nothing is zeroed
  const bool fp6_pair = neg_table == FPQ_INT_NEG && pos_table == FPQ_E2M3_POS;
  if (!fp6_pair && !(neg_table == FPQ_E1M2_NEG && pos_table == FPQ_E2M1_POS)) return FPQ_ERR_TABLE;
  const Lut16Host& dual = lut16_host(neg_table, pos_table);   // host arithmetic only: the table travels in the kernel's arguments
  if (!dual.tab_valid) return FPQ_ERR_TABLE;
  if (tokens < 0 || outs < 0 || k < 0) return FPQ_ERR_ARG;
  if (w_scale_dtype != FPQ_F32) return FPQ_ERR_DTYPE;   // the kernels exist for fp32 weight scales only (fpq_gemm_w6.h)
  // outs % 128: an output tile is one quantization group wide.  The LDS image of the 128-row tiling with a 6-bit activation is the
  // largest of the four, so it stands for all (about 116 KiB at k = 8192: the k limit is the tighter one today)
  if (k % 128 != 0 || k > 128 * 64 || outs % 128 != 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF ||
      GemmW6Cfg<4, 4>::lds_fc1((int)(k / 128), false, dual.args.shift) > 160 * 1024)
    return FPQ_ERR_SHAPE;
  if (km && !w6_km_sizes(tokens, outs)) return FPQ_ERR_SHAPE;
  if (tokens == 0 || outs == 0) return FPQ_OK;
  if (k == 0 || !a_codes || !a_scales || !w_codes || !w_scales || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (uintptr_t)out | (uintptr_t)gelu_out) & 15) != 0 || ((uintptr_t)bias & 7) != 0 ||
      ((uintptr_t)nan_flag & 7) != 0)
    return FPQ_ERR_ARG;
  if (!w6_scales_aligned(a_scales, w_scales, km)) return FPQ_ERR_ARG;
  GemmFc1 xe;
  xe.a = dual.args;
  xe.tab = dual.tab;
  xe.h_out = (_Float16*)gelu_out;
  if (fp6_pair) nan_flag = nullptr;
  xe.nan_flag = (uint32_t*)nan_flag;
  const int G = (int)(k / 128);
  const bool a4 = a_table == FPQ_E2M1;
  GemmEpi epi;
  if (int rc = gemm_epilogue(nullptr, &epi)) return rc;
  if (km) epi.km_w_rows = (int)outs;
  const GemmCall c{a_codes, a_scales, w_codes, w_scales, bias, out, tokens, outs, k, epi, (hipStream_t)stream};
  auto run = [&](const auto& x) {   // (the table's size comes from the pair: 2^(16 - shift) entries behind the scale tiles)
    return gemm_glds_tiling(tokens, outs, false, false) == 30
               ? launch_w6_form<2>(c, a_table, w_table, GemmW6Cfg<2, 4>::lds_fc1(G, a4, x.a.shift), x, km)
               : launch_w6_form<4>(c, a_table, w_table, GemmW6Cfg<4, 4>::lds_fc1(G, a4, x.a.shift), x, km);
  };
  GemmFc1X xx;
  static_cast<GemmFc1&>(xx) = xe;
  const int rc = fp6_pair ? run(xx) : run(xe);
  if (rc) return rc;
  return nan_flag ? fpq_internal_zero_if_flag(out, tokens * outs * 2, nan_flag, stream) : FPQ_OK;
}

// mat_qkv on the W6 GEMM: gemm_w6_mx_impl's checks in its order, the split descriptor where gemm_a6w4_mx_impl checks it (behind the
// sizes, in front of the dtype); out's alignment is not checked - every tile belongs to a part.  The callers have checked the tables.
int gemm_w6_split_impl(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                       int w_scale_dtype, int w_table, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                       const fpq_gemm_split_t* split, const GemmQkNorm* qkn, bool km, fpq_stream_t stream) {
  if (tokens < 0 || outs < 0 || k < 0) return FPQ_ERR_ARG;
  GemmEpi epi;
  if (int rc = gemm_epilogue(nullptr, &epi)) return rc;
  if (int rc = gemm_split(split, nullptr, tokens, outs, true, &epi)) return rc;
  if (w_scale_dtype != FPQ_F32) return FPQ_ERR_DTYPE;   // the kernels exist for fp32 weight scales only (fpq_gemm_w6.h)
  if (k % 128 != 0 || k > 128 * 64 || outs % 8 != 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF ||
      GemmW6Cfg<4, 4>::lds((int)(k / 128), false) > 160 * 1024)
    return FPQ_ERR_SHAPE;
  if (km && !w6_km_sizes(tokens, outs)) return FPQ_ERR_SHAPE;
  if (tokens == 0 || outs == 0) return FPQ_OK;
  if (k == 0 || !a_codes || !a_scales || !w_codes || !w_scales) return FPQ_ERR_ARG;
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes) & 15) != 0 || ((uintptr_t)bias & 7) != 0) return FPQ_ERR_ARG;
  if (!w6_scales_aligned(a_scales, w_scales, km)) return FPQ_ERR_ARG;
  if (km) epi.km_w_rows = w6_km_w_rows(outs);   // (outs = n_parts * part_cols, part_cols % 128 == 0: exactly outs)
  // out: the first part's tensor (not written through)
  const GemmCall c{a_codes, a_scales, w_codes, w_scales, bias, split->out[0], tokens, outs, k, epi, (hipStream_t)stream};
  const int G = (int)(k / 128);
  const bool a4 = a_table == FPQ_E2M1;
  auto tile = [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    const size_t lds = GemmW6Cfg<MT, 4>::lds(G, a4);
    if (qkn) return launch_w6_form<MT>(c, a_table, w_table, lds, *qkn, km);
    return launch_w6_form<MT>(c, a_table, w_table, lds, GemmSplit{}, km);
  };
  return gemm_glds_tiling(tokens, outs, false, false) == 30 ? tile(Int<2>{}) : tile(Int<4>{});
}
// the two split entry points' own checks in front of gemm_w6_split_impl: the tables go first, as in every W6 entry point
int gemm_w6_split_entry(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                        int w_scale_dtype, int w_table, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                        const fpq_gemm_split_t* split, bool km, fpq_stream_t stream) {
  if (!w6_tables(a_table, w_table)) return FPQ_ERR_TABLE;
  if (!split) return FPQ_ERR_ARG;
  return gemm_w6_split_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, bias, tokens, outs, k, split, nullptr, km,
                            stream);
}
int gemm_w6_split_qknorm_entry(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                               int w_scale_dtype, int w_table, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                               const fpq_gemm_split_t* split, const float* q_head_scale, bool km, fpq_stream_t stream) {
  if (!w6_tables(a_table, w_table)) return FPQ_ERR_TABLE;
  GemmQkNorm qkn;
  if (int rc = gemm_qknorm(split, bias, q_head_scale, &qkn)) return rc;
  return gemm_w6_split_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, nullptr, tokens, outs, k, split, &qkn, km,
                            stream);
}
}  // namespace

extern "C" {

// Every form has an entry point per operand layout (include/fpq.h): row-major codes with fp16 activation scales, and - the _km
// twins, same argument lists - k-major images with fp32 scale images.  No kmajor flag on the row-major ones.
int fpq_gemm_w6_mx(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                   int w_scale_dtype, int w_table, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                   const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  return gemm_w6_mx_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, bias, out, tokens, outs, k, epilogue, false,
                         stream);
}
int fpq_gemm_w6_mx_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                      int w_scale_dtype, int w_table, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                      const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  return gemm_w6_mx_impl(a_image, a_scales, a_table, w_image, w_scales, w_scale_dtype, w_table, bias, out, tokens, outs, k, epilogue, true,
                         stream);
}

int fpq_gemm_w6_gelu_dual(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                          int w_scale_dtype, int w_table, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                          int64_t k, void* nan_flag, fpq_stream_t stream) {
  return gemm_w6_gelu_dual_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, bias, out, gelu_out, tokens, outs, k,
                                nan_flag, false, stream);
}
int fpq_gemm_w6_gelu_dual_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                             int w_scale_dtype, int w_table, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                             int64_t k, void* nan_flag, fpq_stream_t stream) {
  return gemm_w6_gelu_dual_impl(a_image, a_scales, a_table, w_image, w_scales, w_scale_dtype, w_table, bias, out, gelu_out, tokens, outs, k,
                                nan_flag, true, stream);
}
// the same with the tail's dual pair and the layout as arguments (include/fpq.h, GF6)
int fpq_gemm_w6_gelu_dual_pair(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                               int w_scale_dtype, int w_table, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                               int64_t k, void* nan_flag, int neg_table, int pos_table, int kmajor, fpq_stream_t stream) {
  return gemm_w6_gelu_dual_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, bias, out, gelu_out, tokens, outs, k,
                                nan_flag, kmajor != 0, stream, neg_table, pos_table);
}

// mat_qkv on the W6 GEMM: the split output, and the q / k norm in that epilogue (include/fpq.h)
int fpq_gemm_w6_mx_split(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                         int w_scale_dtype, int w_table, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                         const fpq_gemm_split_t* split, fpq_stream_t stream) {
  return gemm_w6_split_entry(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, bias, tokens, outs, k, split, false, stream);
}
int fpq_gemm_w6_mx_split_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                            int w_scale_dtype, int w_table, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                            const fpq_gemm_split_t* split, fpq_stream_t stream) {
  return gemm_w6_split_entry(a_image, a_scales, a_table, w_image, w_scales, w_scale_dtype, w_table, bias, tokens, outs, k, split, true, stream);
}
int fpq_gemm_w6_mx_split_qknorm(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                                int w_scale_dtype, int w_table, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                const fpq_gemm_split_t* split, const float* q_head_scale, fpq_stream_t stream) {
  return gemm_w6_split_qknorm_entry(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, bias, tokens, outs, k, split,
                                    q_head_scale, false, stream);
}
int fpq_gemm_w6_mx_split_qknorm_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                                   int w_scale_dtype, int w_table, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                   const fpq_gemm_split_t* split, const float* q_head_scale, fpq_stream_t stream) {
  return gemm_w6_split_qknorm_entry(a_image, a_scales, a_table, w_image, w_scales, w_scale_dtype, w_table, bias, tokens, outs, k, split,
                                    q_head_scale, true, stream);
}

}  // extern "C"
