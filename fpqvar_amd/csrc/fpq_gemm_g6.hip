// fpq_gemm_g6.hip - the per-group(128) GEMMs with a 6-bit side (include/fpq.h, fpq_gemm_g6.h): "A6W4", E1M2 / E3M0 activations
// against E2M1 weights, and "W6", E1M2 / E3M0 weights against E2M1, E1M2 or E3M0 activations.  One translation unit of
// libfpq_hip.so, beside fpq_gemm.hip: 172 kernels of one text (52 A6W4, 120 W6: formats x two tilings, in five forms - plain, fc1
// tail, its NaN-excluding twin, split output, split output with the q / k norm - each on row-major operands and on k-major
// images) that compile while fpq_gemm.hip and fpq_adaln.hip, the build's longest unit, do - and, counted apart, the 20 kernels of
// the squared-error form (8 A6W4, 12 W6; row-major only).
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_gemm_fp4.h"
#include "fpq_gemm_fp8.h"
#include "fpq_gemm_fp6.h"
#include "fpq_gemm_g6.h"
#include "fpq_gemm_launch.h"

// An operand format's row bytes per group: 64 of nibbles (FPQ_E2M1) or 96 of 6-bit codes (FPQ_E1M2, FPQ_E3M0)
int g6_seg(int table) { return table == FPQ_E2M1 ? 64 : 96; }

// The families' formats.  a6w4: the call came in by an A6W4 entry point, which has no weight table and passes FPQ_E2M1 - a 6-bit
// activation against the FP4 GEMM's weight; otherwise by a W6 one - FPQ_E1M2 / FPQ_E3M0 weights (FPQ_E2M1 is refused: that
// weight's GEMMs are the A6W4 and the FP4 one) against any FP4 activation format.  Behind this check w_table == FPQ_E2M1 <=> a6w4.
bool g6_tables(int a_table, int w_table, bool a6w4) {
  if (a6w4) return w_table == FPQ_E2M1 && (a_table == FPQ_E1M2 || a_table == FPQ_E3M0);
  return (a_table == FPQ_E2M1 || a_table == FPQ_E1M2 || a_table == FPQ_E3M0) && (w_table == FPQ_E1M2 || w_table == FPQ_E3M0);
}

// THE kernel choice: 32 MT x 128 tiles and epilogue XE - GemmNoFc1: the plain kernel; GemmFc1 / GemmFc1X: the fc1 tail / its
// NaN-excluding twin; GemmSplit: the split output (c.epi's sp_* fields set; the kernel takes no further argument); GemmQkNorm: the
// split output with the q / k norm.  a_table / w_table: as g6_tables has passed them (cbsz / blgp 4, 2, 3 for FPQ_E2M1, FPQ_E1M2,
// FPQ_E3M0; w_table FPQ_E2M1: the A6W4 kernels); lds: GemmG6Cfg's figure for that epilogue; km: the operands are k-major images
// (c.epi.km_w_rows set).
// Every kernel exists for fp32 weight scales; for fp16 ones only the row-major A6W4 plain, fc1 and fc1x kernels do (fpq_gemm_g6.h).
template <int MT, typename XE>
int launch_g6(const GemmCall& c, int a_table, int w_table, int w_scale_dtype, size_t lds, XE xe, bool km) {
  using Cfg = GemmG6Cfg<MT, 4>;
  constexpr bool kSplit = __is_same(XE, GemmSplit) || __is_same(XE, GemmQkNorm);
  if (lds > 160 * 1024) return FPQ_ERR_SHAPE;
  const bool f16 = w_scale_dtype == FPQ_F16 && w_table == FPQ_E2M1 && !kSplit && !km;
  if (w_scale_dtype != FPQ_F32 && !f16) return FPQ_ERR_DTYPE;
  auto go = [&](auto kernel) {   // the launch, with the form's extra argument
    if constexpr (__is_same(XE, GemmFc1X)) {
      const GemmFc1& x1 = xe;
      return gemm_launch(kernel, Cfg::BM, Cfg::BN, 256, lds, c, x1);
    } else if constexpr (__is_same(XE, GemmFc1) || __is_same(XE, GemmQkNorm) || __is_same(XE, GemmSqErr)) {
      return gemm_launch(kernel, Cfg::BM, Cfg::BN, 256, lds, c, xe);
    } else {
      return gemm_launch(kernel, Cfg::BM, Cfg::BN, 256, lds, c);
    }
  };
  auto formats = [&](auto tw, auto fa, auto fw) {
    using Tw = decltype(tw);
    constexpr int FA = decltype(fa)::value, FW = decltype(fw)::value;
    // a form's four kernels: the A6W4 names are templates over <Tsw, MT, NT, FA>, the W6 ones over <Tsw, MT, NT, FA, FW>
#define FPQ_G6_PICK(a6w4_, a6w4_km_, w6_, w6_km_)                \
  if constexpr (FW != 4) {                                       \
    if (km) return go(w6_km_<float, MT, 4, FA, FW>);             \
    return go(w6_<float, MT, 4, FA, FW>);                        \
  } else {                                                       \
    if constexpr (__is_same(Tw, float))                          \
      if (km) return go(a6w4_km_<float, MT, 4, FA>);             \
    return go(a6w4_<Tw, MT, 4, FA>);                             \
  }
    if constexpr (__is_same(XE, GemmSqErr)) {   // row-major only (km is refused by the caller: there is no such entry point)
      if constexpr (FW != 4) return go(gemm_w6_sqerr_kernel<float, MT, 4, FA, FW>);
      else return go(gemm_a6w4_sqerr_kernel<Tw, MT, 4, FA>);
    } else if constexpr (__is_same(XE, GemmFc1)) {
      FPQ_G6_PICK(gemm_a6w4_fc1_kernel, gemm_a6w4_fc1_km_kernel, gemm_w6_fc1_kernel, gemm_w6_fc1_km_kernel)
    } else if constexpr (__is_same(XE, GemmFc1X)) {
      FPQ_G6_PICK(gemm_a6w4_fc1x_kernel, gemm_a6w4_fc1x_km_kernel, gemm_w6_fc1x_kernel, gemm_w6_fc1x_km_kernel)
    } else if constexpr (__is_same(XE, GemmQkNorm)) {
      FPQ_G6_PICK(gemm_a6w4_qkn_kernel, gemm_a6w4_qkn_km_kernel, gemm_w6_qkn_kernel, gemm_w6_qkn_km_kernel)
    } else if constexpr (__is_same(XE, GemmSplit)) {
      FPQ_G6_PICK(gemm_a6w4_split_kernel, gemm_a6w4_split_km_kernel, gemm_w6_split_kernel, gemm_w6_split_km_kernel)
    } else {
      FPQ_G6_PICK(gemm_a6w4_kernel, gemm_a6w4_km_kernel, gemm_w6_kernel, gemm_w6_km_kernel)
    }
#undef FPQ_G6_PICK
  };
  auto activation = [&](auto tw, auto fw) {   // (nibbles on both sides are the FP4 GEMM's)
    if constexpr (decltype(fw)::value != 4)
      if (a_table == FPQ_E2M1) return formats(tw, Int<4>{}, fw);
    return a_table == FPQ_E1M2 ? formats(tw, Int<2>{}, fw) : formats(tw, Int<3>{}, fw);
  };
  if (w_table == FPQ_E2M1) {
    if constexpr (!kSplit)
      if (f16) return activation(_Float16{}, Int<4>{});
    return activation(float{}, Int<4>{});
  }
  return w_table == FPQ_E1M2 ? activation(float{}, Int<2>{}) : activation(float{}, Int<3>{});
}

// What the entry points share beside the row-major checks when the operands are k-major images (include/fpq.h): behind the shape
// rules, tokens and outs below 2^28 (32-bit lane offsets into three planes of the scale images) ...
bool g6_km_sizes(int64_t tokens, int64_t outs) { return tokens < (1ll << 28) && outs < (1ll << 28); }
// ... and behind the pointer checks the scales' alignment: both fp32 scale images 16 bytes, row-major scales their dtype
bool g6_scales_aligned(const void* a_scales, const void* w_scales, int w_scale_dtype, bool km) {
  if (km) return (((uintptr_t)a_scales | (uintptr_t)w_scales) & 15) == 0;
  return ((uintptr_t)a_scales & 1) == 0 && ((uintptr_t)w_scales & (w_scale_dtype == FPQ_F16 ? 1 : 3)) == 0;
}
// the weight-scale dtypes a form takes: fp32, and fp16 where the kernels for it exist (f16_form: A6W4, row-major, plain or fc1)
bool g6_w_scale_dtype(int w_scale_dtype, bool f16_form) { return w_scale_dtype == FPQ_F32 || (f16_form && w_scale_dtype == FPQ_F16); }

// The Linear of both families: plain (+ gate / residual tail), or - split / qkn - mat_qkv's split output (the FP6 family's rules:
// whole batch entries, every part 8-byte aligned) and the q / k norm in front of it.  a6w4: see g6_tables; it also says that fp16
// weight scales are allowed (on the row-major plain form: the images and the split forms are fp32 only).
// Two LDS-DMA tilings, chosen as fpq_gemm_fp4_mx_ex chooses between the same two (FPQ_GEMM_CFG 20 / 30 forces one); no
// register-staged form: K is limited by the scale tiles as there, and the bias is read four outputs at a time.
// The refusals in every entry point's order: table(s), negative sizes, epilogue, split descriptor, weight-scale dtype, shape,
// k-major sizes, empty problem, pointers, alignments.
int gemm_g6_mx_impl(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                    int w_scale_dtype, int w_table, bool a6w4, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                    const fpq_gemm_epilogue_t* epilogue, bool km, fpq_stream_t stream, const fpq_gemm_split_t* split = nullptr,
                    const GemmQkNorm* qkn = nullptr, const GemmSqErrCall* sq = nullptr) {
  // sq: the squared-error form (include/fpq.h, fpq_gemm_a6w4_sqerr / fpq_gemm_w6_sqerr; row-major, no epilogue, no split): `out` is
  // not looked at, the form's own checks follow the family's, then the finish launch
  if (!g6_tables(a_table, w_table, a6w4)) return FPQ_ERR_TABLE;
  if (tokens < 0 || outs < 0 || k < 0) return FPQ_ERR_ARG;
  GemmEpi epi;
  if (int rc = gemm_epilogue(epilogue, &epi)) return rc;
  if (split) {
    if (int rc = gemm_split(split, epilogue, tokens, outs, true, &epi)) return rc;
    out = split->out[0];   // (not written through: every tile belongs to a part, and out's alignment is not asked for)
  }
  if (!g6_w_scale_dtype(w_scale_dtype, a6w4 && !km && !split)) return FPQ_ERR_DTYPE;
  // The LDS image (the 128-row tiling with a 6-bit activation has the largest) is 112 KiB at k = 8192, so the k limit is the
  // tighter one and this test cannot fire.  It stands where each family had it, so that no refusal changes place: the W6 entry
  // points made it here, the A6W4 ones leave it to launch_g6, behind the pointer checks.
  const int G = (int)(k / 128), a_seg = g6_seg(a_table), w_seg = g6_seg(w_table);
  if (k % 128 != 0 || k > 128 * 64 || outs % 8 != 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF ||
      (!a6w4 && GemmG6Cfg<4, 4>::lds(G, 96, w_seg) > 160 * 1024))
    return FPQ_ERR_SHAPE;
  if (km && !g6_km_sizes(tokens, outs)) return FPQ_ERR_SHAPE;
  GemmSqErr sqx{};
  if (tokens == 0 || outs == 0) {
    if (!sq) return FPQ_OK;
    if (int rc = gemm_sqerr_args(*sq, true, &sqx)) return rc;
    return gemm_sqerr_finish(*sq, 0, 0, 64, stream);
  }
  if (k == 0 || !a_codes || !a_scales || !w_codes || !w_scales || (!sq && !out)) return FPQ_ERR_ARG;
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (split || sq ? 0 : (uintptr_t)out)) & 15) != 0 || ((uintptr_t)bias & 7) != 0) return FPQ_ERR_ARG;
  if (!g6_scales_aligned(a_scales, w_scales, w_scale_dtype, km)) return FPQ_ERR_ARG;
  if (sq)
    if (int rc = gemm_sqerr_args(*sq, false, &sqx)) return rc;
  if (km) epi.km_w_rows = (int)((outs + 63) / 64 * 64);   // (split: outs = n_parts * part_cols, part_cols % 128 == 0 - exactly outs)
  const GemmCall c{a_codes, a_scales, w_codes, w_scales, bias, out, tokens, outs, k, epi, (hipStream_t)stream};
  auto tile = [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    const size_t lds = GemmG6Cfg<MT, 4>::lds(G, a_seg, w_seg);
    if (sq) {
      if (int rc = launch_g6<MT>(c, a_table, w_table, w_scale_dtype, lds, sqx, false)) return rc;
      return gemm_sqerr_finish(*sq, tokens, outs, GemmG6Cfg<MT, 4>::BM, stream);
    }
    if (qkn) return launch_g6<MT>(c, a_table, w_table, w_scale_dtype, lds, *qkn, km);
    if (split) return launch_g6<MT>(c, a_table, w_table, w_scale_dtype, lds, GemmSplit{}, km);
    return launch_g6<MT>(c, a_table, w_table, w_scale_dtype, lds, GemmNoFc1{}, km);
  };
  return gemm_glds_tiling(tokens, outs, false, false) == 30 ? tile(Int<2>{}) : tile(Int<4>{});
}
// the two split entry points' own checks in front of gemm_g6_mx_impl: the tables go first, as in every entry point of the families
int gemm_g6_split_entry(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                        int w_scale_dtype, int w_table, bool a6w4, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                        const fpq_gemm_split_t* split, bool km, fpq_stream_t stream) {
  if (!g6_tables(a_table, w_table, a6w4)) return FPQ_ERR_TABLE;
  if (!split) return FPQ_ERR_ARG;
  return gemm_g6_mx_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, a6w4, bias, nullptr, tokens, outs, k, nullptr,
                         km, stream, split);
}
int gemm_g6_split_qknorm_entry(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                               int w_scale_dtype, int w_table, bool a6w4, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                               const fpq_gemm_split_t* split, const float* q_head_scale, bool km, fpq_stream_t stream) {
  if (!g6_tables(a_table, w_table, a6w4)) return FPQ_ERR_TABLE;
  GemmQkNorm qkn;
  if (int rc = gemm_qknorm(split, bias, q_head_scale, &qkn)) return rc;
  return gemm_g6_mx_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, a6w4, nullptr, nullptr, tokens, outs, k,
                         nullptr, km, stream, split, &qkn);
}

// fc1 of both families: the fc1 tail of fpq_gemm_fp4_gelu_dual in this GEMM's epilogue (gemm_*_fc1_kernel); operands, tables,
// a6w4, refusal order and tilings of gemm_g6_mx_impl; tail, gelu_out, nan_flag and fix-up launch of fpq_gemm_fp4_gelu_dual;
// km as there (outs % 128 == 0: the weight image has exactly outs rows)
int gemm_g6_gelu_dual_impl(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                           int w_scale_dtype, int w_table, bool a6w4, const void* bias, void* out, void* gelu_out, int64_t tokens,
                           int64_t outs, int64_t k, void* nan_flag, bool km, fpq_stream_t stream, int neg_table = FPQ_E1M2_NEG,
                           int pos_table = FPQ_E2M1_POS) {
  if (!g6_tables(a_table, w_table, a6w4)) return FPQ_ERR_TABLE;
  // the tail's dual pair (fpq_gemm_*_gelu_dual_pair): fc2's 4-bit format with the reference's global clamp (the NaN flag), or its
  // 6-bit one, which has no clamp - the flag is not raised and nothing is zeroed
  const bool fp6_pair = neg_table == FPQ_INT_NEG && pos_table == FPQ_E2M3_POS;
  if (!fp6_pair && !(neg_table == FPQ_E1M2_NEG && pos_table == FPQ_E2M1_POS)) return FPQ_ERR_TABLE;
  const Lut16Host& dual = lut16_host(neg_table, pos_table);   // host arithmetic only: the table travels in the kernel's arguments
  if (!dual.tab_valid) return FPQ_ERR_TABLE;
  if (tokens < 0 || outs < 0 || k < 0) return FPQ_ERR_ARG;
  if (!g6_w_scale_dtype(w_scale_dtype, a6w4 && !km)) return FPQ_ERR_DTYPE;
  // outs % 128: an output tile is one quantization group wide.  The LDS image of the 128-row tiling with a 6-bit activation is the
  // family's largest, so it stands for all (105 / 116 KiB at k = 8192: the k limit is the tighter one today)
  const int G = (int)(k / 128), a_seg = g6_seg(a_table), w_seg = g6_seg(w_table);
  if (k % 128 != 0 || k > 128 * 64 || outs % 128 != 0 || tokens > 0x7FFFFFFF || outs > 0x7FFFFFFF ||
      GemmG6Cfg<4, 4>::lds_fc1(G, 96, w_seg, dual.args.shift) > 160 * 1024)
    return FPQ_ERR_SHAPE;
  if (km && !g6_km_sizes(tokens, outs)) return FPQ_ERR_SHAPE;
  if (tokens == 0 || outs == 0) return FPQ_OK;
  if (k == 0 || !a_codes || !a_scales || !w_codes || !w_scales || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (uintptr_t)out | (uintptr_t)gelu_out) & 15) != 0 || ((uintptr_t)bias & 7) != 0 ||
      ((uintptr_t)nan_flag & 7) != 0)
    return FPQ_ERR_ARG;
  if (!g6_scales_aligned(a_scales, w_scales, w_scale_dtype, km)) return FPQ_ERR_ARG;
  GemmFc1 xe;
  xe.a = dual.args;
  xe.tab = dual.tab;
  xe.h_out = (_Float16*)gelu_out;
  if (fp6_pair) nan_flag = nullptr;
  xe.nan_flag = (uint32_t*)nan_flag;
  GemmEpi epi;
  if (int rc = gemm_epilogue(nullptr, &epi)) return rc;
  if (km) epi.km_w_rows = (int)outs;
  const GemmCall c{a_codes, a_scales, w_codes, w_scales, bias, out, tokens, outs, k, epi, (hipStream_t)stream};
  auto run = [&](const auto& x) {   // (the table's size comes from the pair: 2^(16 - shift) entries behind the scale tiles)
    return gemm_glds_tiling(tokens, outs, false, false) == 30
               ? launch_g6<2>(c, a_table, w_table, w_scale_dtype, GemmG6Cfg<2, 4>::lds_fc1(G, a_seg, w_seg, x.a.shift), x, km)
               : launch_g6<4>(c, a_table, w_table, w_scale_dtype, GemmG6Cfg<4, 4>::lds_fc1(G, a_seg, w_seg, x.a.shift), x, km);
  };
  GemmFc1X xx;
  static_cast<GemmFc1&>(xx) = xe;
  const int rc = fp6_pair ? run(xx) : run(xe);
  if (rc) return rc;
  return nan_flag ? fpq_internal_zero_if_flag(out, tokens * outs * 2, nan_flag, stream) : FPQ_OK;
}
}  // namespace

extern "C" {

// ---- A6W4 (include/fpq.h): the weight is the FP4 GEMM's, so there is no weight table; fp16 weight scales on the row-major plain and
// fc1 forms; the plain and fc1 forms have _km twins, the split ones and _gelu_dual_pair take the layout as a flag ----
int fpq_gemm_a6w4_mx(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                     int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                     const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  return gemm_g6_mx_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, FPQ_E2M1, true, bias, out, tokens, outs, k, epilogue,
                         false, stream);
}
int fpq_gemm_a6w4_mx_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                        int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                        const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  return gemm_g6_mx_impl(a_image, a_scales, a_table, w_image, w_scales, w_scale_dtype, FPQ_E2M1, true, bias, out, tokens, outs, k, epilogue,
                         true, stream);
}
int fpq_gemm_a6w4_mx_split(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                           int w_scale_dtype, const void* bias, int64_t tokens, int64_t outs, int64_t k, const fpq_gemm_split_t* split,
                           int kmajor, fpq_stream_t stream) {
  return gemm_g6_split_entry(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, FPQ_E2M1, true, bias, tokens, outs, k, split,
                             kmajor != 0, stream);
}
int fpq_gemm_a6w4_mx_split_qknorm(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                                  int w_scale_dtype, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                  const fpq_gemm_split_t* split, const float* q_head_scale, int kmajor, fpq_stream_t stream) {
  return gemm_g6_split_qknorm_entry(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, FPQ_E2M1, true, bias, tokens, outs, k, split,
                                    q_head_scale, kmajor != 0, stream);
}
int fpq_gemm_a6w4_gelu_dual(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                            int w_scale_dtype, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs, int64_t k,
                            void* nan_flag, fpq_stream_t stream) {
  return gemm_g6_gelu_dual_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, FPQ_E2M1, true, bias, out, gelu_out, tokens, outs,
                                k, nan_flag, false, stream);
}
int fpq_gemm_a6w4_gelu_dual_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                               int w_scale_dtype, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs, int64_t k,
                               void* nan_flag, fpq_stream_t stream) {
  return gemm_g6_gelu_dual_impl(a_image, a_scales, a_table, w_image, w_scales, w_scale_dtype, FPQ_E2M1, true, bias, out, gelu_out, tokens, outs,
                                k, nan_flag, true, stream);
}
// the same with the tail's dual pair and the layout as arguments (include/fpq.h, GF6)
int fpq_gemm_a6w4_gelu_dual_pair(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                                 int w_scale_dtype, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs, int64_t k,
                                 void* nan_flag, int neg_table, int pos_table, int kmajor, fpq_stream_t stream) {
  return gemm_g6_gelu_dual_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, FPQ_E2M1, true, bias, out, gelu_out, tokens, outs,
                                k, nan_flag, kmajor != 0, stream, neg_table, pos_table);
}

// the squared-error forms of the two families (include/fpq.h, "THE SQUARED-ERROR FORMS"): the plain row-major Linear's checks, no
// output tensor, no epilogue
int fpq_gemm_a6w4_sqerr(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                        int w_scale_dtype, const void* bias, const void* ref, int ref_dtype, const float* row_weight, float* loss_out,
                        void* workspace, int64_t tokens, int64_t outs, int64_t k, fpq_stream_t stream) {
  const GemmSqErrCall sq{ref, ref_dtype, row_weight, loss_out, workspace};
  return gemm_g6_mx_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, FPQ_E2M1, true, bias, nullptr, tokens, outs, k, nullptr,
                         false, stream, nullptr, nullptr, &sq);
}
int fpq_gemm_w6_sqerr(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                      int w_scale_dtype, int w_table, const void* bias, const void* ref, int ref_dtype, const float* row_weight,
                      float* loss_out, void* workspace, int64_t tokens, int64_t outs, int64_t k, fpq_stream_t stream) {
  const GemmSqErrCall sq{ref, ref_dtype, row_weight, loss_out, workspace};
  return gemm_g6_mx_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, false, bias, nullptr, tokens, outs, k, nullptr,
                         false, stream, nullptr, nullptr, &sq);
}

// ---- W6 (include/fpq.h): a weight table; fp32 weight scales only; every form has a _km twin with the same argument list, no kmajor
// flag on the row-major ones (fpq_gemm_w6_gelu_dual_pair apart) ----
int fpq_gemm_w6_mx(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                   int w_scale_dtype, int w_table, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                   const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  return gemm_g6_mx_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, false, bias, out, tokens, outs, k, epilogue,
                         false, stream);
}
int fpq_gemm_w6_mx_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                      int w_scale_dtype, int w_table, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                      const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
  return gemm_g6_mx_impl(a_image, a_scales, a_table, w_image, w_scales, w_scale_dtype, w_table, false, bias, out, tokens, outs, k, epilogue,
                         true, stream);
}
int fpq_gemm_w6_mx_split(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                         int w_scale_dtype, int w_table, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                         const fpq_gemm_split_t* split, fpq_stream_t stream) {
  return gemm_g6_split_entry(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, false, bias, tokens, outs, k, split, false,
                             stream);
}
int fpq_gemm_w6_mx_split_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                            int w_scale_dtype, int w_table, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                            const fpq_gemm_split_t* split, fpq_stream_t stream) {
  return gemm_g6_split_entry(a_image, a_scales, a_table, w_image, w_scales, w_scale_dtype, w_table, false, bias, tokens, outs, k, split, true,
                             stream);
}
int fpq_gemm_w6_mx_split_qknorm(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                                int w_scale_dtype, int w_table, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                const fpq_gemm_split_t* split, const float* q_head_scale, fpq_stream_t stream) {
  return gemm_g6_split_qknorm_entry(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, false, bias, tokens, outs, k, split,
                                    q_head_scale, false, stream);
}
int fpq_gemm_w6_mx_split_qknorm_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                                   int w_scale_dtype, int w_table, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                   const fpq_gemm_split_t* split, const float* q_head_scale, fpq_stream_t stream) {
  return gemm_g6_split_qknorm_entry(a_image, a_scales, a_table, w_image, w_scales, w_scale_dtype, w_table, false, bias, tokens, outs, k, split,
                                    q_head_scale, true, stream);
}
int fpq_gemm_w6_gelu_dual(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                          int w_scale_dtype, int w_table, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                          int64_t k, void* nan_flag, fpq_stream_t stream) {
  return gemm_g6_gelu_dual_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, false, bias, out, gelu_out, tokens, outs,
                                k, nan_flag, false, stream);
}
int fpq_gemm_w6_gelu_dual_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                             int w_scale_dtype, int w_table, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                             int64_t k, void* nan_flag, fpq_stream_t stream) {
  return gemm_g6_gelu_dual_impl(a_image, a_scales, a_table, w_image, w_scales, w_scale_dtype, w_table, false, bias, out, gelu_out, tokens, outs,
                                k, nan_flag, true, stream);
}
int fpq_gemm_w6_gelu_dual_pair(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                               int w_scale_dtype, int w_table, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                               int64_t k, void* nan_flag, int neg_table, int pos_table, int kmajor, fpq_stream_t stream) {
  return gemm_g6_gelu_dual_impl(a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, false, bias, out, gelu_out, tokens, outs,
                                k, nan_flag, kmajor != 0, stream, neg_table, pos_table);
}

}  // extern "C"
