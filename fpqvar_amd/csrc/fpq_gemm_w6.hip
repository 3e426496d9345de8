// fpq_gemm_w6.hip - the per-group(128) GEMM with a 6-bit WEIGHT fragment (E1M2 / E3M0 weights against E2M1, E1M2 or E3M0
// activations; include/fpq.h, fpq_gemm_w6.h).  One translation unit of libfpq_hip.so, beside fpq_gemm.hip: twelve kernels
// (three activation formats x two weight formats x two tilings) that compile while that unit does.
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
template <int MT>
int launch_w6(const GemmCall& c, int a_table, int w_table) {
  using Cfg = GemmW6Cfg<MT, 4>;
  const size_t lds = Cfg::lds((int)(c.k / 128), a_table == FPQ_E2M1);
  if (lds > 160 * 1024) return FPQ_ERR_SHAPE;
  auto formats = [&](auto fa, auto fw) {
    return gemm_launch(gemm_w6_kernel<float, MT, 4, decltype(fa)::value, decltype(fw)::value>, Cfg::BM, Cfg::BN, 256, lds, c);
  };
  auto weight = [&](auto fa) { return w_table == FPQ_E1M2 ? formats(fa, Int<2>{}) : formats(fa, Int<3>{}); };
  return a_table == FPQ_E2M1 ? weight(Int<4>{}) : a_table == FPQ_E1M2 ? weight(Int<2>{}) : weight(Int<3>{});
}
}  // namespace

extern "C" {

// Two LDS-DMA tilings, chosen as fpq_gemm_a6w4_mx chooses between the same two (FPQ_GEMM_CFG 20 / 30 forces one); the checks in
// that entry point's order
int fpq_gemm_w6_mx(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                   int w_scale_dtype, int w_table, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                   const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream) {
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
  if (tokens == 0 || outs == 0) return FPQ_OK;
  if (k == 0 || !a_codes || !a_scales || !w_codes || !w_scales || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (uintptr_t)out) & 15) != 0 || ((uintptr_t)bias & 7) != 0) return FPQ_ERR_ARG;
  if (((uintptr_t)a_scales & 1) != 0 || ((uintptr_t)w_scales & 3) != 0) return FPQ_ERR_ARG;
  const GemmCall c{a_codes, a_scales, w_codes, w_scales, bias, out, tokens, outs, k, epi, (hipStream_t)stream};
  return gemm_glds_tiling(tokens, outs, false, false) == 30 ? launch_w6<2>(c, a_table, w_table) : launch_w6<4>(c, a_table, w_table);
}

}  // extern "C"
