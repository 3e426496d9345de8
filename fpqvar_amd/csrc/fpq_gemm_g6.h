// fpq_gemm_g6.h - the per-group(128) GEMM of fpq_gemm_fp4.h with a 6-BIT SIDE:
//     out[t,o] = fp16(bias[o] + sum_g sa[t,g] sw[o,g] dot128(La[t,g,:], Lw[o,g,:]))
// The matrix instruction decodes only E2M1 from nibbles, but it takes a format selector per operand, FP6 operands run at the FP4
// rate, every E1M2 level is an E2M3 number and every E3M0 level an E3M2 number (fpq_codes_g6.h).  So an E1M2 / E3M0 operand
// travels as the dense 6-bit codes fpq_quant_rows_codes_g6 writes for it (selector 2 = FP6 E2M3, 3 = BF6 E3M2) and an E2M1 one
// as the nibbles the library already holds (selector 4).  Two families of kernels, one text (fpq_gemm_g6_kernel.h):
//   * "A6W4": a 6-bit ACTIVATION (cbsz = FA = 2 / 3) against E2M1 weights (blgp = 4).  The reference's mixed W4A4 model gives
//     fc1 / mat_qkv an E3M0 or E1M2 activation format in most blocks and keeps the weights E2M1 (SURVEY.md;
//     quantize_VAR_mixed_fp4_datatype); one stored FP4 weight, row-major or k-major, serves this GEMM and the FP4 one.
//   * "W6": a 6-bit WEIGHT (blgp = FW = 2 / 3) against an E2M1, E1M2 or E3M0 activation (FA = 4 / 2 / 3).  The format search
//     (format_search.py) chooses a weight format per layer among E1M2, E2M1 and E3M0; the E2M1 weights run on the FP4 and A6W4 GEMMs.
// Both parents of a fragment form hand a lane the same 32 consecutive k of k-block lane >> 4 (24 bytes of 6-bit codes / 16 bytes
// of nibbles), so the forms meet in one instruction as they are (the kernel text names them).  Scale tiles, the per-group step
// t = fl(d_g sa), acc = fma(t, sw, acc) in plain fp32 VALU and the register epilogue are gemm_fp4_glds_kernel's, so the result is
// bit-equal to the same fp32 model (include/fpq.h).
// A stage is BM * a_seg / 1024 + BN * w_seg / 1024 LDS-DMA pieces of 1 KiB (a_seg, w_seg: 64 bytes of nibbles or 96 of 6-bit
// codes per row and group), dealt round-robin over the four wavefronts (14 pieces for the A6W4 64 x 128 tile, 16 / 20 / 18 / 24 for
// W6: a short last round is a wavefront-uniform test); two stages, one barrier per group.
// Included by fpq_gemm_g6.hip, a translation unit of its own.
#pragma once

// Five forms per family, each on row-major operands (fp16 activation scales) and on K-MAJOR IMAGES (FPQ_G6_KM; include/fpq.h:
// fp32 scale images; only the LDS-DMA sources and the scale-tile load differ - same LDS image, main loop, epilogues and bits):
//   gemm_*_kernel        the plain Linear (+ gate / residual tail);
//   gemm_*_fc1_kernel    fc1 with the FFN's GELU(tanh) and fc2's dual-format input quantizer in the epilogue - the fc1 tail of
//                        gemm_fp4_glds_kernel (FPQ_GEMM_FC1_TAIL: same 128-wide, 128-aligned tiles, same lane-to-output mapping,
//                        same two-stage ring whose idle buffer takes the maxima exchange), so fc2's input is bit-equal to the
//                        stand-alone quantizer on the same GELU values whichever GEMM computed fc1;
//   gemm_*_fc1x_kernel   (FPQ_G6_FC1 == 2) the same with the tail of a dual pair that has no global clamp (fpq_gemm_*_gelu_dual_pair
//                        with INT- / E2M3+): a NaN stays out of its group's maxima;
//   gemm_*_split_kernel  mat_qkv's split output (include/fpq.h, fpq_gemm_*_mx_split): the plain epilogue's values to the parts' own
//                        destinations;
//   gemm_*_qkn_kernel    the split output with the q / k L2 norm in front (fpq_gemm_*_mx_split_qknorm).
// A sixth form on row-major operands only, counted apart (8 A6W4 kernels, 12 W6 ones):
//   gemm_*_sqerr_kernel  no output tensor: the format search's loss of the plain form's values against a reference
//                        (fpq_gemm_*_sqerr; the squared-error tail of fpq_gemm_fp4.h).
// Only the register epilogue and the extra kernel argument differ between the forms.  launch_g6 (fpq_gemm_g6.hip) instantiates
// them per (FA, FW, MT) for fp32 weight scales - what quantize_mx, quantize_g6 and the Linears hold, and what the images take
// anyway - and the row-major A6W4 plain, fc1 and fc1x kernels for fp16 ones too: 52 A6W4 kernels and 120 W6 ones, none above
// 157 registers.

// ---- A6W4: <Tsw, MT, NT, FA> ----
#define FPQ_G6_W4 1
#define FPQ_G6_KERNEL gemm_a6w4_kernel
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_W4 1
#define FPQ_G6_KERNEL gemm_a6w4_fc1_kernel
#define FPQ_G6_FC1 1
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_W4 1
#define FPQ_G6_KERNEL gemm_a6w4_fc1x_kernel
#define FPQ_G6_FC1 2
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_W4 1
#define FPQ_G6_KERNEL gemm_a6w4_split_kernel
#define FPQ_G6_OUT 1
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_W4 1
#define FPQ_G6_KERNEL gemm_a6w4_qkn_kernel
#define FPQ_G6_OUT 2
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_W4 1
#define FPQ_G6_KERNEL gemm_a6w4_sqerr_kernel
#define FPQ_G6_OUT 3
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_W4 1
#define FPQ_G6_KM 1
#define FPQ_G6_KERNEL gemm_a6w4_km_kernel
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_W4 1
#define FPQ_G6_KM 1
#define FPQ_G6_KERNEL gemm_a6w4_fc1_km_kernel
#define FPQ_G6_FC1 1
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_W4 1
#define FPQ_G6_KM 1
#define FPQ_G6_KERNEL gemm_a6w4_fc1x_km_kernel
#define FPQ_G6_FC1 2
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_W4 1
#define FPQ_G6_KM 1
#define FPQ_G6_KERNEL gemm_a6w4_split_km_kernel
#define FPQ_G6_OUT 1
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_W4 1
#define FPQ_G6_KM 1
#define FPQ_G6_KERNEL gemm_a6w4_qkn_km_kernel
#define FPQ_G6_OUT 2
#include "fpq_gemm_g6_kernel.h"

// ---- W6: <Tsw, MT, NT, FA, FW> ----
#define FPQ_G6_KERNEL gemm_w6_kernel
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_KERNEL gemm_w6_fc1_kernel
#define FPQ_G6_FC1 1
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_KERNEL gemm_w6_fc1x_kernel
#define FPQ_G6_FC1 2
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_KERNEL gemm_w6_split_kernel
#define FPQ_G6_OUT 1
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_KERNEL gemm_w6_qkn_kernel
#define FPQ_G6_OUT 2
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_KERNEL gemm_w6_sqerr_kernel
#define FPQ_G6_OUT 3
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_KM 1
#define FPQ_G6_KERNEL gemm_w6_km_kernel
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_KM 1
#define FPQ_G6_KERNEL gemm_w6_fc1_km_kernel
#define FPQ_G6_FC1 1
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_KM 1
#define FPQ_G6_KERNEL gemm_w6_fc1x_km_kernel
#define FPQ_G6_FC1 2
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_KM 1
#define FPQ_G6_KERNEL gemm_w6_split_km_kernel
#define FPQ_G6_OUT 1
#include "fpq_gemm_g6_kernel.h"
#define FPQ_G6_KM 1
#define FPQ_G6_KERNEL gemm_w6_qkn_km_kernel
#define FPQ_G6_OUT 2
#include "fpq_gemm_g6_kernel.h"

template <int MT, int NT>
struct GemmG6Cfg {
  static constexpr int BM = 32 * MT, BN = 32 * NT;
  // two stages (a_seg / w_seg: 64 or 96 B per activation / weight row) + the scale tiles, groups rounded up to four
  static size_t lds(int G, int a_seg, int w_seg) {
    return 2 * ((size_t)BM * a_seg + (size_t)BN * w_seg) + (size_t)((G + 3) & ~3) * (BM + BN) * 4;
  }
  // + the dual quantizer's bucket table
  static size_t lds_fc1(int G, int a_seg, int w_seg, int shift) { return lds(G, a_seg, w_seg) + ((size_t)2 << (16 - shift)); }
};
