// fpq_gemm_w6.h - the per-group(128) GEMM of fpq_gemm_a6w4.h with a 6-bit WEIGHT fragment:
//     out[t,o] = fp16(bias[o] + sum_g sa[t,g] sw[o,g] dot128(La[t,g,:], Lw[o,g,:]))
// The format search (format_search.py) chooses a weight format per layer among E1M2, E2M1 and E3M0; the FP4 GEMM and the A6W4
// GEMM run the E2M1 weights.  Every E1M2 level is an E2M3 number and every E3M0 level an E3M2 number (fpq_codes_g6.h), so an
// E1M2 / E3M0 weight travels as the dense 6-bit codes fpq_quant_rows_codes_g6 writes for it (blgp = FW: 2 = FP6 E2M3, 3 = BF6
// E3M2) and the activation in whichever form its own format has: E2M1 nibbles (cbsz = FA = 4) or 6-bit codes (FA = 2 / 3).
// Included by fpq_gemm_w6.hip, a translation unit of its own (fpq_gemm.hip's compile time is the build's longest but one).
//
// One kernel text, compiled per (FA, FW, MT).  All three parents hand a lane the same 32 consecutive k of k-block lane >> 4
// (24 bytes of 6-bit codes / 16 bytes of nibbles), so the fragment forms meet in one instruction as they are:
//   * W tile: the FP6 kernel's weight side - 32-row, 3 KiB super-blocks, rows dealt over a wavefront's NT tiles, fp6_rot, three
//     ds_read_b64 per fragment;
//   * A tile, FA = 4: the FP4 kernel's 16-row 1 KiB blocks (glds_chunk_perm, one ds_read_b128 per fragment);
//     FA = 2 / 3: the A6W4 kernel's super-blocks;
//   * main loop, scale tiles, the per-group step t = fl(d_g sa), acc = fma(t, sw, acc) in plain fp32 VALU, the software pipeline
//     and the register epilogue (+ gate / residual tail) are gemm_a6w4_kernel's: the same fp32 model (include/fpq.h).
// A stage is BM / 16 (FA = 4) or 3 BM / 32 activation pieces + 3 BN / 32 weight pieces of 1 KiB, dealt round-robin over the four
// wavefronts (16 / 20 / 18 / 24 pieces: a short last round is a wavefront-uniform test); two stages, one barrier per group.
// Row-major operands with fp16 activation scales, or k-major images with fp32 scale images (FPQ_W6_KM below); instantiated for
// fp32 weight scales only (what quantize_g6 writes for a weight).
#pragma once

// The kernel's text is fpq_gemm_w6_kernel.h, compiled under four names per operand layout (as fpq_gemm_a6w4.h compiles
// fpq_gemm_a6w4_kernel.h): only the register epilogue and the extra kernel argument differ.
//   gemm_w6_kernel        the plain Linear (+ gate / residual tail);
//   gemm_w6_fc1_kernel    fc1 with the FFN's GELU(tanh) and fc2's dual-format input quantizer in the epilogue - the fc1 tail of
//                         gemm_fp4_glds_kernel / gemm_a6w4_fc1_kernel (FPQ_GEMM_FC1_TAIL: same 128-wide, 128-aligned tiles, same
//                         lane-to-output mapping, same two-stage ring whose idle buffer takes the maxima exchange), so fc2's input is
//                         bit-equal to the stand-alone quantizer on the same GELU values whichever GEMM computed fc1;
//   gemm_w6_split_kernel  mat_qkv's split output (include/fpq.h, fpq_gemm_w6_mx_split): the plain epilogue's values to the parts' own
//                         destinations;
//   gemm_w6_qkn_kernel    the split output with the q / k L2 norm in front (fpq_gemm_w6_mx_split_qknorm).
// Each for the same twelve (FA, FW, MT), fp32 weight scales: 48 kernels, none above 157 registers.
//   gemm_w6_fc1x_kernel   (FPQ_W6_FC1 == 2; and gemm_w6_fc1x_km_kernel) the fc1 kernel with the tail of a dual pair that has no global clamp
//                         (fpq_gemm_w6_gelu_dual_pair with INT- / E2M3+): a NaN stays out of its group's maxima
// Each form also on K-MAJOR IMAGES (FPQ_W6_KM; include/fpq.h): gemm_w6_km_kernel, gemm_w6_fc1_km_kernel, gemm_w6_split_km_kernel,
// gemm_w6_qkn_km_kernel, another 48 - the activation side's 4-bit (FA = 4) or 6-bit image, the dealt 6-bit weight image an FP6Linear
// holds, and both fp32 scale images.  Only the LDS-DMA sources and the scale-tile load differ: same LDS image, same main loop, same
// epilogues, same bits.
#define FPQ_W6_KM 0
#define FPQ_W6_KERNEL gemm_w6_kernel
#define FPQ_W6_FC1 0
#define FPQ_W6_OUT 0
#include "fpq_gemm_w6_kernel.h"
#undef FPQ_W6_KERNEL
#undef FPQ_W6_FC1
#undef FPQ_W6_OUT
#define FPQ_W6_KERNEL gemm_w6_fc1_kernel
#define FPQ_W6_FC1 1
#define FPQ_W6_OUT 0
#include "fpq_gemm_w6_kernel.h"
#undef FPQ_W6_KERNEL
#undef FPQ_W6_FC1
#undef FPQ_W6_OUT
#define FPQ_W6_KERNEL gemm_w6_fc1x_kernel
#define FPQ_W6_FC1 2
#define FPQ_W6_OUT 0
#include "fpq_gemm_w6_kernel.h"
#undef FPQ_W6_KERNEL
#undef FPQ_W6_FC1
#undef FPQ_W6_OUT
#define FPQ_W6_KERNEL gemm_w6_split_kernel
#define FPQ_W6_FC1 0
#define FPQ_W6_OUT 1
#include "fpq_gemm_w6_kernel.h"
#undef FPQ_W6_KERNEL
#undef FPQ_W6_FC1
#undef FPQ_W6_OUT
#define FPQ_W6_KERNEL gemm_w6_qkn_kernel
#define FPQ_W6_FC1 0
#define FPQ_W6_OUT 2
#include "fpq_gemm_w6_kernel.h"
#undef FPQ_W6_KERNEL
#undef FPQ_W6_FC1
#undef FPQ_W6_OUT
#undef FPQ_W6_KM
#define FPQ_W6_KM 1
#define FPQ_W6_KERNEL gemm_w6_km_kernel
#define FPQ_W6_FC1 0
#define FPQ_W6_OUT 0
#include "fpq_gemm_w6_kernel.h"
#undef FPQ_W6_KERNEL
#undef FPQ_W6_FC1
#undef FPQ_W6_OUT
#define FPQ_W6_KERNEL gemm_w6_fc1_km_kernel
#define FPQ_W6_FC1 1
#define FPQ_W6_OUT 0
#include "fpq_gemm_w6_kernel.h"
#undef FPQ_W6_KERNEL
#undef FPQ_W6_FC1
#undef FPQ_W6_OUT
#define FPQ_W6_KERNEL gemm_w6_fc1x_km_kernel
#define FPQ_W6_FC1 2
#define FPQ_W6_OUT 0
#include "fpq_gemm_w6_kernel.h"
#undef FPQ_W6_KERNEL
#undef FPQ_W6_FC1
#undef FPQ_W6_OUT
#define FPQ_W6_KERNEL gemm_w6_split_km_kernel
#define FPQ_W6_FC1 0
#define FPQ_W6_OUT 1
#include "fpq_gemm_w6_kernel.h"
#undef FPQ_W6_KERNEL
#undef FPQ_W6_FC1
#undef FPQ_W6_OUT
#define FPQ_W6_KERNEL gemm_w6_qkn_km_kernel
#define FPQ_W6_FC1 0
#define FPQ_W6_OUT 2
#include "fpq_gemm_w6_kernel.h"
#undef FPQ_W6_KERNEL
#undef FPQ_W6_FC1
#undef FPQ_W6_OUT
#undef FPQ_W6_KM


template <int MT, int NT>
struct GemmW6Cfg {
  static constexpr int BM = 32 * MT, BN = 32 * NT;
  // two stages (64 or 96 B per activation row, 96 per weight row) + the scale tiles, groups rounded up to four
  static size_t lds(int G, bool a4) {
    return 2 * ((size_t)BM * (a4 ? 64 : 96) + (size_t)BN * 96) + (size_t)((G + 3) & ~3) * (BM + BN) * 4;
  }
  static size_t lds_fc1(int G, bool a4, int shift) { return lds(G, a4) + ((size_t)2 << (16 - shift)); }   // + the dual quantizer's bucket table
};
