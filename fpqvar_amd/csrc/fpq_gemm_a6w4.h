// fpq_gemm_a6w4.h - the per-group(128) GEMM of fpq_gemm_fp4.h with a 6-bit ACTIVATION fragment against the same FP4 weights:
//     out[t,o] = fp16(bias[o] + sum_g sa[t,g] sw[o,g] dot128(La[t,g,:], Lw[o,g,:]))
// The reference's mixed W4A4 model gives fc1 / mat_qkv an E3M0 or E1M2 activation format in most blocks and keeps the weights
// E2M1 (quantize_VAR_mixed_fp4_datatype).  The matrix instruction decodes only E2M1 from nibbles, but it takes a
// format selector per operand, FP6 operands run at the FP4 rate, every E1M2 level is an E2M3 number and every E3M0 level an
// E3M2 number: the activation travels as dense 6-bit codes (cbsz = FA: 2 = FP6 E2M3 holding E1M2 levels, 3 = BF6 E3M2 holding
// E3M0 levels), the weight as the nibbles the library already holds (blgp = 4).  Included by fpq_gemm.hip after fpq_gemm_fp6.h.
//
// Both parent kernels hand a lane the same 32 consecutive k of k-block lane >> 4 (24 bytes of 6-bit codes / 16 bytes of
// nibbles), so the two fragment forms meet in one instruction as they are:
//   * A tile: the FP6 kernel's 32-row, 3 KiB super-blocks (fp6_rot, three ds_read_b64 per fragment);
//   * W tile: the FP4 kernel's 16-row 1 KiB blocks, rows dealt over a wavefront's NT tiles (one ds_read_b128 per fragment);
//   * scale tiles, the per-group step t = fl(d_g sa), acc = fma(t, sw, acc) in plain fp32 VALU and the register epilogue are
//     gemm_fp4_glds_kernel's, so the result is bit-equal to the same fp32 model (include/fpq.h).
// A stage is 3 BM / 32 + BN / 16 LDS-DMA pieces of 1 KiB, dealt round-robin over the four wavefronts (14 pieces for the
// 64 x 128 tile: the last round is two pieces short, a wavefront-uniform test); two stages, one barrier per group.
#pragma once

// The kernel's text is fpq_gemm_a6w4_kernel.h, compiled under two names: gemm_a6w4_kernel, the plain Linear (+ gate / residual tail),
// and gemm_a6w4_fc1_kernel, fc1 with the FFN's GELU(tanh) and fc2's dual-format input quantizer in the epilogue - the fc1 tail of
// gemm_fp4_glds_kernel (FPQ_GEMM_FC1_TAIL, fpq_gemm_fp4.h: same 128-wide, 128-aligned tiles, same lane-to-output mapping, same
// two-stage ring whose idle buffer takes the maxima exchange), so fc2's input is bit-equal to the stand-alone quantizer on the
// same GELU values whichever GEMM computed fc1.
// Each form also on K-MAJOR IMAGES (FPQ_A6W4_KM; include/fpq.h): gemm_a6w4_km_kernel, gemm_a6w4_fc1_km_kernel - the activation
// side's 6-bit image, the FP4 GEMM's dealt weight image and both fp32 scale images, so that one stored k-major FP4 weight
// serves both GEMMs as the row-major one does.  Same main loop, same epilogues, same bits.
// gemm_a6w4_fc1x_kernel / gemm_a6w4_fc1x_km_kernel (FPQ_A6W4_FC1 == 2): the fc1 kernels with the tail of a dual pair that has no global
// clamp (fpq_gemm_a6w4_gelu_dual_pair with INT- / E2M3+): a NaN stays out of its group's maxima.  The fc1 kernels themselves are untouched.
// mat_qkv's two output forms (FPQ_A6W4_OUT; include/fpq.h, fpq_gemm_a6w4_mx_split / _split_qknorm), row-major and on k-major images:
// gemm_a6w4_split_kernel / gemm_a6w4_split_km_kernel write the plain epilogue's values to the parts' own destinations,
// gemm_a6w4_qkn_kernel / gemm_a6w4_qkn_km_kernel with the q / k L2 norm in front.  Only the register epilogue differs.  They are
// instantiated for fp32 weight scales only - what quantize_mx and FP4Linear hold, and what the km kernels take anyway; the entry
// points refuse fp16 ones (FPQ_ERR_DTYPE): 16 kernels instead of 24 in a unit whose compile time is the build's longest but one.
#define FPQ_A6W4_OUT 0
#define FPQ_A6W4_KM 0
#define FPQ_A6W4_KERNEL gemm_a6w4_kernel
#define FPQ_A6W4_FC1 0
#include "fpq_gemm_a6w4_kernel.h"
#undef FPQ_A6W4_KERNEL
#undef FPQ_A6W4_FC1
#define FPQ_A6W4_KERNEL gemm_a6w4_fc1_kernel
#define FPQ_A6W4_FC1 1
#include "fpq_gemm_a6w4_kernel.h"
#undef FPQ_A6W4_KERNEL
#undef FPQ_A6W4_FC1
#define FPQ_A6W4_KERNEL gemm_a6w4_fc1x_kernel
#define FPQ_A6W4_FC1 2
#include "fpq_gemm_a6w4_kernel.h"
#undef FPQ_A6W4_KERNEL
#undef FPQ_A6W4_FC1
#undef FPQ_A6W4_KM
#define FPQ_A6W4_KM 1
#define FPQ_A6W4_KERNEL gemm_a6w4_km_kernel
#define FPQ_A6W4_FC1 0
#include "fpq_gemm_a6w4_kernel.h"
#undef FPQ_A6W4_KERNEL
#undef FPQ_A6W4_FC1
#define FPQ_A6W4_KERNEL gemm_a6w4_fc1_km_kernel
#define FPQ_A6W4_FC1 1
#include "fpq_gemm_a6w4_kernel.h"
#undef FPQ_A6W4_KERNEL
#undef FPQ_A6W4_FC1
#define FPQ_A6W4_KERNEL gemm_a6w4_fc1x_km_kernel
#define FPQ_A6W4_FC1 2
#include "fpq_gemm_a6w4_kernel.h"
#undef FPQ_A6W4_KERNEL
#undef FPQ_A6W4_FC1
#define FPQ_A6W4_FC1 0
#undef FPQ_A6W4_OUT
#define FPQ_A6W4_KERNEL gemm_a6w4_split_km_kernel
#define FPQ_A6W4_OUT 1
#include "fpq_gemm_a6w4_kernel.h"
#undef FPQ_A6W4_KERNEL
#undef FPQ_A6W4_OUT
#define FPQ_A6W4_KERNEL gemm_a6w4_qkn_km_kernel
#define FPQ_A6W4_OUT 2
#include "fpq_gemm_a6w4_kernel.h"
#undef FPQ_A6W4_KERNEL
#undef FPQ_A6W4_KM
#define FPQ_A6W4_KM 0
#undef FPQ_A6W4_OUT
#define FPQ_A6W4_KERNEL gemm_a6w4_split_kernel
#define FPQ_A6W4_OUT 1
#include "fpq_gemm_a6w4_kernel.h"
#undef FPQ_A6W4_KERNEL
#undef FPQ_A6W4_OUT
#define FPQ_A6W4_KERNEL gemm_a6w4_qkn_kernel
#define FPQ_A6W4_OUT 2
#include "fpq_gemm_a6w4_kernel.h"
#undef FPQ_A6W4_KERNEL
#undef FPQ_A6W4_OUT
#undef FPQ_A6W4_FC1
#undef FPQ_A6W4_KM

template <int MT, int NT>
struct GemmA6W4Cfg {
  static constexpr int BM = 32 * MT, BN = 32 * NT;
  static size_t lds(int G) {   // two stages (96 B per activation row, 64 per weight row) + the scale tiles, groups rounded up to four
    return 2 * ((size_t)BM * 96 + (size_t)BN * 64) + (size_t)((G + 3) & ~3) * (BM + BN) * 4;
  }
  static size_t lds_fc1(int G, int shift) { return lds(G) + ((size_t)2 << (16 - shift)); }   // + the dual quantizer's bucket table
};
