// fpq_gemm_fp6.h - the row-scaled GEMM of fpq_gemm_fp8.h with the operands in the 6-bit packed form of the same
// matrix instruction (cbsz = blgp = 2, FP6 E2M3): 96 bytes per row and 128-element K step instead of 128, i.e. 25 %
// less LDS-DMA and fragment traffic in a kernel that is bound by exactly that.  Included after fpq_gemm_fp8.h.
//
// The instruction selects the format of each operand separately: FA (cbsz) decodes the A operand = the ACTIVATION fragment `af`,
// FB (blgp) the B operand = the WEIGHT fragment `bf[n]`; 2 = FP6 E2M3, 3 = BF6 E3M2 (sign, 3 exponent bits with bias 3, 2 mantissa
// bits), both in the same dense 6-bit packing.  Nothing else in the kernel depends on the format: the LDS image, the chunk
// rotation, km6_off, the dealt weight order and the 96-byte segments are properties of the packing.  The kernel's text is
// fpq_gemm_fp6_kernel.h, compiled as gemm_fp6_rows_kernel for (2, 2) and as gemm_fp6_rows_bf6_kernel<.., FA, FB> for the other pairs.
//
// Operand layout, probed on hardware (tools/probe/mfma_fp6_probe.hip): lane l supplies row l & 15, k-block l >> 4 =
// 32 consecutive elements as a 192-bit little-endian string, element j in bits [6j, 6j+6): sign, 2 exponent bits
// (bias 1), 3 mantissa bits - which is just the dense 6-bit packing of the row, 24 bytes per k-block.
//
// LDS image: 32-row "super-blocks" of 96-byte rows (3072 B = three 1 KiB LDS-DMA pieces; piece p, lane j -> 16-byte
// chunk p*64 + j of the super-block = row ci / 6, physical chunk ci % 6).  Physical chunk pc of row r holds logical
// chunk (pc - rot(r)) mod 6, rot(r) = (r >> 3) & 1 (found by exhaustive search): the three ds_read_b64 of a fragment
// (bytes 24*kb + 8t of row l & 15) are conflict-free in both 32-lane groups.
#pragma once

FPQ_NOPK __device__ __forceinline__ int fp6_rot(int r) { return (r >> 3) & 1; }
// The fragment reads MUST stay ds_read_b64 (two 32-lane groups, 64 banks: the layout above is conflict-free for exactly that
// instruction).  Left as plain loads, the compiler pairs the reads of tile rows 1536 bytes apart into ds_read2st64_b64 - two
// accesses served in 16-lane groups over 32 banks (MI355X_MICROARCH.md, LDS) - which conflict: rounds 1 - 4 ran with six of
// them per K step, SQ_LDS_BANK_CONFLICT = 48 cycles per step = 1.5 per MFMA (profiles/r04_pmc_gemm6.txt; the FP4 / FP8 GEMMs
// read 16 bytes with ds_read_b128, which has no paired form).  A volatile access is not merged.
// (spelled with the LDS address space: a volatile access through a generic pointer becomes a flat load)
typedef const volatile __attribute__((address_space(3))) u32x2* fpq_lds_v64_ptr;
#define FPQ_LDS_READ64(ptr) (*(fpq_lds_v64_ptr)(const __attribute__((address_space(3))) void*)(ptr))

// -DFPQ_GEMM6_STAMPS: diagnostic build (tools/build_variant.sh --gemm stamps6 -DFPQ_GEMM6_STAMPS, tools/gemm6_stamps.py): s_memtime
// stamps between the phases of a K step, summed per wavefront in scalar registers and written once at the end to a buffer of
// their own (fpq_debug_gemm6_stamp_buffer; no output value depends on them): where a wavefront's step time goes.  Each stamp
// waits for the scalar-memory counter, which the LDS reads share: read the SHARES.  No stamp executes in a regular build.
#ifdef FPQ_GEMM6_STAMPS
__device__ unsigned long long* g_gemm6_stamps;   // [wavefronts][8]: wait for the stage, barrier, LDS-DMA issue, fragments + MFMAs, prologue, epilogue, steps
#define FPQ_ST6(k)                                                   \
  do {                                                               \
    __builtin_amdgcn_sched_barrier(0);                               \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();      \
    __builtin_amdgcn_sched_barrier(0);                               \
    st6_sum[k] += t_ - st6_last;                                     \
    st6_last = t_;                                                   \
  } while (0)
#else
#define FPQ_ST6(k) do { } while (0)
#endif

struct GemmSplit {};
// FP6 E2M3 on both sides: the W6A6 run configuration - name, template parameters and text as before the formats could be chosen
#define FPQ_GEMM6_TEMPLATE template <typename Tsa, typename Tsw, int MT, int NT, typename XE = GemmNoFc1>
#define FPQ_GEMM6_KERNEL gemm_fp6_rows_kernel
#define FPQ_GEMM6_FA 2
#define FPQ_GEMM6_FB 2
#include "fpq_gemm_fp6_kernel.h"
#undef FPQ_GEMM6_TEMPLATE
#undef FPQ_GEMM6_KERNEL
#undef FPQ_GEMM6_FA
#undef FPQ_GEMM6_FB
// a pair with a BF6 E3M2 side: (FA, FB) = (3, 2) E3M2 activations x E2M3 weights, (2, 3), (3, 3)
#define FPQ_GEMM6_TEMPLATE template <typename Tsa, typename Tsw, int MT, int NT, typename XE, int FA, int FB>
#define FPQ_GEMM6_KERNEL gemm_fp6_rows_bf6_kernel
#define FPQ_GEMM6_FA FA
#define FPQ_GEMM6_FB FB
#include "fpq_gemm_fp6_kernel.h"
#undef FPQ_GEMM6_TEMPLATE
#undef FPQ_GEMM6_KERNEL
#undef FPQ_GEMM6_FA
#undef FPQ_GEMM6_FB
// the squared-error tail (XE = GemmSqErr only; include/fpq.h, fpq_gemm_f6_rows_sqerr), any format pair: a name of its own, so
// that the two above keep exactly the instantiations they had
#define FPQ_GEMM6_TEMPLATE template <typename Tsa, typename Tsw, int MT, int NT, typename XE, int FA, int FB>
#define FPQ_GEMM6_KERNEL gemm_f6_rows_sqerr_kernel
#define FPQ_GEMM6_FA FA
#define FPQ_GEMM6_FB FB
#include "fpq_gemm_fp6_kernel.h"
#undef FPQ_GEMM6_TEMPLATE
#undef FPQ_GEMM6_KERNEL
#undef FPQ_GEMM6_FA
#undef FPQ_GEMM6_FB

template <int MT, int NT>
struct GemmFp6Cfg {
  static constexpr int BM = 32 * MT, BN = 32 * NT;
  static size_t lds() {
    return 2 * (size_t)(BM + BN) * 96 + (size_t)(BM + 2 * BN) * 4;   // two stages + row scales, column scales, bias as fp32
  }
};
