// fpq_gemm_fp6_kernel.h - the text of the row-scaled FP6 GEMM kernel.  NOT a header of its own: fpq_gemm_fp6.h includes it once per
// kernel it defines, with
//   FPQ_GEMM6_TEMPLATE   the template head (Tsa, Tsw: scale dtypes; MT, NT: 16-row tiles per wavefront; XE: the epilogue)
//   FPQ_GEMM6_KERNEL     the kernel's name
//   FPQ_GEMM6_FA / _FB   the MFMA's format selectors: cbsz decodes A = the activation fragment `af`, blgp decodes B = the weight
//                        fragment `bf[n]`; 2 = FP6 E2M3, 3 = BF6 E3M2
// (one text, compiled under two names, instead of one template with two more parameters: the E2M3 x E2M3 kernel keeps the symbol
// and, instruction for instruction, the machine code it had before the formats could be chosen - a body shared through an
// inlined function did not: profiles/r08_bf6_isa.txt)
//
// XE = GemmNoFc1: the plain epilogue (+ gate / residual tail); XE = GemmSplit: the split output (GemmEpi's sp_* fields);
// XE = GemmQkNorm: the split output with the q / k norm (fpq_gemm_fp4.h), as in gemm_fp4_glds_kernel; XE = GemmSqErr: the
// squared-error tail (fpq_gemm_fp4.h) - compiled under a third name, gemm_f6_rows_sqerr_kernel, for all four format pairs.
FPQ_GEMM6_TEMPLATE
__global__ __launch_bounds__(256, 2) FPQ_NOPK void FPQ_GEMM6_KERNEL(const uint8_t* __restrict__ A,
                                                                   const Tsa* __restrict__ sa,
                                                                   const uint8_t* __restrict__ W,
                                                                   const Tsw* __restrict__ sw,
                                                                   const _Float16* __restrict__ bias,
                                                                   _Float16* out, int T, int O, int C, GemmEpi epi, XE xe) {
  constexpr bool SPLIT = __is_same(XE, GemmSplit), QKN = __is_same(XE, GemmQkNorm);
  constexpr int WR = 2, WC = 2, BM = 16 * MT * WR, BN = 16 * NT * WC;
  static_assert((FPQ_GEMM6_FA == 2 || FPQ_GEMM6_FA == 3) && (FPQ_GEMM6_FB == 2 || FPQ_GEMM6_FB == 3), "operand formats: 2 = FP6 E2M3, 3 = BF6 E3M2");
  static_assert(BM % 32 == 0 && BN % 32 == 0, "tiles are made of 32-row super-blocks");
  constexpr int ASB = BM / 32, BSB = BN / 32, NSB = ASB + BSB, STAGE = NSB * 3072;
  constexpr int NPIECE = 3 * NSB;
  static_assert(NPIECE % 4 == 0 && NPIECE / 4 < 16, "pieces are dealt round-robin to the four wavefronts");
  constexpr int PIECES = NPIECE / 4;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int steps = C >> 7, row_bytes = (C >> 2) * 3;
  FPQ_GEMM_TILE_WALK(BM, BN);   // fpq_gemm_fp4.h
#ifdef FPQ_GEMM6_STAMPS
  unsigned long long st6_sum[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long st6_last = __builtin_amdgcn_s_memtime();
#endif

  // LDS-DMA sources: scalar base per operand + 32-bit lane offset, in assembly with explicit waits (as in gemm_fp4_glds_kernel)
  static_assert((3 * ASB) % 4 == 0, "the A / W boundary falls between two rounds of the four wavefronts");
  constexpr int APIECES = 3 * ASB / 4;              // a wavefront's pieces i < APIECES are rows of A
  // K-major images (epi.km_w_rows != 0, as in gemm_fp4_glds_kernel): plane s holds every row's 96 bytes of K step s, [steps][rows][96],
  // chunks already rotated as in the LDS image, weight rows in dealt order: a super-block's three pieces are 3 KiB contiguous
  // (70 against 100 - 150 cycles to issue a piece; profiles/r05_lds_dma_issue.txt, r05_gemm6_stamps.txt).
  const bool km = epi.km_w_rows != 0;
  const int row_stride = km ? 96 : row_bytes;
  const int64_t a_step = km ? (int64_t)T * 96 : 96, w_step = km ? (int64_t)epi.km_w_rows * 96 : 96;
  const uint8_t* const gbase[2] = {A + (int64_t)t0 * row_stride, W + (int64_t)o0 * row_stride};
  const int w_rows = km ? epi.km_w_rows : O;
  uint32_t voff[PIECES];
#pragma unroll
  for (int i = 0; i < PIECES; ++i) {
    const int piece = wave + 4 * i;                 // super-block piece / 3, part piece % 3
    const int sb = piece / 3, ci = (piece % 3) * 64 + lane;
    const int r = ci / 6, pc = ci - 6 * r;          // row inside the super-block, physical chunk
    int c = pc - fp6_rot(r);
    c = c < 0 ? c + 6 : c;                          // logical chunk this lane fetches
    c = km ? pc : c;                                // (the image holds the rotated order)
    if (sb < ASB) {
      const int t = t0 + sb * 32 + r;
      voff[i] = (uint32_t)((t < T ? t : T - 1) - t0) * (uint32_t)row_stride + (uint32_t)(c * 16);
    } else {
      const int ti = 2 * (sb - ASB) + (r >> 4);      // 16-row tile of the weight side; its rows are dealt over a wavefront's
      const int o = km ? o0 + (sb - ASB) * 32 + r : o0 + (ti / NT) * (16 * NT) + NT * (r & 15) + ti % NT;   // NT tiles (FPQ_GEMM_ROWS_EPILOGUE)
      voff[i] = (uint32_t)((o < w_rows ? o : w_rows - 1) - o0) * (uint32_t)row_stride + (uint32_t)(c * 16);
    }
  }
#define FPQ_GLDS6_ONE(s, buf, i_)                                                                                   \
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"                                     \
               :                                                                                                    \
               : "v"(voff[i_]), "s"(gbase[(i_) < APIECES ? 0 : 1] + (s) * ((i_) < APIECES ? a_step : w_step)),                                      \
                 "s"((uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(smem + (buf) * STAGE +         \
                                                                                   (wave + 4 * (i_)) * 1024))      \
               : "m0")
#define FPQ_GLDS6_ISSUE(s, buf) _Pragma("unroll") for (int i_ = 0; i_ < PIECES; ++i_) FPQ_GLDS6_ONE(s, buf, i_)
  FPQ_GLDS6_ISSUE(0, 0);
  FPQ_GEMM_ROWS_STAGE_SCALES(STAGE);
  v4f_t qkn_b = v4f_t{0, 0, 0, 0};   // (QKN) the fp32 bias of the lane's four outputs and s_h of the wavefront's head in part 0, requested here
  float qkn_s = 1.0f;
  if constexpr (QKN) {
    const int o = o0 + wn * (16 * NT) + NT * (lane & 15);
    if (xe.bias) qkn_b = *(const v4f_t*)(xe.bias + (o < O ? o : O - 4));
    if (o0 < epi.sp_cols) qkn_s = xe.q_scale[(o0 + wn * (16 * NT)) >> 6];
  }

  v4f_t acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = v4f_t{0, 0, 0, 0};

  // the three 8-byte pieces of this lane's fragment inside a 16-row half of a super-block
  const int fr = lane & 15, kb = lane >> 4;
  int foff[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int b = kb * 24 + 8 * t;
    int pc = (b >> 4) + fp6_rot(fr);
    pc = pc >= 6 ? pc - 6 : pc;
    foff[t] = fr * 96 + pc * 16 + (b & 15);
  }
  const int a_base = wm * MT * 1536, b_base = ASB * 3072 + wn * NT * 1536;   // tile row mt -> 1536 * mt (two per super-block)

  // Two LDS stages, one barrier per step; the LDS-DMA pieces of step s+1 are issued in one burst behind the barrier.
  // History of that choice on mat_qkv [65536 x 1920 -> 5760] (ms): with the compiler's form of the load (per-lane 64-bit
  // pointers) the burst measured 0.81 and one piece after every third MFMA 0.75 - 0.79, so rounds 1 - 3 interleaved;
  // with scalar base + lane offset in assembly (round 4) the burst is the faster one: 0.627 interleaved, 0.603 burst.
  // Also measured: register staging (global_load + ds_write) 0.85 - 0.88, a three-stage ring with counted vmcnt 0.92,
  // requesting tile row m + 1's fragment before the MFMAs of row m (no gain: the SIMD's second wavefront covers it).
  FPQ_ST6(4);
  for (int s = 0; s < steps; ++s) {
    FPQ_GLDS_WAIT();   // the compiler does not see the LDS-DMA loads
    FPQ_ST6(0);
    FPQ_SYNC();   // stage s has landed; the other buffer's readers are done
    FPQ_ST6(1);
    const uint8_t* st = smem + (s & 1) * STAGE;
    if (s + 1 < steps) { FPQ_GLDS6_ISSUE(s + 1, (s + 1) & 1); }   // (one piece behind every third MFMA instead: re-measured on k-major operands, profiles/r05_kmajor_ab.txt)
    FPQ_ST6(2);
    v8i_t bf[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const uint8_t* p = st + b_base + n * 1536;
      const u32x2 q0 = FPQ_LDS_READ64(p + foff[0]), q1 = FPQ_LDS_READ64(p + foff[1]), q2 = FPQ_LDS_READ64(p + foff[2]);
      bf[n] = v8i_t{(int)q0[0], (int)q0[1], (int)q1[0], (int)q1[1], (int)q2[0], (int)q2[1], 0, 0};
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const uint8_t* p = st + a_base + m * 1536;
      const u32x2 q0 = FPQ_LDS_READ64(p + foff[0]), q1 = FPQ_LDS_READ64(p + foff[1]), q2 = FPQ_LDS_READ64(p + foff[2]);
      const v8i_t af = v8i_t{(int)q0[0], (int)q0[1], (int)q1[0], (int)q1[1], (int)q2[0], (int)q2[1], 0, 0};
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bf[n], acc[m][n], FPQ_GEMM6_FA, FPQ_GEMM6_FB, 0, 0, 0, 0);   // cbsz: format of af, blgp: of bf; unscaled
        // a scheduling fence after every third MFMA - where the interleaved form issued its pieces: without the fences the
        // compiler's order of the rows' ds_reads and MFMAs is 5 % slower (0.635 against 0.603 ms), measured both ways
        // (a fence after every MFMA, every second or every fourth measures the same; in the FP8 kernel fences cost 2 %)
        if ((m * NT + n) % 3 == 2) {
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    FPQ_ST6(3);
  }
#undef FPQ_GLDS6_ISSUE
#undef FPQ_GLDS6_ONE
  if constexpr (__is_same(XE, GemmSqErr)) {   // scratch: the stage buffer the last K step did not read
    FPQ_GEMM_ROWS_EPILOGUE_SQERR(smem + (steps & 1) * STAGE);
  } else if constexpr (SPLIT || QKN) {
    FPQ_GEMM_ROWS_EPILOGUE_SPLIT(QKN, qkn_b, qkn_s);
  } else {
    FPQ_GEMM_ROWS_EPILOGUE();
  }
#ifdef FPQ_GEMM6_STAMPS
  FPQ_ST6(5);
  if (lane == 0 && g_gemm6_stamps) {
    unsigned long long* dst = g_gemm6_stamps + ((int64_t)blockIdx.x * 4 + wave) * 8;
#pragma unroll
    for (int k = 0; k < 6; ++k) dst[k] = st6_sum[k];
    dst[6] = (unsigned long long)steps;
    dst[7] = 1;
  }
#endif
}
