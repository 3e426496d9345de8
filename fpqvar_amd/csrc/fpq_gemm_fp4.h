// fpq_gemm_fp4.h - F2: a REAL low-precision consumer for the quantized
// activations and weights.  Included by fpq_gemm.hip inside its anonymous namespace (the operand-emitting quantizer: fpq_codes_mx.h).
//
// The reference fake-quantizes and then runs an fp16 GEMM on the de-quantized tensors
// (tr/quant_utils.py:765-767: F.linear(act_quant(x), W_q)).  With per-group(128) FP4-E2M1 on both
// sides the same product is
//     y[t,o] = sum_g  s_a[t,g] * s_w[o,g] * ( sum_{k in g} La[t,k] * Lw[o,k] )
// and the inner 128-term dot product of FP4 levels is exactly ONE gfx950 block-scaled MFMA
// (v_mfma_scale_f32_16x16x128_f8f6f4, FP4 operands, unit E8M0 scales): exact products, fp32
// accumulation.  The two per-group scales (arbitrary fp16/fp32 numbers, not powers of two) are
// applied to the 16x16 partial tile in the packed-fp32 VALU.
//
// Operand layout (probed on hardware, tools/probe/mfma_fp4_probe.hip): lane l supplies row l&15
// of A (column l&15 of B), k-block l>>4 = 32 consecutive k as 32 nibbles (16 bytes, low nibble
// first); D: column l&15, rows 4*(l>>4) + reg.  Nibble = OCP E2M1: bit 3 sign, bits 2:0 magnitude
// index into {0, .5, 1, 1.5, 2, 3, 4, 6}.
//
// Numerics: more exact than the reference (it rounds every de-quantized value to fp16 before its
// GEMM); the parity contract for this entry point is a tolerance, not bit equality.
#pragma once

typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef float v4f_t __attribute__((ext_vector_type(4)));
typedef float v2f_t __attribute__((ext_vector_type(2)));

// Byte offset of (row, 16-byte chunk kb) in the LDS image of an operand tile (64 B per row).
// ds_read_b128 serves a wavefront in four fixed 16-lane groups - {0-3,12-15,20-27}, {4-11,16-19,28-31} and
// the same +32 (MI355X_MICROARCH.md, LDS) - and with lane = (kb << 4) | row each group mixes two k-blocks.
// Layout: per 16 rows one 1 KiB block = 4 planes (one per kb) of 16 slots; row r sits in slot
// (r&3)*4 + (r>>2) of its plane, planes 2 and 3 rotated by two slots.  Every read group then covers 16
// distinct 16-byte slots (conflict-free); the staging writes (4 lanes per row) are 2-way.
__device__ __forceinline__ int gemm_lds_off(int row, int kb) {
  const int r = row & 15;
  return ((row >> 4) << 10) + (kb << 8) + (((((r & 3) << 2) + (r >> 2) + ((kb >> 1) << 1)) & 15) << 4);
}

// Workgroup = WR x WC wavefronts, each owning MT x NT MFMA tiles (16x16): tile BM = 16*MT*WR tokens by
// BN = 16*NT*WC outputs.
// Optional tail of every GEMM epilogue below: out = residual + y * gate[t / rows_per_gate, :] with y the fp16 Linear
// output, each operation in fp16 with one rounding - what torch computes for the AdaLN blocks'
// `x = x + attn(...).mul_(gamma1)` / `x + ffn(...).mul(gamma2)` (tr/basic_var.py:264,267; gamma is [B, 1, C]).
struct GemmEpi {
  const _Float16* gate;    // [ceil(T / rows_per_gate), O] or nullptr
  const _Float16* resid;   // [T, O] or nullptr; may alias out
  int rows_per_gate;
  // K-MAJOR OPERAND IMAGES (include/fpq.h, "k-major operand images"; the FP4 and FP6 LDS-DMA kernels): 0 = row-major codes,
  // else the image rows of the weight side (outs rounded up to 64; the activation side has exactly T).
  int km_w_rows;
  // SPLIT OUTPUT (include/fpq.h, fpq_gemm_split_t; the FP4 LDS-DMA kernel's plain epilogue, the FP6 kernel's GemmSplit / GemmQkNorm): sp_cols != 0: the outputs are sp_cols-wide
  // column parts with a destination each - token t = b * sp_rpb + l of part p goes to row b * sp_bstride[p] + sp_row0[p] + l of
  // sp_out[p] (sp_stride[p] elements per row).  mat_qkv writes q to its own tensor and k, v straight into the KV cache's slots.
  int sp_cols, sp_rpb;
  _Float16* sp_out[3];
  int64_t sp_stride[3], sp_bstride[3], sp_row0[3];
};
typedef _Float16 fpq_h2_t __attribute__((ext_vector_type(2)));
typedef _Float16 fpq_h4_t __attribute__((ext_vector_type(4)));

// b4: the lane's fp16 bias (bias_h, FPQ_GEMM_LANE_BIAS) widened where the register epilogues and the fc1 tail add it
#define FPQ_GEMM_BIAS_F32()                                                                                         \
  v4f_t b4 = v4f_t{0, 0, 0, 0};                                                                                     \
  _Pragma("unroll") for (int n = 0; n < NT; ++n) b4[n] = (float)bias_h[n]

// The four 8-byte stores of a lane (rows t_first .. +3, outputs o .. o+3)
#define FPQ_GEMM_ROWS_STORE(y_, t_first_, tc_, o_, oc_)                                                             \
  do {                                                                                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                                \
        if ((t_first_) + i_ < T && (o_) < O)                                                                        \
          __builtin_nontemporal_store(__builtin_bit_cast(u32x2, (y_)[i_]), (u32x2*)(out + (int64_t)(tc_)[i_] * O + (oc_))); \
  } while (0)

// The gate / residual tail of the register epilogues (gemm_fp4_glds_kernel, gemm_a6w4_kernel, FPQ_GEMM_ROWS_EPILOGUE), written
// once.  _SETUP in front of the loop over the tile rows: a gate row that spans at least the wavefront's WROWS_ rows costs ONE
// division per tile (gq0_, gr0_) and a comparison per row instead of a division per row - 32 of them were a fifth of a tile's
// vector instructions.  _ROWS for tile row m_: y_ = fpq_h4_t[4] (rows tc_[0..3], clamped to T - 1; outputs oc_ .. oc_ + 3) becomes
// resid + y_ * gate.  Loads are unconditional on clamped rows.  Names from the kernel: epi, t0, wm, lane, T, O.
#define FPQ_GEMM_GATE_SETUP(WROWS_)                                                                                 \
  const bool gate_far_ = epi.gate && epi.rows_per_gate >= (WROWS_);                                                 \
  int gq0_ = 0, gr0_ = 0, gq_last_ = 0;                                                                             \
  if (epi.gate) {                                                                                                   \
    const int gfirst_ = t0 + wm * (WROWS_) + 4 * (lane >> 4);                                                       \
    gq0_ = gfirst_ / epi.rows_per_gate;                                                                             \
    gr0_ = gfirst_ - gq0_ * epi.rows_per_gate;                                                                      \
    gq_last_ = (T - 1) / epi.rows_per_gate;                                                                         \
  }
#define FPQ_GEMM_GATE_RESID_ROWS(y_, tc_, m_, oc_)                                                                  \
  do {                                                                                                              \
    if (epi.gate) {                                                                                                 \
      fpq_h4_t gt_[4];                                                                                              \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                            \
        const int goff_ = gr0_ + (m_) * 16 + i_;                                                                    \
        int gq_ = gate_far_ ? gq0_ + (goff_ >= epi.rows_per_gate ? 1 : 0) : (tc_)[i_] / epi.rows_per_gate;          \
        gq_ = gq_ < gq_last_ ? gq_ : gq_last_;                                                                      \
        gt_[i_] = *(const fpq_h4_t*)(epi.gate + (int64_t)gq_ * O + (oc_));                                          \
      }                                                                                                             \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) (y_)[i_] = (y_)[i_] * gt_[i_];                               \
    }                                                                                                               \
    if (epi.resid) {                                                                                                \
      fpq_h4_t rs_[4];                                                                                              \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) rs_[i_] = *(const fpq_h4_t*)(epi.resid + (int64_t)(tc_)[i_] * O + (oc_)); \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) (y_)[i_] = rs_[i_] + (y_)[i_];                               \
    }                                                                                                               \
  } while (0)

// The split output (GemmEpi's sp_* fields) of gemm_fp4_glds_kernel and FPQ_GEMM_ROWS_EPILOGUE_SPLIT, written once.  A tile lies
// inside ONE part (sp_cols % 128 == 0).  _SETUP in front of the loop over the tile rows: the part's destination, and the batch
// entry / row of the wavefront's first row - one division per tile while a batch entry spans the wavefront's WROWS_ rows.
// on_: whether the output is split at all (the FP4 kernel's plain epilogue serves both: epi.sp_cols; the split epilogue: true).
// _STORE: row i_ of tile row m_ (token t_first_ + i_) goes out as one non-temporal 8-byte store; t_ is the token a row that does
// NOT span a batch entry is divided from - each kernel's own expression (clamped in the FP4 kernel, plain in the row-scaled ones).
#define FPQ_GEMM_SPLIT_SETUP(WROWS_, on_)                                                                           \
  const int sp_part_ = (on_) ? o0 / epi.sp_cols : 0;                                                                \
  _Float16* const sp_base_ = sp_part_ == 0 ? epi.sp_out[0] : sp_part_ == 1 ? epi.sp_out[1] : epi.sp_out[2];         \
  const int64_t sp_stride_ = sp_part_ == 0 ? epi.sp_stride[0] : sp_part_ == 1 ? epi.sp_stride[1] : epi.sp_stride[2]; \
  const int64_t sp_bstride_ = sp_part_ == 0 ? epi.sp_bstride[0] : sp_part_ == 1 ? epi.sp_bstride[1] : epi.sp_bstride[2]; \
  const int64_t sp_row0_ = sp_part_ == 0 ? epi.sp_row0[0] : sp_part_ == 1 ? epi.sp_row0[1] : epi.sp_row0[2];        \
  const bool sp_far_ = (on_) && epi.sp_rpb >= (WROWS_);                                                             \
  int sb0_ = 0, sr0_ = 0;                                                                                           \
  if (on_) {                                                                                                        \
    const int sfirst_ = t0 + wm * (WROWS_) + 4 * (lane >> 4);                                                       \
    sb0_ = sfirst_ / epi.sp_rpb;                                                                                    \
    sr0_ = sfirst_ - sb0_ * epi.sp_rpb;                                                                             \
  }
#define FPQ_GEMM_SPLIT_STORE(y_, m_, i_, t_, t_first_, o_, oc_l_)                                                   \
  do {                                                                                                              \
    const int soff_ = sr0_ + (m_) * 16 + (i_);                                                                      \
    int bb_, ll_;                                                                                                   \
    if (sp_far_) {                                                                                                  \
      const int wrap_ = soff_ >= epi.sp_rpb ? 1 : 0;                                                                \
      bb_ = sb0_ + wrap_;                                                                                           \
      ll_ = soff_ - wrap_ * epi.sp_rpb;                                                                             \
    } else {                                                                                                        \
      bb_ = (t_) / epi.sp_rpb;                                                                                      \
      ll_ = (t_) - bb_ * epi.sp_rpb;                                                                                \
    }                                                                                                               \
    if ((t_first_) + (i_) < T && (o_) < O)                                                                          \
      __builtin_nontemporal_store(__builtin_bit_cast(u32x2, (y_)),                                                  \
                                  (u32x2*)(sp_base_ + ((int64_t)bb_ * sp_bstride_ + sp_row0_ + ll_) * sp_stride_ + (oc_l_))); \
  } while (0)

// (macros, not functions: the kernels carry different target attributes and a callee is only inlined into a kernel
// with the same ones)
#define FPQ_GEMM_EPI_VEC(y, e, t, o, O)                                                                \
  do {                                                                                                   \
    if ((e).gate) {                                                                                      \
      const u32x4 g_ = *(const u32x4*)((e).gate + (int64_t)((t) / (e).rows_per_gate) * (O) + (o));       \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                   \
          (y)[i_] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(fpq_h2_t, (uint32_t)(y)[i_]) *      \
                                                     __builtin_bit_cast(fpq_h2_t, (uint32_t)g_[i_]));    \
    }                                                                                                    \
    if ((e).resid) {                                                                                     \
      const u32x4 r_ = *(const u32x4*)((e).resid + (int64_t)(t) * (O) + (o));                            \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                   \
          (y)[i_] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(fpq_h2_t, (uint32_t)r_[i_]) +       \
                                                     __builtin_bit_cast(fpq_h2_t, (uint32_t)(y)[i_]));   \
    }                                                                                                    \
  } while (0)
#define FPQ_GEMM_EPI_ONE(y, e, t, o, O)                                                                  \
  do {                                                                                                   \
    if ((e).gate) (y) = (y) * (e).gate[(int64_t)((t) / (e).rows_per_gate) * (O) + (o)];                  \
    if ((e).resid) (y) = (e).resid[(int64_t)(t) * (O) + (o)] + (y);                                      \
  } while (0)

template <typename Tsw, int MT, int NT, int WR, int WC>
__global__ __launch_bounds__(64 * WR * WC) void gemm_fp4_kernel(const uint8_t* __restrict__ A,
                                                               const _Float16* __restrict__ sa,
                                                               const uint8_t* __restrict__ W, const Tsw* __restrict__ sw,
                                                               const _Float16* __restrict__ bias,
                                                               _Float16* out, int T, int O, int C, GemmEpi epi) {
  constexpr int BM = 16 * MT * WR, BN = 16 * NT * WC, NTHR = 64 * WR * WC;
  constexpr int ABYTES = BM * 64, BBYTES = BN * 64, STAGE = ABYTES + BBYTES;
  constexpr int HA = (BM * 4 + NTHR - 1) / NTHR, HB = (BN * 4 + NTHR - 1) / NTHR;   // staging chunks per thread
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int G = C >> 7, row_bytes = C >> 1;
  uint8_t* lAB = smem;                              // [2][A | B]
  float* lsa = (float*)(smem + 2 * STAGE);          // [G][BM]
  float* lsw = lsa + G * BM;                        // [G][BN]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WC, wn = wave % WC;
  // XCD-aware tile order (workgroups are dealt round-robin over the 8 XCDs, each with its own 4 MiB L2):
  // XCD k owns a contiguous band of `cpx` column tiles and walks all row tiles of that band, so its
  // slice of W stays L2-resident and an A tile is re-used by cpx consecutive workgroups.
  const int n_col = (O + BN - 1) / BN, n_row = (T + BM - 1) / BM;
  const int cpx = (n_col + 7) >> 3;
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int col_blk = xcd * cpx + local % cpx, row_blk = local / cpx;
  if (col_blk >= n_col || row_blk >= n_row) return;   // uniform over the workgroup
  const int t0 = row_blk * BM, o0 = col_blk * BN;

  // scales of this tile, transposed to [g][row] and widened to fp32
  for (int i = tid; i < G * BM; i += NTHR) {
    const int r = i % BM, g = i / BM;
    lsa[i] = (t0 + r < T) ? (float)sa[(int64_t)(t0 + r) * G + g] : 0.0f;
  }
  for (int i = tid; i < G * BN; i += NTHR) {
    const int r = i % BN, g = i / BN;
    lsw[i] = (o0 + r < O) ? (float)sw[(int64_t)(o0 + r) * G + g] : 0.0f;
  }

  v4f_t acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = v4f_t{0, 0, 0, 0};

  // staging: chunk id = h*NTHR + tid -> (row = id >> 2, kb = id & 3): 4 lanes fetch one row's 64 bytes.
  // Software pipeline: group g+2 is in flight in registers and group g+1 is being written to the other
  // LDS buffer while group g is multiplied; one barrier per group.
  // Rows past the end of A / W are clamped to the last valid row: their products land in output rows /
  // columns the epilogue never stores, and unconditional loads keep the loop free of exec-mask branches.
  static_assert((BM * 4) % NTHR == 0 && (BN * 4) % NTHR == 0, "tile chunks must divide evenly over the threads");
  const uint8_t* pa[HA];
  const uint8_t* pb[HB];
  int la[HA], lb[HB];
#pragma unroll
  for (int h = 0; h < HA; ++h) {
    const int id = h * NTHR + tid, r = id >> 2, kb = id & 3;
    const int t = t0 + r < T ? t0 + r : T - 1;
    la[h] = gemm_lds_off(r, kb);
    pa[h] = A + (int64_t)t * row_bytes + kb * 16;
  }
#pragma unroll
  for (int h = 0; h < HB; ++h) {
    const int id = h * NTHR + tid, r = id >> 2, kb = id & 3;
    const int o = o0 + r < O ? o0 + r : O - 1;
    lb[h] = gemm_lds_off(r, kb);
    pb[h] = W + (int64_t)o * row_bytes + kb * 16;
  }
  u32x4 ga[HA], gb[HB];
  auto fetch = [&](int g) {
#pragma unroll
    for (int h = 0; h < HA; ++h) ga[h] = *(const u32x4*)(pa[h] + g * 64);
#pragma unroll
    for (int h = 0; h < HB; ++h) gb[h] = *(const u32x4*)(pb[h] + g * 64);
  };
  auto stage = [&](int buf) {
    uint8_t* base = lAB + buf * STAGE;
#pragma unroll
    for (int h = 0; h < HA; ++h) *(u32x4*)(base + la[h]) = ga[h];
#pragma unroll
    for (int h = 0; h < HB; ++h) *(u32x4*)(base + ABYTES + lb[h]) = gb[h];
  };
  fetch(0);
  stage(0);
  if (G > 1) fetch(1);
  __syncthreads();   // buffer 0 and the scale tiles are visible
  for (int g = 0; g < G; ++g) {
    const uint8_t* lA = lAB + (g & 1) * STAGE;
    const uint8_t* lB = lA + ABYTES;
    if (g + 1 < G) {   // the other buffer was last read in iteration g-1, a barrier has passed since
      stage((g + 1) & 1);
      if (g + 2 < G) fetch(g + 2);
    }
    v8i_t af[MT], bf[NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const u32x4 v = *(const u32x4*)(lA + gemm_lds_off((wm * MT + m) * 16 + (lane & 15), lane >> 4));
      af[m] = v8i_t{(int)v[0], (int)v[1], (int)v[2], (int)v[3], 0, 0, 0, 0};
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const u32x4 v = *(const u32x4*)(lB + gemm_lds_off((wn * NT + n) * 16 + (lane & 15), lane >> 4));
      bf[n] = v8i_t{(int)v[0], (int)v[1], (int)v[2], (int)v[3], 0, 0, 0, 0};
    }
    v4f_t sa4[MT];
    float sw1[NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) sa4[m] = *(const v4f_t*)(lsa + g * BM + (wm * MT + m) * 16 + 4 * (lane >> 4));
#pragma unroll
    for (int n = 0; n < NT; ++n) sw1[n] = lsw[g * BN + (wn * NT + n) * 16 + (lane & 15)];
    // NT independent MFMAs per tile row, then their scale-and-accumulate in the packed-fp32 VALU: the
    // matrix pipe works on row m+1 while the VALU finishes row m
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      v4f_t d[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n)
        d[n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[m], bf[n], v4f_t{0, 0, 0, 0}, 4, 4, 0, 0, 0, 0);   // literal zero scales select the unscaled instruction (x1.0, probed)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const v4f_t p = sa4[m] * sw1[n];
        acc[m][n] = __builtin_elementwise_fma(d[n], p, acc[m][n]);
      }
    }
    __syncthreads();   // group g consumed, group g+1 staged
  }

  // epilogue: bias, fp16, transpose each wavefront tile through LDS for 16-byte row stores
  constexpr int WROWS = 16 * MT, WCOLS = 16 * NT, LDW = WCOLS + 8;
  _Float16* lo = (_Float16*)smem + wave * (WROWS * LDW);
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int col = n * 16 + (lane & 15);
      const int o = o0 + wn * WCOLS + col;
      const float b = (bias && o < O) ? (float)bias[o] : 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) lo[(m * 16 + 4 * (lane >> 4) + i) * LDW + col] = (_Float16)(acc[m][n][i] + b);
    }
  __syncthreads();
  constexpr int PIECES = WROWS * (WCOLS / 8);
#pragma unroll
  for (int pass = 0; pass < (PIECES + 63) / 64; ++pass) {
    const int piece = pass * 64 + lane;
    if (piece < PIECES) {
      const int r = piece / (WCOLS / 8), cpc = piece % (WCOLS / 8);
      const int t = t0 + wm * WROWS + r, o = o0 + wn * WCOLS + cpc * 8;
      if (t < T && o + 8 <= O) {
        u32x4 y = *(const u32x4*)(lo + r * LDW + cpc * 8);
        FPQ_GEMM_EPI_VEC(y, epi, t, o, O);
        *(u32x4*)(out + (int64_t)t * O + o) = y;
      } else if (t < T) {
        for (int e = 0; e < 8; ++e)
          if (o + e < O) {
            _Float16 y = lo[r * LDW + cpc * 8 + e];
            FPQ_GEMM_EPI_ONE(y, epi, t, o + e, O);
            out[(int64_t)t * O + o + e] = y;
          }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Second-generation kernel: operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4, no staging
// registers, no ds_write), wavefront tile 16*MT x 16*NT (128 x 64) so that one pair of fragment reads
// feeds more matrix work, two waves per SIMD.  What the measurements in tools/probe/ say about this chip:
//   * v_mfma_f32_16x16x128_f8f6f4 (FP4) issues every ~8.5 ns per SIMD (7.9 PFLOP/s chip-wide);
//   * VALU work does not hide behind it (mfma + 8 v_fma = 18.5 ns vs 8.5 + 12.1 separately), and
//     v_pk_fma_f32 costs as much as two v_fma_f32;
//   * the scaled form (v_mfma_scale_*) pays an extra VALU slot for its scale operands.
// So the per-group scale-and-accumulate (2 multiplies + 1 fma per output element and group) is the real
// bound of this formulation (~19 ns per MFMA, ~3.5 PFLOP/s), and everything else has to stay out of its way.
//
// LDS image of a 16-row x 64-byte block (1 KiB, written by ONE LDS-DMA instruction, lane j -> bytes 16j):
// lane j = 4*q + c fetches row q, 16-byte chunk c ^ pi[q >> 2], pi = (0,2,3,1): four consecutive lanes read
// one row's 64 contiguous bytes from memory, and the fragment reads (lane l: row l & 15, chunk l >> 4,
// ds_read_b128 served in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, +32) touch 16 distinct
// 16-byte slots per group (checked exhaustively offline): conflict-free on both sides.
#define FPQ_NOPK __attribute__((target("no-packed-fp32-ops")))   // callees must carry the kernel's target features to be inlined
// __syncthreads() spelled out (the header's inline function does not carry the attribute and would become a call)
#define FPQ_SYNC()                                             \
  do {                                                         \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     \
    __builtin_amdgcn_s_barrier();                              \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");     \
  } while (0)
FPQ_NOPK __device__ __forceinline__ int glds_chunk_perm(int q) { return (0x78 >> ((q >> 2) << 1)) & 3; }   // pi = 0,2,3,1

// Scale tiles -> LDS as fp32 [G][rows]: one thread per tile row (activation rows first, then weight rows) walks
// that row's G consecutive scales; rows past the end of the tensor read as zero (their outputs are never stored).
template <typename Tsw, int BM, int BN, int NTHR>
FPQ_NOPK __device__ __forceinline__ void load_scale_tiles(const _Float16* __restrict__ sa, const Tsw* __restrict__ sw, float* lsa,
                                                 float* lsw, int t0, int o0, int T, int O, int G, int tid) {
  // a row's scales in batches of GB loads, all in flight before the first is stored (round 4; batches of 5 were three
  // dependent trips to L2 for the 15 groups of C = 1920 in a prologue that every tile waits for)
#ifndef FPQ_GEMM_SCALE_BATCH
#define FPQ_GEMM_SCALE_BATCH 16
#endif
  constexpr int GB = FPQ_GEMM_SCALE_BATCH;
  for (int r = tid; r < BM + BN; r += NTHR) {
    if (r < BM) {   // wave-uniform: BM is a multiple of 64
      const bool ok = t0 + r < T;
      const _Float16* src = sa + (int64_t)(ok ? t0 + r : 0) * G;
      for (int g0 = 0; g0 < G; g0 += GB) {
        _Float16 v[GB];
#pragma unroll
        for (int i = 0; i < GB; ++i) v[i] = src[g0 + i < G ? g0 + i : G - 1];
#pragma unroll
        for (int i = 0; i < GB; ++i)
          if (g0 + i < G) lsa[(g0 + i) * BM + r] = ok ? (float)v[i] : 0.0f;
      }
    } else {
      const int c = r - BM;
      const bool ok = o0 + c < O;
      const Tsw* src = sw + (int64_t)(ok ? o0 + c : 0) * G;
      for (int g0 = 0; g0 < G; g0 += GB) {
        Tsw v[GB];
#pragma unroll
        for (int i = 0; i < GB; ++i) v[i] = src[g0 + i < G ? g0 + i : G - 1];
#pragma unroll
        for (int i = 0; i < GB; ++i)
          if (g0 + i < G) lsw[(g0 + i) * BN + c] = ok ? (float)v[i] : 0.0f;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// The fc1 tail (round 5): everything between the fc1 GEMM and fc2's GEMM in the reference's FFN
//     h  = F.gelu(fc1(x), approximate="tanh")                              tr/basic_var.py:120      (fp16 tensor, fp32 arithmetic)
//     q  = fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(h, 4, 128)            tr/quant_utils.py:415-452, bound at :991
// as the epilogue of gemm_fp4_glds_kernel: every tile is BN = 128 outputs wide and starts at a multiple of 128, i.e. it
// holds WHOLE quantization groups - one per token row - so both scales of a group are tile-local.
//   * y = half(acc + bias) exactly as the plain epilogue rounds it (the Linear output the reference's GELU sees);
//   * h = half(gelu(float(y))), gelu_tanh_fast below: within one fp16 ulp of torch's F.gelu(y, approximate="tanh") on every
//     fp16 input, checked exhaustively (tests/test_gpu_fc1_fused.py; torch's formula in torch's operation order with the
//     device library's tanh restated, tools/probe/gelu_probe.hip, is bit-equal to torch and three times the instructions);
//   * per token row the maxima of the negative and of the positive side over the lane's four outputs, the 16 lanes of the
//     row (a DPP reduce-scatter) and the two wavefronts that share the group (LDS), one thread per row turns them into the two scales
//     (row_scale16, dual_poison: the arithmetic of rows16_lut_subwave_kernel<DUAL>), and every lane quantizes its own
//     values with quant_pair16_dual = one packed pair of quant_vec16<DUAL>: bit-equal to the stand-alone quantizer on h;
//   * "any NaN in the tensor => the whole result is zero" (the reference's global clamp, tr/quant_utils.py:421-422) keeps
//     its flag + fix-up launch (fpq_kernels.hip, zero_if_flag_kernel): a row that saw a NaN raises the flag.
// LDS: the bucket table behind the scale tiles (staged in the prologue); the maxima exchange and the row scales in the
// stage buffer the last K group does not use.
struct GemmNoFc1 {};
struct GemmFc1 {
  _Float16* h_out;       // nullptr, or fp16 [T, O] receiving h (the tensor the quantizer saw)
  uint32_t* nan_flag;    // nullptr, or the 8-byte scratch of fpq_quant_rows_dual
  Lut16Args a;           // the (e1m2_neg, e2m1_pos) bucket table's arguments ...
  Lut16Tab tab;          // ... and the table itself, by value (as the stand-alone quantizers take it)
};
struct GemmFc1X : GemmFc1 {};   // host side only: selects the kernels whose tail keeps a NaN out of the maxima (FPQ_GEMM_FC1_TAIL_X)

// (the GELU itself - gelu_tanh_fast - lives in fpq_fast16.h: the stand-alone fused quantizer uses it too)

// ---------------------------------------------------------------------------------------------------
// mat_qkv of an attention block with attn_l2_norm (round 6; include/fpq.h fpq_gemm_fp4_mx_split_qknorm), the split epilogue with
//     y = float(half(acc)) + b32            the fp16 Linear output (mat_qkv has no bias), then the fp32 cat(q_bias, 0, v_bias)
//     part 0 (q): half(y / max(||y||_2, 1e-12) * s_h)      part 1 (k): half(y / max(||y||_2, 1e-12))      part 2 (v): half(y)
// per (token, head) over the head's 64 columns (tr/basic_var.py:173-183).  Lanes: a wavefront owns 64 consecutive outputs of a
// 128-aligned tile, a lane four of them (4q .. 4q + 3, see the dealt weight rows), so a token row's head is the 16 lanes of one DPP
// row - four in-lane FMAs and four DPP steps per row, no LDS, no barrier.  The quotient: a real square root, one real division per
// row (1 / n) and per element q = y (1/n) + (y - q n)(1/n) - the correctly rounded quotient but for rare ties.
struct GemmQkNorm {
  const float* bias;      // fp32 [3 * part_cols] or nullptr (16-byte aligned)
  const float* q_scale;   // fp32 [part_cols / 64]: exp(min(scale_mul_1H11, log 100))
};

// sum over the 16 lanes of a DPP row; every lane ends with the same bits (each step adds a value and its mirror image)
FPQ_NOPK __device__ __forceinline__ float row_sum16(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
  return v;
}

// The q / k norm of one (token, head) row, shared by the FP4 and FP6 GEMMs' split epilogues (include/fpq.h, "THE Q / K L2 NORM"):
// yf_ = a lane's NT consecutive values of the row (float[NT]), the 16 lanes of its DPP row hold the head's 64; q rows (part_ == 0)
// are scaled by s_h_.  (A macro: as an inlined function the same lines leave the FP4 kernel with its multiplies' operands swapped.)
#define FPQ_QK_NORM_ROW(yf_, part_, s_h_)                                                                           \
  do {                                                                                                              \
    float ss = (yf_)[0] * (yf_)[0];                                                                                 \
    _Pragma("unroll") for (int n = 1; n < NT; ++n) ss = __builtin_fmaf((yf_)[n], (yf_)[n], ss);                     \
    float nrm = __builtin_sqrtf(row_sum16(ss));                                                                     \
    nrm = nrm < 1e-12f ? 1e-12f : nrm;   /* clamp_min(eps) (a NaN stays a NaN) */                                   \
    const float inv = 1.0f / nrm;                                                                                   \
    const float nrm_r = nrm < __builtin_inff() ? nrm : 0.0f;   /* inf / NaN norm: the residual step adds y * 0 */   \
    _Pragma("unroll") for (int n = 0; n < NT; ++n) {                                                                \
      float q = (yf_)[n] * inv;                                                                                     \
      q = __builtin_fmaf(__builtin_fmaf(-q, nrm_r, (yf_)[n]), inv, q);                                              \
      (yf_)[n] = (part_) == 0 ? q * (s_h_) : q;                                                                     \
    }                                                                                                               \
  } while (0)

// One step of the maxima's reduce-scatter over the 16 lanes of a DPP row: rows r and r + N / 2 are paired, a lane keeps the
// one its bit selects and hands the other to its partner (DPP control CTRL), taking the partner's in return: N rows in, N / 2
// out, each now the maximum over twice as many lanes.  N == 1: plain exchange-and-max.  Packed pairs, unsigned compare.
template <int N, int CTRL>
FPQ_NOPK __device__ __forceinline__ void pk_max_scatter_step(uint32_t* key, bool bit) {
  if constexpr (N == 1) {
    key[0] = pk_max_u16(key[0], (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key[0], CTRL, 0xF, 0xF, true));
  } else {
#pragma unroll
    for (int r = 0; r < N / 2; ++r) {
      const uint32_t keep = bit ? key[r + N / 2] : key[r], send = bit ? key[r] : key[r + N / 2];
      key[r] = pk_max_u16(keep, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send, CTRL, 0xF, 0xF, true));
    }
  }
}

// a packed fp16 pair with its NaN halves cleared to +0 (vec_absmax16_dual's mask: 0xFFFF where |pattern| > 0x7C00)
FPQ_NOPK __device__ __forceinline__ uint32_t pk_nan_to_zero16(uint32_t w) {
  return w & ~pk_ashr_i16(pk_sub_u16(0x7C007C00u, w & 0x7FFF7FFFu), 15);
}

// one packed pair of quant_vec16<DUAL> (fpq_fast16.h): each half takes the reciprocal and the scale of its sign's side
FPQ_NOPK __device__ __forceinline__ uint32_t quant_pair16_dual(uint32_t wk, const uint16_t* lut, int shift, float ih_n, uint32_t s2_n,
                                                               float ih_p, uint32_t s2_p) {
  const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)wk, 15, 1), m1 = (uint32_t)((int)wk >> 31);   // all ones: negative
  const float h0 = u2f((fbits16(ih_n) & m0) | (fbits16(ih_p) & ~m0)), h1 = u2f((fbits16(ih_n) & m1) | (fbits16(ih_p) & ~m1));
  const uint32_t mp = pk_ashr_i16(wk, 15);
  const uint32_t sc = (s2_n & mp) | (s2_p & ~mp);
  const uint32_t rb = div_pair16(wk, h0, 0.0f, h1, 0.0f);
  const uint32_t u = pk_sub_u16(rb, pk_lshr_u16(rb, 15));   // negative patterns: magnitude - 1
  return pk_mul_f16(lut_pair16(lut, u, shift), sc);
}

// THE fc1 tail (see the comment above GemmFc1) of the register epilogues with 128-wide tiles - gemm_fp4_glds_kernel<.., GemmFc1>,
// gemm_a6w4_fc1_kernel - written once; it ends the kernel (every store is in it).  Row r of the tile = wm * WROWS + m * 16 +
// 4 * (lane >> 4) + i.  STAGE_: the bytes of one stage buffer of the kernel's two-stage ring; the exchange and the row scales go
// into buffer (G & 1), the one the last K group does not read.  Names from the kernel: smem, G, BM, MT, NT, WROWS, acc, bias_h, xe
// (GemmFc1), lut (the staged bucket table), t0, wm, wn, lane, tid, T, O, o, oc, out.
//   * The two maxima of a row travel as ONE packed key, both halves compared unsigned: low half = the unsigned maximum of the fp16
//     patterns (the most negative value, or a negative NaN), high half = their signed maximum with the sign bit flipped (the
//     largest positive value, or a positive NaN) - dual_max_acc of fpq_fast16.h, finished by the row's thread further down.
//   * Maxima over the 16 lanes that share a row: a reduce-scatter (the NR rows of a lane are halved four times, each step one DPP
//     exchange per surviving row: 30 exchanges for 32 rows, where reducing every row over all lanes takes 128) - afterwards lane
//     j of a DPP row holds the finished keys of NR / 16 rows (one row per lane pair for NR = 8), row index = the lane's bits,
//     highest first, then the position in `key`.
//   * The NaN flag is raised with the builtin: atomicOr() is a header function without the kernels' target attribute - it would
//     become a call.
//   * NANX_ (a compile-time constant; the kernels with it are instantiations of their own): the dual pair has NO global clamp (INT- /
//     E2M3+, fp6_quant_int_neg_e2m3_pos_per_group_cuda), so a NaN must stay out of its group's two maxima - vec_absmax16_dual's
//     rule, "NaN belongs to neither" - instead of riding in the key as the largest value of its side: the NaN halves are cleared in
//     the values the key is made of (never in hw, which is quantized and stored), three instructions per packed pair.
#define FPQ_GEMM_FC1_TAIL(STAGE_) FPQ_GEMM_FC1_TAIL_X(STAGE_, false)
#define FPQ_GEMM_FC1_TAIL_X(STAGE_, NANX_)                                                                          \
  do {                                                                                                              \
    FPQ_GEMM_BIAS_F32();                                                                                            \
    uint32_t* xch = (uint32_t*)(smem + (G & 1) * (STAGE_));  /* [2 (wn)][BM]: packed (max|h| over h < 0) | (max h over h > 0) << 16 */ \
    u32x4* rsc = (u32x4*)(xch + 2 * BM);                     /* [BM]: {1 / s_neg, 1 / s_pos, s_neg x 2, s_pos x 2} */ \
    static_assert(2 * BM * 4 + BM * 16 <= (STAGE_), "exchange + row scales fit the idle stage buffer");             \
    uint32_t hw[MT][4][2];                                                                                          \
    constexpr int NR = 4 * MT;                                                                                      \
    uint32_t key[NR];                                                                                               \
    _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                                                \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                               \
        float g[NT];                                                                                                \
        _Pragma("unroll") for (int n = 0; n < NT; ++n) g[n] = gelu_tanh_fast((float)(_Float16)(acc[m][n][i] + b4[n])); \
        const uint32_t w0 = f2h2(g[0], g[1]), w1 = f2h2(g[2], g[3]);                                                \
        hw[m][i][0] = w0;                                                                                           \
        hw[m][i][1] = w1;                                                                                           \
        const uint32_t k0 = (NANX_) ? pk_nan_to_zero16(w0) : w0, k1 = (NANX_) ? pk_nan_to_zero16(w1) : w1;          \
        const uint32_t un = pk_max_u16(k0, k1), sg = pk_max_i16(k0, k1) ^ 0x80008000u;                              \
        key[4 * m + i] = pk_max_u16(__builtin_amdgcn_perm(sg, un, 0x05040100u), __builtin_amdgcn_perm(sg, un, 0x07060302u)); \
      }                                                                                                             \
      if (xe.h_out) {                                                                                               \
        const int t_first = t0 + wm * WROWS + m * 16 + 4 * (lane >> 4);                                             \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                               \
          if (t_first + i < T && o < O)                                                                             \
            __builtin_nontemporal_store(u32x2{hw[m][i][0], hw[m][i][1]}, (u32x2*)(xe.h_out + (int64_t)(t_first + i) * O + oc)); \
      }                                                                                                             \
    }                                                                                                               \
    {                                                                                                               \
      const int j = lane & 15;                                                                                      \
      pk_max_scatter_step<NR, 0x128>(key, (j & 8) != 0);                               /* row_ror:8       partner j ^ 8 */ \
      pk_max_scatter_step<(NR >= 2 ? NR / 2 : 1), 0x141>(key, (j & 4) != 0);           /* row_half_mirror partner 7 - (j & 7) */ \
      pk_max_scatter_step<(NR >= 4 ? NR / 4 : 1), 0x4E>(key, (j & 2) != 0);            /* quad_perm [2,3,0,1] */    \
      pk_max_scatter_step<(NR >= 8 ? NR / 8 : 1), 0xB1>(key, (j & 1) != 0);            /* quad_perm [1,0,3,2] */    \
      constexpr int NF = NR >= 16 ? NR / 16 : 1;                                       /* finished rows per lane */ \
      constexpr int HALVINGS = NR >= 16 ? 4 : 3;                                       /* NR = 8: the last step is a plain exchange */ \
      const int rho0 = (HALVINGS == 4 ? j : (j >> 1)) * NF;                            /* row m * 4 + i of key[0] */ \
      uint32_t* dst = xch + wn * BM + wm * WROWS + (rho0 >> 2) * 16 + 4 * (lane >> 4) + (rho0 & 3);                 \
      if constexpr (NF == 2) *(u32x2*)dst = u32x2{key[0], key[1]};                     /* rows i, i + 1 of one tile row block */ \
      else dst[0] = key[0];                                                                                         \
    }                                                                                                               \
    FPQ_SYNC();                                                                                                     \
    if (tid < BM) {   /* one thread per token row: the group's two scales */                                        \
      const uint32_t k = pk_max_u16(xch[tid], xch[BM + tid]);                          /* the two wavefronts that share the group */ \
      const uint32_t un = k & 0xFFFFu, sgv = (k >> 16) ^ 0x8000u;                                                   \
      const uint32_t mn = (un & 0x8000u) ? (un & 0x7FFFu) : 0u, mp = (sgv & 0x8000u) ? 0u : sgv;   /* dual_max_finish */ \
      if ((mn > 0x7C00u || mp > 0x7C00u) && xe.nan_flag && t0 + tid < T)   /* a NaN in this group */                \
        __hip_atomic_fetch_or(xe.nan_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                         \
      RowScale16 sn = row_scale16(mn, xe.a.fneg.gmax, xe.a.inv_gneg), sp = row_scale16(mp, xe.a.fpos.gmax, xe.a.inv_gpos); \
      dual_poison(sn, sp);                                                                                          \
      rsc[tid] = u32x4{fbits16(sn.inv), fbits16(sp.inv), sn.s16x2, sp.s16x2};                                       \
    }                                                                                                               \
    FPQ_SYNC();                                                                                                     \
    _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                                                \
      const int r_first = wm * WROWS + m * 16 + 4 * (lane >> 4);                                                    \
      u32x2 q[4];                                                                                                   \
      int tq[4];                                                                                                    \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                               \
        const u32x4 sc = rsc[r_first + i];                                                                          \
        q[i][0] = quant_pair16_dual(hw[m][i][0], lut, xe.a.shift, u2f(sc[0]), sc[2], u2f(sc[1]), sc[3]);            \
        q[i][1] = quant_pair16_dual(hw[m][i][1], lut, xe.a.shift, u2f(sc[0]), sc[2], u2f(sc[1]), sc[3]);            \
        tq[i] = t0 + r_first + i;                                                                                   \
      }                                                                                                             \
      FPQ_GEMM_ROWS_STORE(q, t0 + r_first, tq, o, oc);                                                              \
    }                                                                                                               \
  } while (0)

// ---------------------------------------------------------------------------------------------------
// THE STAGES OF THE PER-GROUP(128) LDS-DMA KERNELS - gemm_fp4_glds_kernel and gemm_fp4_ring_kernel below, and the text of the
// kernels with a 6-bit side (fpq_gemm_g6_kernel.h) - written once.  Macros, like the tails above: a body shared through an
// inlined function has twice come out as other machine code (the note at FPQ_QK_NORM_ROW, profiles/r08_bf6_isa.txt); as macros
// every kernel is, instruction for instruction, what its own copy of these lines gave (profiles/gemm_shared_stages_isa.txt).
// What a kernel keeps: its template head, name and launch bounds, the LDS-DMA lane offsets and the issue of a stage, the
// staging schedule (two stages or the ring), the row-major scale tiles with their visible wait, and the call of the fc1 tail.

// The tile walk (the row-scaled FP6 / FP8 kernels walk the same way): lane, wavefront (uniform, in a scalar register) and its
// place wm x wn among the 2 x 2 of the workgroup, then the XCD-aware tile order - workgroups are dealt round-robin over the 8
// XCDs, each with its own 4 MiB L2: XCD k owns a contiguous band of `cpx` column tiles and walks all row tiles of that band, so
// its slice of W stays L2-resident and an A tile is re-used by cpx consecutive workgroups.  Defines tid, lane, wave, wm, wn, t0, o0.
#define FPQ_GEMM_TILE_WALK(BM_, BN_)                                                                                \
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);                    \
  const int wm = wave >> 1, wn = wave & 1;                                                                          \
  const int n_col = (O + (BN_) - 1) / (BN_), n_row = (T + (BM_) - 1) / (BM_);                                       \
  const int cpx = (n_col + 7) >> 3;                                                                                 \
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;                                                          \
  const int col_blk = xcd * cpx + local % cpx, row_blk = local / cpx;                                               \
  if (col_blk >= n_col || row_blk >= n_row) return;   /* uniform over the workgroup */                              \
  const int t0 = row_blk * (BM_), o0 = col_blk * (BN_)

// One LDS-DMA instruction: 64 lanes x 16 bytes from (uniform 64-bit base_ + the lane's 32-bit voff_) to the 1 KiB at lds_.
// Spelled in assembly - the compiler folds base + offset into a loop-invariant per-lane pointer and adds a group's step to each
// with a 64-bit vector addition - and WITHOUT a memory clobber (with one, -4 % instead of +3 %: it pins every LDS read of the
// group behind it; the loads write the stage nobody reads, and the barriers order them).  The compiler does not see these loads:
// the wait for them is spelled out in front of the barrier that hands a stage to its readers, FPQ_GLDS_WAIT (vmcnt(0); the ring
// counts, glds_wait_vm).
#define FPQ_GLDS_LOAD(voff_, base_, lds_)                                                                           \
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"                                     \
               :                                                                                                    \
               : "v"(voff_), "s"(base_), "s"((uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(lds_)) \
               : "m0")
#define FPQ_GLDS_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

// K-MAJOR SCALE IMAGES (include/fpq.h) -> the scale tiles: sa_ / sw_ are fp32 planes [G][rows rounded up to 4] (activations) and
// [G][km_w_rows] (weights, natural output order) - the tile's scales of a group are 4 BM (4 BN) contiguous bytes, exactly one
// row of lsa (lsw): they come in by LDS-DMA like the codes, 256 / BM groups per 1 KiB activation piece and two per weight piece,
// no register round trip, no conversion, no ds_write.  (Row-major fp16 / fp32 scales cost 90 strided load instructions + as many
// LDS writes per tile: 8 % of the kernel, profiles/r05_kmajor_ab.txt.)  Pieces dealt round-robin over the four wavefronts; a last
// piece's surplus groups re-read the last one (their LDS rows are the padding up to Gp); rows clamped to the image's last four.
// A wavefront has 0 .. n of these pieces, so they cannot be counted: they are requested in front of every stage, and the main
// loop's first wait covers them - the compiler has issued no load of its own that it would have to wait for.
// Names from the kernel: BM, BN, G, T, t0, o0, lane, wave, epi, lsa, lsw.
#define FPQ_GEMM_KM_SCALE_TILES(sa_, sw_)                                                                           \
  do {                                                                                                              \
    constexpr int APG = 256 / BM, LPG_A = BM / 4;          /* groups per piece, lanes per group (activation side) */ \
    const int Tpad = (T + 3) & ~3, n_a = (G + APG - 1) / APG, n_w = (G + 1) >> 1;                                   \
    const float* sa_km = (const float*)(sa_);                                                                       \
    const float* sw_km = (const float*)(sw_);                                                                       \
    for (int p = wave; p < n_a + n_w; p += 4) {                                                                     \
      const bool is_a = p < n_a;                                                                                    \
      const int g0 = is_a ? p * APG : (p - n_a) * 2;                                                                \
      const int sub = is_a ? lane / LPG_A : lane >> 5, l4 = is_a ? lane % LPG_A : lane & 31;                        \
      const int grp = g0 + sub < G ? g0 + sub : G - 1;                                                              \
      const int rows = is_a ? Tpad : epi.km_w_rows, r0 = is_a ? t0 : o0;                                            \
      int r4 = r0 + 4 * l4;                                                                                         \
      r4 = r4 < rows - 4 ? r4 : rows - 4;                                                                           \
      const uint32_t vo = (uint32_t)(((grp - g0) * rows + (r4 - r0)) * 4);                                          \
      const float* sbase = (is_a ? sa_km : sw_km) + ((int64_t)g0 * rows + r0);                                      \
      FPQ_GLDS_LOAD(vo, sbase, is_a ? lsa + g0 * BM : lsw + g0 * BN);                                               \
    }                                                                                                               \
  } while (0)

// What a lane's epilogue reads from memory, requested in the prologue and not between the last MFMA and the stores: the fp16
// bias of its four consecutive outputs o .. o + 3 (see the dealt weight rows; oc = o clamped into the tensor) and, QKN_, the q / k
// norm's fp32 bias and s_h of its head in part 0 (qkn_bias_, qkn_scale_: GemmQkNorm's fields).  Defines WROWS, WCOLS, o, oc,
// bias_h, qkn_b, qkn_s.
#define FPQ_GEMM_LANE_BIAS(QKN_, qkn_bias_, qkn_scale_)                                                             \
  constexpr int WROWS = 16 * MT, WCOLS = 16 * NT;                                                                   \
  const int o = o0 + wn * WCOLS + NT * (lane & 15);                                                                 \
  const int oc = o < O ? o : O - 4;                                                                                 \
  fpq_h4_t bias_h = fpq_h4_t{0, 0, 0, 0};                                                                           \
  if (bias) bias_h = *(const fpq_h4_t*)(bias + oc);                                                                 \
  v4f_t qkn_b = v4f_t{0, 0, 0, 0};                                                                                  \
  float qkn_s = 1.0f;                                                                                               \
  if constexpr (QKN_) {                                                                                             \
    if (qkn_bias_) qkn_b = *(const v4f_t*)((qkn_bias_) + oc);                                                       \
    if (o0 < epi.sp_cols) qkn_s = (qkn_scale_)[oc >> 6];                                                            \
  }

// a nibble fragment (32 consecutive k of one row): one ds_read_b128 at p_, the upper half of the MFMA operand unused
#define FPQ_GEMM_READ_NIB(dst_, p_)                                                                                 \
  do {                                                                                                              \
    const u32x4 q_ = *(const u32x4*)(p_);                                                                           \
    dst_ = v8i_t{(int)q_[0], (int)q_[1], (int)q_[2], (int)q_[3], 0, 0, 0, 0};                                       \
  } while (0)

// K group g_ from the stage at st_: acc[m][n] += (d * sa) * sw over the wavefront's MT x NT tiles, d = one MFMA of 128 k.
// READ_A_ / READ_B_ (dst, stage, byte offset of the 16-row tile in the wavefront's part of the stage) read a side's fragment -
// the kernel's own: FPQ_GEMM_READ_NIB or three ds_read_b64 of 6-bit codes, and the ORDER in which the stage, the tile's offset
// and the lane's are added, which the machine code follows (profiles/gemm_shared_stages_isa.txt); A_TILE_ / W_TILE_ are the
// bytes from tile to tile; FA_ / FW_ the MFMA's format selectors (cbsz decodes the activation fragment, blgp the weight
// fragment); literal zero scale operands select the unscaled instruction (x 1.0; tools/probe/mfma_fp4_probe.hip).
// Names from the kernel: MT, NT, BM, BN, lsa, lsw, sa_off, sw_off, acc.
// Software pipeline over the tile rows: the ds_reads of row m+1 are issued first, then the NT MFMAs of row m, then the
// scale-and-accumulate of row m-1 - VALU work that does not depend on the MFMAs in flight, so no hazard wait states are needed
// and 8 of each MFMA's 16 cycles of vector issue are hidden behind it.  (Left to itself the compiler issues each row's reads
// right before their use and the VALU right behind its own MFMAs, with s_nops in between.)  Issue order inside a row: one MFMA,
// then the 8 VALU ops of one finished tile, NT times - an in-order wavefront that issues its MFMAs back to back just waits for
// the matrix pipe with its VALU idle.
#define FPQ_GEMM_GROUP(g_, st_, READ_A_, READ_B_, A_TILE_, W_TILE_, FA_, FW_)                                       \
  do {                                                                                                              \
    v8i_t bf[NT];                                                                                                   \
    _Pragma("unroll") for (int n = 0; n < NT; ++n) READ_B_(bf[n], st_, n * (W_TILE_));                              \
    const v4f_t sw1 = *(const v4f_t*)(lsw + (g_) * BN + sw_off);                                                    \
    v8i_t af;                                                                                                       \
    READ_A_(af, st_, 0);                                                                                            \
    v4f_t sa4 = *(const v4f_t*)(lsa + (g_) * BM + sa_off);                                                          \
    v4f_t d_prev[NT], sa4_prev = sa4;                                                                               \
    _Pragma("unroll") for (int n = 0; n < NT; ++n) d_prev[n] = v4f_t{0, 0, 0, 0};                                   \
    _Pragma("unroll") for (int m = 0; m <= MT; ++m) {                                                               \
      v8i_t af_n = af;                                                                                              \
      v4f_t sa4_n = sa4;                                                                                            \
      if (m + 1 < MT) {                                                                                             \
        READ_A_(af_n, st_, (m + 1) * (A_TILE_));                                                                    \
        sa4_n = *(const v4f_t*)(lsa + (g_) * BM + sa_off + (m + 1) * 16);                                           \
      }                                                                                                             \
      __builtin_amdgcn_sched_barrier(0);                                                                            \
      v4f_t d[NT];                                                                                                  \
      if (m < MT) {                                                                                                 \
        _Pragma("unroll") for (int n = 0; n < NT; ++n)                                                              \
          d[n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bf[n], v4f_t{0, 0, 0, 0}, FA_, FW_, 0, 0, 0, 0); \
      }                                                                                                             \
      if (m > 0) {                                                                                                  \
        _Pragma("unroll") for (int n = 0; n < NT; ++n)                                                              \
          _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                           \
            const float t = d_prev[n][i] * sa4_prev[i];                                                             \
            acc[m - 1][n][i] = __builtin_fmaf(t, sw1[n], acc[m - 1][n][i]);                                         \
          }                                                                                                         \
      }                                                                                                             \
      if (m > 0 && m < MT) {                                                                                        \
        _Pragma("unroll") for (int n = 0; n < NT; ++n) {                                                            \
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                        \
          __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);                                                        \
        }                                                                                                           \
      }                                                                                                             \
      __builtin_amdgcn_sched_barrier(0);                                                                            \
      if (m < MT) {                                                                                                 \
        _Pragma("unroll") for (int n = 0; n < NT; ++n) d_prev[n] = d[n];                                            \
        sa4_prev = sa4;                                                                                             \
      }                                                                                                             \
      af = af_n;                                                                                                    \
      sa4 = sa4_n;                                                                                                  \
    }                                                                                                               \
  } while (0)

// The epilogue from the registers (round 4): a lane's results of row i in the NT tiles are four consecutive outputs -> + bias,
// one rounding to fp16 (QKN_: the q / k norm of the row's head instead, FPQ_QK_NORM_ROW), gate / residual (GATE_, a constant:
// whether the form has that tail), one 8-byte store; 16 lanes write 128 contiguous bytes.  split_: whether the output is split
// (FPQ_GEMM_SPLIT_SETUP's on_: epi.sp_cols where one kernel serves both outputs, or a constant).  Rounds 1-3 turned the tile
// through LDS for 16-byte row stores (64 x (add, convert, ds_write_b16), two barriers, the re-read: ~330 of the ~2850 vector
// instructions of a wavefront's tile at K = 1920).  outs % 8 == 0 and o % 4 == 0: o < O means o + 4 <= O.
// Loads are unconditional on clamped addresses (a lane past the edge reads what a neighbour reads and stores nothing): a load
// inside a divergent branch is waited for inside it.  Requesting the gate / residual rows one tile row ahead of their use - the
// compiler may not move a load above a store that could alias it, and the residual may BE the output - was measured: 13 % slower
// with the fused tail (round 4).  The one-tensor stores are non-temporal: a round of tiles writes as much as an XCD's L2 holds -
// the operands should stay there; +1-2 %.  Names from the kernel: MT, NT, WROWS, acc, bias_h, qkn_b, qkn_s, o, oc, t0, o0, wm,
// lane, T, O, out, epi.
#define FPQ_GEMM_REG_EPILOGUE(QKN_, GATE_, split_)                                                                  \
  do {                                                                                                              \
    FPQ_GEMM_BIAS_F32();                                                                                            \
    FPQ_GEMM_GATE_SETUP(WROWS);                                                                                     \
    FPQ_GEMM_SPLIT_SETUP(WROWS, split_);                                                                            \
    _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                                                \
      const int t_first = t0 + wm * WROWS + m * 16 + 4 * (lane >> 4);                                               \
      fpq_h4_t y[4];                                                                                                \
      if constexpr (QKN_) {                                                                                         \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                             \
          float yf[NT];                                                                                             \
          _Pragma("unroll") for (int n = 0; n < NT; ++n) yf[n] = (float)(_Float16)acc[m][n][i] + qkn_b[n];          \
          if (sp_part_ < 2) FPQ_QK_NORM_ROW(yf, sp_part_, qkn_s);   /* uniform over the tile */                     \
          _Pragma("unroll") for (int n = 0; n < NT; ++n) y[i][n] = (_Float16)yf[n];                                 \
        }                                                                                                           \
      } else {                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                               \
          _Pragma("unroll") for (int n = 0; n < NT; ++n) y[i][n] = (_Float16)(acc[m][n][i] + b4[n]);                \
      }                                                                                                             \
      int tc[4];                                                                                                    \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) tc[i] = t_first + i < T ? t_first + i : T - 1;                  \
      if constexpr (GATE_) FPQ_GEMM_GATE_RESID_ROWS(y, tc, m, oc);                                                  \
      if (split_) {   /* uniform: four 8-byte stores to the part's rows */                                          \
        const int oc_l = oc - sp_part_ * epi.sp_cols;                                                               \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) FPQ_GEMM_SPLIT_STORE(y[i], m, i, tc[i], t_first, o, oc_l);    \
        continue;                                                                                                   \
      }                                                                                                             \
      FPQ_GEMM_ROWS_STORE(y, t_first, tc, o, oc);                                                                   \
    }                                                                                                               \
  } while (0)

// ---------------------------------------------------------------------------------------------------
// THE SQUARED-ERROR TAIL (include/fpq.h, fpq_gemm_*_sqerr; the format search's loss): the register epilogues' y16 - bit for bit
// what the plain form stores - is not stored; the workgroup leaves ONE fp32,
//     partial[tile] = sum over the tile's rows t < T of  w[t] * sum over its outputs o < O of (f32(ref[t, o]) - f32(y16[t, o]))^2,
// and a second launch (sqerr_finish_kernel, fpq_kernels.hip) adds the tiles' partials in a fixed order.  No atomics, no memset:
// every partial the finish reads was written by this launch, so the workspace's old content never shows.
// Written once for the per-group kernels (FPQ_GEMM_SQERR_EPILOGUE: gemm_fp4_glds_kernel<.., GemmSqErr>, gemm_a6w4_sqerr_kernel,
// gemm_w6_sqerr_kernel) and the row-scaled one (FPQ_GEMM_ROWS_EPILOGUE_SQERR, fpq_gemm_fp8.h: gemm_f6_rows_sqerr_kernel).
// The additions a term passes through, in order (tests/gemm_sqerr_model.py restates them; include/fpq.h carries the bound):
//     4 in the lane's four outputs of a row (s += e e, the first to 0), 4 MT over the lane's rows (acc += w s, the first to 0),
//     6 in the wavefront's butterfly (lane ^ 32 .. lane ^ 1: both partners add the same pair), 3 over the four wavefronts; in
//     the finish ceil(tiles / 256) in a lane, 6 and 3 again:   D = 4 MT + ceil(tiles / 256) + 22,
// and c = 3 roundings besides them (the difference, the square, the weight).  No fused multiply-add (-ffp-contract=off).
// Edges: a row t >= T or a column group o >= O holds a clamped duplicate (perhaps non-finite) - it is SELECTED away, never
// multiplied by zero.  The ref / weight loads are unconditional on clamped addresses, as the stores' neighbours above are, and
// stand behind the main loop: a load the compiler sees in the prologue puts vmcnt waits into the loop.
struct GemmSqErr {
  const void* ref;        // [T, O] fp16 or fp32 (ref_f32), 16-byte aligned
  const float* row_w;     // fp32 [T]
  float* partials;        // one fp32 per tile: index row_blk * n_col + col_blk of the launch's tiling
  int ref_f32;
};

// rows tc_[0..3] (t_first_ + i clamped to T - 1), outputs oc_ .. oc_ + 3 (o_ clamped to O - 4) of y_ = fpq_h4_t[4] into se_acc.
// Names from the kernel: xe (GemmSqErr), T, O.
#define FPQ_GEMM_SQERR_ROWS(y_, t_first_, tc_, o_, oc_)                                                             \
  do {                                                                                                              \
    float rw_[4], rf_[4][4];                                                                                        \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) rw_[i_] = xe.row_w[(tc_)[i_]];                                 \
    if (xe.ref_f32) {   /* uniform */                                                                               \
      v4f_t r32_[4];                                                                                                \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) r32_[i_] = *(const v4f_t*)((const float*)xe.ref + (int64_t)(tc_)[i_] * O + (oc_)); \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                              \
        _Pragma("unroll") for (int n_ = 0; n_ < 4; ++n_) rf_[i_][n_] = r32_[i_][n_];                                \
    } else {                                                                                                        \
      fpq_h4_t r16_[4];                                                                                             \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) r16_[i_] = *(const fpq_h4_t*)((const _Float16*)xe.ref + (int64_t)(tc_)[i_] * O + (oc_)); \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                              \
        _Pragma("unroll") for (int n_ = 0; n_ < 4; ++n_) rf_[i_][n_] = (float)r16_[i_][n_];                         \
    }                                                                                                               \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                              \
      float s_ = 0.0f;                                                                                              \
      _Pragma("unroll") for (int n_ = 0; n_ < 4; ++n_) {                                                            \
        const float e_ = rf_[i_][n_] - (float)(y_)[i_][n_];                                                         \
        s_ += e_ * e_;                                                                                              \
      }                                                                                                             \
      const float ws_ = rw_[i_] * s_;                                                                               \
      se_acc += ((t_first_) + i_ < T && (o_) < O) ? ws_ : 0.0f;                                                     \
    }                                                                                                               \
  } while (0)
// se_acc over the wavefront (the butterfly of lanes_sum64, fpq_kernels.hip, spelled with the builtin: __shfl_xor is a header
// function without the kernels' target attribute - it would become a call), the four wavefronts in order through scratch_ (16
// bytes of LDS nobody reads any more: the stage buffer the last K group did not use), one store per workgroup.
// Names from the kernel: xe, lane, wave, tid, row_blk, col_blk, n_col.
#define FPQ_GEMM_SQERR_FINISH(scratch_)                                                                             \
  do {                                                                                                              \
    float v_ = se_acc;                                                                                              \
    _Pragma("unroll") for (int m_ = 32; m_ >= 1; m_ >>= 1)                                                          \
      v_ += __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ m_) << 2, __builtin_bit_cast(int, v_))); \
    float* xw_ = (float*)(scratch_);                                                                                \
    if (lane == 0) xw_[wave] = v_;                                                                                  \
    FPQ_SYNC();                                                                                                     \
    if (tid == 0) {                                                                                                 \
      float s_ = xw_[0];                                                                                            \
      _Pragma("unroll") for (int i_ = 1; i_ < 4; ++i_) s_ += xw_[i_];                                               \
      xe.partials[row_blk * n_col + col_blk] = s_;                                                                  \
    }                                                                                                               \
  } while (0)
// the per-group kernels' epilogue with this tail: y as FPQ_GEMM_REG_EPILOGUE's plain branch rounds it.  Names as there.
#define FPQ_GEMM_SQERR_EPILOGUE(scratch_)                                                                           \
  do {                                                                                                              \
    FPQ_GEMM_BIAS_F32();                                                                                            \
    float se_acc = 0.0f;                                                                                            \
    _Pragma("unroll") for (int m = 0; m < MT; ++m) {                                                                \
      const int t_first = t0 + wm * WROWS + m * 16 + 4 * (lane >> 4);                                               \
      fpq_h4_t y[4];                                                                                                \
      _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                 \
        _Pragma("unroll") for (int n = 0; n < NT; ++n) y[i][n] = (_Float16)(acc[m][n][i] + b4[n]);                  \
      int tc[4];                                                                                                    \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) tc[i] = t_first + i < T ? t_first + i : T - 1;                  \
      FPQ_GEMM_SQERR_ROWS(y, t_first, tc, o, oc);                                                                   \
    }                                                                                                               \
    FPQ_GEMM_SQERR_FINISH(scratch_);                                                                                \
  } while (0)

// What the two FP4 kernels below (nibbles on both sides, row-major or k-major at run time) share beyond that.
// _SOURCES: the LDS-DMA sources of a wavefront's pieces (block = wave + 4 * i of the stage), group 0.
// The weight rows are DEALT over a wavefront's NT = 4 blocks (round 4): row q of block n holds output 4*q + n of the
// wavefront's 64, so the lane that holds column q of the NT result tiles holds four CONSECUTIVE outputs 4*q .. 4*q + 3
// and the epilogue stores 8 bytes per lane, 128 contiguous bytes per 16 lanes, straight from the accumulators.
// Addressing (round 4): a UNIFORM 64-bit base per operand (the tile's first row) + a 32-bit lane offset (row inside the
// tile, clamped to the tensor's last row, and 16-byte chunk) that never changes: the step from group to group (64 bytes)
// is scalar arithmetic and the load takes scalar base + vector offset (FPQ_GLDS_LOAD).  Rows past the end of a tensor are
// clamped to its last row: their products land where the epilogue never stores.
// K-major images (epi.km_w_rows != 0): plane g holds every row's 64 bytes of group g, [G][rows][64], the 16-byte chunks of a row
// already in the LDS image's order and the weight rows in dealt order - a piece is 1 KiB CONTIGUOUS (8 whole 128-byte lines)
// instead of 16 rows' half lines row_bytes apart: 70 against 105 cycles to issue, profiles/r05_lds_dma_issue.txt.
// Names from the kernel: A, W, T, O, epi, row_bytes, t0, o0, lane, wave, NT, ABLK, PIECES.  Defines km, a_step, w_step, gbase, voff.
#define FPQ_FP4_GLDS_SOURCES()                                                                                      \
  static_assert(NT == 4, "the epilogue packs a lane's NT results of one row into one 8-byte store");               \
  static_assert(ABLK % 4 == 0, "a wavefront's pieces i < ABLK / 4 are rows of A, the rest rows of W");              \
  const bool km = epi.km_w_rows != 0;                                                                               \
  const int row_stride = km ? 64 : row_bytes;                                                                       \
  const int64_t a_step = km ? (int64_t)T * 64 : 64, w_step = km ? (int64_t)epi.km_w_rows * 64 : 64;                 \
  const uint8_t* const gbase[2] = {A + (int64_t)t0 * row_stride, W + (int64_t)o0 * row_stride};                     \
  uint32_t voff[PIECES];                                                                                            \
  {                                                                                                                 \
    const int q = lane >> 2, kb = km ? (lane & 3) : (lane & 3) ^ glds_chunk_perm(q);                                \
    const int w_rows = km ? epi.km_w_rows : O;                                                                      \
    _Pragma("unroll") for (int i = 0; i < PIECES; ++i) {                                                            \
      const int blk = wave + 4 * i;                                                                                 \
      if (blk < ABLK) {                                                                                             \
        const int t = t0 + blk * 16 + q;                                                                            \
        voff[i] = (uint32_t)((t < T ? t : T - 1) - t0) * (uint32_t)row_stride + (uint32_t)(kb * 16);                \
      } else {                                                                                                      \
        const int wb = blk - ABLK;                                                                                  \
        const int o = km ? o0 + wb * 16 + q : o0 + (wb / NT) * (16 * NT) + NT * q + wb % NT;                        \
        voff[i] = (uint32_t)((o < w_rows ? o : w_rows - 1) - o0) * (uint32_t)row_stride + (uint32_t)(kb * 16);      \
      }                                                                                                             \
    }                                                                                                               \
  }
// group g's pieces of this wavefront into stage buffer buf
#define FPQ_FP4_GLDS_ISSUE(g, buf)                                                                                  \
  _Pragma("unroll") for (int i_ = 0; i_ < PIECES; ++i_)                                                             \
      FPQ_GLDS_LOAD(voff[i_], gbase[i_ < ABLK / 4 ? 0 : 1] + (g) * (i_ < ABLK / 4 ? a_step : w_step),               \
                    smem + (buf) * STAGE + (wave + 4 * i_) * 1024)
// the fragment read offsets inside a stage (row lane & 15, chunk lane >> 4 of a 16-row block) and inside the scale tiles
// (outputs 4q .. 4q+3: tile n holds 4q + n)
#define FPQ_FP4_FRAG_OFFSETS()                                                                                      \
  const int frag_off = ((lane & 15) << 6) + ((((lane >> 4) ^ glds_chunk_perm(lane & 15)) & 3) << 4);                \
  const int a_off = wm * MT * 1024 + frag_off, b_off = (ABLK + wn * NT) * 1024 + frag_off;                          \
  const int sa_off = wm * MT * 16 + 4 * (lane >> 4), sw_off = wn * NT * 16 + NT * (lane & 15)
#define FPQ_FP4_READ_A(dst_, st_, tile_) FPQ_GEMM_READ_NIB(dst_, (st_) + a_off + (tile_))
#define FPQ_FP4_READ_W(dst_, st_, tile_) FPQ_GEMM_READ_NIB(dst_, (st_) + b_off + (tile_))

// target("no-packed-fp32-ops"): beside MFMAs a packed fp32 op costs as much as two scalar ones and blocks the issue
// port twice as long (tools/probe/valu_mfma_overlap.hip); with the feature off the compiler emits scalar
// v_mul_f32 / v_fma_f32 and schedules them - and the MFMA hazard wait states - itself.
// XE = GemmNoFc1: the plain Linear (+ gate / residual tail); XE = GemmFc1: the fc1 tail above; XE = GemmQkNorm: the split
// output with the q / k norm above; XE = GemmSqErr: the squared-error tail above (row-major operands, no output tensor).
template <typename Tsw, int MT, int NT, typename XE = GemmNoFc1>
__global__ __launch_bounds__(256, (MT * NT > 16 ? 2 : 3)) FPQ_NOPK void gemm_fp4_glds_kernel(const uint8_t* __restrict__ A,
                                                              const _Float16* __restrict__ sa,
                                                              const uint8_t* __restrict__ W, const Tsw* __restrict__ sw,
                                                              const _Float16* __restrict__ bias,
                                                              _Float16* out, int T, int O, int C, GemmEpi epi, XE xe) {
  constexpr bool FC1 = __is_same(XE, GemmFc1), QKN = __is_same(XE, GemmQkNorm);
  constexpr int WR = 2, WC = 2, BM = 16 * MT * WR, BN = 16 * NT * WC, NTHR = 256;
  constexpr int ABLK = BM / 16, BBLK = BN / 16, NBLK = ABLK + BBLK, STAGE = NBLK * 1024;
  static_assert(NBLK % 4 == 0, "blocks are dealt round-robin to the four wavefronts");
  constexpr int PIECES = NBLK / 4;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int G = C >> 7, row_bytes = C >> 1;
  float* lsa = (float*)(smem + 2 * STAGE);   // [G][BM]
  const int Gp = (G + 3) & ~3;               // the scale tiles' LDS-DMA pieces cover up to four groups each: room for a whole last piece
  float* lsw = lsa + Gp * BM;                // [G][BN]
  FPQ_GEMM_TILE_WALK(BM, BN);

  // Issuing a stage's pieces between the MFMAs of the previous one instead of in front of them: 2.5 x slower (measured).
  // A persistent form (one workgroup per resident slot looping over its tiles, the next tile's stage 0 and scale tiles
  // requested in front of the current tile's stores): 5 - 10 % slower than one workgroup per tile (measured, round 4).
  FPQ_FP4_GLDS_SOURCES();
  FPQ_FP4_GLDS_ISSUE(0, 0);

  if (km) {
    FPQ_GEMM_KM_SCALE_TILES(sa, sw);
  } else {
    load_scale_tiles<Tsw, BM, BN, NTHR>(sa, sw, lsa, lsw, t0, o0, T, O, G, tid);
    // A wait the COMPILER sees (the builtin, not assembly): its scoreboard still carries the scale loads above, whose last
    // waits it counted without knowing of the stage-0 pieces in the same queue - left like that, it protects their
    // destination registers with vmcnt waits inside the main loop, and those wait for the stage just requested.
    // (It has to stand in THIS branch: behind the join, under a second `if (!km)`, the compiler's scoreboard keeps the loads
    // pending on the path it cannot rule out, and the loop got its vmcnt(0) back - 8 % - profiles/r05_kmajor_ab.txt.)
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  }
  uint16_t* lut = nullptr;
  if constexpr (FC1) {   // the dual quantizer's bucket table, behind the scale tiles; visible after the first barrier of the main loop
    lut = (uint16_t*)(lsw + Gp * BN);
    lut16_stage(lut, xe.tab, xe.a.shift);
  }

  FPQ_GEMM_LANE_BIAS(QKN, xe.bias, xe.q_scale);

  v4f_t acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = v4f_t{0, 0, 0, 0};
  FPQ_FP4_FRAG_OFFSETS();

  for (int g = 0; g < G; ++g) {
    FPQ_GLDS_WAIT();
    FPQ_SYNC();   // stage g has landed; stage g^1's readers are done
    if (g + 1 < G) { FPQ_FP4_GLDS_ISSUE(g + 1, (g + 1) & 1); }
    const uint8_t* st = smem + (g & 1) * STAGE;
    FPQ_GEMM_GROUP(g, st, FPQ_FP4_READ_A, FPQ_FP4_READ_W, 1024, 1024, 4, 4);
  }
  if constexpr (FC1) {
    FPQ_GEMM_FC1_TAIL(STAGE);
    return;
  }
  if constexpr (__is_same(XE, GemmSqErr)) {   // the loss against xe.ref instead of the output; buffer G & 1: the fc1 tail's idle one
    FPQ_GEMM_SQERR_EPILOGUE(smem + (G & 1) * STAGE);
    return;
  }
  FPQ_GEMM_REG_EPILOGUE(QKN, true, epi.sp_cols);   // (this epilogue serves the one-tensor output too)
}

// ---------------------------------------------------------------------------------------------------
// The deep-ring small-M form of gemm_fp4_glds_kernel<.., 2, 4> (FPQ_GEMM_CFG 40): the same 64 x 128 tile, LDS block image, dealt
// weight rows, XCD tile order, clamped lane offsets, per-group arithmetic (t = d * sa; acc = fma(t, sw, acc), g ascending) and
// register epilogues - every output is bit-equal to FPQ_GEMM_CFG 30.  What differs is the staging.  The loop above is
// `wait vmcnt(0) -> barrier -> request group g + 1 -> multiply group g`: one group in flight, a tile pays G dependent trips to
// memory, and at the first scale steps (30 - 240 workgroups on 256 CUs) no second workgroup hides them.  Here:
//   * a ring of S = FPQ_GEMM_RING_STAGES stage buffers, group g in buffer g % S;
//   * the first min(S - 1, G) groups requested up front, behind everything else the prologue puts into the memory queue (the
//     k-major scale pieces, the row-major scale loads and their visible wait, the bias) - the queue retires in order, so the
//     wait for group 0 covers all of it, and a visible wait in front of the ring cannot drain it;
//   * iteration g: `wait -> barrier -> request group g + S - 1 -> multiply group g`.  The request goes to buffer (g - 1) % S, last
//     read in iteration g - 1, behind the barrier every reader of it has passed (write after read); buffer g % S is read behind
//     the wait of the wavefronts that requested it and that same barrier (read after write);
//   * the wait is COUNTED: in front of it groups g .. min(G, g + S - 1) - 1 are outstanding, so min(G - 1 - g, S - 2) groups may
//     stay in flight - s_waitcnt vmcnt(PIECES * (S - 2)) in the steady loop (which always requests: g + S - 1 < G), and PIECES *
//     (G - 1 - g), ..., PIECES, 0 over the last S - 1 groups, which request nothing (no piece of a group >= G is ever issued: a
//     k-major plane past G is past the allocation) - a uniform switch in a loop of its own (FPQ_RING_TAIL_WAIT).
// A visible load younger than the ring (none is left in the loops) could only make a wait stricter, never laxer.
// The fc1 tail's scratch stays `(G & 1) * STAGE`: S is even, so buffer G & 1 is not the last group's, (G - 1) % S - the parities
// differ; every request has landed (the last wait is vmcnt(0)) and every other buffer's readers are behind the last barrier.
// LDS: S stages + the scale tiles (+ the bucket table): 12 S + 12 KiB at K = 1920, 12 S + 48 KiB at K = 8192 - with S = 8 one
// workgroup per CU (108 / 144 KiB), with S = 4 two (60 / 96 KiB).
// MEASURED (profiles/gemm_fp4_ring_small_steps.txt): it pays nowhere at the models' shapes.  With at most one tile per CU it is
// 0.2 / 0.4 / 0.7 us SLOWER than cfg 30's 7.8 - 8.1 us at K = 1920 with S = 4 / 6 / 8, past that 1.2 x (S = 4) to 2 x (S = 6, 8:
// one workgroup per CU) slower.  The flat 8 us are a 3.4 us floor (K = 128) + 0.33 us per group, and that step does not move with
// the depth of the ring: it is the lone wavefront's own chain per group (three LDS-DMA issues, fragment reads, eight MFMAs with
// their scale stage, the barrier), not a trip to memory.  S = 4 is the least slow of the three and is what ships; the default
// tiling never chooses 40 (gemm_glds_tiling, fpq_gemm.hip).
#ifndef FPQ_GEMM_RING_STAGES
#define FPQ_GEMM_RING_STAGES 4   // {4, 6, 8} measured: profiles/gemm_fp4_ring_small_steps.txt
#endif
template <int N>
FPQ_NOPK __device__ __forceinline__ void glds_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

template <typename Tsw, typename XE = GemmNoFc1>
__global__ __launch_bounds__(256, 3) FPQ_NOPK void gemm_fp4_ring_kernel(const uint8_t* __restrict__ A,
                                                              const _Float16* __restrict__ sa,
                                                              const uint8_t* __restrict__ W, const Tsw* __restrict__ sw,
                                                              const _Float16* __restrict__ bias,
                                                              _Float16* out, int T, int O, int C, GemmEpi epi, XE xe) {
  constexpr bool FC1 = __is_same(XE, GemmFc1), QKN = __is_same(XE, GemmQkNorm);
  constexpr int S = FPQ_GEMM_RING_STAGES, MT = 2, NT = 4;
  constexpr int WR = 2, WC = 2, BM = 16 * MT * WR, BN = 16 * NT * WC, NTHR = 256;
  constexpr int ABLK = BM / 16, BBLK = BN / 16, NBLK = ABLK + BBLK, STAGE = NBLK * 1024;
  constexpr int PIECES = NBLK / 4;   // LDS-DMA pieces per wavefront and stage
  static_assert(S >= 4 && S % 2 == 0, "an even ring: the fc1 tail's scratch, buffer G & 1, is never the last group's");
  static_assert(PIECES * (S - 2) <= 63, "vmcnt is a 6-bit counter");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int G = C >> 7, row_bytes = C >> 1;
  float* lsa = (float*)(smem + S * STAGE);   // [G][BM]
  const int Gp = (G + 3) & ~3;
  float* lsw = lsa + Gp * BM;                // [G][BN]
  FPQ_GEMM_TILE_WALK(BM, BN);
  FPQ_FP4_GLDS_SOURCES();

  if (km) {
    // the k-major scale images IN FRONT of the ring: being older than group 0, its wait covers them
    FPQ_GEMM_KM_SCALE_TILES(sa, sw);
  } else {
    load_scale_tiles<Tsw, BM, BN, NTHR>(sa, sw, lsa, lsw, t0, o0, T, O, G, tid);
    // the wait the compiler sees (gemm_fp4_glds_kernel: it has to stand in this branch); the ring is requested behind it
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  }
  // the tile's bias, the q / k norm's fp32 bias and head scale: in front of the ring too
  FPQ_GEMM_LANE_BIAS(QKN, xe.bias, xe.q_scale);
  // the ring's first min(S - 1, G) groups
#pragma unroll
  for (int i = 0; i < S - 1; ++i)
    if (i < G) { FPQ_FP4_GLDS_ISSUE(i, i); }   // uniform

  uint16_t* lut = nullptr;
  if constexpr (FC1) {   // the dual quantizer's bucket table, behind the scale tiles; visible after the first barrier of the main loop
    lut = (uint16_t*)(lsw + Gp * BN);
    lut16_stage(lut, xe.tab, xe.a.shift);
  }

  v4f_t acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = v4f_t{0, 0, 0, 0};
  FPQ_FP4_FRAG_OFFSETS();

  // the last S - 1 groups' waits: rem_ = G - 1 - g groups are behind group g in the queue, all of them may stay in flight
  // (counts past S - 2 never occur: they repeat the steady one)
#define FPQ_RING_TAIL_WAIT(rem_)                                                                                    \
  switch (rem_) {                                                                                                   \
    case 0: glds_wait_vm<0>(); break;   /* the last group: everything has landed */                                 \
    case 1: glds_wait_vm<PIECES * (1 < S - 2 ? 1 : S - 2)>(); break;                                                \
    case 2: glds_wait_vm<PIECES * (2 < S - 2 ? 2 : S - 2)>(); break;                                                \
    case 3: glds_wait_vm<PIECES * (3 < S - 2 ? 3 : S - 2)>(); break;                                                \
    case 4: glds_wait_vm<PIECES * (4 < S - 2 ? 4 : S - 2)>(); break;                                                \
    case 5: glds_wait_vm<PIECES * (5 < S - 2 ? 5 : S - 2)>(); break;                                                \
    default: glds_wait_vm<PIECES * (S - 2)>(); break;                                                               \
  }
  static_assert(S - 2 <= 6, "FPQ_RING_TAIL_WAIT spells the counts out up to S - 2 = 6");

  int g = 0, rb = 0;   // rb = g % S: the buffer group g is read from; the request of iteration g goes to the one before it
  for (; g + S - 1 < G; ++g) {   // the steady state: S - 2 groups stay in flight across the barrier
    glds_wait_vm<PIECES * (S - 2)>();
    FPQ_SYNC();   // group g has landed for every wavefront; buffer (g - 1) % S's readers are done
    const int wb = rb == 0 ? S - 1 : rb - 1;
    FPQ_FP4_GLDS_ISSUE(g + S - 1, wb);
    const uint8_t* st = smem + rb * STAGE;
    FPQ_GEMM_GROUP(g, st, FPQ_FP4_READ_A, FPQ_FP4_READ_W, 1024, 1024, 4, 4);
    rb = rb + 1 == S ? 0 : rb + 1;
  }
  for (; g < G; ++g) {   // the drain: nothing is requested any more
    FPQ_RING_TAIL_WAIT(G - 1 - g);
    FPQ_SYNC();
    const uint8_t* st = smem + rb * STAGE;
    FPQ_GEMM_GROUP(g, st, FPQ_FP4_READ_A, FPQ_FP4_READ_W, 1024, 1024, 4, 4);
    rb = rb + 1 == S ? 0 : rb + 1;
  }
#undef FPQ_RING_TAIL_WAIT

  if constexpr (FC1) {
    FPQ_GEMM_FC1_TAIL(STAGE);
    return;
  }
  FPQ_GEMM_REG_EPILOGUE(QKN, true, epi.sp_cols);
}
#undef FPQ_FP4_GLDS_SOURCES
#undef FPQ_FP4_GLDS_ISSUE
#undef FPQ_FP4_FRAG_OFFSETS
#undef FPQ_FP4_READ_A
#undef FPQ_FP4_READ_W

// the ring kernel's tile and LDS figure: S stages + the scale tiles, groups rounded up to four
struct GemmRingCfg {
  static constexpr int BM = 64, BN = 128, S = FPQ_GEMM_RING_STAGES;
  static size_t lds(int G) { return (size_t)S * (BM + BN) * 64 + (size_t)((G + 3) & ~3) * (BM + BN) * 4; }
  static size_t lds_fc1(int G, int shift) { return lds(G) + ((size_t)2 << (16 - shift)); }
};

template <int MT, int NT>
struct GemmGldsCfg {
  static constexpr int BM = 32 * MT, BN = 32 * NT;
  static size_t lds(int G) {   // two stages + the scale tiles, groups rounded up to four (the plain epilogue uses no LDS)
    return 2 * (size_t)(BM + BN) * 64 + (size_t)((G + 3) & ~3) * (BM + BN) * 4;
  }
  static size_t lds_fc1(int G, int shift) { return lds(G) + ((size_t)2 << (16 - shift)); }   // + the dual quantizer's bucket table
};

template <int MT, int NT, int WR, int WC>
struct GemmCfg {
  static constexpr int BM = 16 * MT * WR, BN = 16 * NT * WC, NTHR = 64 * WR * WC;
  static size_t lds(int G) {
    size_t main = 2 * (size_t)(BM + BN) * 64 + (size_t)G * (BM + BN) * 4;
    size_t epi = (size_t)WR * WC * (16 * MT) * (16 * NT + 8) * 2;
    return main > epi ? main : epi;
  }
};
