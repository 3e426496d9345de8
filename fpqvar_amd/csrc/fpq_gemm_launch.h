// fpq_gemm_launch.h - what the GEMM entry points of fpq_gemm.hip and fpq_gemm_g6.hip share on the host: the
// epilogue, split-output and q / k norm descriptors -> the kernels' form, the tile choice of the per-group LDS-DMA kernels, the
// launch.  Included inside the unit's anonymous namespace, behind fpq_gemm_fp4.h (GemmEpi, GemmQkNorm).
#pragma once

// ---- what the GEMM entry points below share: argument descriptors -> the kernels' form, the tile choice, the launch ----------

// validates an optional epilogue descriptor and turns it into the kernels' form
int gemm_epilogue(const fpq_gemm_epilogue_t* ep, GemmEpi* epi) {
  *epi = GemmEpi{};
  epi->rows_per_gate = 1;
  epi->sp_rpb = 1;
  if (!ep) return FPQ_OK;
  if (ep->gate && (ep->rows_per_gate < 1 || ep->rows_per_gate > 0x7FFFFFFF)) return FPQ_ERR_ARG;
  if ((((uintptr_t)ep->gate | (uintptr_t)ep->residual) & 15) != 0) return FPQ_ERR_ARG;
  epi->gate = (const _Float16*)ep->gate;
  epi->resid = (const _Float16*)ep->residual;
  if (ep->gate) epi->rows_per_gate = (int)ep->rows_per_gate;
  return FPQ_OK;
}

// validates a split-output descriptor (include/fpq.h, fpq_gemm_split_t: the outputs leave in column parts, each to its own rows; no
// gate / residual tail with it) and fills GemmEpi's sp_* fields.  whole_batches: tokens % rows_per_batch == 0 is required too -
// the one rule on which the two families differ: the FP6 entry points ask for it, the FP4 ones never did.
int gemm_split(const fpq_gemm_split_t* split, const fpq_gemm_epilogue_t* epilogue, int64_t tokens, int64_t outs, bool whole_batches,
               GemmEpi* epi) {
  if (epilogue || split->n_parts < 1 || split->n_parts > 3 || split->part_cols <= 0 || split->part_cols % 128 != 0 ||
      outs != split->n_parts * split->part_cols || split->rows_per_batch < 1 || split->rows_per_batch > 0x7FFFFFFF ||
      (whole_batches && tokens % split->rows_per_batch != 0))
    return FPQ_ERR_ARG;
  epi->sp_cols = (int)split->part_cols;
  epi->sp_rpb = (int)split->rows_per_batch;
  for (int p = 0; p < split->n_parts; ++p) {
    if (!split->out[p] || ((uintptr_t)split->out[p] & 7) != 0 || split->row_stride[p] < split->part_cols || split->row_stride[p] % 4 != 0 ||
        split->batch_stride[p] < 0 || split->row0[p] < 0)
      return FPQ_ERR_ARG;
    epi->sp_out[p] = (_Float16*)split->out[p];
    epi->sp_stride[p] = split->row_stride[p];
    epi->sp_bstride[p] = split->batch_stride[p];
    epi->sp_row0[p] = split->row0[p];
  }
  return FPQ_OK;
}

// the q / k norm forms' own arguments (include/fpq.h, "THE Q / K L2 NORM"): parts q, k, v of heads of 64 columns; the fp32 bias is
// read four outputs (16 bytes) at a time
int gemm_qknorm(const fpq_gemm_split_t* split, const float* bias, const float* q_head_scale, GemmQkNorm* qkn) {
  if (!split || split->n_parts != 3) return FPQ_ERR_ARG;
  if (!q_head_scale || ((uintptr_t)q_head_scale & 3) != 0 || ((uintptr_t)bias & 15) != 0) return FPQ_ERR_ARG;
  *qkn = GemmQkNorm{bias, q_head_scale};
  return FPQ_OK;
}

// The tiling of the per-group LDS-DMA kernels (gemm_fp4_glds_kernel, gemm_a6w4_kernel, their fc1 forms): 10 / 20 / 30 = 256 x 128,
// 128 x 128, 64 x 128 tiles behind a two-stage ring.
// Default: 128 x 128 tiles (three workgroups per CU); 256 x 128 tiles (two per CU) from 4000 of them
// on (round 4: 2 - 5 % faster at [65536 x 1920] x {1920, 5760, 7680} and from 16 900 tokens on for the wide Linears, 3 - 5 %
// slower between 1000 and 4000 tiles) while two of them fit a CU's 160 KB of LDS (the scale tiles grow with K: from K = 3840 on
// only one would, and the smaller tile is 15 % faster there - tools/gemm_k_sweep.py); 64 x 128 tiles while the 128 x 128 ones
// would fill less than half of the chip's 768 slots (the first scale steps of a generation: 8.4 against 11.4 us at 100 tokens;
// tools/gemm_small_steps.py).
// 40 = gemm_fp4_ring_kernel, the 64 x 128 tile behind a deep stage ring (fpq_gemm_fp4.h): the FP4 GEMM has it (have_ring), the
// A6W4 GEMM does not - for it 40 means "not set".  The default NEVER chooses it: measured against 30 and the default at every
// row count of d30's and d36-512's scale steps (K = 1920, 2304; k-major, both orders, against a 30-vs-30 spread of 0.2 us) it
// wins at no tile count and no outs - 0.2 us slower while a grid has at most one tile per CU, 1.2 x beyond
// (profiles/gemm_fp4_ring_small_steps.txt) - so there is no rule for it beside the tile-count rule below.
// FPQ_GEMM_CFG (experiments, tests) forces one of the tilings the caller has; have_256: whether it has the 256 x 128 one at all,
// big_fits_twice: whether two of those tiles fit a CU's LDS at this K.
int gemm_glds_tiling(int64_t tokens, int64_t outs, bool have_256, bool big_fits_twice, bool have_ring = false) {
  const int want = fpq_opt(OPT_FPQ_GEMM_CFG, 0);
  if ((want == 10 && have_256) || want == 20 || want == 30 || (want == 40 && have_ring)) return want;
  const int64_t big_tiles = ((tokens + 255) / 256) * ((outs + 127) / 128);
  const int64_t mid_tiles = ((tokens + 127) / 128) * ((outs + 127) / 128);
  return mid_tiles <= 384 ? 30 : (have_256 && big_tiles >= 4000 && big_fits_twice) ? 10 : 20;
}

// workgroups of a launch over BM x BN tiles: the column tiles rounded up to the 8 XCDs (the kernels' XCD-aware tile order), or
// FPQ_ERR_SHAPE when a grid cannot hold them
int64_t gemm_grid(int64_t tokens, int64_t outs, int BM, int BN) {
  const int64_t n_col = (outs + BN - 1) / BN, n_row = (tokens + BM - 1) / BM;
  const int64_t n_wg = 8 * ((n_col + 7) / 8) * n_row;
  return n_wg > 0x7FFFFFFF ? (int64_t)FPQ_ERR_SHAPE : n_wg;
}

// ---- the squared-error forms (include/fpq.h, fpq_gemm_*_sqerr; fpq_gemm_fp4.h, GemmSqErr) -------------------------------------
// the form's own arguments as its entry point received them
struct GemmSqErrCall {
  const void* ref;
  int ref_dtype;
  const float* row_weight;
  float* loss_out;
  void* workspace;
};
// one fp32 partial per tile of the smallest tiling any family launches (64 x 128), at least one
int64_t gemm_sqerr_workspace_bytes(int64_t tokens, int64_t outs) {
  const int64_t tiles = ((tokens + 63) / 64) * ((outs + 127) / 128);
  return 4 * (tiles < 1 ? 1 : tiles);
}
// The form's checks, BEHIND the family's own: a NULL or misaligned pointer, then the reference's dtype.  An empty problem
// (empty: tokens == 0 or outs == 0) reads neither ref nor row_weight - their pointers are not looked at.
int gemm_sqerr_args(const GemmSqErrCall& s, bool empty, GemmSqErr* xe) {
  if (!s.loss_out || !s.workspace || (((uintptr_t)s.loss_out | (uintptr_t)s.workspace) & 3) != 0) return FPQ_ERR_ARG;
  if (!empty && (!s.ref || !s.row_weight || (((uintptr_t)s.ref | (uintptr_t)s.row_weight) & 15) != 0)) return FPQ_ERR_ARG;
  if (s.ref_dtype != FPQ_F16 && s.ref_dtype != FPQ_F32) return FPQ_ERR_DTYPE;
  *xe = GemmSqErr{s.ref, s.row_weight, (float*)s.workspace, s.ref_dtype == FPQ_F32 ? 1 : 0};
  return FPQ_OK;
}
// the second launch: the partials of the BM x 128 tiles the first one wrote (an empty problem: none, and 0.0f is stored)
int gemm_sqerr_finish(const GemmSqErrCall& s, int64_t tokens, int64_t outs, int BM, fpq_stream_t stream) {
  const int64_t tiles = ((tokens + BM - 1) / BM) * ((outs + 127) / 128);   // <= the launch's grid, which fits 31 bits
  return fpq_internal_sqerr_finish((const float*)s.workspace, (int)tiles, s.loss_out, stream);
}

// the arguments every GEMM kernel takes, as the entry point received (and checked) them
struct GemmCall {
  const uint8_t* a_codes;
  const void* a_scales;
  const uint8_t* w_codes;
  const void* w_scales;
  const void* bias;
  void* out;
  int64_t tokens, outs, k;
  GemmEpi epi;
  hipStream_t st;
};

// THE launch: the grid for the kernel's tile, the scale pointers in the kernel's own types, the epilogue's extra argument if it
// takes one (xe: GemmNoFc1 / GemmFc1 / GemmQkNorm / GemmSplit)
template <typename Tsa, typename Tsw, typename... XE>
int gemm_launch(void (*kernel)(const uint8_t*, const Tsa*, const uint8_t*, const Tsw*, const _Float16*, _Float16*, int, int, int, GemmEpi, XE...),
                int BM, int BN, unsigned threads, size_t lds, const GemmCall& c, XE... xe) {
  const int64_t n_wg = gemm_grid(c.tokens, c.outs, BM, BN);
  if (n_wg < 0) return (int)n_wg;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_wg), dim3(threads), lds, c.st, c.a_codes, (const Tsa*)c.a_scales, c.w_codes,
                     (const Tsw*)c.w_scales, (const _Float16*)c.bias, (_Float16*)c.out, (int)c.tokens, (int)c.outs, (int)c.k, c.epi, xe...);
  return check_launch();
}
