// fpq_adaln_launch.h - the host dispatch of the adaLN producer (fpq_adaln.h): which form of adaln_mfma_kernel a call launches and on which
// grid.  Included inside the anonymous namespace of fpq_adaln.hip (RESID = false: the producers) and of fpq_resid_adaln.hip (RESID = true:
// the same producers with the gated residual folded into their row load), after fpq_adaln.h.  One text, so that the fused entry points
// pick the variant - TIGHT, PAIR2, the paired slot, the hardware levels, MAXC, the workgroup cut - their twins pick for a shape and dtype:
// several of those sum a row's statistics in another order, and the fused forms' contract is bit equality with the twin.
#pragma once

struct AdalnResid {   // RESID: the three tensors of the gated residual (include/fpq.h, fpq_resid_adaln_*)
  const void* y;
  const void* gate;
  void* x_out;
};

template <bool RESID, typename Tin, typename Tmod>
int launch_adaln_rotate_quant(const void* x, void* out, void* h_out, void* y_out, int64_t rows, int64_t cols,
                              const AdaLnArgs& ad, const float* smooth, const uint32_t sign[4], int table_id,
                              hipStream_t st, uint16_t* code_scales = nullptr,
                              int token_mode = 0 /*1: per-token values, 2: per-token E4M3 codes, 3: per-token packed 6-bit codes*/,
                              const Lut16Tab* token_code_tab = nullptr,
                              bool km = false /* FP4 / 6-bit codes into a k-major image (include/fpq.h): adaln_mfma_kernel only */,
                              bool g6 = false /* per group, code_scales: dense 6-bit group codes of table_id instead of FP4 - the A6W4
                                                 GEMM's (E1M2 / E3M0) or the full tables' (E2M3 / E3M2); adaln_mfma_kernel only */,
                              const AdalnResid* resid = nullptr /* RESID */) {
  const Lut16Host& h = lut16_host(table_id, table_id);
  if (!h.tab_valid) return FPQ_ERR_TABLE;
  if (g6 && (cols / 8 > 64 * 5 || !code_scales || token_mode || RESID)) return FPQ_ERR_SHAPE;
  const bool full6 = table_id == FPQ_E2M3 || table_id == FPQ_E3M2;   // the table fpq_gf6_quant_rows_codes stages
  const Lut16Tab& tab = token_mode >= 2 ? *token_code_tab
                        : g6 ? (full6 ? lut16_codes6(table_id) : lut16_codes_g6(table_id))
                             : (code_scales && !token_mode ? lut16_mx_codes_e2m1() : h.tab);
  RotArgs r;
  r.code_scales = code_scales;
  r.code_bits = (token_mode == 3 || g6) ? 6 : 8;
  r.km_rows = km ? (uint32_t)rows : 0u;
  r.km_gpr = fast_div((uint32_t)(cols / 128));
  if (km) {
    const bool fp4_codes = code_scales && !token_mode;
    if (!(fp4_codes || token_mode == 3) || !km_image_fits(rows, (token_mode == 3 || g6) ? cols / 4 * 3 : cols / 2)) return FPQ_ERR_SHAPE;
    if (cols / 8 > 64 * 5) return FPQ_ERR_SHAPE;   // rows beyond one wavefront: the first generation writes row-major codes only
  }
  r.smooth = smooth;
  for (int i = 0; i < 4; ++i) r.sign[i] = sign[i];
  r.c_h = h2f(f2h(1.0f / __builtin_sqrtf(128.0f)));
  r.vec_per_row = cols / 8;
  {
    // fpq_adaln.h: fp16 or fp32 rows of up to 2560 channels, one batch entry per workgroup
    constexpr bool X32 = sizeof(Tin) == 4;
    if (r.vec_per_row <= 64 * 5) {
      if (h.args.shift < 6) return FPQ_ERR_TABLE;   // symmetric tables only (<= 2 x 512 buckets)
      const int64_t L = ad.rows_per_batch;
      const int64_t n_batches = (rows + L - 1) / L;
      const bool rows_env = fpq_opt_set(OPT_FPQ_ADALN_ROWS);
      // Large launches: chunks of 16 rows (4 per wavefront) amortise the staging of the modulation; small launches (the
      // early scale steps of a generation: 100 .. 3600 rows) are latency-bound and want every CU busy: one row per wavefront
      // (profiles/r02_small_steps.json; round 4, cold inputs, 4 / 8 / 12 / 16 rows per workgroup over the ten steps of d30 and
      // d36-512: 4 is the best or within 2 % of it up to 10 000 rows, 8 from 16 900 on - profiles/r04_adaln_rows_sweep.txt).
      // FPQ_ADALN_ROWS=n: n rows per workgroup everywhere; FPQ_ADALN_TAIL=rows: how many rows at the end of the grid go to
      // each of two finer tiers (8 and 4 rows per workgroup).  The tiers are OFF by default (0): they never beat a plain grid
      // of 8 - 12 rows (profiles/r03_adaln_partition.txt); the tier decode stays reachable through the variable and is
      // covered by tests/test_gpu_parity.py::test_adaln_tail_tiers_switch in a child process.
      // (third generation, large launches: 8 rows = two per wavefront for the stream-bound forms - E2M1 values out, fp32
      // rows; 12 for the forms bound by vector issue - operands out or a bucket table, from fp16 rows - where the
      // prologue's instructions per row count: 73.3 -> 70.5 us for codes, 89.7 -> 87.1 for E4M3 bytes, 96.2 -> 93.4 for
      // per-token E2M3 values; profiles/r03_adaln_partition.txt)
      const bool issue_bound = !X32 && (code_scales != nullptr || token_mode != 0 || table_id != FPQ_E2M1);
      int rows_per_wg = rows_env ? fpq_opt(OPT_FPQ_ADALN_ROWS, 0) : (rows >= 8192 ? (issue_bound && rows >= 32768 ? 12 : 8) : 4);
      if (rows_per_wg < 1) rows_per_wg = 1;
      // rows of exactly 8 groups (C = 1024): two rows per tile (fpq_adaln.h, PAIR2) - workgroups of an even number of rows
      const bool pair2 = !X32 && r.vec_per_row == 128 && token_mode == 0 && !h_out && !y_out && !g6 &&
                         !fpq_flag(OPT_FPQ_ADALN_NO_PAIR2);
      if (pair2) rows_per_wg = rows_env ? ((rows_per_wg + 1) & ~1) : (rows >= 8192 ? 16 : 8);
      const int64_t per_batch = (L + rows_per_wg - 1) / rows_per_wg;
      if (n_batches * per_batch > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
      std::conditional_t<RESID, AdalnTiersResid, AdalnTiers> tiers = {};
      if constexpr (RESID) {
        tiers.y = resid->y;
        tiers.gate = resid->gate;
        tiers.x_out = resid->x_out;
      }
      const int tail_rows = fpq_opt(OPT_FPQ_ADALN_TAIL, 0);
      int64_t nb2 = 0, nb1 = 0;
      if (tail_rows > 0 && rows_per_wg > 4) {
        nb2 = (tail_rows + L - 1) / L;                                   // batch entries cut into chunks of 4 rows
        if (rows_per_wg > 8) nb1 = (tail_rows + L - 1) / L;              // ... of 8 rows
        if (nb2 > n_batches) nb2 = n_batches;
        if (nb1 > n_batches - nb2) nb1 = n_batches - nb2;
      }
      tiers.rows[0] = rows_per_wg;
      tiers.rows[1] = 8;
      tiers.rows[2] = 4;
      for (int t = 0; t < 3; ++t) tiers.per_batch[t] = (int)((L + tiers.rows[t] - 1) / tiers.rows[t]);
      tiers.batches[0] = (int)(n_batches - nb1 - nb2);
      tiers.batches[1] = (int)nb1;
      {
        const int64_t nb_of[3] = {n_batches - nb1 - nb2, nb1, nb2};
        for (int t = 0; t < 3; ++t) {   // id / d == (id * ceil(2^32 / d)) >> 32 whenever id * d < 2^32
          const uint64_t d = (uint64_t)tiers.per_batch[t], ids = (uint64_t)nb_of[t] * d;
          tiers.magic[t] = (d >= 2 && ids * d < (1ull << 32)) ? (uint32_t)(((1ull << 32) + d - 1) / d) : 0u;
        }
      }
      const int64_t n_wg3 = (int64_t)tiers.batches[0] * tiers.per_batch[0] + nb1 * tiers.per_batch[1] + nb2 * tiers.per_batch[2];
      if (n_wg3 > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
      const dim3 g3((unsigned)n_wg3);
      const size_t lds2 = 0;   // table, modulation planes and images live in static LDS
      // E2M1 values per group: levels from the FP4 conversion hardware, no table (fpq_adaln.h)
      const bool hw4 = table_id == FPQ_E2M1 && !token_mode && !fpq_flag(OPT_FPQ_NO_HW4);
      const bool tight_ok = FPQ_ADALN_TIGHT && !fpq_flag(OPT_FPQ_ADALN_NO_TIGHT);
      // E2M3 / E3M2 values (per group, or per token: token_mode 1): levels from the FP6 conversion hardware, no table
      const int hw6 = (token_mode <= 1 && !code_scales && !fpq_flag(OPT_FPQ_NO_HW6)) ? (table_id == FPQ_E2M3 ? 1 : table_id == FPQ_E3M2 ? 2 : 0) : 0;
#ifdef FPQ_ADALN_STAMPS
#define FPQ_ADALN_EMIT (h_out != nullptr)   /* diagnostic build: y_out alone is the stamp buffer */
#else
#define FPQ_ADALN_EMIT (h_out || y_out)
#endif
      const bool emit = FPQ_ADALN_EMIT;
      auto go = [&](auto kern) { return launch(kern, g3, lds2, st, x, out, h_out, y_out, rows, ad, r, h.args, tab, tiers); };
      // the form of adaln_mfma_kernel for rows of up to M x 64 vectors: CODES - operands out; EMIT - h / the rotated rows go out
      // too; TOKEN - one scale per row
      auto pick = [&](auto m, auto codes, auto emits, auto token) {
        constexpr int M = m.value;
        constexpr bool CODES = codes.value, EMIT = emits.value, TOKEN = token.value;
        if constexpr ((M == 4 || M == 5) && !CODES && !EMIT) {   // E2M3 / E3M2 values, rows of 13 .. 20 groups: hardware levels
          if (hw6 == 1) return go(adaln_mfma_kernel<Tmod, M, false, false, TOKEN, X32, false, false, 4, false, 1, false, RESID>);
          if (hw6 == 2) return go(adaln_mfma_kernel<Tmod, M, false, false, TOKEN, X32, false, false, 4, false, 2, false, RESID>);
        }
        if constexpr (CODES && !EMIT && !TOKEN && !RESID) {   // 6-bit group operands: one form per row length, modulation and row dtype
          if (g6) return go(adaln_mfma_kernel<Tmod, M, true, false, false, X32, false, false, 4, false, 0, true>);
        }
        if constexpr (M == 2 && !X32 && !EMIT && !TOKEN) {
          if (pair2)
            return with_bool(hw4, [&](auto hw) {
              return go(adaln_mfma_kernel<Tmod, 4, CODES, false, false, false, hw.value, false, 4, true, 0, false, RESID>);
            });
        }
        if constexpr (!TOKEN) {
          if constexpr (M == 4 && !X32 && !EMIT && !CODES) {
            if (hw4 && tight_ok && r.vec_per_row == 240)   // VAR-d30: 31 KiB of LDS, five workgroups per CU
              return go(adaln_mfma_kernel<Tmod, M, CODES, EMIT, TOKEN, X32, true, true, 4, false, 0, false, RESID>);
          }
          if (hw4) return go(adaln_mfma_kernel<Tmod, M, CODES, EMIT, TOKEN, X32, true, false, 4, false, 0, false, RESID>);
        }
        return go(adaln_mfma_kernel<Tmod, M, CODES, EMIT, TOKEN, X32, false, false, 4, false, 0, false, RESID>);
      };
      // MAXC = ceil(vectors per row / 64), exactly: 1 .. 5 (vec_per_row <= 64 * 5 above)
      return with_int<1, 2, 3, 4, 5>((int)((r.vec_per_row + 63) / 64), [&](auto m) {
        if (token_mode >= 2) return pick(m, Bool<true>{}, Bool<false>{}, Bool<true>{});
        if (token_mode == 1) return with_bool(emit, [&](auto e) { return pick(m, Bool<false>{}, e, Bool<true>{}); });
        if (code_scales) return pick(m, Bool<true>{}, Bool<false>{}, Bool<false>{});
        return with_bool(emit, [&](auto e) { return pick(m, Bool<false>{}, e, Bool<false>{}); });
      });
    }
  }
  if constexpr (RESID) {
    return FPQ_ERR_SHAPE;   // the first-generation kernel has no fused form (refused by the entry points before they get here)
  } else {
    // rows beyond one wavefront (2560 < C <= 4096, per group only): the first generation, one workgroup per row
    const size_t lds = 0;   // the bucket table lives in static LDS (fpq_fast16.h)
    const dim3 g((unsigned)(rows < 8192 ? rows : 8192));   // every workgroup stages the table once, then walks rows
    return with_bool(code_scales != nullptr, [&](auto codes) {
      return launch(adaln_rotate_quant16_kernel<Tin, Tmod, codes.value>, g, lds, st, x, out, h_out, y_out, rows, ad, r, h.args, tab);
    });
  }
}

// the checks and the argument block every entry point of the family shares.  RESID: x is the residual stream, `resid` the tensors in
// front of it; their checks come after the twin's own, in the order include/fpq.h gives.
template <bool RESID = false>
int adaln_rotate_quant_impl(const void* x, void* out, void* h_out, void* rotated_out, void* code_scales,
                            int64_t rows, int64_t cols, int in_dtype, const void* scale, const void* shift,
                            int mod_dtype, int64_t rows_per_batch, float eps, const float* smooth,
                            const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream,
                            int token_mode = 0, const Lut16Tab* token_code_tab = nullptr, bool km = false, bool g6 = false,
                            const AdalnResid* resid = nullptr) {
  if (rows < 0 || cols < 0 || rows_per_batch <= 0 || !sign_mask_host) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype) || !is_f16_or_f32(mod_dtype)) return FPQ_ERR_DTYPE;
  if (cols % 128 != 0 || cols > 4096) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !out || !scale || !shift) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)h_out | (uintptr_t)rotated_out | (uintptr_t)scale |
        (uintptr_t)shift | (uintptr_t)smooth) & 15) != 0)
    return FPQ_ERR_ARG;
  AdaLnArgs ad;
  ad.scale = scale;
  ad.shift = shift;
  ad.mod_is_f16 = mod_dtype == FPQ_F16;
  ad.rows_per_batch = rows_per_batch;
  ad.eps = eps;
  ad.cols = cols;
  // One wavefront per row while the row fits 5 vectors per lane (C <= 2560: no barrier in the row
  // loop; measured 0.180 ms vs 0.199 ms per [65500 x 1920] on MI355X), one workgroup per row beyond.
  if (token_mode && cols / 8 > 64 * 5) return FPQ_ERR_SHAPE;   // the per-token form keeps a row inside one wavefront: C <= 2560
  if constexpr (RESID) {
    if (!resid || !resid->y || !resid->gate || !resid->x_out) return FPQ_ERR_ARG;
    if ((((uintptr_t)resid->y | (uintptr_t)resid->gate | (uintptr_t)resid->x_out) & 15) != 0) return FPQ_ERR_ARG;
    if (cols > 2560) return FPQ_ERR_SHAPE;   // the first-generation wide kernel gets no fused form
  }
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(in_dtype, [&](auto ti) {
    return with_dtype(mod_dtype, [&](auto tm) {
      return launch_adaln_rotate_quant<RESID, decltype(ti), decltype(tm)>(x, out, h_out, rotated_out, rows, cols, ad, smooth, sign_mask_host,
                                                                          table_id, st, (uint16_t*)code_scales, token_mode, token_code_tab, km, g6,
                                                                          resid);
    });
  });
}
