// fpq_rotate.hip - the online rotation in front of the per-group quantizer (fpq_rotate_quant_rows*, the transform on the
// matrix cores: fpq_rotate_mfma.h) and the operand emitters of the row-scaled FP8 / FP6 GEMMs (fpq_quant_rows_codes_fp8 /
// _fp6* / _f6: fpq_codes_fp8.h, fpq_codes_fp6.h), with their C ABI.  The FP4 emitter, fpq_quant_rows_codes_mx, stays with the
// codes of fpq_kernels.hip, whose codes128_kernel its fp32 form launches.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_rotate_mfma.h"
#include "fpq_codes_fp8.h"
#include "fpq_codes_fp6.h"

template <typename Tin>
int launch_rotate_quant(const void* x, void* out, void* rot_out, int64_t rows, int64_t cols, const float* smooth,
                        const uint32_t sign[4], int table_id, hipStream_t st, uint16_t* code_scales = nullptr,
                        bool km = false /* codes into a k-major image (include/fpq.h) */,
                        bool g6 = false /* code_scales: dense 6-bit group codes of table_id instead of FP4 - the A6W4 GEMM's (E1M2 /
                                           E3M0) or the full tables' (E2M3 / E3M2: fpq_gf6_rotate_quant_rows_codes) */) {
  const Lut16Host& h = lut16_host(table_id, table_id);
  if (!h.tab_valid) return FPQ_ERR_TABLE;
  const bool full6 = table_id == FPQ_E2M3 || table_id == FPQ_E3M2;   // the table fpq_gf6_quant_rows_codes stages
  const Lut16Tab& tab = g6 ? (full6 ? lut16_codes6(table_id) : lut16_codes_g6(table_id)) : code_scales ? lut16_mx_codes_e2m1() : h.tab;
  RotArgs r;
  r.code_scales = code_scales;
  r.code_bits = g6 ? 6 : 8;
  r.km_rows = km ? (uint32_t)rows : 0u;
  r.km_gpr = fast_div((uint32_t)(cols / 128));
  if (km && (!code_scales || !km_image_fits(rows, g6 ? cols / 4 * 3 : cols / 2))) return FPQ_ERR_SHAPE;
  r.smooth = smooth;
  for (int i = 0; i < 4; ++i) r.sign[i] = sign[i];
  r.c_h = h2f(f2h(1.0f / __builtin_sqrtf(128.0f)));   // torch.tensor(128).sqrt() is float32; autocast makes Q fp16
  r.vec_per_row = cols / 8;
  const int64_t n_vec = rows * (cols / 8);
  const size_t lds = 0;   // the bucket table lives in static LDS (fpq_fast16.h)
  // The transform on the matrix cores (fpq_rotate_mfma.h), one 32-group tile per wavefront.
  // Every workgroup the same number of passes over its tiles.  With a bucket table to stage per workgroup the grid is
  // two generations of the FPQ_ROT_WAVES workgroups a CU holds (3072: 84.2 us against 85.9 for one generation, round 2).
  // The table-free E2M1 forms have next to no prologue and want SHORT workgroups - the grid drains faster at its end:
  // values out, 3072 / 7680 / 12288 / 16384 workgroups: 83.2 / 82.2 / 82.1 / 80.3 us (one pass each at [65536 x 1920]);
  // codes out: 57.3 / 52.8 / 53.0 / 53.6 us (profiles/r03_rotate_grid.txt).  FPQ_ROT_WGS overrides.
  const bool hw4 = table_id == FPQ_E2M1 && !fpq_flag(OPT_FPQ_NO_HW4);   // E2M1 values or FP4 operands: levels / codes from the conversion hardware
  // 6-bit group operands of the full tables: codes from the FP6 conversion hardware (rq_store_codes6_hw), table-free like the E2M1 forms
  const bool hw6 = g6 && full6 && h.args.shift >= 6 /* its rare table path: <= 2 x 512 buckets */ && !fpq_flag(OPT_FPQ_NO_HW6);
  const int64_t per_wg = (int64_t)(kBlock / 64) * kRqTileVec;
  const int64_t wg_tiles = (n_vec + per_wg - 1) / per_wg;
  const int64_t resident_env = fpq_opt(OPT_FPQ_ROT_WGS, 0);
  // (with a smoothing vector every workgroup stages it - 7.5 KiB at C = 1920 - so a few passes each: 7680 / 2560; the 6-bit codes
  // into a k-major image are the exception - at [65536 x 1920 / 2304] 8192 workgroups take 82.5 - 147.5 us where 2560 take 92.0 -
  // 168.5 and the table form 92.1 - 168.0, fp16 and fp32 rows alike; row-major codes keep 2560: 67.0 against 71.8 us on fp16 rows -
  // profiles/gf6_producers_ab.txt, the --grid section)
  const int64_t resident = resident_env > 0 ? resident_env : !(hw4 || hw6) ? 2 * 256ll * FPQ_ROT_WAVES
                           : smooth ? (code_scales ? (hw6 && km ? 8192 : 2560) : 7680) : code_scales ? 8192 : 16384;
  const int64_t passes = (wg_tiles + resident - 1) / resident;
  const dim3 mgrid((unsigned)((wg_tiles + passes - 1) / passes));
  auto go = [&](auto emit, auto codes) {   // EMIT: the rotated rows go out too; CODES: FP4 operands instead of values
    constexpr bool EMIT = emit.value, CODES = codes.value;
    return with_bool(smooth != nullptr, [&](auto sm) {
      constexpr bool SMOOTH = sm.value;
      return with_bool(hw4, [&](auto hw) {
        return launch(rotate_quant_mfma_kernel<Tin, EMIT, SMOOTH, CODES, hw.value>, mgrid, lds, st, x, out, rot_out, n_vec, r, h.args, tab);
      });
    });
  };
  if (g6)   // (never E2M1; E1M2 / E3M0 and FPQ_NO_HW6: the table form)
    return with_bool(smooth != nullptr, [&](auto sm) {
      if (hw6 && table_id == FPQ_E2M3)
        return launch(rotate_quant_mfma_kernel<Tin, false, sm.value, true, false, true, 1>, mgrid, lds, st, x, out, rot_out, n_vec, r, h.args, tab);
      if (hw6)
        return launch(rotate_quant_mfma_kernel<Tin, false, sm.value, true, false, true, 2>, mgrid, lds, st, x, out, rot_out, n_vec, r, h.args, tab);
      return launch(rotate_quant_mfma_kernel<Tin, false, sm.value, true, false, true>, mgrid, lds, st, x, out, rot_out, n_vec, r, h.args, tab);
    });
  if (code_scales) return go(Bool<false>{}, Bool<true>{});
  if (rot_out) return go(Bool<true>{}, Bool<false>{});
  return go(Bool<false>{}, Bool<false>{});
}

}  // namespace

extern "C" {

static int rotate_quant_impl(const void* x, void* out, void* rotated_out, void* code_scales, int64_t rows, int64_t cols,
                             int in_dtype, const float* smooth, const uint32_t* sign_mask_host, int table_id,
                             fpq_stream_t stream, bool km = false, bool g6 = false) {
  if (rows < 0 || cols < 0 || !sign_mask_host) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (cols % 128 != 0) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)rotated_out | (uintptr_t)smooth) & 15) != 0) return FPQ_ERR_ARG;
  return with_dtype(in_dtype, [&](auto t) {
    return launch_rotate_quant<decltype(t)>(x, out, rotated_out, rows, cols, smooth, sign_mask_host, table_id, (hipStream_t)stream,
                                            (uint16_t*)code_scales, km, g6);
  });
}

int fpq_rotate_quant_rows(const void* x, void* out, void* rotated_out, int64_t rows, int64_t cols, int in_dtype,
                          const float* smooth, const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream) {
  return rotate_quant_impl(x, out, rotated_out, nullptr, rows, cols, in_dtype, smooth, sign_mask_host, table_id, stream);
}

int fpq_rotate_quant_rows_codes_mx(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                   const float* smooth, const uint32_t* sign_mask_host, fpq_stream_t stream) {
  if (rows > 0 && cols > 0 && !scales) return FPQ_ERR_ARG;
  return rotate_quant_impl(x, codes, nullptr, scales, rows, cols, in_dtype, smooth, sign_mask_host, FPQ_E2M1, stream);
}
int fpq_rotate_quant_rows_codes_mx_km(const void* x, uint8_t* image, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                      const float* smooth, const uint32_t* sign_mask_host, fpq_stream_t stream) {
  if (rows > 0 && cols > 0 && !scales) return FPQ_ERR_ARG;
  return rotate_quant_impl(x, image, nullptr, scales, rows, cols, in_dtype, smooth, sign_mask_host, FPQ_E2M1, stream, true);
}

// the A6W4 GEMM's activation operands (include/fpq.h): what fpq_quant_rows_codes_g6 / fpq_a6w4_quant_rows_codes_km make of the rotated rows
int fpq_a6w4_rotate_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                     const float* smooth, const uint32_t* sign_mask_host, int table_id, int kmajor, fpq_stream_t stream) {
  if (rows < 0 || cols < 0 || !sign_mask_host) return FPQ_ERR_ARG;
  if (table_id != FPQ_E1M2 && table_id != FPQ_E3M0) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (cols % 128 != 0 || (kmajor && !km_image_fits(rows, cols / 4 * 3))) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !codes || !scales) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)codes | (uintptr_t)scales | (uintptr_t)smooth) & 15) != 0) return FPQ_ERR_ARG;
  return rotate_quant_impl(x, codes, nullptr, scales, rows, cols, in_dtype, smooth, sign_mask_host, table_id, stream, kmajor != 0, true);
}

// the same on the FULL FP6 tables (include/fpq.h, GF6): what fpq_gf6_quant_rows_codes makes of the rotated rows
int fpq_gf6_rotate_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                    const float* smooth, const uint32_t* sign_mask_host, int table_id, int kmajor, fpq_stream_t stream) {
  if (rows < 0 || cols < 0 || !sign_mask_host) return FPQ_ERR_ARG;
  if (table_id != FPQ_E2M3 && table_id != FPQ_E3M2) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (cols % 128 != 0 || (kmajor && !km_image_fits(rows, cols / 4 * 3))) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !codes || !scales) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)codes | (uintptr_t)scales | (uintptr_t)smooth) & 15) != 0) return FPQ_ERR_ARG;
  return rotate_quant_impl(x, codes, nullptr, scales, rows, cols, in_dtype, smooth, sign_mask_host, table_id, stream, kmajor != 0, true);
}

int fpq_quant_rows_codes_fp8(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id,
                             int in_dtype, fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !codes || !scales) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == FPQ_F16 && cols % 8 == 0 && cols <= 4096 && (((uintptr_t)x | (uintptr_t)codes) & 15) == 0 &&
      lut16_host(table_id, table_id).tab_valid) {
    const Lut16Host& h = lut16_host(table_id, table_id);
    const size_t lds = 0;   // the bucket table lives in static LDS (fpq_fast16.h)
    const int64_t wgs = (rows + kBlock / 64 - 1) / (kBlock / 64);
    const dim3 gw(grid_for(wgs, 8192));
    const int maxc = (int)((cols / 8 + 63) / 64);
    return with_int<2, 4, 8>(step_for(maxc, {2, 4, 8}), [&](auto m) {
      return launch(rows16_codes8_wave_kernel<m.value>, gw, lds, st, x, codes, scales, rows, cols, h.args, lut16_codes8(table_id));
    });
  }
  return with_dtype(in_dtype, [&](auto t) {
    return launch(rows_codes_fp8_kernel<decltype(t)>, grid_for(rows, 65535), 0, st, x, codes, scales, rows, cols, make_fmt(table_id));
  });
}

static int quant_rows_codes_fp6_impl(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id,
                                     int in_dtype, bool km, fpq_stream_t stream) {
  // table_id: FPQ_E2M3 or FPQ_E3M2, checked by the entry points (the _fp6 forms take E2M3 only)
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (cols % 32 != 0 || (km && (cols % 128 != 0 || !km_image_fits(rows, cols / 4 * 3)))) return FPQ_ERR_SHAPE;
  const uint32_t km_rows = km ? (uint32_t)rows : 0u;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !codes || !scales) return FPQ_ERR_ARG;
  if ((((uintptr_t)codes) & 7) != 0) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == FPQ_F16 && cols <= 8192 && (((uintptr_t)x) & 15) == 0) {
    const Lut16Host& h = lut16_host(table_id, table_id);
    const size_t lds = 0;   // the bucket table lives in static LDS (fpq_fast16.h)
    const int64_t wgs = (rows + kBlock / 64 - 1) / (kBlock / 64);
    const dim3 gw(grid_for(wgs, 8192));
    const int maxc = (int)((cols / 32 + 63) / 64);
    return with_int<1, 2, 4>(step_for(maxc, {1, 2, 4}), [&](auto m) {
      return launch(rows16_codes6_wave_kernel<m.value>, gw, lds, st, x, codes, scales, rows, cols, h.args, lut16_codes6(table_id), km_rows);
    });
  }
  return with_dtype(in_dtype, [&](auto t) {
    return with_bool(table_id == FPQ_E3M2, [&](auto bf6) {
      return launch(rows_codes_fp6_kernel<decltype(t), bf6.value>, grid_for(rows, 65535), 0, st, x, codes, scales, rows, cols,
                    make_fmt(table_id), km_rows);
    });
  });
}
int fpq_quant_rows_codes_fp6(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id,
                             int in_dtype, fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (table_id != FPQ_E2M3) return FPQ_ERR_TABLE;
  return quant_rows_codes_fp6_impl(x, codes, scales, rows, cols, table_id, in_dtype, false, stream);
}
int fpq_quant_rows_codes_fp6_km(const void* x, uint8_t* image, void* scales, int64_t rows, int64_t cols, int table_id,
                                int in_dtype, fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (table_id != FPQ_E2M3) return FPQ_ERR_TABLE;
  return quant_rows_codes_fp6_impl(x, image, scales, rows, cols, table_id, in_dtype, true, stream);
}
int fpq_quant_rows_codes_f6(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id, int in_dtype,
                            int kmajor, fpq_stream_t stream) {
  if (table_id != FPQ_E2M3 && table_id != FPQ_E3M2) return FPQ_ERR_TABLE;
  return quant_rows_codes_fp6_impl(x, codes, scales, rows, cols, table_id, in_dtype, kmajor != 0, stream);
}

}  // extern "C"
