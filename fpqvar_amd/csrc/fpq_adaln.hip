// fpq_adaln.hip - the adaLN producer (fpq_adaln.h: LayerNorm, modulation, rotation and quantizer in one launch) and its ten
// C entry points.  A unit of its own because its ~230 kernel forms take longer to compile than the rest of the quantizers
// together: an edit elsewhere does not recompile them.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_rotate_mfma.h"
#include "fpq_adaln.h"
#include "fpq_adaln_launch.h"   // launch_adaln_rotate_quant, adaln_rotate_quant_impl: shared with fpq_resid_adaln.hip

}  // namespace

extern "C" {

int fpq_adaln_rotate_quant_rows(const void* x, void* out, void* h_out, void* rotated_out, int64_t rows, int64_t cols,
                                int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                int64_t rows_per_batch, float eps, const float* smooth,
                                const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream) {
  return adaln_rotate_quant_impl(x, out, h_out, rotated_out, nullptr, rows, cols, in_dtype, scale, shift, mod_dtype,
                                 rows_per_batch, eps, smooth, sign_mask_host, table_id, stream);
}

int fpq_adaln_rotate_quant_rows_codes_mx(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols,
                                         int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                         int64_t rows_per_batch, float eps, const float* smooth,
                                         const uint32_t* sign_mask_host, fpq_stream_t stream) {
  if (rows > 0 && cols > 0 && !scales) return FPQ_ERR_ARG;
  return adaln_rotate_quant_impl(x, codes, nullptr, nullptr, scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                 rows_per_batch, eps, smooth, sign_mask_host, FPQ_E2M1, stream);
}
int fpq_adaln_rotate_quant_rows_codes_mx_km(const void* x, uint8_t* image, void* scales, int64_t rows, int64_t cols,
                                            int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                            int64_t rows_per_batch, float eps, const float* smooth,
                                            const uint32_t* sign_mask_host, fpq_stream_t stream) {
  if (rows > 0 && cols > 0 && !scales) return FPQ_ERR_ARG;
  return adaln_rotate_quant_impl(x, image, nullptr, nullptr, scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                 rows_per_batch, eps, smooth, sign_mask_host, FPQ_E2M1, stream, 0, nullptr, true);
}

int fpq_adaln_rotate_quant_token_rows(const void* x, void* out, void* h_out, void* rotated_out, void* row_scales,
                                      int64_t rows, int64_t cols, int in_dtype, const void* scale, const void* shift,
                                      int mod_dtype, int64_t rows_per_batch, float eps, const float* smooth,
                                      const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream) {
  if ((((uintptr_t)row_scales) & 1) != 0) return FPQ_ERR_ARG;
  return adaln_rotate_quant_impl(x, out, h_out, rotated_out, row_scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                 rows_per_batch, eps, smooth, sign_mask_host, table_id, stream, 1, nullptr);
}

int fpq_adaln_rotate_quant_token_rows_codes_fp8(const void* x, uint8_t* codes, void* row_scales, int64_t rows, int64_t cols,
                                                int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                                int64_t rows_per_batch, float eps, const float* smooth,
                                                const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream) {
  if (rows > 0 && cols > 0 && !row_scales) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  return adaln_rotate_quant_impl(x, codes, nullptr, nullptr, row_scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                 rows_per_batch, eps, smooth, sign_mask_host, table_id, stream, 2, &lut16_codes8(table_id));
}

int fpq_adaln_rotate_quant_token_rows_codes_fp6(const void* x, uint8_t* codes, void* row_scales, int64_t rows, int64_t cols,
                                                int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                                int64_t rows_per_batch, float eps, const float* smooth,
                                                const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream) {
  if (rows > 0 && cols > 0 && !row_scales) return FPQ_ERR_ARG;
  if (table_id != FPQ_E2M3) return FPQ_ERR_TABLE;
  if (cols % 32 != 0) return FPQ_ERR_SHAPE;
  if ((((uintptr_t)codes) & 7) != 0) return FPQ_ERR_ARG;
  return adaln_rotate_quant_impl(x, codes, nullptr, nullptr, row_scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                 rows_per_batch, eps, smooth, sign_mask_host, table_id, stream, 3, &lut16_codes6_e2m3());
}
int fpq_adaln_rotate_quant_token_rows_codes_fp6_km(const void* x, uint8_t* image, void* row_scales, int64_t rows, int64_t cols,
                                                   int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                                   int64_t rows_per_batch, float eps, const float* smooth,
                                                   const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream) {
  if (rows > 0 && cols > 0 && !row_scales) return FPQ_ERR_ARG;
  if (table_id != FPQ_E2M3) return FPQ_ERR_TABLE;
  if (cols % 128 != 0) return FPQ_ERR_SHAPE;
  return adaln_rotate_quant_impl(x, image, nullptr, nullptr, row_scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                 rows_per_batch, eps, smooth, sign_mask_host, table_id, stream, 3, &lut16_codes6_e2m3(), true);
}
// the two above with the operand format as an argument: FPQ_E2M3 (FP6) or FPQ_E3M2 (BF6) codes, row-major or the k-major image
int fpq_adaln_rotate_quant_token_rows_codes_f6(const void* x, uint8_t* codes, void* row_scales, int64_t rows, int64_t cols,
                                               int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                               int64_t rows_per_batch, float eps, const float* smooth,
                                               const uint32_t* sign_mask_host, int table_id, int kmajor, fpq_stream_t stream) {
  if (table_id != FPQ_E2M3 && table_id != FPQ_E3M2) return FPQ_ERR_TABLE;
  if (rows > 0 && cols > 0 && !row_scales) return FPQ_ERR_ARG;
  if (cols % (kmajor ? 128 : 32) != 0) return FPQ_ERR_SHAPE;
  if ((((uintptr_t)codes) & 7) != 0) return FPQ_ERR_ARG;
  return adaln_rotate_quant_impl(x, codes, nullptr, nullptr, row_scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                 rows_per_batch, eps, smooth, sign_mask_host, table_id, stream, 3, &lut16_codes6(table_id), kmajor != 0);
}


// the A6W4 GEMM's activation operands (include/fpq.h): what fpq_quant_rows_codes_g6 / fpq_a6w4_quant_rows_codes_km make of the
// rotated rows of fpq_adaln_rotate_quant_rows; the matrix-core kernel only (cols <= 2560)
int fpq_a6w4_adaln_rotate_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                           const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                           const float* smooth, const uint32_t* sign_mask_host, int table_id, int kmajor,
                                           fpq_stream_t stream) {
  if (rows < 0 || cols < 0 || rows_per_batch <= 0 || !sign_mask_host) return FPQ_ERR_ARG;
  if (table_id != FPQ_E1M2 && table_id != FPQ_E3M0) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype) || !is_f16_or_f32(mod_dtype)) return FPQ_ERR_DTYPE;
  if (cols % 128 != 0 || cols > 2560 || (kmajor && !km_image_fits(rows, cols / 4 * 3))) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !codes || !scales || !scale || !shift) return FPQ_ERR_ARG;
  if ((((uintptr_t)codes | (uintptr_t)scales) & 15) != 0) return FPQ_ERR_ARG;   // (x, scale, shift, smooth: checked below)
  return adaln_rotate_quant_impl(x, codes, nullptr, nullptr, scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                 rows_per_batch, eps, smooth, sign_mask_host, table_id, stream, 0, nullptr, kmajor != 0, true);
}

// the same on the FULL FP6 tables (include/fpq.h, GF6): what fpq_gf6_quant_rows_codes makes of the rotated rows
int fpq_gf6_adaln_rotate_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                          const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                          const float* smooth, const uint32_t* sign_mask_host, int table_id, int kmajor,
                                          fpq_stream_t stream) {
  if (rows < 0 || cols < 0 || rows_per_batch <= 0 || !sign_mask_host) return FPQ_ERR_ARG;
  if (table_id != FPQ_E2M3 && table_id != FPQ_E3M2) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype) || !is_f16_or_f32(mod_dtype)) return FPQ_ERR_DTYPE;
  if (cols % 128 != 0 || cols > 2560 || (kmajor && !km_image_fits(rows, cols / 4 * 3))) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !codes || !scales || !scale || !shift) return FPQ_ERR_ARG;
  if ((((uintptr_t)codes | (uintptr_t)scales) & 15) != 0) return FPQ_ERR_ARG;   // (x, scale, shift, smooth: checked below)
  return adaln_rotate_quant_impl(x, codes, nullptr, nullptr, scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                 rows_per_batch, eps, smooth, sign_mask_host, table_id, stream, 0, nullptr, kmajor != 0, true);
}

}  // extern "C"
