// fpq_fulltoken.hip - the full-width rotation and the full-width adaLN producer in front of the PER-TOKEN FP6 quantizer (W6A6:
// fpq_fullrot_quant_token_rows*, fpq_fullrot_adaln_quant_token_rows* - fpq_fulltoken.h), with their C ABI: both fronts x the
// per-token tail.  A unit of its own: its 32 kernels compile beside the 24 + 24 of fpq_fullrot.hip and fpq_fulladaln.hip.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_rotate_mfma.h"   // the operand vector types, rq_rsrc
#include "fpq_codes_fp8.h"     // codes8_vec16
#include "fpq_adaln.h"         // wave_sum_dpp
#include "fpq_fullrot.h"
#include "fpq_fulladaln.h"
#include "fpq_fulltoken.h"
#include "fpq_fullrot_launch.h"
}  // namespace

extern "C" {

int fpq_fullrot_quant_token_rows(const void* x, void* out, void* rotated_out, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                 const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream) {
  return fullrot_run<true, false>({x, out, nullptr, rotated_out, row_scales, rows, cols, in_dtype, smooth, sign_words_host, table_id, stream, false, false});
}

int fpq_fullrot_quant_token_rows_codes_f6(const void* x, uint8_t* codes, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                          const float* smooth, const uint32_t* sign_words_host, int table_id, int kmajor,
                                          fpq_stream_t stream) {
  if (rows > 0 && fullrot_width_built(cols) && !row_scales) return FPQ_ERR_ARG;
  return fullrot_run<true, false>({x, codes, nullptr, nullptr, row_scales, rows, cols, in_dtype, smooth, sign_words_host, table_id, stream, true, kmajor != 0});
}

int fpq_fullrot_adaln_quant_token_rows(const void* x, void* out, void* h_out, void* rotated_out, void* row_scales, int64_t rows,
                                       int64_t cols, int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                       int64_t rows_per_batch, float eps, const float* smooth, const uint32_t* sign_words_host,
                                       int table_id, fpq_stream_t stream) {
  const FullRotMod m = {scale, shift, mod_dtype, rows_per_batch, eps};
  return fullrot_run<true, true>({x, out, h_out, rotated_out, row_scales, rows, cols, in_dtype, smooth, sign_words_host, table_id, stream, false, false}, &m);
}

int fpq_fullrot_adaln_quant_token_rows_codes_f6(const void* x, uint8_t* codes, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                                const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                                const float* smooth, const uint32_t* sign_words_host, int table_id, int kmajor,
                                                fpq_stream_t stream) {
  if (rows > 0 && fullrot_width_built(cols) && !row_scales) return FPQ_ERR_ARG;
  const FullRotMod m = {scale, shift, mod_dtype, rows_per_batch, eps};
  return fullrot_run<true, true>({x, codes, nullptr, nullptr, row_scales, rows, cols, in_dtype, smooth, sign_words_host, table_id, stream, true, kmajor != 0}, &m);
}

}  // extern "C"
