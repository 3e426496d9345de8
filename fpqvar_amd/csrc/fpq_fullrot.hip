// fpq_fullrot.hip - the full-width online rotation in front of the per-group quantizer (fpq_fullrot_quant_rows*: both Hadamard
// factors on the matrix cores, fpq_fullrot.h), with its C ABI: FrPlainFront x the per-group tail, 24 kernels.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_rotate_mfma.h"   // the operand vector types, rq_rsrc
#include "fpq_fullrot.h"
#include "fpq_fullrot_launch.h"
}  // namespace

extern "C" {

int fpq_fullrot_quant_rows(const void* x, void* out, void* rotated_out, int64_t rows, int64_t cols, int in_dtype, const float* smooth,
                           const uint32_t* sign_words_host, int table_id, fpq_stream_t stream) {
  return fullrot_run<false, false>({x, out, nullptr, rotated_out, nullptr, rows, cols, in_dtype, smooth, sign_words_host, table_id, stream, false, false});
}

int fpq_fullrot_quant_rows_codes_mx(const void* x, void* codes, void* scales, int64_t rows, int64_t cols, int in_dtype, const float* smooth,
                                    const uint32_t* sign_words_host, int kmajor, fpq_stream_t stream) {
  if (rows > 0 && fullrot_width_built(cols) && !scales) return FPQ_ERR_ARG;
  return fullrot_run<false, false>({x, codes, nullptr, nullptr, scales, rows, cols, in_dtype, smooth, sign_words_host, FPQ_E2M1, stream, true, kmajor != 0});
}

}  // extern "C"
