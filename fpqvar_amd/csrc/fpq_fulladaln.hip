// fpq_fulladaln.hip - the full-width adaLN producer (fpq_fullrot_adaln_quant_rows*: LayerNorm + modulate in front of the full-width
// rotation and the per-group quantizer, one launch - fpq_fulladaln.h), with its C ABI: FrAdalnFront x the per-group tail.  A unit of
// its own: its 24 kernels compile beside fpq_fullrot.hip's 24.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_rotate_mfma.h"   // the operand vector types, rq_rsrc
#include "fpq_adaln.h"         // wave_sum_dpp
#include "fpq_fullrot.h"
#include "fpq_fulladaln.h"
#include "fpq_fullrot_launch.h"
}  // namespace

extern "C" {

int fpq_fullrot_adaln_quant_rows(const void* x, void* out, void* h_out, void* rotated_out, int64_t rows, int64_t cols, int in_dtype,
                                 const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                 const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream) {
  const FullRotMod m = {scale, shift, mod_dtype, rows_per_batch, eps};
  return fullrot_run<false, true>({x, out, h_out, rotated_out, nullptr, rows, cols, in_dtype, smooth, sign_words_host, table_id, stream, false, false}, &m);
}

int fpq_fullrot_adaln_quant_rows_codes_mx(const void* x, void* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                          const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                          const float* smooth, const uint32_t* sign_words_host, int kmajor, fpq_stream_t stream) {
  if (rows > 0 && fullrot_width_built(cols) && !scales) return FPQ_ERR_ARG;
  const FullRotMod m = {scale, shift, mod_dtype, rows_per_batch, eps};
  return fullrot_run<false, true>({x, codes, nullptr, nullptr, scales, rows, cols, in_dtype, smooth, sign_words_host, FPQ_E2M1, stream, true, kmajor != 0}, &m);
}

}  // extern "C"
