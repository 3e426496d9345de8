// fpq_resid_adaln.hip - the adaLN producer with the gated residual in front of it folded into its row load (fpq_adaln.h, RESID):
//     x_new = residual + y.mul(gate)        written to x_out
//     ...   = the producer on x_new         every other output byte for byte the twin entry point's of fpq_adaln.hip
// in one launch instead of fpq_gate_residual (or torch's mul and add on an fp32 stream) + the producer.  A unit of its own: the RESID
// forms of adaln_mfma_kernel compile beside fpq_adaln.hip, whose kernels and compile time stay what they were.  The dispatch is
// fpq_adaln.hip's (fpq_adaln_launch.h), so a call runs the variant its twin would.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_rotate_mfma.h"
#include "fpq_adaln.h"
#include "fpq_adaln_launch.h"

}  // namespace

extern "C" {

int fpq_resid_adaln_rotate_quant_rows(const void* y, const void* gate, void* x_out, const void* residual, void* out, void* h_out,
                                      void* rotated_out, int64_t rows, int64_t cols, int in_dtype, const void* scale,
                                      const void* shift, int mod_dtype, int64_t rows_per_batch, float eps, const float* smooth,
                                      const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream) {
  const AdalnResid rs = {y, gate, x_out};
  return adaln_rotate_quant_impl<true>(residual, out, h_out, rotated_out, nullptr, rows, cols, in_dtype, scale, shift, mod_dtype,
                                       rows_per_batch, eps, smooth, sign_mask_host, table_id, stream, 0, nullptr, false, false, &rs);
}

int fpq_resid_adaln_rotate_quant_rows_codes_mx(const void* y, const void* gate, void* x_out, const void* residual, uint8_t* codes,
                                               void* scales, int64_t rows, int64_t cols, int in_dtype, const void* scale,
                                               const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                               const float* smooth, const uint32_t* sign_mask_host, int kmajor, fpq_stream_t stream) {
  if (rows > 0 && cols > 0 && !scales) return FPQ_ERR_ARG;
  const AdalnResid rs = {y, gate, x_out};
  return adaln_rotate_quant_impl<true>(residual, codes, nullptr, nullptr, scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                       rows_per_batch, eps, smooth, sign_mask_host, FPQ_E2M1, stream, 0, nullptr, kmajor != 0, false, &rs);
}

int fpq_resid_adaln_rotate_quant_token_rows(const void* y, const void* gate, void* x_out, const void* residual, void* out,
                                            void* h_out, void* rotated_out, void* row_scales, int64_t rows, int64_t cols,
                                            int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                            int64_t rows_per_batch, float eps, const float* smooth,
                                            const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream) {
  if ((((uintptr_t)row_scales) & 1) != 0) return FPQ_ERR_ARG;
  const AdalnResid rs = {y, gate, x_out};
  return adaln_rotate_quant_impl<true>(residual, out, h_out, rotated_out, row_scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                       rows_per_batch, eps, smooth, sign_mask_host, table_id, stream, 1, nullptr, false, false, &rs);
}

int fpq_resid_adaln_rotate_quant_token_rows_codes_f6(const void* y, const void* gate, void* x_out, const void* residual,
                                                     uint8_t* codes, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                                     const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch,
                                                     float eps, const float* smooth, const uint32_t* sign_mask_host, int table_id,
                                                     int kmajor, fpq_stream_t stream) {
  if (table_id != FPQ_E2M3 && table_id != FPQ_E3M2) return FPQ_ERR_TABLE;
  if (rows > 0 && cols > 0 && !row_scales) return FPQ_ERR_ARG;
  if (cols % (kmajor ? 128 : 32) != 0) return FPQ_ERR_SHAPE;
  if ((((uintptr_t)codes) & 7) != 0) return FPQ_ERR_ARG;
  const AdalnResid rs = {y, gate, x_out};
  return adaln_rotate_quant_impl<true>(residual, codes, nullptr, nullptr, row_scales, rows, cols, in_dtype, scale, shift, mod_dtype,
                                       rows_per_batch, eps, smooth, sign_mask_host, table_id, stream, 3, &lut16_codes6(table_id),
                                       kmajor != 0, false, &rs);
}

}  // extern "C"
