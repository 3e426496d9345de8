// fpq_fulladaln.hip - the full-width adaLN producer (fpq_fullrot_adaln_quant_rows*: LayerNorm + modulate in front of the full-width
// rotation and the per-group quantizer, one launch - fpq_fulladaln.h), with its C ABI.  A unit of its own: its 24 kernels compile
// beside fpq_fullrot.hip's 24, whose compile time stays what it was.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_rotate_mfma.h"   // the operand vector types, rq_rsrc
#include "fpq_adaln.h"         // wave_sum_dpp
#include "fpq_fullrot.h"
#include "fpq_fulladaln.h"

template <int K, int M, typename Tin, typename Tmod>
int launch_fulladaln(const void* x, void* out, void* h_out, void* rot_out, int64_t rows, const FullAdalnArgs& ad, const float* smooth,
                     const uint32_t* sign_words, int table_id, hipStream_t st, uint16_t* code_scales, bool km) {
  const Lut16Host& h = lut16_host(table_id, table_id);
  if (!h.tab_valid) return FPQ_ERR_TABLE;
  const Lut16Tab& tab = code_scales ? lut16_mx_codes_e2m1() : h.tab;
  const FullRotArgs r = fullrot_args(K * M, rows, smooth, sign_words, code_scales, km);
  const dim3 grid(fullrot_grid(rows));
  if (code_scales) return launch(fullrot_adaln_kernel<K, M, Tin, Tmod, 2>, grid, 0, st, x, out, rot_out, rows, r, ad, h.args, tab);
  if (h_out || rot_out) return launch(fullrot_adaln_kernel<K, M, Tin, Tmod, 1>, grid, 0, st, x, out, rot_out, rows, r, ad, h.args, tab);
  return launch(fullrot_adaln_kernel<K, M, Tin, Tmod, 0>, grid, 0, st, x, out, rot_out, rows, r, ad, h.args, tab);
}

}  // namespace

extern "C" {

static int fulladaln_impl(const void* x, void* out, void* h_out, void* rotated_out, void* code_scales, int64_t rows, int64_t cols,
                          int in_dtype, const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                          const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream, bool km) {
  if (rows < 0 || cols < 0 || !sign_words_host || rows_per_batch <= 0 || rows % rows_per_batch != 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype) || !is_f16_or_f32(mod_dtype)) return FPQ_ERR_DTYPE;
  if (!fullrot_width_built(cols) || rows >= (1ll << 31) || (km && !km_image_fits(rows, cols / 2))) return FPQ_ERR_SHAPE;
  if (rows == 0) return FPQ_OK;
  if (!x || !out || !scale || !shift) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)h_out | (uintptr_t)rotated_out | (uintptr_t)code_scales | (uintptr_t)scale |
        (uintptr_t)shift | (uintptr_t)smooth) & 15) != 0)
    return FPQ_ERR_ARG;
  FullAdalnArgs ad;
  ad.scale = scale;
  ad.shift = shift;
  ad.h_out = (uint16_t*)h_out;
  ad.rows_per_batch = (uint32_t)rows_per_batch;   // a divisor of rows < 2^31
  ad.eps = eps;
  return with_dtype(in_dtype, [&](auto ti) {
    return with_dtype(mod_dtype, [&](auto tm) {
      using Tin = decltype(ti);
      using Tmod = decltype(tm);
      if (cols == 1920)
        return launch_fulladaln<60, 32, Tin, Tmod>(x, out, h_out, rotated_out, rows, ad, smooth, sign_words_host, table_id, (hipStream_t)stream,
                                                   (uint16_t*)code_scales, km);
      return launch_fulladaln<36, 64, Tin, Tmod>(x, out, h_out, rotated_out, rows, ad, smooth, sign_words_host, table_id, (hipStream_t)stream,
                                                 (uint16_t*)code_scales, km);
    });
  });
}

int fpq_fullrot_adaln_quant_rows(const void* x, void* out, void* h_out, void* rotated_out, int64_t rows, int64_t cols, int in_dtype,
                                 const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                 const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream) {
  return fulladaln_impl(x, out, h_out, rotated_out, nullptr, rows, cols, in_dtype, scale, shift, mod_dtype, rows_per_batch, eps, smooth,
                        sign_words_host, table_id, stream, false);
}

int fpq_fullrot_adaln_quant_rows_codes_mx(const void* x, void* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                          const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                          const float* smooth, const uint32_t* sign_words_host, int kmajor, fpq_stream_t stream) {
  if (rows > 0 && fullrot_width_built(cols) && !scales) return FPQ_ERR_ARG;
  return fulladaln_impl(x, codes, nullptr, nullptr, scales, rows, cols, in_dtype, scale, shift, mod_dtype, rows_per_batch, eps, smooth,
                        sign_words_host, FPQ_E2M1, stream, kmajor != 0);
}

}  // extern "C"
