// fpq_fullrot.hip - the full-width online rotation in front of the per-group quantizer (fpq_fullrot_quant_rows*: both Hadamard
// factors on the matrix cores, fpq_fullrot.h), with its C ABI.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_rotate_mfma.h"   // the operand vector types, rq_rsrc
#include "fpq_fullrot.h"

template <int K, int M, typename Tin>
int launch_fullrot(const void* x, void* out, void* rot_out, int64_t rows, const float* smooth, const uint32_t* sign_words, int table_id,
                   hipStream_t st, uint16_t* code_scales, bool km) {
  const Lut16Host& h = lut16_host(table_id, table_id);
  if (!h.tab_valid) return FPQ_ERR_TABLE;
  const Lut16Tab& tab = code_scales ? lut16_mx_codes_e2m1() : h.tab;
  const FullRotArgs r = fullrot_args(K * M, rows, smooth, sign_words, code_scales, km);
  const dim3 grid(fullrot_grid(rows));
  return with_bool(smooth != nullptr, [&](auto sm) {
    constexpr bool SMOOTH = sm.value;
    if (code_scales) return launch(fullrot_quant_kernel<K, M, Tin, SMOOTH, 2>, grid, 0, st, x, out, rot_out, rows, r, h.args, tab);
    if (rot_out) return launch(fullrot_quant_kernel<K, M, Tin, SMOOTH, 1>, grid, 0, st, x, out, rot_out, rows, r, h.args, tab);
    return launch(fullrot_quant_kernel<K, M, Tin, SMOOTH, 0>, grid, 0, st, x, out, rot_out, rows, r, h.args, tab);
  });
}

}  // namespace

extern "C" {

static int fullrot_impl(const void* x, void* out, void* rotated_out, void* code_scales, int64_t rows, int64_t cols, int in_dtype,
                        const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream, bool km) {
  if (rows < 0 || cols < 0 || !sign_words_host) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (!fullrot_width_built(cols) || rows >= (1ll << 31) || (km && !km_image_fits(rows, cols / 2))) return FPQ_ERR_SHAPE;
  if (rows == 0) return FPQ_OK;
  if (!x || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)rotated_out | (uintptr_t)code_scales | (uintptr_t)smooth) & 15) != 0) return FPQ_ERR_ARG;
  return with_dtype(in_dtype, [&](auto t) {
    using Tin = decltype(t);
    if (cols == 1920)
      return launch_fullrot<60, 32, Tin>(x, out, rotated_out, rows, smooth, sign_words_host, table_id, (hipStream_t)stream, (uint16_t*)code_scales, km);
    return launch_fullrot<36, 64, Tin>(x, out, rotated_out, rows, smooth, sign_words_host, table_id, (hipStream_t)stream, (uint16_t*)code_scales, km);
  });
}

int fpq_fullrot_quant_rows(const void* x, void* out, void* rotated_out, int64_t rows, int64_t cols, int in_dtype, const float* smooth,
                           const uint32_t* sign_words_host, int table_id, fpq_stream_t stream) {
  return fullrot_impl(x, out, rotated_out, nullptr, rows, cols, in_dtype, smooth, sign_words_host, table_id, stream, false);
}

int fpq_fullrot_quant_rows_codes_mx(const void* x, void* codes, void* scales, int64_t rows, int64_t cols, int in_dtype, const float* smooth,
                                    const uint32_t* sign_words_host, int kmajor, fpq_stream_t stream) {
  if (rows > 0 && fullrot_width_built(cols) && !scales) return FPQ_ERR_ARG;
  return fullrot_impl(x, codes, nullptr, scales, rows, cols, in_dtype, smooth, sign_words_host, FPQ_E2M1, stream, kmajor != 0);
}

}  // extern "C"
