// fpq_fulltoken.hip - the full-width rotation and the full-width adaLN producer in front of the PER-TOKEN FP6 quantizer (W6A6:
// fpq_fullrot_quant_token_rows*, fpq_fullrot_adaln_quant_token_rows* - fpq_fulltoken.h), with their C ABI.  A unit of its own: its
// 32 kernels compile beside the 24 + 24 of fpq_fullrot.hip and fpq_fulladaln.hip, whose code objects stay what they were.
#include "fpq_common.h"

namespace {
#include "fpq_fast16.h"
#include "fpq_rotate_mfma.h"   // the operand vector types, rq_rsrc
#include "fpq_codes_fp8.h"     // codes8_vec16
#include "fpq_adaln.h"         // wave_sum_dpp
#include "fpq_fullrot.h"
#include "fpq_fulladaln.h"
#include "fpq_fulltoken.h"

inline bool is_fp6_table(int table_id) { return table_id == FPQ_E2M3 || table_id == FPQ_E3M2; }

// codes: the operand form (row_scales is not null); the level table of table_id otherwise
template <int K, int M, typename Tin>
int launch_fulltok(const void* x, void* out, void* rot_out, int64_t rows, const float* smooth, const uint32_t* sign_words, int table_id,
                   hipStream_t st, uint16_t* row_scales, bool codes, bool km) {
  const Lut16Host& h = lut16_host(table_id, table_id);
  if (!h.tab_valid) return FPQ_ERR_TABLE;
  const Lut16Tab& tab = codes ? lut16_codes6(table_id) : h.tab;
  const FullRotArgs r = fullrot_args(K * M, rows, smooth, sign_words, row_scales, km);
  const dim3 grid(fullrot_grid(rows));
  return with_bool(smooth != nullptr, [&](auto sm) {
    constexpr bool SMOOTH = sm.value;
    if (codes) return launch(fulltok_quant_kernel<K, M, Tin, SMOOTH, 1>, grid, 0, st, x, out, rot_out, rows, r, h.args, tab);
    return launch(fulltok_quant_kernel<K, M, Tin, SMOOTH, 0>, grid, 0, st, x, out, rot_out, rows, r, h.args, tab);
  });
}

template <int K, int M, typename Tin, typename Tmod>
int launch_fulltok_adaln(const void* x, void* out, void* rot_out, int64_t rows, const FullAdalnArgs& ad, const float* smooth,
                         const uint32_t* sign_words, int table_id, hipStream_t st, uint16_t* row_scales, bool codes, bool km) {
  const Lut16Host& h = lut16_host(table_id, table_id);
  if (!h.tab_valid) return FPQ_ERR_TABLE;
  const Lut16Tab& tab = codes ? lut16_codes6(table_id) : h.tab;
  const FullRotArgs r = fullrot_args(K * M, rows, smooth, sign_words, row_scales, km);
  const dim3 grid(fullrot_grid(rows));
  if (codes) return launch(fulltok_adaln_kernel<K, M, Tin, Tmod, 1>, grid, 0, st, x, out, rot_out, rows, r, ad, h.args, tab);
  return launch(fulltok_adaln_kernel<K, M, Tin, Tmod, 0>, grid, 0, st, x, out, rot_out, rows, r, ad, h.args, tab);
}

}  // namespace

extern "C" {

static int fulltok_impl(const void* x, void* out, void* rotated_out, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                        const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream, bool codes, bool km) {
  if (rows < 0 || cols < 0 || !sign_words_host) return FPQ_ERR_ARG;
  if (!is_fp6_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (!fullrot_width_built(cols) || rows >= (1ll << 31) || (km && !km_image_fits(rows, cols / 4 * 3))) return FPQ_ERR_SHAPE;
  if (rows == 0) return FPQ_OK;
  if (!x || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)rotated_out | (uintptr_t)row_scales | (uintptr_t)smooth) & 15) != 0) return FPQ_ERR_ARG;
  return with_dtype(in_dtype, [&](auto t) {
    using Tin = decltype(t);
    if (cols == 1920)
      return launch_fulltok<60, 32, Tin>(x, out, rotated_out, rows, smooth, sign_words_host, table_id, (hipStream_t)stream, (uint16_t*)row_scales,
                                         codes, km);
    return launch_fulltok<36, 64, Tin>(x, out, rotated_out, rows, smooth, sign_words_host, table_id, (hipStream_t)stream, (uint16_t*)row_scales,
                                       codes, km);
  });
}

int fpq_fullrot_quant_token_rows(const void* x, void* out, void* rotated_out, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                 const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream) {
  return fulltok_impl(x, out, rotated_out, row_scales, rows, cols, in_dtype, smooth, sign_words_host, table_id, stream, false, false);
}

int fpq_fullrot_quant_token_rows_codes_f6(const void* x, uint8_t* codes, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                          const float* smooth, const uint32_t* sign_words_host, int table_id, int kmajor,
                                          fpq_stream_t stream) {
  if (rows > 0 && fullrot_width_built(cols) && !row_scales) return FPQ_ERR_ARG;
  return fulltok_impl(x, codes, nullptr, row_scales, rows, cols, in_dtype, smooth, sign_words_host, table_id, stream, true, kmajor != 0);
}

static int fulltok_adaln_impl(const void* x, void* out, void* h_out, void* rotated_out, void* row_scales, int64_t rows, int64_t cols,
                              int in_dtype, const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                              const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream, bool codes, bool km) {
  if (rows < 0 || cols < 0 || !sign_words_host || rows_per_batch <= 0 || rows % rows_per_batch != 0) return FPQ_ERR_ARG;
  if (!is_fp6_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype) || !is_f16_or_f32(mod_dtype)) return FPQ_ERR_DTYPE;
  if (!fullrot_width_built(cols) || rows >= (1ll << 31) || (km && !km_image_fits(rows, cols / 4 * 3))) return FPQ_ERR_SHAPE;
  if (rows == 0) return FPQ_OK;
  if (!x || !out || !scale || !shift) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)h_out | (uintptr_t)rotated_out | (uintptr_t)row_scales | (uintptr_t)scale |
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
        return launch_fulltok_adaln<60, 32, Tin, Tmod>(x, out, rotated_out, rows, ad, smooth, sign_words_host, table_id, (hipStream_t)stream,
                                                       (uint16_t*)row_scales, codes, km);
      return launch_fulltok_adaln<36, 64, Tin, Tmod>(x, out, rotated_out, rows, ad, smooth, sign_words_host, table_id, (hipStream_t)stream,
                                                     (uint16_t*)row_scales, codes, km);
    });
  });
}

int fpq_fullrot_adaln_quant_token_rows(const void* x, void* out, void* h_out, void* rotated_out, void* row_scales, int64_t rows,
                                       int64_t cols, int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                       int64_t rows_per_batch, float eps, const float* smooth, const uint32_t* sign_words_host,
                                       int table_id, fpq_stream_t stream) {
  return fulltok_adaln_impl(x, out, h_out, rotated_out, row_scales, rows, cols, in_dtype, scale, shift, mod_dtype, rows_per_batch, eps,
                            smooth, sign_words_host, table_id, stream, false, false);
}

int fpq_fullrot_adaln_quant_token_rows_codes_f6(const void* x, uint8_t* codes, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                                const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                                const float* smooth, const uint32_t* sign_words_host, int table_id, int kmajor,
                                                fpq_stream_t stream) {
  if (rows > 0 && fullrot_width_built(cols) && !row_scales) return FPQ_ERR_ARG;
  return fulltok_adaln_impl(x, codes, nullptr, nullptr, row_scales, rows, cols, in_dtype, scale, shift, mod_dtype, rows_per_batch, eps,
                            smooth, sign_words_host, table_id, stream, true, kmajor != 0);
}

}  // extern "C"
