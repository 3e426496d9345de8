// fpq_fullrot_launch.h - the host side of the full-width producers (fpq_fullrot.h): the checks of the eight fpq_fullrot_* entry points
// (include/fpq.h) and the launch of fullrot_rows_kernel<Front, Tail>.  Included inside the anonymous namespace of fpq_fullrot.hip,
// fpq_fulladaln.hip and fpq_fulltoken.hip, behind the kernel headers each of them needs.  A unit compiles the (front, tail) pairs of
// the fullrot_run<TOKEN, ADALN> it calls, and no others: three units of 24, 24 and 32 kernels that compile side by side.
#pragma once

template <int K, int M, typename Tin, typename Tmod, bool EMIT>
struct FrAdalnFront;   // fpq_fulladaln.h: included by the units that run it

// One call.  A pointer the entry point does not have is null.
struct FullRotCall {
  const void* x;
  void* out;        // the values, or the operand codes
  void* h_out;      // adaLN front, values: h, or null
  void* rot_out;    // values: the rotated rows, or null
  void* scales;     // codes: their scales (FullRotArgs::code_scales); per-token values: the row scales, or null
  int64_t rows, cols;
  int in_dtype;
  const float* smooth;
  const uint32_t* sign_words;
  int table_id;
  fpq_stream_t stream;
  bool codes, km;   // operand codes instead of values; into the k-major image
};
struct FullRotMod {   // what a call with the adaLN front adds
  const void* scale;
  const void* shift;
  int mod_dtype;
  int64_t rows_per_batch;
  float eps;
};

inline bool is_fp6_table(int table_id) { return table_id == FPQ_E2M3 || table_id == FPQ_E3M2; }

// The refusals, in the order include/fpq.h gives.  TOKEN: the two FP6 tables and 6-bit codes (3 bytes per 4 elements of the k-major
// image), else the symmetric tables and FP4 codes; m: the adaLN front's block, or null.  FPQ_OK for no rows: nothing to launch
template <bool TOKEN>
int fullrot_check(const FullRotCall& c, const FullRotMod* m) {
  if (c.rows < 0 || c.cols < 0 || !c.sign_words || (m && (m->rows_per_batch <= 0 || c.rows % m->rows_per_batch != 0))) return FPQ_ERR_ARG;
  if (!(TOKEN ? is_fp6_table(c.table_id) : is_symmetric_table(c.table_id))) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(c.in_dtype) || (m && !is_f16_or_f32(m->mod_dtype))) return FPQ_ERR_DTYPE;
  if (!fullrot_width_built(c.cols) || c.rows >= (1ll << 31) || (c.km && !km_image_fits(c.rows, TOKEN ? c.cols / 4 * 3 : c.cols / 2)))
    return FPQ_ERR_SHAPE;
  if (c.rows == 0) return FPQ_OK;
  if (!c.x || !c.out || (m && (!m->scale || !m->shift))) return FPQ_ERR_ARG;
  const uintptr_t mod = m ? (uintptr_t)m->scale | (uintptr_t)m->shift : 0;
  if ((((uintptr_t)c.x | (uintptr_t)c.out | (uintptr_t)c.h_out | (uintptr_t)c.rot_out | (uintptr_t)c.scales | mod | (uintptr_t)c.smooth) & 15) != 0)
    return FPQ_ERR_ARG;
  return FPQ_OK;
}

// The launch of one width and dtype pair: the table the tail stages, the argument blocks, the grid, and the (front, tail) pair of the
// call.  Plain front: `smooth` is a template parameter (SMOOTH) and Tmod is not used; adaLN front: a run-time select (fpq_fulladaln.h)
template <bool TOKEN, bool ADALN, int K, int M, typename Tin, typename Tmod>
int fullrot_launch(const FullRotCall& c, const FullAdalnArgs& ad) {
  const Lut16Host& h = lut16_host(c.table_id, c.table_id);
  if (!h.tab_valid) return FPQ_ERR_TABLE;
  const Lut16Tab& tab = !c.codes ? h.tab : TOKEN ? lut16_codes6(c.table_id) : lut16_mx_codes_e2m1();
  const FullRotArgs r = fullrot_args(K * M, c.rows, c.smooth, c.sign_words, (uint16_t*)c.scales, c.km);
  const dim3 grid(fullrot_grid(c.rows));
  const hipStream_t st = (hipStream_t)c.stream;
  auto go = [&](auto mode) {
    using Tail = FrTail<TOKEN, decltype(mode)::value, ADALN>;   // the per-group kEmit behind the adaLN front: h alone may be asked for
    if constexpr (ADALN) {
      return launch(fullrot_rows_kernel<FrAdalnFront<K, M, Tin, Tmod, Tail::EMIT>, Tail, FullAdalnArgs>, grid, 0, st, c.x, c.out, c.rot_out,
                    c.rows, r, ad, h.args, tab);
    } else {
      return with_bool(c.smooth != nullptr, [&](auto sm) {
        return launch(fullrot_rows_kernel<FrPlainFront<K, M, Tin, decltype(sm)::value>, Tail>, grid, 0, st, c.x, c.out, c.rot_out, c.rows, r,
                      h.args, tab);
      });
    }
  };
  if (c.codes) return go(std::integral_constant<FrMode, FrMode::kCodes>{});
  if constexpr (!TOKEN)   // (the per-token tail has no such form: the intermediates of its values are run-time pointers)
    if (c.h_out || c.rot_out) return go(std::integral_constant<FrMode, FrMode::kEmit>{});
  return go(std::integral_constant<FrMode, FrMode::kValues>{});
}

// An entry point behind its own early refusals: the checks, then the launch for the call's dtypes and width
template <bool TOKEN, bool ADALN>
int fullrot_run(const FullRotCall& c, const FullRotMod* m = nullptr) {
  const int rc = fullrot_check<TOKEN>(c, m);
  if (rc != FPQ_OK || c.rows == 0) return rc;
  FullAdalnArgs ad = {};
  if constexpr (ADALN) {
    ad.scale = m->scale;
    ad.shift = m->shift;
    ad.h_out = (uint16_t*)c.h_out;
    ad.rows_per_batch = (uint32_t)m->rows_per_batch;   // a divisor of rows < 2^31
    ad.eps = m->eps;
  }
  static_assert(kFullRotWidths[0] == FrGeom<60, 32>::C && kFullRotWidths[1] == FrGeom<36, 64>::C && sizeof(kFullRotWidths) == 2 * sizeof(int));
  auto width = [&](auto ti, auto tm) {
    using Tin = decltype(ti);
    using Tmod = decltype(tm);
    if (c.cols == kFullRotWidths[0]) return fullrot_launch<TOKEN, ADALN, 60, 32, Tin, Tmod>(c, ad);
    return fullrot_launch<TOKEN, ADALN, 36, 64, Tin, Tmod>(c, ad);
  };
  return with_dtype(c.in_dtype, [&](auto ti) {
    if constexpr (ADALN) return with_dtype(m->mod_dtype, [&](auto tm) { return width(ti, tm); });
    else return width(ti, ti);
  });
}
