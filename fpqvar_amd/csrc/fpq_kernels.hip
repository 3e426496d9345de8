// fpq_kernels.hip - gfx950 (MI355X) fake-quantization kernels behind include/fpq.h: the row and element quantizers, codes and
// their decode, the KV step and pack, the option table, and their C ABI.  The library's other translation units: fpq_rotate.hip
// (online rotation, FP8 / FP6 operand emitters), fpq_adaln.hip (the adaLN producer), fpq_gemm.hip (matrix-core consumers,
// attention) and fpq_build_tag.hip.
//
// What the reference computes (PKU-SEC-Lab/FPQVAR, tr/ = models_fp_quant_transform_rotate/):
//   quant/quant_kernel.cu:25-37        nearest entry of a value table, last index wins ties,
//                                      best distance starts at 102400 -> NaN/Inf/far give 0.0
//   tr/quant_utils.py:265-282 ...      ~11 torch ops around that kernel: absmax per row,
//                                      scale = absmax / max|table|, x / scale, fp32 cast,
//                                      kernel, q * scale, cast back
// Here each of those Python bodies is ONE launch: 16-byte coalesced loads, the row
// kept in registers between the absmax reduction and the rounding, cross-lane
// reduction with shuffles (rows of <= 1 KiB live inside one wavefront) or through
// LDS (long rows, one workgroup per row), and the table lookup replaced by a closed
// form on the minifloat structure (no K-step scan).  HBM traffic is the
// algorithmic minimum: every input byte read once, every output byte written once.
//
// Bit-exactness notes
//   * all scale / normalise arithmetic is IEEE fp32 (`/` is correctly rounded:
//     -fhip-fp32-correctly-rounded-divide-sqrt is hipcc's default; contraction is
//     switched off at build time) with the same intermediate roundings to x's dtype
//     that torch performs (fp16 ops = fp32 compute + one rounding);
//   * absmax is taken on the integer bit patterns of |x| so that NaN (largest
//     pattern) propagates exactly like torch's max;
//   * closed form: for r = |xn|, levels of a sign-magnitude minifloat with
//     subnormals have spacing 2^(max(e,emin)-M); a tie between two levels goes to
//     the larger VALUE (the scan's `<=`), i.e. up in magnitude for xn > 0 and down
//     for xn < 0.  tests/ prove it equal to the scan on every fp16 input and on fp32
//     neighbourhoods of every midpoint; fpq_quant_nearest keeps the literal scan.
#include "fpq_common.h"
#include <string.h>

// Experiment switches (fpq_common.h, FPQ_OPTION_LIST; include/fpq.h, fpq_set_option): the table every translation unit
// reads.  The initialiser below is the ONLY place in the library that touches the environment.
int fpq_option_table[FPQ_OPT_COUNT];
namespace {
struct FpqOptionDesc { const char* name; int is_flag; };
const FpqOptionDesc kOptionDescs[FPQ_OPT_COUNT] = {
#define FPQ_OPT_DESC(name, is_flag) {#name, is_flag},
    FPQ_OPTION_LIST(FPQ_OPT_DESC)
#undef FPQ_OPT_DESC
};
struct FpqOptionInit {
  FpqOptionInit() {
    for (int i = 0; i < FPQ_OPT_COUNT; ++i) {
      const char* e = getenv(kOptionDescs[i].name);
      fpq_option_table[i] = (!e || !*e) ? FPQ_OPTION_DEFAULT : kOptionDescs[i].is_flag ? (strcmp(e, "0") != 0) : atoi(e);
    }
  }
} fpq_option_init;
int option_index(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < FPQ_OPT_COUNT; ++i)
    if (strcmp(name, kOptionDescs[i].name) == 0) return i;
  return -1;
}
}  // namespace

namespace {

// ---------------------------------------------------------------------------------
// Kernel 1: rows of <= 1 KiB - LPR lanes of one wavefront own a row, one 16-byte
// load per lane, the row never leaves registers.  Grid-stride over wave tiles,
// UNROLL independent loads in flight per lane.
// ---------------------------------------------------------------------------------
template <typename Tin, typename Tout, int LPR, bool DUAL, int UNROLL>
__global__ __launch_bounds__(kBlock) void rows_subwave_kernel(const u32x4* __restrict__ x,
                                                             void* __restrict__ outv, int64_t n_vec,
                                                             Fmt fs, DualArgs dual) {
  constexpr int V = DT<Tin>::kVec;
  // a workgroup owns contiguous tiles of kBlock*UNROLL vectors, dispatched in address order
  constexpr int64_t stride = kBlock;
  const int64_t tile_vecs = (int64_t)kBlock * UNROLL;
  const int64_t tiles = (n_vec + tile_vecs - 1) / tile_vecs;
  float clip = fs.preclamp;
  bool clip_nan = false;
  const bool has_clip = DUAL ? (dual.clip_absmax != nullptr) : (fs.preclamp > 0.0f);
  if (DUAL && has_clip) clip = clip_value<Tin>(dual, &clip_nan);
  bool saw_nan = false;

  // n_vec is a multiple of LPR (whole rows) and LPR divides 64, so a row never
  // straddles the `live` boundary inside a wavefront.
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t v0 = tile * tile_vecs + threadIdx.x;
    u32x4 raw[UNROLL];
    bool live[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      int64_t v = v0 + u * stride;
      live[u] = v < n_vec;
      raw[u] = live[u] ? __builtin_nontemporal_load(x + v) : u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      float xf[V];
      uint32_t mneg = 0, mpos = 0;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float e = DT<Tin>::get(raw[u], i);
        if (has_clip) e = clamp_like_torch(e, clip, clip_nan);
        xf[i] = e;
        uint32_t ab = DT<Tin>::absbits(e);
        if (DUAL) {
          uint32_t bn = (e <= 0.0f) ? ab : 0u, bp = (e > 0.0f) ? ab : 0u;
          saw_nan |= DT<Tin>::bits_nan(ab);
          mneg = mneg > bn ? mneg : bn;
          mpos = mpos > bp ? mpos : bp;
        } else {
          mneg = mneg > ab ? mneg : ab;
        }
      }
      mneg = lanes_max<LPR>(mneg);
      if (DUAL) mpos = lanes_max<LPR>(mpos);
      if (!live[u]) continue;
      float p[V];
      if (DUAL) {
        float sn = scale_of<Tin>(mneg, dual.fneg.gmax), sp = scale_of<Tin>(mpos, dual.fpos.gmax);
#pragma unroll
        for (int i = 0; i < V; ++i) p[i] = quant_dual<Tin>(xf[i], sn, sp, dual.fneg, dual.fpos);
      } else {
        float s = scale_of<Tin>(mneg, fs.gmax);
#pragma unroll
        for (int i = 0; i < V; ++i) p[i] = quant_sym<Tin>(xf[i], s, fs);
      }
      int64_t v = v0 + u * stride;
      if constexpr (sizeof(Tout) == sizeof(Tin)) {
        u32x4 o = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < V; ++i) DT<Tout>::put(o, i, p[i]);
        __builtin_nontemporal_store(o, (u32x4*)outv + v);
      } else if constexpr (sizeof(Tout) < sizeof(Tin)) {  // f32 -> f16: 4 halves = 8 bytes
        u32x2 o = {f2h(p[0]) | (f2h(p[1]) << 16), f2h(p[2]) | (f2h(p[3]) << 16)};
        __builtin_nontemporal_store(o, (u32x2*)outv + v);
      } else {  // f16 -> f32: 8 floats = 32 bytes
        u32x4 o0 = {fbits(p[0]), fbits(p[1]), fbits(p[2]), fbits(p[3])};
        u32x4 o1 = {fbits(p[4]), fbits(p[5]), fbits(p[6]), fbits(p[7])};
        __builtin_nontemporal_store(o0, (u32x4*)outv + 2 * v);
        __builtin_nontemporal_store(o1, (u32x4*)outv + 2 * v + 1);
      }
    }
  }
  if (DUAL && saw_nan && dual.nan_flag) atomicOr(dual.nan_flag, 1u);
}

// ---------------------------------------------------------------------------------
// Kernel 2: long rows (per-token 1920 / 7680 / 2304 / 9216 ...): one workgroup per
// row, up to MAXC 16-byte vectors per lane kept in registers between the
// reduction (shuffles + LDS) and the rounding; longer rows are re-read (L2).
// ---------------------------------------------------------------------------------

template <typename Tin, typename Tout, bool DUAL, int MAXC>
__global__ __launch_bounds__(kBlock) void rows_block_kernel(const Tin* __restrict__ x,
                                                           Tout* __restrict__ out, int64_t rows,
                                                           int64_t cols, Fmt fs, DualArgs dual) {
  constexpr int V = DT<Tin>::kVec;
  __shared__ uint32_t sh[kBlock / 64];
  const int64_t vec_per_row = cols / V;  // cols % V == 0 guaranteed by the host
  float clip = fs.preclamp;
  bool clip_nan = false;
  const bool has_clip = DUAL ? (dual.clip_absmax != nullptr) : (fs.preclamp > 0.0f);
  if (DUAL && has_clip) clip = clip_value<Tin>(dual, &clip_nan);
  bool saw_nan = false;

  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const u32x4* xr = (const u32x4*)(x + row * cols);
    u32x4 raw[MAXC];
    uint32_t mneg = 0, mpos = 0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      int64_t v = (int64_t)c * kBlock + threadIdx.x;
      raw[c] = (v < vec_per_row) ? __builtin_nontemporal_load(xr + v) : u32x4{0, 0, 0, 0};
    }
    auto scan = [&](const u32x4& r) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float e = DT<Tin>::get(r, i);
        if (has_clip) e = clamp_like_torch(e, clip, clip_nan);
        uint32_t ab = DT<Tin>::absbits(e);
        if (DUAL) {
          uint32_t bn = (e <= 0.0f) ? ab : 0u, bp = (e > 0.0f) ? ab : 0u;
          saw_nan |= DT<Tin>::bits_nan(ab);
          mneg = mneg > bn ? mneg : bn;
          mpos = mpos > bp ? mpos : bp;
        } else {
          mneg = mneg > ab ? mneg : ab;
        }
      }
    };
#pragma unroll
    for (int c = 0; c < MAXC; ++c) scan(raw[c]);
    for (int64_t v = (int64_t)MAXC * kBlock + threadIdx.x; v < vec_per_row; v += kBlock) scan(xr[v]);
    mneg = block_max(mneg, sh);
    if (DUAL) mpos = block_max(mpos, sh);
    float sn = scale_of<Tin>(mneg, DUAL ? dual.fneg.gmax : fs.gmax);
    float sp = DUAL ? scale_of<Tin>(mpos, dual.fpos.gmax) : 0.0f;

    auto emit = [&](const u32x4& r, int64_t v) {
      float p[V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float e = DT<Tin>::get(r, i);
        if (has_clip) e = clamp_like_torch(e, clip, clip_nan);
        p[i] = DUAL ? quant_dual<Tin>(e, sn, sp, dual.fneg, dual.fpos) : quant_sym<Tin>(e, sn, fs);
      }
      Tout* o = out + row * cols + v * V;
      if constexpr (sizeof(Tout) == 2) {
        uint32_t w[V / 2];
#pragma unroll
        for (int i = 0; i < V / 2; ++i) w[i] = f2h(p[2 * i]) | (f2h(p[2 * i + 1]) << 16);
        if constexpr (V == 8)
          __builtin_nontemporal_store(u32x4{w[0], w[1], w[2], w[3]}, (u32x4*)o);
        else
          __builtin_nontemporal_store(u32x2{w[0], w[1]}, (u32x2*)o);
      } else {
#pragma unroll
        for (int i = 0; i < V; i += 4)
          __builtin_nontemporal_store(u32x4{fbits(p[i]), fbits(p[i + 1]), fbits(p[i + 2]), fbits(p[i + 3])},
                                      (u32x4*)(o + i));
      }
    };
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      int64_t v = (int64_t)c * kBlock + threadIdx.x;
      if (v < vec_per_row) emit(raw[c], v);
    }
    for (int64_t v = (int64_t)MAXC * kBlock + threadIdx.x; v < vec_per_row; v += kBlock) emit(xr[v], v);
  }
  if (DUAL && saw_nan && dual.nan_flag) atomicOr(dual.nan_flag, 1u);
}

// ---------------------------------------------------------------------------------
// Kernel 3: ragged / unaligned rows - scalar accesses, one workgroup per row.
// ---------------------------------------------------------------------------------
template <typename Tin, typename Tout, bool DUAL>
__global__ __launch_bounds__(kBlock) void rows_scalar_kernel(const Tin* __restrict__ x,
                                                            Tout* __restrict__ out, int64_t rows,
                                                            int64_t cols, Fmt fs, DualArgs dual) {
  __shared__ uint32_t sh[kBlock / 64];
  float clip = fs.preclamp;
  bool clip_nan = false;
  const bool has_clip = DUAL ? (dual.clip_absmax != nullptr) : (fs.preclamp > 0.0f);
  if (DUAL && has_clip) clip = clip_value<Tin>(dual, &clip_nan);
  bool saw_nan = false;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const Tin* xr = x + row * cols;
    uint32_t mneg = 0, mpos = 0;
    for (int64_t c = threadIdx.x; c < cols; c += kBlock) {
      float e = load_scalar<Tin>(xr + c);
      if (has_clip) e = clamp_like_torch(e, clip, clip_nan);
      uint32_t ab = DT<Tin>::absbits(e);
      if (DUAL) {
        uint32_t bn = (e <= 0.0f) ? ab : 0u, bp = (e > 0.0f) ? ab : 0u;
        saw_nan |= DT<Tin>::bits_nan(ab);
        mneg = mneg > bn ? mneg : bn;
        mpos = mpos > bp ? mpos : bp;
      } else {
        mneg = mneg > ab ? mneg : ab;
      }
    }
    mneg = block_max(mneg, sh);
    if (DUAL) mpos = block_max(mpos, sh);
    float sn = scale_of<Tin>(mneg, DUAL ? dual.fneg.gmax : fs.gmax);
    float sp = DUAL ? scale_of<Tin>(mpos, dual.fpos.gmax) : 0.0f;
    for (int64_t c = threadIdx.x; c < cols; c += kBlock) {
      float e = load_scalar<Tin>(xr + c);
      if (has_clip) e = clamp_like_torch(e, clip, clip_nan);
      float p = DUAL ? quant_dual<Tin>(e, sn, sp, dual.fneg, dual.fpos) : quant_sym<Tin>(e, sn, fs);
      store_scalar<Tout>(out + row * cols + c, p);
    }
  }
  if (DUAL && saw_nan && dual.nan_flag) atomicOr(dual.nan_flag, 1u);
}

// ---------------------------------------------------------------------------------
// "neg reverse" rows (models_fp_quant/quant_utils.py:454-495): the non-positive half is
// shifted up by m = |row min| before it is quantized and shifted back afterwards.
// Three row reductions (min, max|shifted|, max positive), all on data held in registers.
// ---------------------------------------------------------------------------------
// key whose MAX is the row MIN with torch.min's NaN propagation (NaN -> 0xFFFFFFFF)
__device__ __forceinline__ uint32_t min_key(float e) {
  uint32_t b = fbits(e);
  uint32_t ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // increasing in e
  return (e != e) ? 0xFFFFFFFFu : ~ord;
}
__device__ __forceinline__ float abs_from_min_key(uint32_t k) {
  uint32_t ord = ~k;
  uint32_t b = (ord & 0x80000000u) ? (ord & 0x7FFFFFFFu) : ~ord;
  return (k == 0xFFFFFFFFu) ? __builtin_nanf("") : fabsf(u2f(b));
}

template <typename T>
__device__ __forceinline__ float negrev_shifted(float xf, float m) {
  return DT<T>::round(((xf <= 0.0f) ? xf : 0.0f) + m);
}

template <typename T>
__device__ __forceinline__ float quant_negrev(float xf, float xnr, float m, float snr, float sp, const Fmt& f) {
  float a = div_round<T>(xnr, snr);
  float b = div_round<T>((xf > 0.0f) ? xf : 0.0f, sp);
  uint32_t na = (a < 0.0f) ? 1u : 0u;
  float qa = quant_mag(fabsf(a), na, f);
  qa = (na && qa != 0.0f) ? -qa : qa;
  float qb = quant_mag(b, 0u, f);  // b >= 0 or NaN
  float t = qa * snr;
  t = t - m;
  float u = qb * sp;
  return t + u;
}

template <typename T, int LPR, int UNROLL>
__global__ __launch_bounds__(kBlock) void rows_negrev_subwave_kernel(const u32x4* __restrict__ x,
                                                                    u32x4* __restrict__ out, int64_t n_vec,
                                                                    Fmt fs) {
  constexpr int V = DT<T>::kVec;
  const int64_t tile_vecs = (int64_t)kBlock * UNROLL;
  const int64_t tiles = (n_vec + tile_vecs - 1) / tile_vecs;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t v0 = tile * tile_vecs + threadIdx.x;
    u32x4 raw[UNROLL];
    bool live[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      int64_t v = v0 + (int64_t)u * kBlock;
      live[u] = v < n_vec;
      raw[u] = live[u] ? __builtin_nontemporal_load(x + v) : u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      float xf[V], xnr[V];
      uint32_t kmin = 0, mpos = 0, mnr = 0;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float e = DT<T>::get(raw[u], i);
        xf[i] = e;
        uint32_t k = min_key(e), bp = (e > 0.0f) ? DT<T>::absbits(e) : 0u;
        kmin = kmin > k ? kmin : k;
        mpos = mpos > bp ? mpos : bp;
      }
      kmin = lanes_max<LPR>(kmin);
      mpos = lanes_max<LPR>(mpos);
      const float m = abs_from_min_key(kmin);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        xnr[i] = negrev_shifted<T>(xf[i], m);
        uint32_t ab = DT<T>::absbits(xnr[i]);
        mnr = mnr > ab ? mnr : ab;
      }
      mnr = lanes_max<LPR>(mnr);
      if (!live[u]) continue;
      const float snr = scale_of<T>(mnr, fs.gmax), sp = scale_of<T>(mpos, fs.gmax);
      u32x4 o = {0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < V; ++i) DT<T>::put(o, i, quant_negrev<T>(xf[i], xnr[i], m, snr, sp, fs));
      __builtin_nontemporal_store(o, out + v0 + (int64_t)u * kBlock);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void rows_negrev_scalar_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                                   int64_t rows, int64_t cols, Fmt fs) {
  __shared__ uint32_t sh[kBlock / 64];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* xr = x + row * cols;
    uint32_t kmin = 0, mpos = 0, mnr = 0;
    for (int64_t c = threadIdx.x; c < cols; c += kBlock) {
      float e = load_scalar<T>(xr + c);
      uint32_t k = min_key(e), bp = (e > 0.0f) ? DT<T>::absbits(e) : 0u;
      kmin = kmin > k ? kmin : k;
      mpos = mpos > bp ? mpos : bp;
    }
    kmin = block_max(kmin, sh);
    mpos = block_max(mpos, sh);
    const float m = abs_from_min_key(kmin);
    for (int64_t c = threadIdx.x; c < cols; c += kBlock) {
      uint32_t ab = DT<T>::absbits(negrev_shifted<T>(load_scalar<T>(xr + c), m));
      mnr = mnr > ab ? mnr : ab;
    }
    mnr = block_max(mnr, sh);
    const float snr = scale_of<T>(mnr, fs.gmax), sp = scale_of<T>(mpos, fs.gmax);
    for (int64_t c = threadIdx.x; c < cols; c += kBlock) {
      float e = load_scalar<T>(xr + c);
      store_scalar<T>(out + row * cols + c, quant_negrev<T>(e, negrev_shifted<T>(e, m), m, snr, sp, fs));
    }
  }
}

#include "fpq_fast16.h"
#include "fpq_fast32.h"
#include "fpq_codes_mx.h"    // the FP4 operand emitter (fpq_quant_rows_codes_mx: it shares codes128_kernel with fpq_quant_rows_codes)
#include "fpq_codes_fp8.h"   // (codes8_vec16, the 6-bit code lookup of fpq_kv_pack)
#include "fpq_codes_g6.h"    // the A6W4 GEMM's activation emitter (fpq_quant_rows_codes_g6)
#include "fpq_packed_operands.h"   // packed-file codewords <-> weight operands (fpq_packed_to_operands, fpq_operands_to_packed)
#include "fpq_kv_codes.h"    // the packed KV cache's producer (fpq_kv_pack; its consumer is the attention kernel, fpq_gemm.hip)

// ---------------------------------------------------------------------------------
// L0: literal scan (quant/quant_kernel.cu:25-37), any table of k <= 256 floats.
// The table index is wave-uniform, so table[j] is a scalar load (SGPR broadcast).
// ---------------------------------------------------------------------------------
// One element through the closed form of a built-in table (side: 0 symmetric, 1 values <= 0 only, 2 values >= 0 only)
__device__ __forceinline__ float nearest_closed(float xv, const Fmt& f, int side) {
  if (side == 0) {
    uint32_t neg = xv < 0.0f ? 1u : 0u;
    float qm = quant_mag(fabsf(xv), neg, f);
    return (neg && qm != 0.0f) ? -qm : qm;
  }
  if (side == 1) {
    // table holds only values <= 0: positive inputs fall on 0 (if within reach)
    // (0.0 is also what "nothing within reach" yields, so no reach test is needed here)
    float qm = (xv <= 0.0f) ? quant_mag(fabsf(xv), 1u, f) : 0.0f;
    return (qm != 0.0f) ? -qm : 0.0f;
  }
  return (xv > 0.0f) ? quant_mag(xv, 0u, f) : 0.0f;
}

// The value tables this library knows in closed form, as the reference spells them (sorted, FP6 with two zeros).
// Handed to the scan kernel by value: every workgroup compares the caller's table with them (bit for bit) once,
// and a recognised table takes the closed form (~20 VALU ops per element) instead of the K-step scan
// (3 ops per entry: 45 for K = 15, 190 for K = 64).  Same function of (x, table) either way - the closed form is
// checked against the scan on every fp16 value, the neighbourhoods of every entry / midpoint / reach limit and
// 2^26 random fp32 patterns per table (tests/test_gpu_parity.py).
struct KnownTables {
  float v[272];                 // all tables back to back (262 entries)
  Fmt fmt[FPQ_NUM_TABLES];
  int16_t off[FPQ_NUM_TABLES], k[FPQ_NUM_TABLES];
  int8_t side[FPQ_NUM_TABLES];
};

template <typename T>
__global__ __launch_bounds__(kBlock) void nearest_scan_kernel(const T* __restrict__ x,
                                                             const float* __restrict__ table,
                                                             T* __restrict__ z, int64_t n, int k,
                                                             KnownTables known) {
  __shared__ float tab[256];
  __shared__ int match;
  if ((int)threadIdx.x < k) tab[threadIdx.x] = table[threadIdx.x];
  if (threadIdx.x == 0) match = -1;
  __syncthreads();
  if ((int)threadIdx.x < FPQ_NUM_TABLES && known.k[threadIdx.x] == k) {
    bool same = true;
    const float* kv = known.v + known.off[threadIdx.x];
    for (int j = 0; j < k; ++j) same &= fbits(tab[j]) == fbits(kv[j]);
    if (same) match = (int)threadIdx.x;   // the built-in tables are pairwise different: at most one writer
  }
  __syncthreads();
  const int id = match;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  if (id >= 0) {
    const Fmt f = known.fmt[id];
    const int side = known.side[id];
    if constexpr (sizeof(T) == 4) {
      if ((((uintptr_t)x | (uintptr_t)z) & 15) == 0) {   // 16 bytes per lane, two vectors in flight
        const int64_t n_vec = n >> 2;
        const u32x4* xv = (const u32x4*)x;
        u32x4* zv = (u32x4*)z;
        for (int64_t v = (int64_t)blockIdx.x * (2 * kBlock) + threadIdx.x; v < n_vec; v += 2 * stride) {
          const bool two = v + kBlock < n_vec;
          u32x4 a = __builtin_nontemporal_load(xv + v);
          u32x4 b = two ? __builtin_nontemporal_load(xv + v + kBlock) : u32x4{0, 0, 0, 0};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a[e] = fbits(nearest_closed(u2f(a[e]), f, side));
            b[e] = fbits(nearest_closed(u2f(b[e]), f, side));
          }
          __builtin_nontemporal_store(a, zv + v);
          if (two) __builtin_nontemporal_store(b, zv + v + kBlock);
        }
        for (int64_t i = (n_vec << 2) + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
          z[i] = (T)nearest_closed((float)x[i], f, side);
        return;
      }
    }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
      z[i] = (T)nearest_closed((float)x[i], f, side);
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    float xv = (float)x[i];
    float best = 102400.0f, zv = 0.0f;
    for (int j = 0; j < k; ++j) {
      float y = tab[j];
      float d = fabsf(xv - y);
      if (d <= best) {
        best = d;
        zv = y;
      }
    }
    z[i] = (T)zv;
  }
}

// quantize_to_nearest_grid (tr/quant_utils.py:209-230): grid[argmin_j |x - grid_j|] with torch.argmin's rules -
// the FIRST minimal index wins, a NaN or +-Inf input selects grid[0] - for any table; float32 result.
template <typename T>
__global__ __launch_bounds__(kBlock) void nearest_argmin_kernel(const T* __restrict__ x, const float* __restrict__ table,
                                                               float* __restrict__ z, int64_t n, int k) {
  __shared__ float tab[256];
  if ((int)threadIdx.x < k) tab[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const float xv = (float)x[i];
    float best = __builtin_inff(), zv = tab[0];
    for (int j = 0; j < k; ++j) {
      const float y = tab[j];
      const float d = fabsf(xv - y);
      if (d < best) {   // NaN and Inf distances never win: index 0 stays
        best = d;
        zv = y;
      }
    }
    z[i] = zv;
  }
}

__global__ __launch_bounds__(kBlock) void nearest_builtin_kernel(const float* __restrict__ x,
                                                                float* __restrict__ z, int64_t n, Fmt f,
                                                                int side /*0 sym, 1 neg-only, 2 pos-only*/) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const float q = nearest_closed(x[i], f, side);
    z[i] = q;
  }
}

// ---------------------------------------------------------------------------------
// "any NaN in the tensor => the whole result is zero" (the reference's global clamp with a
// NaN bound, tr/quant_utils.py:421-422): second launch, a handful of workgroups that read ONE word and exit when the
// flag is clear - no atomic, no barrier on that path (round 3 drew a ticket per workgroup on every call: 64 device-scope
// atomics on one address, ~11 ns each and serialised, tools/probe/ticket_cost.hip - 3 us of the 7 us a 100-row call took).
// Only when the flag is up: scratch[0] = the flag the quantizer raised, scratch[1] = a ticket counter; every workgroup
// zero-fills its share and takes a ticket AFTER it has read the flag, the one that draws the last ticket clears both
// words - the scratch is zero again when the launch ends (no memset per call, and a captured graph can be replayed).
// (One launch instead of two would need every workgroup of the quantizer to release its stores and count itself:
// profiles/r04_ticket_cost.txt - the chip's eight L2s are not coherent with each other, the release is an L2 write-back
// per workgroup, 4 - 40 times the kernel's own time.)
// ---------------------------------------------------------------------------------
constexpr int kFixupBlocks = 64;
__global__ __launch_bounds__(kBlock) void zero_if_flag_kernel(uint8_t* __restrict__ out, int64_t n_bytes, uint32_t* scratch) {
  // the quantizer's atomicOr is visible to a plain (scalar) load here: kernel boundary; uniform branch
  if (__hip_atomic_load(scratch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t n16 = ((uintptr_t)out & 15) == 0 ? n_bytes / 16 : 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n16; i += stride) ((u32x4*)out)[i] = u32x4{0, 0, 0, 0};
  for (int64_t i = n16 * 16 + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_bytes; i += stride) out[i] = 0;
  __syncthreads();   // every wavefront of this workgroup has read the flag
  if (threadIdx.x == 0 && atomicAdd(scratch + 1, 1u) == gridDim.x - 1) {   // every workgroup has read the flag by now
    __hip_atomic_store(scratch, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(scratch + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------------
// absmax over a whole tensor (bit-pattern max, NaN propagates), atomicMax combine
// ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void absmax_kernel(const T* __restrict__ x, int64_t n,
                                                       uint32_t* __restrict__ out) {
  __shared__ uint32_t sh[kBlock / 64];
  constexpr int V = DT<T>::kVec;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t nv = n / V;
  uint32_t m = 0;
  const u32x4* xv = (const u32x4*)x;
  const bool aligned = ((uintptr_t)x & 15) == 0;
  if (aligned) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < nv; v += stride) {
      u32x4 r = xv[v];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        uint32_t ab = DT<T>::absbits(DT<T>::get(r, i));
        m = m > ab ? m : ab;
      }
    }
  }
  for (int64_t i = (aligned ? nv * V : 0) + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    uint32_t ab = DT<T>::absbits(load_scalar<T>(x + i));
    m = m > ab ? m : ab;
  }
  m = block_max(m, sh);
  if (threadIdx.x == 0) atomicMax(out, m);
}

// ---------------------------------------------------------------------------------
// Per-tensor quantizer (BASELINE.json config 1; search/baseline/plot_weight_distribution_for_motivation.py:285-294):
//     scale = x.abs().max() / max|table|      both 0-dim -> float32 whatever x's dtype
//     out   = table[argmin |T(x / scale) - table|] * scale        float32
// Two launches, no memset, no atomics: (1) every workgroup writes the maximum of its slice to `partials`,
// (2) every workgroup of the elementwise launch reduces the <= kMaxBlocks partials (L2-resident) to the same
// scale and quantizes its tile with the argmin rules of quant_sym; workgroup 0 also stores the scale.
// ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void absmax_partials_kernel(const T* __restrict__ x, int64_t n,
                                                                uint32_t* __restrict__ partials) {
  __shared__ uint32_t sh[kBlock / 64];
  constexpr int V = DT<T>::kVec;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const bool aligned = ((uintptr_t)x & 15) == 0;
  const int64_t nv = aligned ? n / V : 0;
  const u32x4* xv = (const u32x4*)x;
  uint32_t m = 0;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < nv; v += stride) {
    const u32x4 r = xv[v];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const uint32_t ab = DT<T>::absbits(DT<T>::get(r, i));
      m = m > ab ? m : ab;
    }
  }
  for (int64_t i = nv * V + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t ab = DT<T>::absbits(load_scalar<T>(x + i));
    m = m > ab ? m : ab;
  }
  m = block_max(m, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void tensor_argmin_kernel(const T* __restrict__ x, float* __restrict__ out, int64_t n,
                                                              const uint32_t* __restrict__ partials, int n_partials,
                                                              float* __restrict__ scale_out, Fmt f) {
  __shared__ uint32_t sh[kBlock / 64];
  constexpr int V = DT<T>::kVec;
  uint32_t m = 0;
  for (int i = threadIdx.x; i < n_partials; i += kBlock) {
    const uint32_t p = partials[i];
    m = m > p ? m : p;
  }
  m = block_max(m, sh);
  const float s = DT<T>::from_absbits(m) / f.gmax;   // float32 division of two 0-dim tensors
  if (blockIdx.x == 0 && threadIdx.x == 0) *scale_out = s;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const bool aligned = (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  const int64_t nv = aligned ? n / V : 0;
  const u32x4* xv = (const u32x4*)x;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < nv; v += stride) {
    const u32x4 r = __builtin_nontemporal_load(xv + v);
    float p[V];
#pragma unroll
    for (int i = 0; i < V; ++i) p[i] = quant_sym<T>(DT<T>::get(r, i), s, f);
#pragma unroll
    for (int i = 0; i < V; i += 4)
      __builtin_nontemporal_store(u32x4{fbits(p[i]), fbits(p[i + 1]), fbits(p[i + 2]), fbits(p[i + 3])},
                                  (u32x4*)(out + v * V + i));
  }
  for (int64_t i = nv * V + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    out[i] = quant_sym<T>(load_scalar<T>(x + i), s, f);
}

// ---------------------------------------------------------------------------------
// The format search's loss (fpq_sqerr_rows_weighted): out[p] = sum_r w[r] sum_c (ref[r, c] - y[p][r, c])^2 for P <= 4
// planes y[p] against ONE reference, everything in fp32.  Two launches, no memset, no atomics, the same bits every call:
// (1) the matrices are one stream of 16-byte vectors (cols is a multiple of a vector, so a vector lies in one row);
//     vector v belongs to lane v % (grid x 256), which walks v, v + grid x 256, ... and carries its (row, column) along
//     by the host's (step_rows, step_cols) - one 32-bit division per lane, none in the loop.  A lane loads the reference
//     vector ONCE and every plane's vector against it: (1 + P) matrices move, not 2 P.  Wide and narrow matrices deal
//     alike: [20 x 5760] fp16 is 14400 vectors on 57 workgroups, [70001 x 8] is 70001 on 274.
// (2) one workgroup sums the <= kSqerrMaxBlocks partials of every plane (L2-resident) in a fixed order.
// The additions a term passes through, in order (tests/sqerr_model.py restates them; include/fpq.h carries the bound):
//     V = 8 (fp16) or 4 (fp32) in its vector (s += d d), then x w[row], n_it = ceil(vectors / (grid x 256)) in the lane
//     (acc += w s), 6 in the wavefront's butterfly, 3 over the workgroup's four wavefronts; in (2) at most
//     kSqerrMaxBlocks / 256 = 8 in a lane, 6 in the butterfly, 3 over the wavefronts:   D = V + n_it + 26,
//     and c = 3 roundings besides them (the difference, the square, the weight).
// ---------------------------------------------------------------------------------
constexpr int kSqerrMaxPlanes = 4;
constexpr int kSqerrMaxBlocks = FPQ_SQERR_WORKSPACE_BYTES / (4 * kSqerrMaxPlanes);
static_assert(kSqerrMaxBlocks == kMaxBlocks, "the workspace holds one partial per plane and resident workgroup");

struct SqerrDeal {
  int64_t n_vec;        // rows x cols / V
  int64_t row_vec;      // cols / V
  int64_t step_rows;    // (grid x 256) / row_vec
  int64_t step_cols;    // (grid x 256) % row_vec
};

__device__ __forceinline__ float lanes_sum64(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);   // both partners add the same pair: every lane ends with the same bits
  return v;
}

template <typename T, int P>
__global__ __launch_bounds__(kBlock) void sqerr_partials_kernel(const u32x4* __restrict__ ref, const u32x4* __restrict__ y,
                                                               const float* __restrict__ w, float* __restrict__ partials,
                                                               SqerrDeal d) {
  __shared__ float sh[P][kBlock / 64];
  constexpr int V = DT<T>::kVec;
  const uint32_t v0 = blockIdx.x * kBlock + threadIdx.x;     // < kSqerrMaxBlocks x 256 = 2^19
  int64_t row = 0, col = v0;
  if (d.row_vec <= (int64_t)v0) {
    row = v0 / (uint32_t)d.row_vec;
    col = v0 - (uint32_t)row * (uint32_t)d.row_vec;
  }
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  float acc[P];
#pragma unroll
  for (int p = 0; p < P; ++p) acc[p] = 0.0f;
  for (int64_t v = v0; v < d.n_vec; v += stride) {
    const u32x4 r = __builtin_nontemporal_load(ref + v);
    u32x4 q[P];
#pragma unroll
    for (int p = 0; p < P; ++p) q[p] = __builtin_nontemporal_load(y + p * d.n_vec + v);
    const float wr = w[row];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float e = DT<T>::get(r, i) - DT<T>::get(q[p], i);
        s += e * e;
      }
      acc[p] += wr * s;
    }
    row += d.step_rows;
    col += d.step_cols;
    if (col >= d.row_vec) {
      col -= d.row_vec;
      ++row;
    }
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const float s = lanes_sum64(acc[p]);
    if ((threadIdx.x & 63) == 0) sh[p][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < P) {
    float s = sh[threadIdx.x][0];
#pragma unroll
    for (int i = 1; i < kBlock / 64; ++i) s += sh[threadIdx.x][i];
    partials[threadIdx.x * gridDim.x + blockIdx.x] = s;
  }
}

// one workgroup: out[p] = the n_partials partials of plane p, lane i taking i, i + 256, ... in order (none: 0)
__global__ __launch_bounds__(kBlock) void sqerr_finish_kernel(const float* __restrict__ partials, int n_partials, int planes,
                                                             float* __restrict__ out) {
  __shared__ float sh[kSqerrMaxPlanes][kBlock / 64];
  for (int p = 0; p < planes; ++p) {
    float s = 0.0f;
    for (int i = threadIdx.x; i < n_partials; i += kBlock) s += partials[p * n_partials + i];
    s = lanes_sum64(s);
    if ((threadIdx.x & 63) == 0) sh[p][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < planes) {
    float s = sh[threadIdx.x][0];
#pragma unroll
    for (int i = 1; i < kBlock / 64; ++i) s += sh[threadIdx.x][i];
    out[threadIdx.x] = s;
  }
}

// ---------------------------------------------------------------------------------
// Codewords: one workgroup per row (any cols); code = index in the sorted
// de-duplicated symmetric table.
// ---------------------------------------------------------------------------------
template <typename Tin>
__global__ __launch_bounds__(kBlock) void rows_codes_kernel(const Tin* __restrict__ x,
                                                           uint8_t* __restrict__ codes,
                                                           Tin* __restrict__ scales, int64_t rows,
                                                           int64_t cols, Fmt fs, int pack) {
  __shared__ uint32_t sh[kBlock / 64];
  const int64_t code_cols = pack ? (cols + 1) / 2 : cols;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const Tin* xr = x + row * cols;
    uint32_t m = 0;
    for (int64_t c = threadIdx.x; c < cols; c += kBlock) {
      uint32_t ab = DT<Tin>::absbits(load_scalar<Tin>(xr + c));
      m = m > ab ? m : ab;
    }
    m = block_max(m, sh);
    float s = scale_of<Tin>(m, fs.gmax);
    if (threadIdx.x == 0) store_scalar<Tin>(scales + row, s);
    auto code_of = [&](int64_t c) -> uint32_t {
      if (c >= cols) return (uint32_t)fs.zero_code;
      float xn = DT<Tin>::round(load_scalar<Tin>(xr + c) / s);
      uint32_t neg = (xn < 0.0f) ? 1u : 0u;
      float qm = quant_mag(fabsf(xn), neg, fs);
      int li = level_index(qm, fs);
      return (uint32_t)(neg ? fs.zero_code - li : fs.zero_code + li);
    };
    if (pack) {
      for (int64_t b = threadIdx.x; b < code_cols; b += kBlock)
        codes[row * code_cols + b] = (uint8_t)(code_of(2 * b) | (code_of(2 * b + 1) << 4));
    } else {
      for (int64_t c = threadIdx.x; c < cols; c += kBlock) codes[row * code_cols + c] = (uint8_t)code_of(c);
    }
  }
}

// Vectorised codes for rows of exactly 128 elements (per-group): LPR lanes own a row, 16-byte
// loads, one packed store per lane (FP4: V nibbles, FP6: V bytes), lane 0 of the row writes the scale.
template <typename Tin, bool PACK, bool HW = false>
__device__ __forceinline__ void codes128_body(const u32x4* __restrict__ x, uint8_t* __restrict__ codes,
                                              Tin* __restrict__ scales, int64_t n_vec, const Fmt& fs) {
  constexpr int V = DT<Tin>::kVec;
  constexpr int LPR = 128 / V;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n_vec; v += (int64_t)gridDim.x * kBlock) {
    u32x4 raw = __builtin_nontemporal_load(x + v);
    float xf[V];
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      xf[i] = DT<Tin>::get(raw, i);
      uint32_t ab = DT<Tin>::absbits(xf[i]);
      m = m > ab ? m : ab;
    }
    m = lanes_max<LPR>(m);
    float s = scale_of<Tin>(m, fs.gmax);
    if ((threadIdx.x & (LPR - 1)) == 0) store_scalar<Tin>(scales + v / LPR, s);
    uint32_t c[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float xn = DT<Tin>::round(xf[i] / s);
      uint32_t neg = (xn < 0.0f) ? 1u : 0u;
      float qm = quant_mag(fabsf(xn), neg, fs);
      int li = level_index(qm, fs);
      if constexpr (HW) c[i] = (uint32_t)li | ((neg && li != 0) ? 8u : 0u);   // OCP sign-magnitude nibble
      else c[i] = (uint32_t)(neg ? fs.zero_code - li : fs.zero_code + li);
    }
    if constexpr (PACK && V == 8) {
      uint32_t w = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) w |= c[i] << (4 * i);
      ((uint32_t*)codes)[v] = w;
    } else if constexpr (PACK && V == 4) {
      ((uint16_t*)codes)[v] = (uint16_t)(c[0] | (c[1] << 4) | (c[2] << 8) | (c[3] << 12));
    } else if constexpr (V == 8) {
      u32x2 w = {c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24), c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24)};
      ((u32x2*)codes)[v] = w;
    } else {
      ((uint32_t*)codes)[v] = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    }
  }
}
template <typename Tin, bool PACK, bool HW = false>
__global__ __launch_bounds__(kBlock) void codes128_kernel(const u32x4* __restrict__ x, uint8_t* __restrict__ codes,
                                                         Tin* __restrict__ scales, int64_t n_vec, Fmt fs) {
  codes128_body<Tin, PACK, HW>(x, codes, scales, n_vec, fs);
}
// Many tensors, one launch (fpq_quant_rows_codes_segments): blockIdx.y = segment of a device-resident table, the
// workgroups of the x dimension stride over that segment's vectors (a short segment's surplus workgroups fall through)
struct CodesSeg {
  const void* x;
  uint8_t* codes;
  void* scales;
  int64_t rows;
};
template <typename Tin, bool PACK>
__global__ __launch_bounds__(kBlock) void codes128_segments_kernel(const CodesSeg* __restrict__ segs, Fmt fs) {
  const CodesSeg sg = segs[blockIdx.y];
  codes128_body<Tin, PACK, false>((const u32x4*)sg.x, sg.codes, (Tin*)sg.scales, sg.rows * (128 / DT<Tin>::kVec), fs);
}

// inverse for rows of 128: every lane decodes 8 consecutive elements
template <typename Ts, typename Tout, bool PACK>
__device__ __forceinline__ void decode128_body(const uint8_t* __restrict__ codes, const Ts* __restrict__ scales,
                                               Tout* __restrict__ out, int64_t n_oct, const Fmt& fs) {
  const int nsub = (int)(fs.kmin * fs.inv_step0);
  if constexpr (PACK) {
    // nibble codes (round 4): the two signed levels of every code BYTE from a 256-entry table in LDS, filled once per
    // workgroup from the closed form below - shift, mask, one 8-byte LDS read and two multiplies per pair instead of ~24
    // vector instructions (the decode side of the calibration's packed exchange ran at 0.45 of 8 TB/s on them)
    __shared__ float pair_lut[256][2];
    {
      const int t = threadIdx.x;   // kBlock == 256: one entry per thread
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int li = (int)((t >> (4 * h)) & 15) - fs.zero_code;
        const uint32_t neg = li < 0;
        li = neg ? -li : li;
        const float q = (li < nsub) ? (float)li * fs.step0 : u2f(((uint32_t)li + fs.kmin_code_base) << fs.mshift);
        pair_lut[t][h] = neg ? -q : q;
      }
    }
    __syncthreads();
    // tiles of U x 256 octets: all of a tile's code words are requested before the first is decoded (one octet per
    // thread and trip, as before, cycled workgroups that write 4 KiB each - the rate of the headline quantizer's
    // workgroups, which move twice that)
    constexpr int U = 4;
    const int64_t n_tiles = (n_oct + (int64_t)kBlock * U - 1) / ((int64_t)kBlock * U);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const int64_t v0 = tile * ((int64_t)kBlock * U) + threadIdx.x;
      uint32_t w[U];
      float s[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t v = v0 + u * kBlock;
        w[u] = v < n_oct ? __builtin_nontemporal_load((const uint32_t*)codes + v) : 0u;
        s[u] = v < n_oct ? load_scalar<Ts>(scales + (v >> 4)) : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t v = v0 + u * kBlock;
        float p[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t off = j == 0 ? (w[u] << 3) & 0x7F8u : (w[u] >> (8 * j - 3)) & 0x7F8u;   // byte j of the word, times 8
          const v2f_t q = *(const v2f_t*)((const char*)pair_lut + off);
          p[2 * j] = q[0] * s[u];
          p[2 * j + 1] = q[1] * s[u];
        }
        if (v < n_oct) {
          if constexpr (sizeof(Tout) == 2) {
            __builtin_nontemporal_store(u32x4{f2h2(p[0], p[1]), f2h2(p[2], p[3]), f2h2(p[4], p[5]), f2h2(p[6], p[7])}, (u32x4*)out + v);
          } else {
            __builtin_nontemporal_store(u32x4{fbits(p[0]), fbits(p[1]), fbits(p[2]), fbits(p[3])}, (u32x4*)out + 2 * v);
            __builtin_nontemporal_store(u32x4{fbits(p[4]), fbits(p[5]), fbits(p[6]), fbits(p[7])}, (u32x4*)out + 2 * v + 1);
          }
        }
      }
    }
    return;
  }
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n_oct; v += (int64_t)gridDim.x * kBlock) {
    uint32_t c[8];
    if constexpr (PACK) {
      uint32_t w = ((const uint32_t*)codes)[v];
#pragma unroll
      for (int i = 0; i < 8; ++i) c[i] = (w >> (4 * i)) & 0xFu;
    } else {
      u32x2 w = ((const u32x2*)codes)[v];
#pragma unroll
      for (int i = 0; i < 8; ++i) c[i] = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
    }
    float s = load_scalar<Ts>(scales + (v >> 4));
    float p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int li = (int)c[i] - fs.zero_code;
      uint32_t neg = li < 0;
      li = neg ? -li : li;
      float q = (li < nsub) ? (float)li * fs.step0 : u2f(((uint32_t)li + fs.kmin_code_base) << fs.mshift);
      p[i] = (neg ? -q : q) * s;
    }
    if constexpr (sizeof(Tout) == 2) {
      u32x4 o = {f2h(p[0]) | (f2h(p[1]) << 16), f2h(p[2]) | (f2h(p[3]) << 16), f2h(p[4]) | (f2h(p[5]) << 16),
                 f2h(p[6]) | (f2h(p[7]) << 16)};
      __builtin_nontemporal_store(o, (u32x4*)out + v);
    } else {
      __builtin_nontemporal_store(u32x4{fbits(p[0]), fbits(p[1]), fbits(p[2]), fbits(p[3])}, (u32x4*)out + 2 * v);
      __builtin_nontemporal_store(u32x4{fbits(p[4]), fbits(p[5]), fbits(p[6]), fbits(p[7])}, (u32x4*)out + 2 * v + 1);
    }
  }
}
template <typename Ts, typename Tout, bool PACK>
__global__ __launch_bounds__(kBlock) void decode128_kernel(const uint8_t* __restrict__ codes, const Ts* __restrict__ scales,
                                                          Tout* __restrict__ out, int64_t n_oct, Fmt fs) {
  decode128_body<Ts, Tout, PACK>(codes, scales, out, n_oct, fs);
}
struct DecodeSeg {
  const uint8_t* codes;
  const void* scales;
  void* out;
  int64_t rows;
};
template <typename Ts, typename Tout, bool PACK>
__global__ __launch_bounds__(kBlock) void decode128_segments_kernel(const DecodeSeg* __restrict__ segs, Fmt fs) {
  const DecodeSeg sg = segs[blockIdx.y];
  decode128_body<Ts, Tout, PACK>(sg.codes, (const Ts*)sg.scales, (Tout*)sg.out, sg.rows * 16, fs);
}

template <typename Ts, typename Tout>
__global__ __launch_bounds__(kBlock) void rows_decode_kernel(const uint8_t* __restrict__ codes,
                                                            const Ts* __restrict__ scales,
                                                            Tout* __restrict__ out, int64_t rows, int64_t cols,
                                                            Fmt fs, int pack) {
  const int64_t code_cols = pack ? (cols + 1) / 2 : cols;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    float s = load_scalar<Ts>(scales + row);
    for (int64_t c = threadIdx.x; c < cols; c += kBlock) {
      uint32_t code = pack ? ((codes[row * code_cols + (c >> 1)] >> ((c & 1) * 4)) & 0xF)
                           : codes[row * code_cols + c];
      int li = (int)code - fs.zero_code;
      uint32_t neg = li < 0;
      li = neg ? -li : li;
      // level li: below 2^M levels are li*step0; above, mantissa/exponent from the index
      int nsub = (int)(fs.kmin * fs.inv_step0);  // 2^M
      float q = (li < nsub) ? (float)li * fs.step0 : u2f(((uint32_t)li + fs.kmin_code_base) << fs.mshift);
      q = neg ? -q : q;
      store_scalar<Tout>(out + row * cols + c, q * s);
    }
  }
}


template <typename Tin, typename Tout, bool DUAL>
int launch_rows(const void* x, void* out, int64_t rows, int64_t cols, const Fmt& fs, const DualArgs& dual,
                hipStream_t st) {
  constexpr int V = DT<Tin>::kVec;
  const bool aligned = (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  const int64_t row_bytes = cols * (int64_t)sizeof(Tin);
  if (aligned && cols % V == 0) {
    const int64_t n_vec = rows * (cols / V);
    const int lpr = (int)(cols / V);
    constexpr int U = 2;
    if (row_bytes <= 1024 && (lpr & (lpr - 1)) == 0)   // 1 .. 64 lanes per row: every power of two is in the list
      return with_int<1, 2, 4, 8, 16, 32, 64>(lpr, [&](auto l) {
        return launch(rows_subwave_kernel<Tin, Tout, l.value, DUAL, U>, grid_for(tiles_of(n_vec, U), 1 << 20), 0, st, x, out,
                      n_vec, fs, dual);
      });
    // the output row must stay 16-byte (f16 out of f32 in: 8-byte) aligned per vector
    return with_int<2, 8>(cols / V <= (int64_t)kBlock * 2 ? 2 : 8, [&](auto c) {
      return launch(rows_block_kernel<Tin, Tout, DUAL, c.value>, grid_for(rows, 65535), 0, st, x, out, rows, cols, fs, dual);
    });
  }
  return launch(rows_scalar_kernel<Tin, Tout, DUAL>, grid_for(rows, 65535), 0, st, x, out, rows, cols, fs, dual);
}

template <bool DUAL>
int dispatch_rows(const void* x, void* out, int64_t rows, int64_t cols, int in_dtype, int out_dtype, const Fmt& fs,
                  const DualArgs& dual, hipStream_t st) {
  if (!is_f16_or_f32(in_dtype) || !is_f16_or_f32(out_dtype)) return FPQ_ERR_DTYPE;
  return with_dtype(in_dtype, [&](auto ti) {
    return with_dtype(out_dtype, [&](auto to) {
      return launch_rows<decltype(ti), decltype(to), DUAL>(x, out, rows, cols, fs, dual, st);
    });
  });
}

// ---- fast fp16 -> fp16 path (fpq_fast16.h) ------------------------------------------
inline bool fast16_aligned(const void* x, const void* out, int64_t cols, int in_dtype, int out_dtype) {
  return in_dtype == FPQ_F16 && out_dtype == FPQ_F16 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0 &&
         cols % 8 == 0;
}

// rows that live inside one wavefront
inline bool fast16_eligible(const void* x, const void* out, int64_t cols, int in_dtype, int out_dtype) {
  if (!fast16_aligned(x, out, cols, in_dtype, out_dtype)) return false;
  const int64_t lpr = cols / 8;
  return lpr >= 1 && lpr <= 64 && (lpr & (lpr - 1)) == 0;
}

// long rows: one workgroup per row, at most 8 vectors (64 halves) per lane in registers
inline bool fast16_block_eligible(const void* x, const void* out, int64_t cols, int in_dtype, int out_dtype) {
  return fast16_aligned(x, out, cols, in_dtype, out_dtype) && cols / 8 <= (int64_t)kBlock * 8;
}

// Buckets of a table pair's image, which every workgroup stages in LDS before its first row (fpq_fast16.h): 128 .. 512 for
// the 4-bit tables, their pairs and E3M2; 1024 for E2M3 and the pairs with E2M3_POS; 2 x 1024 for the pairs with INT_NEG.
// kBigTab is where the staging starts to count: 1024 buckets are 2 KiB, a quarter of an 8 KiB tile's own bytes, so from
// there on (>=) the launches below give a workgroup several tiles or rows per staging, and past it (>) the 8 stores per
// lane want many tiles per workgroup on a capped grid.
inline int lut16_buckets(const Lut16Host& h) { return 1 << (16 - h.args.shift); }
constexpr int kBigTab = 1024;

// A table kernel has two forms: the bucket table travels in the kernel arguments (h.tab_valid), or every workgroup
// evaluates the closed form itself (fpq_fast16.h, lut16_fill).  kern_of(Bool<TAB>{}) names the kernel; its last argument is
// the table, and its LDS is static (the bucket table lives there).
template <typename K, typename... A>
int launch_tab(const Lut16Host& h, K kern_of, dim3 grid, hipStream_t st, const A&... args) {
  return with_bool(h.tab_valid, [&](auto tab) { return launch(kern_of(tab), grid, 0, st, args..., h.tab); });
}

// Defaults measured on MI355X with tools/kbench (cold HBM, 4 rotating 252 MB buffer pairs):
// U = 2 with non-temporal loads and stores matches the best plain copy (78 us for
// fp16 [65536x1920] = 6.45 TB/s); grid-stride with a capped grid or U = 8 lose 3-8 %.
#ifndef FPQ_FAST16_U   // vectors per lane of the sub-wavefront row kernels (A/B builds)
#define FPQ_FAST16_U 2
#endif
#ifndef FPQ_FAST16_HW4_U   // ... of the table-free E2M1 form
#define FPQ_FAST16_HW4_U 1
#endif
template <bool DUAL, int U = FPQ_FAST16_U, bool NTL = true, bool NTS = true>
int launch_fast16(const void* x, void* out, int64_t rows, int64_t cols, int neg_id, int pos_id, hipStream_t st,
                  int grid_cap = 1 << 20, uint32_t* nan_flag = nullptr, const void* clip_absmax = nullptr,
                  float clip_strength = 1.0f, bool gelu = false, void* gelu_out = nullptr) {
  const Lut16Host& h = lut16_host(neg_id, pos_id);
  Lut16Args args = h.args;
  args.nan_flag = nan_flag;
  args.clip_absmax = clip_absmax;
  args.clip_strength = clip_strength;
  args.gelu_out = gelu_out;
  const int64_t n_vec = rows * (cols / 8);
  const int lpr = (int)(cols / 8);
  const size_t lds = 0;   // the bucket table lives in static LDS (fpq_fast16.h)
  const dim3 grid(grid_for(tiles_of(n_vec, U), grid_cap));
  // the headline shape - E2M1, groups of 128 - takes its levels from the FP4 conversion hardware (fpq_fast16.h); FPQ_NO_HW4
  // (read at every call: the exhaustive test sweeps both forms in one process) keeps the bucket table
  if constexpr (DUAL) {
    if (gelu) {          // groups of 128, small tables (fpq_gelu_quant_rows_dual checks): GELU in front of the quantizer, one pass
      if (lpr != 16 || clip_absmax) return FPQ_ERR_SHAPE;
      return launch_tab(h, [](auto tab) { return rows16_lut_subwave_kernel<16, true, U, tab.value, NTL, NTS, false, false, 0, true>; },
                        grid, st, x, out, n_vec, args);
    }
    if (clip_absmax) {   // groups of 128 only (fpq_quant_rows_dual checks): the clamping form of the same kernel
      if (lpr != 16) return FPQ_ERR_SHAPE;
      return launch_tab(h, [](auto tab) { return rows16_lut_subwave_kernel<16, true, U, tab.value, NTL, NTS, false, true>; },
                        grid, st, x, out, n_vec, args);
    }
  }
  if constexpr (!DUAL) {
    if (lpr == 16 && neg_id == FPQ_E2M1 && pos_id == FPQ_E2M1 && !fpq_flag(OPT_FPQ_NO_HW4)) {
      // no table to stage, so nothing to amortise over a tile: ONE vector per lane on the full grid, the best plain-copy
      // shape of this chip (profiles/r02_copy_persistent_probe.txt: 0.81 against 0.777 for 8 KiB tiles); same-process
      // A/B against U = 2: 77.0 - 77.5 vs 79.0 - 79.4 us in steady state (profiles/r03_headline_u1.txt)
      constexpr int U1 = FPQ_FAST16_HW4_U;
      return launch(rows16_lut_subwave_kernel<16, false, U1, true, NTL, NTS, true>, grid_for(tiles_of(n_vec, U1), grid_cap), lds,
                    st, x, out, n_vec, args, h.tab);
    }
  }
  if constexpr (!DUAL) {
    // E2M3 / E3M2 per group of 128 and per row of 64 (the KV cache's head rows): levels from the FP6 conversion hardware, four
    // vectors per lane = the 32 values of one conversion, full grid (no table to amortise); FPQ_NO_HW6 keeps the table
    if ((lpr == 16 || lpr == 8) && neg_id == pos_id && (neg_id == FPQ_E2M3 || neg_id == FPQ_E3M2) && !fpq_flag(OPT_FPQ_NO_HW6))
      return with_int<8, 16>(lpr, [&](auto l) {
        constexpr int L = l.value;
        return with_int<1, 2>(neg_id == FPQ_E2M3 ? 1 : 2, [&](auto hw) {   // the conversion: 1 E2M3, 2 E3M2
          return launch(rows16_lut_subwave_kernel<L, false, 4, true, NTL, NTS, false, false, hw.value>,
                        grid_for(tiles_of(n_vec, 4), 1 << 20), lds, st, x, out, n_vec, args, h.tab);
        });
      });
  }
  return with_int<1, 2, 4, 8, 16, 32, 64>(lpr, [&](auto l) {
    constexpr int L = l.value;
    return launch_tab(h, [](auto tab) { return rows16_lut_subwave_kernel<L, DUAL, U, tab.value, NTL, NTS>; }, grid, st, x, out,
                      n_vec, args);
  });
}

template <bool DUAL>
int launch_fast16_pair8(const void* x, void* out, int64_t rows, int neg_id, int pos_id, hipStream_t st,
                        uint32_t* nan_flag = nullptr) {
  const Lut16Host& h = lut16_host(neg_id, pos_id);
  Lut16Args args = h.args;
  args.nan_flag = nan_flag;
  const int64_t n_vec = rows * 16;   // rows of 128 halves
  return launch_tab(h, [](auto tab) { return rows16_lut_pair_kernel<8, DUAL, tab.value>; }, grid_for(tiles_of(n_vec, 2), 1 << 20),
                    st, x, out, n_vec, args);
}

template <bool DUAL>
int launch_fast16_block(const void* x, void* out, int64_t rows, int64_t cols, int neg_id, int pos_id,
                        hipStream_t st, uint32_t* nan_flag = nullptr, bool gelu = false, void* gelu_out = nullptr) {
  const Lut16Host& h = lut16_host(neg_id, pos_id);
  Lut16Args args = h.args;
  args.nan_flag = nan_flag;
  args.gelu_out = gelu_out;
  const size_t lds = 0;   // the bucket table lives in static LDS (fpq_fast16.h)
  const int64_t vec_per_row = cols / 8;
  if (vec_per_row <= 64 * 5 && !fpq_flag(OPT_FPQ_NO_WAVE_ROWS) && !gelu) {
    // one wavefront per row: 4 rows per workgroup pass, enough workgroups to keep every CU busy while the
    // table staging stays amortised
    const int mc = (int)((vec_per_row + 63) / 64);
    int64_t g = (rows + 3) / 4;
    const int64_t capw = h.tab_valid ? 16384 : 2048;
    if (g > capw) g = capw;
    // rows of four or five vectors per lane on E2M3 / E3M2 (per-token FP6 at C = 1920, 2048, 2304): levels from the FP6
    // conversion hardware, no table (fpq_fast16.h, fp6_levels_hw32); FPQ_NO_HW6 (read at every call) keeps the table
    if constexpr (!DUAL) {
      if ((mc == 4 || mc == 5) && neg_id == pos_id && (neg_id == FPQ_E2M3 || neg_id == FPQ_E3M2) && !fpq_flag(OPT_FPQ_NO_HW6)) {
        int64_t g6 = (rows + 3) / 4;
        if (g6 > (1 << 20)) g6 = 1 << 20;   // nothing to amortise: one pass of four rows per workgroup
        return with_int<4, 5>(mc, [&](auto m) {
          constexpr int M = m.value;
          return with_int<1, 2>(neg_id == FPQ_E2M3 ? 1 : 2, [&](auto hw) {   // the conversion: 1 E2M3, 2 E3M2
            return launch(rows16_lut_wave_kernel<false, M, true, hw.value>, (unsigned)g6, lds, st, x, out, rows, cols, args,
                          h.tab);
          });
        });
      }
    }
    return with_int<1, 2, 4, 5>(step_for(mc, {1, 2, 4, 5}), [&](auto m) {
      constexpr int M = m.value;
      return launch_tab(h, [](auto tab) { return rows16_lut_wave_kernel<DUAL, M, tab.value>; }, (unsigned)g, st, x, out, rows, cols,
                        args);
    });
  }
  const int maxc = (int)((vec_per_row + kBlock - 1) / kBlock);
  // enough workgroups to fill the chip several times over, each walking consecutive rows
  // one row per workgroup, dispatched in address order, when the table arrives as a kernel argument (measured on
  // [65536 x 7680]: 0.785 of 8 TB/s vs 0.676 with four consecutive rows per workgroup); a table that every workgroup
  // has to evaluate itself is amortised over more rows
  const int64_t target_wgs = h.tab_valid ? (1 << 20) : 2048;
  int64_t rpb = (rows + target_wgs - 1) / target_wgs;
  if (rpb < 1) rpb = 1;
  if (h.tab_valid && lut16_buckets(h) >= kBigTab) {   // 2 x 512 (E2M3: [16384 x 7680] 86.3 -> 83.4 us) or 2 x 1024 buckets to stage: two rows per workgroup
    rpb = fpq_opt(OPT_FPQ_BIGTAB_RPB, 2);
    if (rpb < 1) rpb = 1;
  }
  const dim3 grid((unsigned)((rows + rpb - 1) / rpb));
  return with_int<1, 2, 4, 5, 8>(step_for(maxc, {1, 2, 4, 5, 8}), [&](auto c) {
    constexpr int C = c.value;
    if constexpr (DUAL) {
      if (gelu)   // GELU in front of the quantizer (fpq_gelu_quant_rows_dual): one workgroup per row for every row length
        return launch_tab(h, [](auto tab) { return rows16_lut_block_kernel<true, C, tab.value, true>; }, grid, st, x, out, rows,
                          cols, rpb, args);
    }
    return launch_tab(h, [](auto tab) { return rows16_lut_block_kernel<DUAL, C, tab.value>; }, grid, st, x, out, rows, cols, rpb,
                      args);
  });
}

// ---- fp32 rows of 128 (weights): fpq_fast32.h -------------------------------------------------
inline bool fast32_eligible(const void* x, const void* out, int64_t cols, int in_dtype, int table_id) {
  return in_dtype == FPQ_F32 && cols == 128 && kTables[table_id].symmetric && (((uintptr_t)x | (uintptr_t)out) & 15) == 0 &&
         !fpq_flag(OPT_FPQ_NO_FAST32);
}

// one tensor (segs == nullptr, `one` by value) or a device-resident segment table (grid.y = segment)
inline int launch_fast32(const Seg32* segs, int n_segs, const Seg32& one, int64_t max_rows, int table_id, int out_dtype,
                         hipStream_t st) {
  constexpr int U = 4;
  const int64_t tiles = tiles_of(max_rows * 32, U);
  if (tiles > 0x7FFFFFFF || n_segs > 65535) return FPQ_ERR_SHAPE;
  const dim3 grid((unsigned)tiles, (unsigned)n_segs);
  return with_dtype(out_dtype, [&](auto to) {
    return launch(groups32_lut_kernel<decltype(to), U>, grid, 0, st, segs, one, lut32_args(table_id));
  });
}

// fp32 groups of 128 -> codes + fp32 scales: one tensor (segs == nullptr) or a device-resident segment table
inline int launch_codes32(const CodesSeg32* segs, int n_segs, const CodesSeg32& one, int64_t max_rows, int table_id, bool pack,
                          hipStream_t st) {
  constexpr int U = 4;
  const int64_t tiles = tiles_of(max_rows * 32, U);
  if (tiles > 0x7FFFFFFF || n_segs > 65535) return FPQ_ERR_SHAPE;
  const dim3 grid((unsigned)tiles, (unsigned)n_segs);
  return with_bool(pack, [&](auto pk) {
    return launch(groups32_codes_kernel<pk.value, U>, grid, 0, st, segs, one, lut32_args(table_id));
  });
}

// long fp32 rows (per-channel weights): one wavefront or one workgroup per row (fpq_fast32.h)
inline bool rows32_eligible(const void* x, const void* out, int64_t cols, int in_dtype, int table_id) {
  return in_dtype == FPQ_F32 && cols % 8 == 0 && cols >= 512 && cols / 4 <= 256 * 10 && kTables[table_id].symmetric &&
         (((uintptr_t)x | (uintptr_t)out) & 15) == 0 && !fpq_flag(OPT_FPQ_NO_FAST32);
}

template <typename Tout>
int launch_rows32(const void* x, void* out, int64_t rows, int64_t cols, int table_id, hipStream_t st) {
  const int64_t vpr = cols / 4;
  auto go = [&](auto lanes, auto m) {   // lanes per row, vectors per lane
    constexpr int L = lanes.value;
    const int64_t wgs = (rows + (kBlock / L) - 1) / (kBlock / L);
    return launch(rows32_lut_kernel<Tout, L, m.value>, grid_for(wgs, 1 << 16), 0, st, x, out, rows, cols, lut32_args(table_id));
  };
  if (vpr <= 64 * 2) return go(Int<64>{}, Int<2>{});
  if (vpr <= 64 * 4) return go(Int<64>{}, Int<4>{});
  if (vpr <= 64 * 8) return go(Int<64>{}, Int<8>{});
  if (vpr <= 256 * 3) return go(Int<256>{}, Int<3>{});
  if (vpr <= 256 * 4) return go(Int<256>{}, Int<4>{});
  if (vpr <= 256 * 6) return go(Int<256>{}, Int<6>{});
  if (vpr <= 256 * 8) return go(Int<256>{}, Int<8>{});
  return go(Int<256>{}, Int<10>{});
}

template <typename T>
int launch_negrev(const void* x, void* out, int64_t rows, int64_t cols, const Fmt& fs, hipStream_t st) {
  constexpr int V = DT<T>::kVec;
  constexpr int U = 2;
  const bool aligned = (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  const int64_t lpr = cols / V;
  if (aligned && cols % V == 0 && lpr <= 64 && (lpr & (lpr - 1)) == 0) {   // 1 .. 64 lanes per row: every power of two is in the list
    const int64_t n_vec = rows * lpr;
    return with_int<1, 2, 4, 8, 16, 32, 64>((int)lpr, [&](auto l) {
      return launch(rows_negrev_subwave_kernel<T, l.value, U>, grid_for(tiles_of(n_vec, U), 1 << 20), 0, st, x, out, n_vec, fs);
    });
  }
  return launch(rows_negrev_scalar_kernel<T>, grid_for(rows, 65535), 0, st, x, out, rows, cols, fs);
}

// the tail of the dual quantizers that were given a NaN flag: any NaN in the input => the whole result is zero
inline int zero_if_flag(void* out, int64_t n_bytes, void* flag, hipStream_t st) {
  return launch(zero_if_flag_kernel, kFixupBlocks, 0, st, out, n_bytes, flag);
}

}  // namespace

// =================================================================================
// C ABI
// =================================================================================
extern "C" {

int fpq_version(void) { return FPQ_VERSION; }

int fpq_internal_zero_if_flag(void* out, int64_t n_bytes, void* scratch, void* stream) {
  return zero_if_flag(out, n_bytes, scratch, (hipStream_t)stream);
}
int fpq_internal_sqerr_finish(const float* partials, int n_partials, float* out, void* stream) {
  return launch(sqerr_finish_kernel, 1, 0, (hipStream_t)stream, partials, n_partials, 1, out);
}

int fpq_set_option(const char* name, int value) {
  const int i = option_index(name);
  if (i < 0) return FPQ_ERR_ARG;
  __atomic_store_n(&fpq_option_table[i], value, __ATOMIC_RELAXED);
  return FPQ_OK;
}
int fpq_get_option(const char* name, int* value_out) {
  const int i = option_index(name);
  if (i < 0 || !value_out) return FPQ_ERR_ARG;
  *value_out = fpq_opt_raw(i);
  return FPQ_OK;
}
const char* fpq_option_name(int index) { return (index >= 0 && index < FPQ_OPT_COUNT) ? kOptionDescs[index].name : nullptr; }

const char* fpq_strerror(int status) {
  switch (status) {
    case FPQ_OK: return "ok";
    case FPQ_ERR_ARG: return "invalid argument (null pointer or negative size)";
    case FPQ_ERR_DTYPE: return "unsupported dtype for this entry point";
    case FPQ_ERR_SHAPE: return "unsupported shape";
    case FPQ_ERR_TABLE: return "unknown table id, or half table passed where a symmetric table is required";
    case FPQ_ERR_LAUNCH: return "HIP kernel launch failed";
    case FPQ_ERR_NO_DEVICE: return "no HIP device";
    default: return "unknown fpq status";
  }
}

int fpq_table_values(int table_id, float* host_out) {
  if (table_id < 0 || table_id >= FPQ_NUM_TABLES) return FPQ_ERR_TABLE;
  float pos[64];
  int np = pos_levels(table_id, pos);
  int n = 0;
  const bool neg_half = (table_id == FPQ_E1M2_NEG || table_id == FPQ_INT_NEG || table_id == FPQ_E2M1_NEG);
  const bool pos_half = (table_id == FPQ_E2M1_POS || table_id == FPQ_E2M3_POS);
  const bool dup_zero = (table_id == FPQ_E2M3 || table_id == FPQ_E3M2);
  if (!pos_half) {
    for (int i = np - 1; i >= 1; --i, ++n)
      if (host_out) host_out[n] = -pos[i];
    if (neg_half || dup_zero) {
      if (host_out) host_out[n] = 0.0f;
      ++n;
    }
  }
  if (!neg_half)
    for (int i = 0; i < np; ++i, ++n)
      if (host_out) host_out[n] = pos[i];
  return n;
}

static const KnownTables& known_tables() {
  static const KnownTables* kt = [] {
    auto* t = new KnownTables();
    int off = 0;
    for (int id = 0; id < FPQ_NUM_TABLES; ++id) {
      t->off[id] = (int16_t)off;
      t->k[id] = (int16_t)fpq_table_values(id, t->v + off);
      off += t->k[id];
      t->fmt[id] = make_fmt(id);
      t->side[id] = kTables[id].symmetric ? 0 : ((id == FPQ_E2M1_POS || id == FPQ_E2M3_POS) ? 2 : 1);
    }
    return t;
  }();
  return *kt;
}

int fpq_quant_nearest(const void* x, const float* table, void* z, int64_t n, int k, int dtype,
                      fpq_stream_t stream) {
  if (n < 0) return FPQ_ERR_ARG;
  if (k < 1 || k > 256) return FPQ_ERR_SHAPE;
  if (dtype != FPQ_F32 && dtype != FPQ_F64) return FPQ_ERR_DTYPE;
  if (n == 0) return FPQ_OK;
  if (!x || !table || !z) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FPQ_F32)
    return launch(nearest_scan_kernel<float>, grid_for(tiles_of(n / 4, 2) + 1, 4096), 0, st, x, table, z, n, k, known_tables());
  return launch(nearest_scan_kernel<double>, grid_for(tiles_of(n, 1)), 0, st, x, table, z, n, k, known_tables());
}

int fpq_quant_nearest_argmin(const void* x, const float* table, float* z, int64_t n, int k, int dtype,
                             fpq_stream_t stream) {
  if (n < 0) return FPQ_ERR_ARG;
  if (k < 1 || k > 256) return FPQ_ERR_SHAPE;
  if (!is_f16_or_f32(dtype)) return FPQ_ERR_DTYPE;
  if (n == 0) return FPQ_OK;
  if (!x || !table || !z) return FPQ_ERR_ARG;
  return with_dtype(dtype, [&](auto t) {
    return launch(nearest_argmin_kernel<decltype(t)>, grid_for(tiles_of(n, 1), 8192), 0, (hipStream_t)stream, x, table, z, n, k);
  });
}

int fpq_quant_nearest_builtin(const float* x, float* z, int64_t n, int table_id, fpq_stream_t stream) {
  if (n < 0) return FPQ_ERR_ARG;
  if (table_id < 0 || table_id >= FPQ_NUM_TABLES) return FPQ_ERR_TABLE;
  if (n == 0) return FPQ_OK;
  if (!x || !z) return FPQ_ERR_ARG;
  int side = kTables[table_id].symmetric ? 0 : ((table_id == FPQ_E1M2_NEG || table_id == FPQ_INT_NEG || table_id == FPQ_E2M1_NEG) ? 1 : 2);
  return launch(nearest_builtin_kernel, grid_for(tiles_of(n, 1)), 0, (hipStream_t)stream, x, z, n, make_fmt(table_id), side);
}

int fpq_quant_rows(const void* x, void* out, int64_t rows, int64_t cols, int table_id, int in_dtype, int out_dtype,
                   fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype) || !is_f16_or_f32(out_dtype)) return FPQ_ERR_DTYPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !out) return FPQ_ERR_ARG;
  if (fast16_eligible(x, out, cols, in_dtype, out_dtype)) {
    // tables of >= 1024 buckets (E2M3, int: 2 KiB to stage per workgroup, a quarter of an 8 KiB tile's own bytes): at most
    // 16384 workgroups, so that at the large shapes every workgroup stages once for two tiles or more - E2M3 g = 128 and
    // KV rows of 64 at [65536 x 1920]: 84.2 -> 80.8 us (caps 10240 .. 24576: 82.3 .. 80.6; U = 4 and U = 1 are slower,
    // profiles/r03_e2m3_grid.txt)
    const int cap = lut16_buckets(lut16_host(table_id, table_id)) >= kBigTab ? 16384 : 1 << 20;
    return launch_fast16<false>(x, out, rows, cols, table_id, table_id, (hipStream_t)stream, cap);
  }
  if (fast16_block_eligible(x, out, cols, in_dtype, out_dtype))
    return launch_fast16_block<false>(x, out, rows, cols, table_id, table_id, (hipStream_t)stream);
  if (fast32_eligible(x, out, cols, in_dtype, table_id)) {
    const Seg32 one = {x, out, rows};
    return launch_fast32(nullptr, 1, one, rows, table_id, out_dtype, (hipStream_t)stream);
  }
  if (rows32_eligible(x, out, cols, in_dtype, table_id))
    return with_dtype(out_dtype, [&](auto to) { return launch_rows32<decltype(to)>(x, out, rows, cols, table_id, (hipStream_t)stream); });
  DualArgs dual = {};
  dual.nan_flag = nullptr;
  return dispatch_rows<false>(x, out, rows, cols, in_dtype, out_dtype, make_fmt(table_id), dual,
                              (hipStream_t)stream);
}

int fpq_quant_rows_multi(const fpq_segment_t* segments_host, int n_segments, int64_t cols, int table_id, int in_dtype,
                         int out_dtype, fpq_stream_t stream) {
  if (n_segments < 0 || cols < 0 || (n_segments > 0 && !segments_host)) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype) || !is_f16_or_f32(out_dtype)) return FPQ_ERR_DTYPE;
  for (int i = 0; i < n_segments; ++i) {
    if (segments_host[i].rows < 0) return FPQ_ERR_ARG;
    if (segments_host[i].rows > 0 && cols > 0 && (!segments_host[i].x || !segments_host[i].out)) return FPQ_ERR_ARG;
  }
  if (n_segments == 0 || cols == 0) return FPQ_OK;
  hipStream_t st = (hipStream_t)stream;
  bool one_launch = in_dtype == FPQ_F16 && out_dtype == FPQ_F16 && n_segments <= kMaxMulti && cols % 8 == 0;
  const int64_t lpr = cols / 8;
  one_launch = one_launch && lpr >= 1 && lpr <= 64 && (lpr & (lpr - 1)) == 0 && lut16_host(table_id, table_id).tab_valid;
  int64_t max_vec = 0;
  for (int i = 0; one_launch && i < n_segments; ++i) {
    if ((((uintptr_t)segments_host[i].x | (uintptr_t)segments_host[i].out) & 15) != 0) one_launch = false;
    max_vec = segments_host[i].rows * lpr > max_vec ? segments_host[i].rows * lpr : max_vec;
  }
  if (!one_launch) {   // anything the fused multi-tensor kernel does not cover: still one C call, one launch per tensor
    for (int i = 0; i < n_segments; ++i)
      if (int rc = fpq_quant_rows(segments_host[i].x, segments_host[i].out, segments_host[i].rows, cols, table_id, in_dtype,
                                  out_dtype, stream))
        return rc;
    return FPQ_OK;
  }
  if (max_vec == 0) return FPQ_OK;
  constexpr int U = 2;
  Multi16 m = {};
  for (int i = 0; i < n_segments; ++i) {
    m.x[i] = (const u32x4*)segments_host[i].x;
    m.out[i] = (u32x4*)segments_host[i].out;
    m.n_vec[i] = segments_host[i].rows * lpr;
  }
  const Lut16Host& h = lut16_host(table_id, table_id);
  const int64_t tiles = tiles_of(max_vec, U);
  if (tiles > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  const dim3 grid((unsigned)tiles, (unsigned)n_segments);
  return with_int<1, 2, 4, 8, 16, 32, 64>((int)lpr, [&](auto l) {
    return launch(rows16_lut_multi_kernel<l.value, U>, grid, 0, st, m, h.args, h.tab);
  });
}

int fpq_quant_rows_segments(const fpq_segment_t* segments_device, int n_segments, int64_t max_rows, int64_t cols,
                            int table_id, int in_dtype, int out_dtype, fpq_stream_t stream) {
  static_assert(sizeof(fpq_segment_t) == sizeof(Seg32), "fpq_segment_t and the kernels' Seg32 share one layout");
  if (n_segments < 0 || max_rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (in_dtype != FPQ_F32 || !is_f16_or_f32(out_dtype)) return FPQ_ERR_DTYPE;
  if (cols != 128) return FPQ_ERR_SHAPE;
  if (n_segments == 0 || max_rows == 0) return FPQ_OK;
  if (!segments_device || (((uintptr_t)segments_device) & 7) != 0) return FPQ_ERR_ARG;
  const Seg32 none = {nullptr, nullptr, 0};
  return launch_fast32((const Seg32*)segments_device, n_segments, none, max_rows, table_id, out_dtype, (hipStream_t)stream);
}

// qn: the q / k norm form (fpq_kv_cache_step_qknorm): its pointers checked by the caller, grid z = 3
static int kv_cache_step_impl(void* cache, int64_t batch, int64_t max_len, int64_t row_elems, int64_t quant_start,
                              int64_t quant_stop, const void* new_k, const void* new_v, int64_t new_batch_pitch,
                              int64_t new_token_pitch, int64_t new_start, int64_t n_new, int64_t group, int table_id,
                              fpq_stream_t stream, const KvStepQkn* qn) {
  if (batch < 0 || max_len < 0 || row_elems <= 0 || n_new < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (quant_start < 0 || quant_stop < quant_start || new_start < quant_stop || new_start + n_new > max_len)
    return FPQ_ERR_ARG;
  if (group != 8 && group != 16 && group != 32 && group != 64 && group != 128 && group != 256 && group != 512)
    return FPQ_ERR_SHAPE;                      // rows of 8 * {1..64} halves, owned by 1..64 lanes
  if (row_elems % group != 0 || batch > 65535) return FPQ_ERR_SHAPE;
  if (new_batch_pitch % 8 != 0 || new_token_pitch % 8 != 0 || new_token_pitch < 0 || new_batch_pitch < 0) return FPQ_ERR_SHAPE;
  const int64_t n_quant = quant_stop - quant_start;
  if (batch == 0 || (n_quant == 0 && n_new == 0)) return FPQ_OK;
  if (!cache || (n_new > 0 && (!new_k || !new_v))) return FPQ_ERR_ARG;
  if ((((uintptr_t)cache | (uintptr_t)new_k | (uintptr_t)new_v) & 15) != 0) return FPQ_ERR_ARG;
  const Lut16Host& h = lut16_host(table_id, table_id);
  if (!h.tab_valid) return FPQ_ERR_TABLE;
  constexpr int U = 2;
  KvStepArgs k;
  k.cache = (u32x4*)cache;
  k.row_vec = (int)(row_elems / 8);
  k.slab_vec = max_len * k.row_vec;
  k.batch = (int)batch;
  k.q_first_vec = quant_start * k.row_vec;
  k.q_vecs = n_quant * k.row_vec;
  const int64_t q_tiles = tiles_of(k.q_vecs, U);
  k.src[0] = (const uint16_t*)new_k;
  k.src[1] = (const uint16_t*)new_v;
  k.src_batch_pitch = new_batch_pitch;
  k.src_token_pitch = new_token_pitch;
  k.new_first_vec = new_start * k.row_vec;
  k.new_vecs = n_new * k.row_vec;
  const int64_t c_tiles = tiles_of(k.new_vecs, U);
  if (q_tiles + c_tiles > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  k.q_tiles = (int)q_tiles;
  const dim3 grid((unsigned)(q_tiles + c_tiles), (unsigned)batch, qn ? 3 : 2);
  const size_t lds = 0;   // the bucket table lives in static LDS (fpq_fast16.h)
  hipStream_t st = (hipStream_t)stream;
  if (qn)   // groups of 64 or 128 (fpq_kv_cache_step_qknorm checks)
    return with_int<8, 16>((int)(group / 8), [&](auto l) {
      return launch(kv16_step_qkn_kernel<l.value, U>, grid, lds, st, k, *qn, h.args, h.tab);
    });
  return with_int<1, 2, 4, 8, 16, 32, 64>((int)(group / 8), [&](auto l) {
    return launch(kv16_step_kernel<l.value, U>, grid, lds, st, k, h.args, h.tab);
  });
}

int fpq_kv_cache_step(void* cache, int64_t batch, int64_t max_len, int64_t row_elems, int64_t quant_start,
                      int64_t quant_stop, const void* new_k, const void* new_v, int64_t new_batch_pitch,
                      int64_t new_token_pitch, int64_t new_start, int64_t n_new, int64_t group, int table_id,
                      fpq_stream_t stream) {
  return kv_cache_step_impl(cache, batch, max_len, row_elems, quant_start, quant_stop, new_k, new_v, new_batch_pitch, new_token_pitch,
                            new_start, n_new, group, table_id, stream, nullptr);
}

int fpq_kv_cache_step_qknorm(void* cache, int64_t batch, int64_t max_len, int64_t row_elems, int64_t quant_start,
                             int64_t quant_stop, const void* new_q, const void* new_k, const void* new_v, int64_t new_batch_pitch,
                             int64_t new_token_pitch, int64_t new_start, int64_t n_new, int64_t group, int table_id,
                             void* q_out, const float* q_head_scale, const float* bias, int64_t head_dim, fpq_stream_t stream) {
  if (head_dim != 64 || row_elems <= 0 || row_elems % 64 != 0 || (group != 64 && group != 128)) return FPQ_ERR_ARG;
  if (!q_head_scale || ((uintptr_t)q_head_scale & 3) != 0 || ((uintptr_t)bias & 15) != 0) return FPQ_ERR_ARG;
  if (n_new > 0 && (!new_q || !q_out || (((uintptr_t)new_q | (uintptr_t)q_out) & 15) != 0)) return FPQ_ERR_ARG;
  KvStepQkn qn;
  qn.q = (const uint16_t*)new_q;
  qn.q_out = (u32x4*)q_out;
  qn.q_scale = q_head_scale;
  qn.bias = bias;
  qn.row_elems = (int)row_elems;
  return kv_cache_step_impl(cache, batch, max_len, row_elems, quant_start, quant_stop, new_k, new_v, new_batch_pitch, new_token_pitch,
                            new_start, n_new, group, table_id, stream, &qn);
}

int fpq_quant_rows_argmin(const void* x, float* out, int64_t rows, int64_t cols, int table_id, int in_dtype,
                          int clamp3, fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !out) return FPQ_ERR_ARG;
  Fmt f = make_fmt(table_id);
  f.argmin = 1;
  f.preclamp = clamp3 ? 3.0f : 0.0f;
  DualArgs dual = {};
  dual.nan_flag = nullptr;
  return dispatch_rows<false>(x, out, rows, cols, in_dtype, FPQ_F32, f, dual, (hipStream_t)stream);
}

int fpq_quant_rows_dual(const void* x, void* out, int64_t rows, int64_t cols, int neg_table, int pos_table,
                        int in_dtype, int out_dtype, const void* clip_absmax, float clip_strength, void* nan_flag,
                        fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_dual_pair(neg_table, pos_table)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype) || !is_f16_or_f32(out_dtype)) return FPQ_ERR_DTYPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !out) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* flag = (uint32_t*)nan_flag;
  if (flag && (((uintptr_t)flag) & 7) != 0) return FPQ_ERR_ARG;
  int rc;
  const bool bigtab = lut16_buckets(lut16_host(neg_table, pos_table)) > kBigTab;
  if (clip_absmax && clip_strength >= 0.0f && cols == 128 && !bigtab && fast16_eligible(x, out, cols, in_dtype, out_dtype)) {
    // the global clamp on the fast path (fp16 groups of 128, strength >= 0; anything else below, through the generic kernel)
    rc = launch_fast16<true>(x, out, rows, cols, neg_table, pos_table, st, 1 << 20, flag, clip_absmax, clip_strength);
  } else if (!clip_absmax && fast16_eligible(x, out, cols, in_dtype, out_dtype)) {
    // int_neg/e2m3_pos needs a 2048-entry table (too big for the kernel arguments): every workgroup
    // evaluates it once, so give each workgroup many tiles (measured: 88 us vs 127 us with a full grid)
    // tables of 2 x 1024 buckets (int_neg / e2m3_pos) cost a workgroup 8 stores per lane to stage: give each
    // workgroup many tiles (capped grid, U = 4); the smaller ones run one tile per workgroup on a full grid
    if (lut16_buckets(lut16_host(neg_table, pos_table)) <= kBigTab)
      rc = launch_fast16<true>(x, out, rows, cols, neg_table, pos_table, st, 1 << 20, flag);
    else {
      const int cap = fpq_opt(OPT_FPQ_BIGTAB_CAP, 16384);   // measured on [65536 x 7680]: 4096 -> 366 us, 16384 -> 348 us, full grid -> 367 us
      rc = launch_fast16<true, 4>(x, out, rows, cols, neg_table, pos_table, st, cap, flag);
    }
  } else if (!clip_absmax && fast16_block_eligible(x, out, cols, in_dtype, out_dtype)) {
    rc = launch_fast16_block<true>(x, out, rows, cols, neg_table, pos_table, st, flag);
  } else {
    DualArgs dual;
    dual.fneg = make_fmt(neg_table);
    dual.fpos = make_fmt(pos_table);
    dual.clip_absmax = clip_absmax;
    dual.clip_strength = clip_strength;
    dual.nan_flag = flag;
    rc = dispatch_rows<true>(x, out, rows, cols, in_dtype, out_dtype, dual.fneg, dual, st);
  }
  if (rc != FPQ_OK || !flag) return rc;
  return zero_if_flag(out, rows * cols * (out_dtype == FPQ_F16 ? 2 : 4), flag, st);
}

int fpq_gelu_quant_rows_dual(const void* x, void* out, void* gelu_out, int64_t rows, int64_t cols, int neg_table, int pos_table,
                             void* nan_flag, fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_dual_pair(neg_table, pos_table)) return FPQ_ERR_TABLE;
  // groups of 128 (rows inside a wavefront) or rows of at most 16384 elements (one workgroup per row: the per-token forms)
  if (cols <= 0 || cols % 8 != 0 || cols > 8 * 8 * kBlock) return FPQ_ERR_SHAPE;
  if (rows == 0) return FPQ_OK;
  if (!x || !out) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)gelu_out) & 15) != 0 || ((uintptr_t)nan_flag & 7) != 0) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* flag = (uint32_t*)nan_flag;
  int rc;
  if (cols != 128)
    rc = launch_fast16_block<true>(x, out, rows, cols, neg_table, pos_table, st, flag, true, gelu_out);
  else if (lut16_buckets(lut16_host(neg_table, pos_table)) <= kBigTab)
    rc = launch_fast16<true>(x, out, rows, cols, neg_table, pos_table, st, 1 << 20, flag, nullptr, 1.0f, true, gelu_out);
  else   // int_neg / e2m3_pos: 2 x 1024 buckets to stage per workgroup - many tiles per workgroup, as fpq_quant_rows_dual
    rc = launch_fast16<true, 4>(x, out, rows, cols, neg_table, pos_table, st, fpq_opt(OPT_FPQ_BIGTAB_CAP, 16384), flag, nullptr, 1.0f, true, gelu_out);
  if (rc != FPQ_OK || !flag) return rc;
  return zero_if_flag(out, rows * cols * 2, flag, st);
}

int fpq_quant_rows_neg_reverse(const void* x, void* out, int64_t rows, int64_t cols, int table_id, int dtype,
                               fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(dtype)) return FPQ_ERR_DTYPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !out) return FPQ_ERR_ARG;
  return with_dtype(dtype, [&](auto t) { return launch_negrev<decltype(t)>(x, out, rows, cols, make_fmt(table_id), (hipStream_t)stream); });
}

int fpq_quant_rows_dual_argmin(const void* x, float* out, int64_t rows, int64_t cols, int neg_table, int pos_table,
                               int in_dtype, const void* clip_absmax, float clip_strength, fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_dual_pair(neg_table, pos_table)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !out) return FPQ_ERR_ARG;
  DualArgs dual;
  dual.fneg = make_fmt(neg_table);
  dual.fpos = make_fmt(pos_table);
  dual.fneg.argmin = dual.fpos.argmin = 1;
  dual.clip_absmax = clip_absmax;
  dual.clip_strength = clip_strength;
  dual.nan_flag = nullptr;
  return dispatch_rows<true>(x, out, rows, cols, in_dtype, FPQ_F32, dual.fneg, dual, (hipStream_t)stream);
}

static int quant_rows_codes_mx_impl(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                    bool km, fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (km && in_dtype != FPQ_F16) return FPQ_ERR_DTYPE;   // fp32 rows (weights): fpq_quant_rows_codes_mx + fpq_codes_to_kmajor
  if (cols % 128 != 0 || (km && !km_image_fits(rows, cols / 2))) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !codes || !scales) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)codes | (uintptr_t)scales) & 15) != 0) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == FPQ_F16) {
    const Lut16Host& h = lut16_host(FPQ_E2M1, FPQ_E2M1);
    const int64_t n_vec = rows * (cols / 8);
    const size_t lds = 0;   // the bucket table lives in static LDS (fpq_fast16.h)
    return launch(rows16_codes_mx_kernel, grid_for(tiles_of(n_vec, 1), 16384), lds, st, x, (uint32_t*)codes, scales, n_vec, h.args,
                  lut16_mx_codes_e2m1(), km ? (uint32_t)rows : 0u, fast_div((uint32_t)(cols / 128)));
  }
  const int64_t n_vec = rows * (cols / 4);
  return launch(codes128_kernel<float, true, true>, grid_for(tiles_of(n_vec, 1), 1 << 20), 0, st, x, codes, scales, n_vec,
                make_fmt(FPQ_E2M1));
}
int fpq_quant_rows_codes_mx(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                            fpq_stream_t stream) {
  return quant_rows_codes_mx_impl(x, codes, scales, rows, cols, in_dtype, false, stream);
}
int fpq_quant_rows_codes_mx_km(const void* x, uint8_t* image, void* scales, int64_t rows, int64_t cols, int in_dtype,
                               fpq_stream_t stream) {
  return quant_rows_codes_mx_impl(x, image, scales, rows, cols, in_dtype, true, stream);
}

// per-group(128) E1M2 / E3M0 quantization to dense 6-bit codes (fpq_codes_g6.h, include/fpq.h)
int fpq_quant_rows_codes_g6(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id, int in_dtype,
                            fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (table_id != FPQ_E1M2 && table_id != FPQ_E3M0) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (cols % 128 != 0) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !codes || !scales) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)codes) & 15) != 0 || ((uintptr_t)scales & (in_dtype == FPQ_F16 ? 1 : 3)) != 0) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == FPQ_F16) {
    const Lut16Host& h = lut16_host(table_id, table_id);
    if (!h.tab_valid) return FPQ_ERR_TABLE;
    const int64_t n_vec = rows * (cols / 8);
    return launch(group6_emit16_kernel, grid_for(tiles_of(n_vec, 1), 16384), 0, st, x, codes, scales, n_vec, h.args,
                  lut16_codes_g6(table_id));
  }
  const int64_t n_blk = rows * (cols / 32);
  return with_bool(table_id == FPQ_E3M0, [&](auto e3m0) {   // (the other table: E1M2)
    return launch(group6_emit_kernel<float, e3m0.value>, grid_for(tiles_of(n_blk, 1), 1 << 20), 0, st, x, codes, scales, n_blk,
                  make_fmt(table_id));
  });
}

// the same quantization of fp16 rows straight into the A6W4 GEMM's k-major images (group6_km_emit16_kernel, include/fpq.h)
int fpq_a6w4_quant_rows_codes_km(const void* x, uint8_t* image, void* scales, int64_t rows, int64_t cols, int table_id, int in_dtype,
                               fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (table_id != FPQ_E1M2 && table_id != FPQ_E3M0) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype) || in_dtype != FPQ_F16) return FPQ_ERR_DTYPE;   // fp32 rows: fpq_quant_rows_codes_g6 + fpq_codes_to_kmajor
  if (cols % 128 != 0 || !km_image_fits(rows, cols / 4 * 3)) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !image || !scales) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)image | (uintptr_t)scales) & 15) != 0) return FPQ_ERR_ARG;
  const Lut16Host& h = lut16_host(table_id, table_id);
  if (!h.tab_valid) return FPQ_ERR_TABLE;
  const int64_t units = (rows + 15) / 16 * (cols / 128);
  return launch(group6_km_emit16_kernel, grid_for(units, 16384), 0, (hipStream_t)stream, x, image, scales, h.args, lut16_codes_g6(table_id),
                (uint32_t)rows, fast_div((uint32_t)(cols / 128)));
}

// per-group(128) quantization on the FULL FP6 tables (E2M3 / E3M2) to dense 6-bit codes, row-major or as the k-major images
// (include/fpq.h).  No kernel of its own: the emitters of fpq_codes_g6.h take their table as data - the fast forms the bucket ->
// code table (lut16_codes6: 1024 buckets for E2M3, inside what they stage), the generic form the closed form of make_fmt.
int fpq_gf6_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id, int in_dtype,
                             int kmajor, fpq_stream_t stream) {
  if (table_id != FPQ_E2M3 && table_id != FPQ_E3M2) return FPQ_ERR_TABLE;
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_f16_or_f32(in_dtype) || (kmajor && in_dtype != FPQ_F16)) return FPQ_ERR_DTYPE;   // fp32 rows as images: row-major + fpq_codes_to_kmajor
  if (cols % 128 != 0 || (kmajor && !km_image_fits(rows, cols / 4 * 3))) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !codes || !scales) return FPQ_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)codes) & 15) != 0) return FPQ_ERR_ARG;
  if (((uintptr_t)scales & (kmajor ? 15 : in_dtype == FPQ_F16 ? 1 : 3)) != 0) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == FPQ_F16) {
    const Lut16Host& h = lut16_host(table_id, table_id);
    if (!h.tab_valid) return FPQ_ERR_TABLE;
    if (kmajor) {
      const int64_t units = (rows + 15) / 16 * (cols / 128);
      return launch(group6_km_emit16_kernel, grid_for(units, 16384), 0, st, x, codes, scales, h.args, lut16_codes6(table_id),
                    (uint32_t)rows, fast_div((uint32_t)(cols / 128)));
    }
    const int64_t n_vec = rows * (cols / 8);
    return launch(group6_emit16_kernel, grid_for(tiles_of(n_vec, 1), 16384), 0, st, x, codes, scales, n_vec, h.args,
                  lut16_codes6(table_id));
  }
  const int64_t n_blk = rows * (cols / 32);
  return with_bool(table_id == FPQ_E3M2, [&](auto bf6) {   // (the other table: E2M3)
    return launch(group6_emit_kernel<float, bf6.value>, grid_for(tiles_of(n_blk, 1), 1 << 20), 0, st, x, codes, scales, n_blk,
                  make_fmt(table_id));
  });
}

// the packed file's codewords -> a GEMM's weight operand, and back (include/fpq.h; fpq_packed_operands.h): one launch each
int fpq_packed_to_operands(const uint8_t* codes, const void* scales, int scale_dtype, uint8_t* w_codes, float* w_scales, int64_t outs,
                           int64_t k, int64_t cols, int table_id, int kmajor, fpq_stream_t stream) {
  PoCall c;
  if (int rc = po_check(outs, k, cols, table_id, kmajor, scale_dtype, &c)) return rc;
  if (outs == 0 || k == 0) return FPQ_OK;
  const bool grouped = cols == 128;   // per channel: the scale vector is not part of the operand
  if (!codes || !w_codes || (grouped && (!scales || !w_scales))) return FPQ_ERR_ARG;
  if (!po_aligned16(codes, w_codes, grouped ? scales : nullptr, grouped ? w_scales : nullptr)) return FPQ_ERR_ARG;
  const dim3 grid(grid_for(tiles_of(c.units, 1), 1 << 16));
  return with_dtype(scale_dtype, [&](auto ts) {
    using Ts = decltype(ts);
    const Ts* sc = grouped ? (const Ts*)scales : nullptr;
    float* wsc = grouped ? w_scales : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (c.mode == kPo44) return launch(packed_to_operands_kernel<kPo44, Ts>, grid, 0, st, codes, sc, w_codes, wsc, outs, c.steps, c.image_rows, c.sh);
    if (c.mode == kPo46) return launch(packed_to_operands_kernel<kPo46, Ts>, grid, 0, st, codes, sc, w_codes, wsc, outs, c.steps, c.image_rows, c.sh);
    return launch(packed_to_operands_kernel<kPo66, Ts>, grid, 0, st, codes, sc, w_codes, wsc, outs, c.steps, c.image_rows, c.sh);
  });
}
int fpq_operands_to_packed(const uint8_t* w_codes, const float* w_scales, uint8_t* codes, float* scales, int64_t outs, int64_t k,
                           int64_t cols, int table_id, int kmajor, fpq_stream_t stream) {
  PoCall c;
  if (int rc = po_check(outs, k, cols, table_id, kmajor, FPQ_F32, &c)) return rc;
  if (outs == 0 || k == 0) return FPQ_OK;
  const bool grouped = cols == 128;
  if (!codes || !w_codes || (grouped && (!scales || !w_scales))) return FPQ_ERR_ARG;
  if (!po_aligned16(codes, w_codes, grouped ? scales : nullptr, grouped ? w_scales : nullptr)) return FPQ_ERR_ARG;
  const dim3 grid(grid_for(tiles_of(outs * c.steps * (c.mode == kPo66 ? 2 : 4), 1), 1 << 16));
  const float* wsc = grouped ? w_scales : nullptr;
  float* sc = grouped ? scales : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (c.mode == kPo44) return launch(operands_to_packed_kernel<kPo44>, grid, 0, st, w_codes, wsc, codes, sc, outs, c.steps, c.image_rows, c.sh);
  if (c.mode == kPo46) return launch(operands_to_packed_kernel<kPo46>, grid, 0, st, w_codes, wsc, codes, sc, outs, c.steps, c.image_rows, c.sh);
  return launch(operands_to_packed_kernel<kPo66>, grid, 0, st, w_codes, wsc, codes, sc, outs, c.steps, c.image_rows, c.sh);
}

int fpq_kv_pack(uint8_t* codes, void* scales, int kv_bit, int64_t batch, int64_t max_len, int64_t heads, int64_t head_dim, int64_t pos,
                const void* new_k, const void* new_v, int64_t new_batch_pitch, int64_t new_token_pitch, int64_t n_new,
                fpq_stream_t stream) {
  if (batch < 0 || max_len < 0 || heads <= 0 || head_dim != 64 || pos < 0 || n_new < 0 || pos + n_new > max_len) return FPQ_ERR_ARG;
  if ((kv_bit != 6 && kv_bit != 4) || (kv_bit == 4 && heads % 2 != 0) || batch > 65535 || heads > (1 << 20)) return FPQ_ERR_ARG;
  if (new_batch_pitch % 8 != 0 || new_token_pitch % 8 != 0 || new_batch_pitch < 0 || new_token_pitch < 0) return FPQ_ERR_ARG;
  if (batch == 0 || n_new == 0) return FPQ_OK;
  if (!codes || !scales || !new_k || !new_v) return FPQ_ERR_ARG;
  if ((((uintptr_t)codes | (uintptr_t)scales | (uintptr_t)new_k | (uintptr_t)new_v) & 15) != 0) return FPQ_ERR_ARG;
  const int table_id = kv_bit == 6 ? FPQ_E2M3 : FPQ_E2M1;
  const Lut16Host& h = lut16_host(table_id, table_id);
  if (!h.tab_valid) return FPQ_ERR_TABLE;
  constexpr int U = 2;
  KvPackArgs k;
  k.src[0] = (const uint16_t*)new_k;
  k.src[1] = (const uint16_t*)new_v;
  k.src_batch_pitch = new_batch_pitch;
  k.src_token_pitch = new_token_pitch;
  k.codes = codes;
  k.scales = (uint16_t*)scales;
  k.codes_slab = batch * max_len * heads * (kv_bit == 6 ? 48 : 32);
  k.scales_slab = batch * max_len * (kv_bit == 6 ? heads : heads / 2);
  k.max_len = max_len;
  k.pos = pos;
  k.row_vec = (int)(heads * 8);
  k.new_vecs = n_new * k.row_vec;
  const int64_t tiles = tiles_of(k.new_vecs, U);
  if (tiles > 0x7FFFFFFF) return FPQ_ERR_ARG;
  const dim3 grid((unsigned)tiles, (unsigned)batch, 2);
  hipStream_t st = (hipStream_t)stream;
  if (kv_bit == 6) return launch(kv_pack_kernel<6, U>, grid, 0, st, k, h.args, lut16_codes6_e2m3());
  return launch(kv_pack_kernel<4, U>, grid, 0, st, k, h.args, lut16_mx_codes_e2m1());
}

int fpq_absmax(const void* x, int64_t n, int dtype, void* out, fpq_stream_t stream) {
  if (n < 0 || !out) return FPQ_ERR_ARG;
  if (!is_f16_or_f32(dtype)) return FPQ_ERR_DTYPE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, 4, st) != hipSuccess) return FPQ_ERR_LAUNCH;
  if (n == 0) return FPQ_OK;
  if (!x) return FPQ_ERR_ARG;
  return with_dtype(dtype, [&](auto t) { return launch(absmax_kernel<decltype(t)>, grid_for(tiles_of(n, 16)), 0, st, x, n, out); });
}

int fpq_quant_tensor_argmin(const void* x, float* out, float* scale_out, void* workspace, int64_t n, int table_id,
                            int in_dtype, fpq_stream_t stream) {
  if (n < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (!scale_out || !workspace || (((uintptr_t)workspace | (uintptr_t)scale_out) & 3) != 0) return FPQ_ERR_ARG;
  if (n > 0 && (!x || !out)) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Fmt f = make_fmt(table_id);
  f.argmin = 1;
  const int g1 = grid_for(tiles_of(n, 16), FPQ_TENSOR_WORKSPACE_BYTES / 4);   // also 1 when n == 0
  return with_dtype(in_dtype, [&](auto t) {
    using T = decltype(t);
    const int g2 = grid_for(tiles_of(n / DT<T>::kVec, 2) + 1, 1 << 16);
    if (int rc = launch(absmax_partials_kernel<T>, g1, 0, st, x, n, workspace)) return rc;
    return launch(tensor_argmin_kernel<T>, g2, 0, st, x, out, n, workspace, g1, scale_out, f);
  });
}

int fpq_sqerr_rows_weighted(const void* ref, const void* y, const float* row_weight, float* out, void* workspace,
                            int64_t rows, int64_t cols, int planes, int dtype, fpq_stream_t stream) {
  if (!ref || !y || !row_weight || !out || !workspace || rows < 0 || cols < 0 || planes < 1 || planes > kSqerrMaxPlanes)
    return FPQ_ERR_ARG;
  if (!is_f16_or_f32(dtype)) return FPQ_ERR_DTYPE;
  const int64_t V = dtype == FPQ_F16 ? 8 : 4;
  if (cols == 0 || cols % V != 0 || rows > 0x7FFFFFFF) return FPQ_ERR_SHAPE;
  if (rows > 0 && cols / V > INT64_MAX / (rows * kSqerrMaxPlanes)) return FPQ_ERR_SHAPE;   // the planes' vectors are counted in 63 bits
  if ((((uintptr_t)ref | (uintptr_t)y | (uintptr_t)row_weight) & 15) != 0 || (((uintptr_t)out | (uintptr_t)workspace) & 3) != 0)
    return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  SqerrDeal d;
  d.row_vec = cols / V;
  d.n_vec = rows * d.row_vec;
  const int g1 = rows == 0 ? 0 : grid_for(tiles_of(d.n_vec, 1), kSqerrMaxBlocks);
  if (g1 > 0) {
    d.step_rows = (int64_t)g1 * kBlock / d.row_vec;
    d.step_cols = (int64_t)g1 * kBlock % d.row_vec;
    const int rc = with_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      return with_int<1, 2, 3, 4>(planes, [&](auto p) {
        return launch(sqerr_partials_kernel<T, p.value>, g1, 0, st, ref, y, row_weight, workspace, d);
      });
    });
    if (rc != FPQ_OK) return rc;
  }
  return launch(sqerr_finish_kernel, 1, 0, st, workspace, g1, planes, out);   // rows == 0: no partials, `planes` zeros
}

int fpq_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id,
                         int in_dtype, int pack_nibbles, fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (pack_nibbles && kTables[table_id].n_pos > 8) return FPQ_ERR_SHAPE;  // FP6 codes do not fit a nibble
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!x || !codes || !scales) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Fmt f = make_fmt(table_id);
  if (in_dtype == FPQ_F32 && cols == 128 && (((uintptr_t)x | (uintptr_t)codes) & 15) == 0 && (((uintptr_t)scales) & 3) == 0 &&
      !fpq_flag(OPT_FPQ_NO_FAST32)) {   // fp32 weights: the approximate-then-verify path (fpq_fast32.h, groups32_codes_kernel)
    const CodesSeg32 one = {x, codes, scales, rows};
    return launch_codes32(nullptr, 1, one, rows, table_id, pack_nibbles != 0, st);
  }
  if (cols == 128 && (((uintptr_t)x | (uintptr_t)codes | (uintptr_t)scales) & 15) == 0) {
    const int64_t n_vec = rows * (in_dtype == FPQ_F16 ? 16 : 32);
    return with_dtype(in_dtype, [&](auto t) {
      return with_bool(pack_nibbles != 0, [&](auto pk) {
        return launch(codes128_kernel<decltype(t), pk.value>, grid_for(tiles_of(n_vec, 1), 1 << 20), 0, st, x, codes, scales, n_vec, f);
      });
    });
  }
  return with_dtype(in_dtype, [&](auto t) {
    return launch(rows_codes_kernel<decltype(t)>, grid_for(rows, 65535), 0, st, x, codes, scales, rows, cols, f, pack_nibbles ? 1 : 0);
  });
}

int fpq_dequant_rows_codes(const uint8_t* codes, const void* scales, void* out, int64_t rows, int64_t cols,
                           int table_id, int scale_dtype, int out_dtype, int pack_nibbles, fpq_stream_t stream) {
  if (rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(scale_dtype) || !is_f16_or_f32(out_dtype)) return FPQ_ERR_DTYPE;
  if (pack_nibbles && kTables[table_id].n_pos > 8) return FPQ_ERR_SHAPE;
  if (rows == 0 || cols == 0) return FPQ_OK;
  if (!codes || !scales || !out) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Fmt f = make_fmt(table_id);
  if (cols == 128 && (((uintptr_t)out | (uintptr_t)codes) & 15) == 0) {
    const int64_t n_oct = rows * 16;
    const int64_t per_wg = pack_nibbles ? 4 * kBlock : kBlock;   // the nibble form decodes tiles of 4 x 256 octets
    const int gv = grid_for((n_oct + per_wg - 1) / per_wg, 1 << 20);
    return with_dtype(scale_dtype, [&](auto ts) {
      return with_dtype(out_dtype, [&](auto to) {
        return with_bool(pack_nibbles != 0, [&](auto pk) {
          return launch(decode128_kernel<decltype(ts), decltype(to), pk.value>, gv, 0, st, codes, scales, out, n_oct, f);
        });
      });
    });
  }
  return with_dtype(scale_dtype, [&](auto ts) {
    return with_dtype(out_dtype, [&](auto to) {
      return launch(rows_decode_kernel<decltype(ts), decltype(to)>, grid_for(rows, 65535), 0, st, codes, scales, out, rows, cols, f,
                    pack_nibbles ? 1 : 0);
    });
  });
}

int fpq_quant_rows_codes_segments(const fpq_codes_segment_t* segments_device, int n_segments, int64_t max_rows,
                                  int64_t cols, int table_id, int in_dtype, int pack_nibbles, fpq_stream_t stream) {
  static_assert(sizeof(fpq_codes_segment_t) == sizeof(CodesSeg), "fpq_codes_segment_t and the kernels' CodesSeg share one layout");
  if (n_segments < 0 || max_rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(in_dtype)) return FPQ_ERR_DTYPE;
  if (cols != 128 || n_segments > 65535) return FPQ_ERR_SHAPE;
  if (pack_nibbles && kTables[table_id].n_pos > 8) return FPQ_ERR_SHAPE;
  if (n_segments == 0 || max_rows == 0) return FPQ_OK;
  if (!segments_device || (((uintptr_t)segments_device) & 7) != 0) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == FPQ_F32 && !fpq_flag(OPT_FPQ_NO_FAST32)) {   // (segments are 16-byte aligned by contract, include/fpq.h)
    static_assert(sizeof(CodesSeg32) == sizeof(CodesSeg), "one segment layout");
    return launch_codes32((const CodesSeg32*)segments_device, n_segments, CodesSeg32{nullptr, nullptr, nullptr, 0}, max_rows, table_id,
                          pack_nibbles != 0, st);
  }
  const Fmt f = make_fmt(table_id);
  const int64_t n_vec = max_rows * (in_dtype == FPQ_F16 ? 16 : 32);
  // a few vectors per thread in the largest segment: the grid's y dimension multiplies it by the segment count
  const dim3 grid((unsigned)grid_for((n_vec + 4 * kBlock - 1) / (4 * kBlock), 1 << 16), (unsigned)n_segments);
  const CodesSeg* sg = (const CodesSeg*)segments_device;
  return with_dtype(in_dtype, [&](auto t) {
    return with_bool(pack_nibbles != 0, [&](auto pk) { return launch(codes128_segments_kernel<decltype(t), pk.value>, grid, 0, st, sg, f); });
  });
}

int fpq_dequant_rows_codes_segments(const fpq_decode_segment_t* segments_device, int n_segments, int64_t max_rows,
                                    int64_t cols, int table_id, int scale_dtype, int out_dtype, int pack_nibbles,
                                    fpq_stream_t stream) {
  static_assert(sizeof(fpq_decode_segment_t) == sizeof(DecodeSeg), "fpq_decode_segment_t and the kernels' DecodeSeg share one layout");
  if (n_segments < 0 || max_rows < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_symmetric_table(table_id)) return FPQ_ERR_TABLE;
  if (!is_f16_or_f32(scale_dtype) || !is_f16_or_f32(out_dtype)) return FPQ_ERR_DTYPE;
  if (cols != 128 || n_segments > 65535) return FPQ_ERR_SHAPE;
  if (pack_nibbles && kTables[table_id].n_pos > 8) return FPQ_ERR_SHAPE;
  if (n_segments == 0 || max_rows == 0) return FPQ_OK;
  if (!segments_device || (((uintptr_t)segments_device) & 7) != 0) return FPQ_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const Fmt f = make_fmt(table_id);
  const int64_t n_oct = max_rows * 16;
  const dim3 grid((unsigned)grid_for((n_oct + 4 * kBlock - 1) / (4 * kBlock), 1 << 16), (unsigned)n_segments);
  const DecodeSeg* sg = (const DecodeSeg*)segments_device;
  return with_dtype(scale_dtype, [&](auto ts) {
    return with_dtype(out_dtype, [&](auto to) {
      return with_bool(pack_nibbles != 0, [&](auto pk) {
        return launch(decode128_segments_kernel<decltype(ts), decltype(to), pk.value>, grid, 0, st, sg, f);
      });
    });
  });
}

}  // extern "C"
