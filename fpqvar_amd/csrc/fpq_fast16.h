// fpq_fast16.h - the fp16 -> fp16 hot path (activations, KV cache).  Included by every translation unit inside its
// anonymous namespace; at its end, the host caches of the bucket tables that the units share.
//
// Same results as the generic kernels (rows_subwave_kernel / rows_block_kernel),
// about a fifth of their VALU work per element:
//
//   * xn = fp16(x / s) costs 3 fp32 ops instead of an IEEE division sequence:
//         y  = x * inv            inv = v_rcp_f32(s)   (once per row)
//         e  = fma(-y, s, x)      exact residual
//         y2 = fma(e, inv, y)     = RN32(x/s * (1 - O(2^-44)))
//     x and s carry 11 significant bits, so x/s is either exactly a 12-bit number
//     (then y2 lands on it exactly and the fp16 tie rounds to even as IEEE does) or at
//     least 2^-23 (relative) away from every 12-bit number, i.e. from every fp16
//     rounding boundary (then y2 is on the same side).  Either way
//     fp16(y2) == fp16(RN32(x/s)) == what torch's fp16 division produces.
//     (Rounding the LAST fma straight to fp16 - v_fma_mixlo_f16 - would be wrong in
//     the tie case: the fp32 rounding is what snaps y2 onto the tie.)
//   * scale = fp16(amax / gmax) the same way with the compile-time-free constant 1/gmax.
//   * the minifloat rounding is a table in LDS indexed by the top bits of xn's fp16
//     pattern: every rounding threshold of every supported table is a multiple of
//     2^shift in that bit pattern (E2M1: shift 8 -> 256 entries; int_neg: shift 5),
//     so bucket -> level is exact.  "tie goes to the larger VALUE" becomes: subtract
//     1 from a negative pattern's magnitude before bucketing.  The entry is the fp16
//     pattern of the (signed) level with the table's zero as +0, so -0.0 never appears.
//     The table is filled per workgroup from the same closed form the generic kernels
//     use (quant_mag), which tests pin to the reference's scan.
//   * out = v_pk_mul_f16(level, scale): the exact product rounded once = fp16(fp32(q*s)).
//   * absmax on packed 16-bit integer patterns (NaN = largest pattern propagates like
//     torch.max), row reduction in DPP (rows of 8/16 lanes never leave a DPP row).
#pragma once

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef uint16_t us2_t __attribute__((ext_vector_type(2)));
typedef int16_t s2_t __attribute__((ext_vector_type(2)));

constexpr int kLutLdsEntries = 2048;   // shift >= 5: at most 2 x 1024 buckets

struct Lut16Args {
  Fmt fneg, fpos;      // identical for the symmetric tables
  float inv_gneg;      // RN32(1 / gmax) per side
  float inv_gpos;
  int shift;           // bucket width = 2^shift fp16 patterns
  uint32_t* nan_flag;  // dual format only: nullptr, or device word OR-ed with 1 when an input is NaN
  const void* clip_absmax;   // dual format per group only (CLIP kernels): device scalar max|x| in x's dtype, or nullptr
  float clip_strength;       // the reference's global clamp to +-strength * max|x| (tr/quant_utils.py:421-422)
  void* gelu_out;            // GELU kernels only: nullptr, or fp16 [rows, cols] receiving the GELU values the quantizer saw
};

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  us2_t r = __builtin_elementwise_max(__builtin_bit_cast(us2_t, a), __builtin_bit_cast(us2_t, b));
  return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t pk_max_i16(uint32_t a, uint32_t b) {
  s2_t r = __builtin_elementwise_max(__builtin_bit_cast(s2_t, a), __builtin_bit_cast(s2_t, b));
  return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t pk_sub_u16(uint32_t a, uint32_t b) {
  us2_t r = __builtin_bit_cast(us2_t, a) - __builtin_bit_cast(us2_t, b);
  return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t pk_lshr_u16(uint32_t a, int n) {
  us2_t r = __builtin_bit_cast(us2_t, a) >> (uint16_t)n;
  return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t pk_ashr_i16(uint32_t a, int n) {
  s2_t r = __builtin_bit_cast(s2_t, a) >> (int16_t)n;
  return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t pk_add_f16(uint32_t a, uint32_t b) {
  h2_t r = __builtin_bit_cast(h2_t, a) + __builtin_bit_cast(h2_t, b);
  return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t pk_mul_f16(uint32_t a, uint32_t b) {
  h2_t r = __builtin_bit_cast(h2_t, a) * __builtin_bit_cast(h2_t, b);
  return __builtin_bit_cast(uint32_t, r);
}

// two fp32 values -> packed fp16 pair with ONE v_cvt_pk_f16_f32 (round to nearest even).  The
// asm barrier keeps both values as rounded fp32 numbers first (see f2h in fpq_common.h).
__device__ __forceinline__ uint32_t f2h2(float lo, float hi) {
  asm volatile("" : "+v"(lo), "+v"(hi));
  typedef float f2c_t __attribute__((ext_vector_type(2)));
  h2_t r = __builtin_convertvector(f2c_t{lo, hi}, h2_t);
  return __builtin_bit_cast(uint32_t, r);
}

// (float)half_lo(w) * b and (float)half_hi(w) * b in one v_fma_mix_f32 each: the fp16 -> fp32
// widening rides on the multiply.  The addend is +0, which only differs from a plain product
// when the product is -0 (x = -0.0); every use below maps +-0 to the same table bucket.
__device__ __forceinline__ float mul_h_lo(uint32_t w, float b) {
  float d;
  asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(w), "v"(b));
  return d;
}
__device__ __forceinline__ float mul_h_hi(uint32_t w, float b) {
  float d;
  asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(w), "v"(b));
  return d;
}

// x - y * s with x an fp16 half of w (widened by the instruction), y and s fp32: the exact residual of the division
// step without a separate fp16 -> fp32 conversion of x
__device__ __forceinline__ float resid_h_lo(uint32_t w, float y, float s) {
  float d;
  asm("v_fma_mix_f32 %0, -%1, %2, %3 op_sel_hi:[0,0,1]" : "=v"(d) : "v"(y), "v"(s), "v"(w));
  return d;
}
__device__ __forceinline__ float resid_h_hi(uint32_t w, float y, float s) {
  float d;
  asm("v_fma_mix_f32 %0, -%1, %2, %3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(d) : "v"(y), "v"(s), "v"(w));
  return d;
}

// D = (float)half_lo(w) * b + c  /  (float)half_hi(w) * b + c (fp32 result)
__device__ __forceinline__ float fmaf_h_lo(uint32_t w, float b, float c) {
  float d;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(w), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ float fmaf_h_hi(uint32_t w, float b, float c) {
  float d;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(w), "v"(b), "v"(c));
  return d;
}

// xn = half(x / s) for the two halves of w, as far as any table can tell: y = fp32(x * inv), inv = RN32(1 / s), then ONE
// v_cvt_pk_f16_f32 for the pair.
//   * inv is the correctly rounded reciprocal (row_scale16: one Newton step on v_rcp_f32 leaves (1/s)(1 - 2^-44), and
//     2^k / b for an 11-bit b is further than that from every fp32 rounding boundary), the product is rounded once:
//     |y / (x/s) - 1| <= (1 + 2^-24)^2 - 1 = 2^-23 + 2^-48.
//   * What the quantizers take from xn is its bucket: the level only changes where half(x/s) crosses a rounding
//     threshold T of the table, i.e. where x/s crosses T moved by the half fp16 ulp of the rounding to fp16: a number
//     c / 2^p with a 12-bit ODD c (T itself has a few bits).  x = a 2^i and s = b 2^j with 11-bit a, b: x/s = c / 2^p would
//     need a = g c for g = gcd(a, b) - impossible, c > 2047 >= a - so |x/s - c/2^p| / (x/s) = |2^q a - b c| / (2^q a) is
//     at least 1 / (4096 * 2047) = 2^-22.9993.  2^-23 + 2^-48 < 2^-22.9993: y is on the same side of every such number
//     as x/s, so half(y) falls into the bucket of half(x/s) - it may be the neighbouring fp16 value INSIDE a bucket,
//     which no caller can observe (they all go xn -> bucket -> level).
//   * The margin is 0.05 %, so the argument is backed by exhaustion: tests/test_gpu_parity.py::
//     test_every_fp16_pair_fast_path_vs_ieee_path pushes all 1.0e9 (group maximum, element) pairs through this path and
//     through the IEEE division for seven table configurations, and ..._hw_levels the same pairs through the
//     hardware-level form of the producers.
// Round 2 carried 1/s as inv + inv_lo and rounded x * inv + x * inv_lo straight to fp16 (the exact quotient, 25 cycles of
// the vector pipe per pair: v_fma_mixlo/hi_f16 cost 8.2 each, tools/probe/valu_issue_cost.hip); this form: 13.
// (The two-term reciprocal measured 21.8 cycles per pair.)
__device__ __forceinline__ uint32_t div_pair16(uint32_t w, float ih0, float il0, float ih1, float il1) {
  (void)il0;
  (void)il1;
  return f2h2(mul_h_lo(w, ih0), mul_h_hi(w, ih1));
}

// the two table entries of a packed pair of bucket patterns as ONE packed register: byte offsets straight from the
// pattern (bucket * 2 == (pattern >> (shift - 1)) & mask), 16-bit loads into the low / high half
__device__ __forceinline__ uint32_t lut_pair16(const uint16_t* lut, uint32_t u, int shift) {
  const uint32_t mask = ((1u << (16 - shift)) - 1u) << 1;
  const uint32_t off0 = (u >> (shift - 1)) & mask, off1 = (u >> (15 + shift)) & mask;
  h2_t q;
  q.x = *(const _Float16*)((const char*)lut + off0);
  q.y = *(const _Float16*)((const char*)lut + off1);
  return __builtin_bit_cast(uint32_t, q);
}

// max over the LPR lanes that own a row; LPR lanes are contiguous and LPR-aligned
template <int LPR>
__device__ __forceinline__ uint32_t row_max_dpp(uint32_t v) {
  auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
  if (LPR >= 2) v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  if (LPR >= 4) v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  if (LPR >= 8) v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true));  // row_half_mirror
  if (LPR >= 16) v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true)); // row_mirror
  if (LPR >= 32) v = mx(v, (uint32_t)__shfl_xor((int)v, 16, 64));
  if (LPR >= 64) v = mx(v, (uint32_t)__shfl_xor((int)v, 32, 64));
  return v;
}

// fp16(a / g) for an fp16-valued a and a constant g given as inv_g = RN32(1/g):
// y = a*inv_g is within 2^-23 of a/g, one residual step makes it RN32(a/g(1+tiny)).
__device__ __forceinline__ uint32_t scale_bits_f16(uint32_t amax_bits, float g, float inv_g) {
  float a = h2f(amax_bits);
  if (!(a < __builtin_inff())) return amax_bits;   // inf -> inf, NaN -> NaN
  float y = a * inv_g;
  float e = __builtin_fmaf(-y, g, a);
  float y2 = __builtin_fmaf(e, inv_g, y);
  return f2h(y2);   // NaN/Inf propagate: amax = inf -> inf, NaN -> NaN
}

__device__ __forceinline__ void lut16_fill(uint16_t* lut, const Lut16Args& a) {
  const int n = 1 << (16 - a.shift);
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    uint32_t u = (uint32_t)i << a.shift;
    bool neg = (u >> 15) != 0;
    float r = h2f(u & 0x7FFFu);   // lowest magnitude pattern of the bucket
    float qm = quant_mag(r, 0u, neg ? a.fneg : a.fpos);
    uint32_t qb = f2h(qm);
    lut[i] = (uint16_t)((neg && qm != 0.0f) ? (qb | 0x8000u) : qb);
  }
}

// E2M1 levels from the FP4 conversion hardware instead of the bucket table:  level = f16_fp4(fp4_f32(float(xn) + 2^-14)).
// The reference's scan sends a tie to the LARGER value on both sides of zero (quant/quant_kernel.cu:25-37); the
// conversion rounds to nearest even.  fp16 values >= 0.25 are multiples of 2^-12 and every rounding boundary of E2M1 is a
// multiple of 0.25, so adding 2^-14 - exact in fp32 - removes every tie and sends it to the side the scan picks; below
// 0.25 nothing is a boundary.  tools/probe/cvt_fp4_probe.hip checks all 63 488 finite fp16 values against the scan on the
// hardware (profiles/r03_cvt_fp4_probe.txt), and the exhaustive (maximum, element) sweep of tests/test_gpu_parity.py runs
// through this path.  Levels that round to zero from below come back as -0: the dequantizing multiply is an fma with +0.
// Non-finite quotients (which saturate to 6 here, where the scan gives 0) only occur under a non-finite scale, and that
// is replaced by NaN (the reference's 0 * inf): scale_nan_if_not_finite.  No table, no LDS traffic.
__device__ __forceinline__ uint32_t e2m1_levels_hw(uint32_t xn2) {
  const float t0 = fmaf_h_lo(xn2, 1.0f, 0x1p-14f), t1 = fmaf_h_hi(xn2, 1.0f, 0x1p-14f);
  const uint32_t code = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(xn2, t0, t1, 1.0f, 0);   // byte 0 of a dead register
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(code, 1.0f, 0));
}
// ... and the hardware E2M1 CODES themselves (sign-magnitude nibbles, the operand format of the FP4 matrix cores,
// fpq_gemm_fp4.h): the two codes of a packed pair land in byte SEL of `acc`; four calls fill a register with the codes of
// 8 consecutive elements, low nibble first.  e2m1_codes_canon turns the -0 codes (negative values that round to zero)
// into +0, as the code table of the table-driven form has them (decode bit-equal to the fake-quantized values).
template <int SEL>
__device__ __forceinline__ uint32_t e2m1_codes_hw(uint32_t acc, uint32_t xn2) {
  const float t0 = fmaf_h_lo(xn2, 1.0f, 0x1p-14f), t1 = fmaf_h_hi(xn2, 1.0f, 0x1p-14f);
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(acc, t0, t1, 1.0f, SEL);
}
__device__ __forceinline__ uint32_t e2m1_codes_canon(uint32_t w) {
  const uint32_t t = (w & 0x77777777u) + 0x77777777u;   // bit 3 of a nibble: its magnitude is not zero (no carry between nibbles)
  return w & (t | 0x77777777u);
}
// the 8 codes of one 16-byte vector (cf. codes_vec16)
__device__ __forceinline__ uint32_t codes_vec16_hw(const u32x4& w, float inv) {
  uint32_t c = 0;
  c = e2m1_codes_hw<0>(c, div_pair16(w[0], inv, 0.f, inv, 0.f));
  c = e2m1_codes_hw<1>(c, div_pair16(w[1], inv, 0.f, inv, 0.f));
  c = e2m1_codes_hw<2>(c, div_pair16(w[2], inv, 0.f, inv, 0.f));
  c = e2m1_codes_hw<3>(c, div_pair16(w[3], inv, 0.f, inv, 0.f));
  return e2m1_codes_canon(c);
}
__device__ __forceinline__ uint32_t pk_fma0_f16(uint32_t a, uint32_t b) {   // a * b + (+0): a -0 product becomes +0
  const h2_t z = {(_Float16)0.0f, (_Float16)0.0f};
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_fma(__builtin_bit_cast(h2_t, a), __builtin_bit_cast(h2_t, b), z));
}
// FP6 levels without a table (round 4), for a lane that holds exactly 32 quotients (16 packed words): the FP6 conversion
// hardware takes two tuples of 16 floats, writes 32 six-bit codes (v_cvt_scalef32_2xpk16_{fp6,bf6}_f32: E2M3 / E3M2) and
// decodes them again (v_cvt_scalef32_pk32_f16_{fp6,bf6}).  It rounds to nearest-even; the reference's scan sends a tie to
// the LARGER value: float(xn) + 2^-17 - exact in fp32 for |xn| < 2^6, far below the distance of any fp16 value from a
// rounding threshold (thresholds are multiples of 2^-5 (E2M3) / 2^-6 (E3M2), fp16 values near them multiples of 2^-14 or
// coarser) - removes every tie towards the larger value and moves nothing else: tools/probe/cvt_fp6_probe.hip runs all
// 63 488 finite fp16 inputs through it against the scan (profiles/r03_cvt_fp6_probe.txt: 0 mismatches but -0 for inputs in
// (-step/2, 0), which the dequantizing fma with +0 repairs, as for E2M1).  Non-finite quotients saturate where the scan
// gives 0: they only occur under a non-finite scale, which scale_nan_if_not_finite turns into NaN (the reference's 0 * inf).
// ~2.2 pipe cycles per element each way (70 per instruction) + the bias: about the cost of the table lookups it
// replaces - what it buys is the staging of 2 KiB of table per workgroup, its barrier, and the LDS latency in every
// wavefront's short life (profiles/r04_pmc_token6.txt: the table form is not bound by vector issue, 39 % busy).
typedef uint32_t fp6_u16v_t __attribute__((ext_vector_type(16)));
typedef uint32_t fp6_u6v_t __attribute__((ext_vector_type(6)));
typedef float fp6_f16v_t __attribute__((ext_vector_type(16)));
// NW < 16: only the first NW packed words are live (a lane's fifth vector on rows of 17 - 20 groups: 8 values in a conversion
// of 32 - the instruction costs the same, but the table, its staging and its barrier still go).
template <bool BF6, int NW = 16>
__device__ __forceinline__ void fp6_levels_hw32(const uint32_t (&xn)[NW], uint32_t (&lv)[NW]) {
  // the two source tuples INTERLEAVE in the result: code 2 i comes from a[i], code 2 i + 1 from b[i] (seen on hardware with
  // distinct inputs - the probe's neighbouring patterns quantize alike and hid it): a = the low halves, b = the high halves
  fp6_f16v_t a, b;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < NW) {
      a[j] = fmaf_h_lo(xn[j], 1.0f, 0x1p-17f);
      b[j] = fmaf_h_hi(xn[j], 1.0f, 0x1p-17f);
    } else {
      a[j] = b[j] = 0.0f;
    }
  }
  fp6_u6v_t c;
  fp6_u16v_t d;
  if constexpr (BF6) {
    asm("v_cvt_scalef32_2xpk16_bf6_f32 %0, %1, %2, 1.0" : "=&v"(c) : "v"(a), "v"(b));   // early clobber: a multi-pass
    asm("v_cvt_scalef32_pk32_f16_bf6 %0, %1, 1.0" : "=&v"(d) : "v"(c));                  // instruction must not write over its sources
  } else {
    asm("v_cvt_scalef32_2xpk16_fp6_f32 %0, %1, %2, 1.0" : "=&v"(c) : "v"(a), "v"(b));
    asm("v_cvt_scalef32_pk32_f16_fp6 %0, %1, 1.0" : "=&v"(d) : "v"(c));
  }
#pragma unroll
  for (int j = 0; j < NW; ++j) lv[j] = d[j];
}

// Quantize the 8 halves of one 16-byte vector.  s16x2 = scale replicated in both halves; inv_hi + inv_lo = 1 / scale
// (0 for a zero scale).  In DUAL mode each element picks the negative or positive side's scale.
__device__ __forceinline__ uint32_t fbits16(float f) { return __builtin_bit_cast(uint32_t, f); }

template <bool DUAL, bool HW4 = false>
__device__ __forceinline__ u32x4 quant_vec16(const u32x4& w, const uint16_t* lut, int shift, float ih_n, float il_n,
                                             uint32_t s16x2_n, float ih_p, float il_p, uint32_t s16x2_p) {
  static_assert(!(DUAL && HW4), "hardware levels: the symmetric E2M1 table only");
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t wk = w[k];
    float h0 = ih_n, h1 = ih_n, l0 = il_n, l1 = il_n;
    uint32_t sc = s16x2_n;
    if (DUAL) {   // sign masks + v_bfi instead of compares and selects: 8 instructions per pair, not 12
      const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)wk, 15, 1), m1 = (uint32_t)((int)wk >> 31);   // all ones: negative
      h0 = u2f((fbits16(ih_n) & m0) | (fbits16(ih_p) & ~m0));  l0 = u2f((fbits16(il_n) & m0) | (fbits16(il_p) & ~m0));
      h1 = u2f((fbits16(ih_n) & m1) | (fbits16(ih_p) & ~m1));  l1 = u2f((fbits16(il_n) & m1) | (fbits16(il_p) & ~m1));
      const uint32_t mp = pk_ashr_i16(wk, 15);
      sc = (s16x2_n & mp) | (s16x2_p & ~mp);
    }
    const uint32_t rb = div_pair16(wk, h0, l0, h1, l1);
    if constexpr (HW4) {
      o[k] = pk_fma0_f16(e2m1_levels_hw(rb), sc);
    } else {
      const uint32_t u = pk_sub_u16(rb, pk_lshr_u16(rb, 15));   // negative patterns: magnitude - 1
      o[k] = pk_mul_f16(lut_pair16(lut, u, shift), sc);
    }
  }
  return o;
}

// Same normalisation and bucketing as quant_vec16, but the table holds 4-bit hardware codes (OCP E2M1
// nibbles, fpq_gemm_fp4.h): returns the 8 codes of the vector packed low nibble first.
__device__ __forceinline__ uint32_t codes_vec16(const u32x4& w, const uint16_t* lut, int shift, float inv_hi, float inv_lo) {
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t rb = div_pair16(w[k], inv_hi, inv_lo, inv_hi, inv_lo);
    const uint32_t u = pk_sub_u16(rb, pk_lshr_u16(rb, 15));
    const uint32_t c0 = lut[(u & 0xFFFFu) >> shift], c1 = lut[u >> (16 + shift)];
    packed |= (c0 | (c1 << 4)) << (8 * k);
  }
  return packed;
}

// |x| patterns of one vector reduced to a per-lane maximum (symmetric tables)
__device__ __forceinline__ uint32_t vec_absmax16(const u32x4& w) {
  uint32_t m = pk_max_u16(pk_max_u16(w[0] & 0x7FFF7FFFu, w[1] & 0x7FFF7FFFu),
                          pk_max_u16(w[2] & 0x7FFF7FFFu, w[3] & 0x7FFF7FFFu));
  uint32_t lo = m & 0xFFFFu, hi = m >> 16;
  return lo > hi ? lo : hi;
}

__device__ __forceinline__ uint32_t pk_min_f16(uint32_t a, uint32_t b) {
  uint32_t d;
  asm("v_pk_min_f16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ uint32_t pk_max_f16(uint32_t a, uint32_t b) {
  uint32_t d;
  asm("v_pk_max_f16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
// torch.clamp(x, -c, c) on a packed pair; c2 = the bound in both halves (c >= 0, not NaN).  v_pk_min / max return the
// other operand for a NaN input, torch keeps the NaN: `keep_nan` restores it (only on the rare path that saw a NaN).
__device__ __forceinline__ uint32_t pk_clamp_f16(uint32_t w, uint32_t c2, bool keep_nan) {
  const uint32_t r = pk_min_f16(pk_max_f16(w, c2 ^ 0x80008000u), c2);
  if (!keep_nan) return r;
  const uint32_t nanm = pk_ashr_i16(pk_sub_u16(0x7C007C00u, w & 0x7FFF7FFFu), 15);   // 0xFFFF where the half is a NaN
  return (r & ~nanm) | (w & nanm);
}

// dual format: max|x| over x <= 0 and over x > 0 separately; NaN belongs to neither
__device__ __forceinline__ uint32_t vec_absmax16_dual(const u32x4& w, uint32_t& mneg, uint32_t& mpos) {
  uint32_t mn = 0, mp = 0, any_nan = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t a = w[k] & 0x7FFF7FFFu;
    uint32_t nanm = pk_ashr_i16(pk_sub_u16(0x7C007C00u, a), 15);   // 0xFFFF where a > 0x7C00
    a &= ~nanm;
    any_nan |= nanm;
    uint32_t sm = pk_ashr_i16(w[k], 15);                            // 0xFFFF where the sign bit is set
    mn = pk_max_u16(mn, a & sm);
    mp = pk_max_u16(mp, a & ~sm);
  }
  uint32_t lo = mn & 0xFFFFu, hi = mn >> 16;
  mneg = lo > hi ? lo : hi;
  lo = mp & 0xFFFFu; hi = mp >> 16;
  mpos = lo > hi ? lo : hi;
  return any_nan;
}

// The same two maxima at two instructions per packed pair instead of ten, for inputs without NaN: as UNSIGNED 16-bit
// integers every negative value beats every positive one and grows with its magnitude, as SIGNED integers every negative
// value loses against +0 - so `un` = unsigned maximum and `sp` = signed maximum of the raw patterns carry max|x| over
// x < 0 and over x > 0.  A NaN (|pattern| > 0x7C00) rides along as the largest value of its side: callers test the
// reduced maxima for > 0x7C00 and, wavefront-uniformly, redo the row with vec_absmax16_dual (rare).
__device__ __forceinline__ void dual_max_acc(const u32x4& w, uint32_t& un, uint32_t& sp) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    un = pk_max_u16(un, w[k]);
    sp = pk_max_i16(sp, w[k]);
  }
}
__device__ __forceinline__ void dual_max_finish(uint32_t un, uint32_t sp, uint32_t& mneg, uint32_t& mpos) {
  const uint32_t ul = un & 0xFFFFu, uh = un >> 16;
  const uint32_t u = ul > uh ? ul : uh;
  mneg = (u & 0x8000u) ? (u & 0x7FFFu) : 0u;
  const int sl = (int)(sp << 16) >> 16, sh = (int)sp >> 16;
  const int sm = sl > sh ? sl : sh;
  mpos = sm > 0 ? (uint32_t)sm : 0u;
}
__device__ __forceinline__ bool dual_max_has_nan(uint32_t mneg, uint32_t mpos) {
  return __builtin_amdgcn_ballot_w64(mneg > 0x7C00u || mpos > 0x7C00u) != 0;
}

struct RowScale16 {
  float sf;         // (float)scale
  float inv;        // 1 / scale = inv + inv_lo, inv = the fp32 nearest (one Newton step on v_rcp_f32), inv_lo the rest;
  float inv_lo;     // both 0 for a zero scale: x / 0 -> level 0 -> +0
  uint32_t s16x2;
};

__device__ __forceinline__ RowScale16 row_scale16(uint32_t amax_bits, float g, float inv_g) {
  RowScale16 r;
  uint32_t sb = scale_bits_f16(amax_bits, g, inv_g);
  r.sf = h2f(sb);
  const float r0 = __builtin_amdgcn_rcpf(r.sf);
  const float r1 = __builtin_fmaf(__builtin_fmaf(-r.sf, r0, 1.0f), r0, r0);
  const float lo = __builtin_fmaf(-r.sf, r1, 1.0f) * r1;          // 1/s - r1, to ~2^-46
  const bool zero = r.sf == 0.0f;
  r.inv = zero ? 0.0f : r1;
  r.inv_lo = zero ? 0.0f : lo;
  r.s16x2 = sb | (sb << 16);
  return r;
}

__device__ __forceinline__ void scale_nan_if_not_finite(RowScale16& s) {
  if (!(s.sf < __builtin_inff())) s.s16x2 = 0x7E007E00u;
}

// dual format: a non-finite scale on either side poisons the whole row (0 * inf = NaN
// is added to every element by the reference's `q_neg*s_neg + q_pos*s_pos`)
__device__ __forceinline__ void dual_poison(RowScale16& n, RowScale16& p) {
  bool bad = !(fabsf(n.sf) < __builtin_inff()) || !(fabsf(p.sf) < __builtin_inff());
  if (bad) {
    n.sf = p.sf = __builtin_nanf("");
    n.s16x2 = p.s16x2 = 0x7E007E00u;
  }
}

// The bucket -> level table, prebuilt on the host (immutable, cached per table pair) and handed over BY VALUE in
// the kernel arguments: no device-side global state, and a workgroup pays a few 2-byte stores per lane instead of
// evaluating the closed form.  Kernel arguments are limited to 4 KiB, the widest table (int_neg / e2m3_pos, buckets
// of 32 patterns) has 2 x 1024 entries - but every table is constant beyond its largest rounding boundary (the
// largest level, for every finite pattern up to the reach limit) and zero for the inf / NaN patterns, so only the
// prefix of each sign half travels: <= 1216 entries for the widest pair.
constexpr int kLutArgEntries = 1280;
struct Lut16Tab {
  uint16_t e[kLutArgEntries];   // positive-half prefix, then negative-half prefix
  uint16_t n_pos, n_neg;        // prefix lengths (buckets)
  uint16_t fill_pos, fill_neg;  // every finite bucket beyond the prefix
};

// expand the by-value table into the workgroup's LDS image [positive half | negative half]
__device__ __forceinline__ void lut16_stage(uint16_t* lut, const Lut16Tab& tab, int shift) {
  const int nh = 1 << (15 - shift), nan0 = 0x7C00 >> shift;
  if (tab.n_pos == 0xFFFFu) {   // small table, stored whole: one plain copy (the common case, kept as cheap as it was)
    for (int i = threadIdx.x; i < 2 * nh; i += blockDim.x) lut[i] = tab.e[i];
    return;
  }
  for (int i = threadIdx.x; i < 2 * nh; i += blockDim.x) {
    const bool neg = i >= nh;
    const int j = neg ? i - nh : i;
    const int np = neg ? tab.n_neg : tab.n_pos, base = neg ? tab.n_pos : 0;
    const uint16_t fill = neg ? tab.fill_neg : tab.fill_pos;
    lut[i] = j < np ? tab.e[base + j] : (j < nan0 ? fill : (uint16_t)0);
  }
}

// host: compress a full image (2^(16-shift) entries); false when it does not have the constant-tail structure or
// the prefixes do not fit
inline bool lut16_compress(const uint16_t* full, int shift, Lut16Tab* out) {
  const int nh = 1 << (15 - shift), nan0 = 0x7C00 >> shift;
  if (2 * nh <= kLutArgEntries) {   // fits whole
    for (int i = 0; i < kLutArgEntries; ++i) out->e[i] = i < 2 * nh ? full[i] : 0;
    out->n_pos = out->n_neg = 0xFFFFu;
    out->fill_pos = out->fill_neg = 0;
    return true;
  }
  int np[2];
  uint16_t fill[2];
  for (int half = 0; half < 2; ++half) {
    const uint16_t* f = full + half * nh;
    for (int j = nan0; j < nh; ++j)
      if (f[j] != 0) return false;
    fill[half] = f[nan0 - 1];
    int n = nan0;
    while (n > 0 && f[n - 1] == fill[half]) --n;
    np[half] = n;
  }
  if (np[0] + np[1] > kLutArgEntries) return false;
  for (int i = 0; i < kLutArgEntries; ++i) out->e[i] = 0;
  for (int j = 0; j < np[0]; ++j) out->e[j] = full[j];
  for (int j = 0; j < np[1]; ++j) out->e[np[0] + j] = full[nh + j];
  out->n_pos = (uint16_t)np[0];
  out->n_neg = (uint16_t)np[1];
  out->fill_pos = fill[0];
  out->fill_neg = fill[1];
  return true;
}

inline void lut16_build_host(uint16_t* lut, const Lut16Args& a) {
  const int n = 1 << (16 - a.shift);
  for (int i = 0; i < n; ++i) {
    uint32_t u = (uint32_t)i << a.shift;
    bool neg = (u >> 15) != 0;
    float r = h2f(u & 0x7FFFu);
    float qm = quant_mag(r, 0u, neg ? a.fneg : a.fpos);
    uint32_t qb = f2h(qm);
    lut[i] = (uint16_t)((neg && qm != 0.0f) ? (qb | 0x8000u) : qb);
  }
}

// ---------------------------------------------------------------------------------
// GELU(tanh) of an fp16 tensor as torch computes it (fp32 arithmetic, one rounding to fp16): the FFN's activation between
// fc1 and fc2's input quantizer (tr/basic_var.py:120), fused into the fc1 GEMM's epilogue (fpq_gemm_fp4.h, GemmFc1) and into
// the stand-alone dual quantizer (rows16_lut_subwave_kernel<..., GELU>).
// torch: aten/src/ATen/native/cuda/ActivationGeluKernel.cu, GeluCUDAKernelImpl, approximate == tanh (opmath = float):
//   kBeta = M_SQRT2 * M_2_SQRTPI * 0.5, kKappa = 0.044715; x_cube = x * x * x; inner = kBeta * (x + kKappa * x_cube);
//   0.5 * x * (1 + tanh(inner))
// The form the epilogue runs (9 vector instructions instead of ~30): gelu(x) = x w, w = (1 + tanh(u)) / 2 = 1 / (1 + 2^m),
// m = -2 log2(e) u = x (c0 + c1 x^2); `(w - 0.5) + 0.5` snaps w to the grid torch's own 1 + tanh(u) lives on (its tanh is an
// fp32 number just below 1 for the deep negatives, where 1 + tanh cancels).  The snap buys parity with torch, not accuracy: without
// it the result is the correctly rounded fp16 of the float64 definition wherever fp32 can decide; with it 272 inputs miss that value
// (269 with x < 0), by up to 1.70 fp16 ulps at x = -5.15625 - as torch's own chain does (profiles/gelu_float64.txt).  Contract, on all
// 65536 inputs and in every kernel this is compiled into (tests/test_gpu_gelu.py): within tests/gelu_model.py's bound of the float64
// definition, and within one fp16 ulp of torch on the GPU (5 inputs differ, by one ulp; profiles/r05_gelu_probe.txt); NaN at NaN, -inf.
__device__ __forceinline__ float gelu_tanh_fast(float x) {
  const float kBeta = (float)(1.41421356237309504880 * 1.12837916709551257390 * 0.5), kKappa = 0.044715f;
  const float c0 = -2.8853900817779268f * kBeta, c1 = c0 * kKappa;   // float arithmetic, as in the probe
  const float m = x * __builtin_fmaf(x * x, c1, c0);
  const float w = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(m));
  return x * ((w - 0.5f) + 0.5f);
}

// ---------------------------------------------------------------------------------
// rows of 1..64 lanes x 16 bytes inside one wavefront (per-group 128, KV c=64, ...).
// A workgroup owns TILE = 256*U consecutive vectors (U*4 KiB, contiguous in HBM);
// workgroups are dispatched in address order, so the chip sweeps the tensor front
// to back.  All U loads are issued before the table is staged and the barrier.
// ---------------------------------------------------------------------------------
// HW4: E2M1 levels from the conversion hardware (above) - no table, no LDS, no barrier.
// CLIP (dual format per group): the reference's global clamp to +-strength * max|x| in front of the quantizer, the
// maximum read from a device scalar (fpq_absmax) - two packed instructions per pair on the fast path instead of the
// generic kernel (0.23 -> of 8 TB/s, profiles/r03_survey_shapes.txt).  Group maxima are taken on the raw words (a NaN
// is still seen) and clamped afterwards (clamping is monotonic).
// HW6 (1: E2M3, 2: E3M2; U = 4: a lane's four vectors are the 32 values of one FP6 conversion, each with the scale of its own
// row): levels from the FP6 conversion hardware (fp6_levels_hw32) - no table, no LDS, no barrier.
// GELU (dual format per group; round 5): x is the fc1 OUTPUT - every element goes through GELU(tanh) (gelu_tanh_fast above: fp32, one
// rounding to fp16, within one fp16 ulp of torch's on every input) before the quantizer sees it: `fc2.act_quant(act(y))` of the
// reference's FFN (tr/basic_var.py:120-121, tr/quant_utils.py:991) in one pass over y instead of two.
template <int LPR, bool DUAL, int U, bool TAB_ARG, bool NTL = true, bool NTS = true, bool HW4 = false, bool CLIP = false, int HW6 = 0,
          bool GELU = false>
__global__ __launch_bounds__(kBlock) void rows16_lut_subwave_kernel(const u32x4* __restrict__ x,
                                                                   u32x4* __restrict__ out, int64_t n_vec,
                                                                   Lut16Args a, Lut16Tab tab) {
  static_assert(HW6 == 0 || (U == 4 && !DUAL && !HW4 && !CLIP), "hardware FP6 levels: symmetric tables, four vectors per lane");
  uint16_t* lut = nullptr;
  if constexpr (!HW4 && HW6 == 0) {
    __shared__ __attribute__((aligned(16))) uint16_t lut_s[kLutLdsEntries];   // static: a compile-time LDS address (a dynamic base is not folded into the ds_read offsets)
    lut = lut_s;
  }
  static_assert(!CLIP || DUAL, "the global clamp belongs to the dual format");
  const int64_t tiles = (n_vec + (int64_t)kBlock * U - 1) / ((int64_t)kBlock * U);
  uint32_t clip2 = 0;
  bool clip_nan = false;
  if constexpr (CLIP) {   // c = half(strength * max|x|), as the reference's fp16 multiply
    const uint32_t cb = f2h(a.clip_strength * h2f(*(const uint16_t*)a.clip_absmax));
    clip_nan = (cb & 0x7FFFu) > 0x7C00u;   // a NaN in the tensor: clamp(x, NaN, NaN) is NaN everywhere -> every output +0
    clip2 = cb | (cb << 16);
  }
  bool first = true;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t v0 = tile * ((int64_t)kBlock * U) + threadIdx.x;
    u32x4 raw[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int64_t v = v0 + u * kBlock;
      live[u] = v < n_vec;
      raw[u] = live[u] ? (NTL ? __builtin_nontemporal_load(x + v) : x[v]) : u32x4{0, 0, 0, 0};
    }
    if constexpr (GELU) {
      static_assert(DUAL && !CLIP && HW6 == 0, "the fused activation belongs to fc2's dual-format input quantizer");
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) raw[u][k] = f2h2(gelu_tanh_fast(h2f(raw[u][k] & 0xFFFFu)), gelu_tanh_fast(h2f(raw[u][k] >> 16)));
        if (a.gelu_out && live[u]) __builtin_nontemporal_store(raw[u], (u32x4*)a.gelu_out + v0 + u * kBlock);
      }
    }
    if constexpr (HW6 != 0) {
      uint32_t q6[16], lv6[16], sc6[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t m = row_max_dpp<LPR>(vec_absmax16(raw[u]));
        RowScale16 s = row_scale16(m, a.fpos.gmax, a.inv_gpos);
        scale_nan_if_not_finite(s);
        sc6[u] = s.s16x2;
#pragma unroll
        for (int k = 0; k < 4; ++k) q6[4 * u + k] = div_pair16(raw[u][k], s.inv, s.inv_lo, s.inv, s.inv_lo);
      }
      fp6_levels_hw32<HW6 == 2>(q6, lv6);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const u32x4 o = {pk_fma0_f16(lv6[4 * u], sc6[u]), pk_fma0_f16(lv6[4 * u + 1], sc6[u]), pk_fma0_f16(lv6[4 * u + 2], sc6[u]),
                         pk_fma0_f16(lv6[4 * u + 3], sc6[u])};
        if (live[u]) {
          if (NTS) __builtin_nontemporal_store(o, out + v0 + u * kBlock);
          else out[v0 + u * kBlock] = o;
        }
      }
      continue;
    }
    if (first && !HW4) {
      if (TAB_ARG) {
        lut16_stage(lut, tab, a.shift);
      } else {
        lut16_fill(lut, a);
      }
      __syncthreads();
      first = false;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      u32x4 o;
      if constexpr (DUAL) {
        uint32_t un = 0, sg = 0, mn, mp;
        dual_max_acc(raw[u], un, sg);
        dual_max_finish(un, sg, mn, mp);
        mn = row_max_dpp<LPR>(mn);
        mp = row_max_dpp<LPR>(mp);
        u32x4 xw = raw[u];
        const bool has_nan = dual_max_has_nan(mn, mp);
        if constexpr (CLIP) {
          const uint32_t cb = clip2 & 0xFFFFu;
          mn = mn < cb ? mn : cb;
          mp = mp < cb ? mp : cb;
#pragma unroll
          for (int k = 0; k < 4; ++k) xw[k] = pk_clamp_f16(xw[k], clip2, has_nan);
        }
        if (__builtin_expect(has_nan, 0)) {   // a NaN somewhere in the wavefront's vectors: the exact rule
          if (vec_absmax16_dual(xw, mn, mp) && a.nan_flag) atomicOr(a.nan_flag, 1u);
          mn = row_max_dpp<LPR>(mn);
          mp = row_max_dpp<LPR>(mp);
        }
        RowScale16 sn = row_scale16(mn, a.fneg.gmax, a.inv_gneg), sp = row_scale16(mp, a.fpos.gmax, a.inv_gpos);
        dual_poison(sn, sp);
        o = quant_vec16<true>(xw, lut, a.shift, sn.inv, sn.inv_lo, sn.s16x2, sp.inv, sp.inv_lo, sp.s16x2);
        if (CLIP && clip_nan) o = u32x4{0, 0, 0, 0};
      } else {
        uint32_t m = row_max_dpp<LPR>(vec_absmax16(raw[u]));
        RowScale16 s = row_scale16(m, a.fpos.gmax, a.inv_gpos);
        if constexpr (HW4) scale_nan_if_not_finite(s);
        o = quant_vec16<false, HW4>(raw[u], lut, a.shift, s.inv, s.inv_lo, s.s16x2, 0.f, 0.f, 0u);
      }
      if (live[u]) {
        if (NTS) __builtin_nontemporal_store(o, out + v0 + u * kBlock);
        else out[v0 + u * kBlock] = o;
      }
    }
  }
}

// Several fp16 tensors, ONE launch (fpq_quant_rows_multi): the same rows as rows16_lut_subwave_kernel, the tensors'
// descriptors travel by value in the kernel arguments (no device-side table, no copy), blockIdx.y selects the tensor,
// workgroups beyond a shorter tensor's end exit at once.  For the places where the reference quantizes independent
// tensors back to back - the cached K and V of a step (tr/basic_var.py:192-200), the samples of a format search.
constexpr int kMaxMulti = 8;
struct Multi16 {
  const u32x4* x[kMaxMulti];
  u32x4* out[kMaxMulti];
  int64_t n_vec[kMaxMulti];
};

template <int LPR, int U>
__global__ __launch_bounds__(kBlock) void rows16_lut_multi_kernel(Multi16 m, Lut16Args a, Lut16Tab tab) {
  __shared__ __attribute__((aligned(16))) uint16_t lut[kLutLdsEntries];
  const int64_t n_vec = m.n_vec[blockIdx.y];
  const int64_t v0 = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
  if ((int64_t)blockIdx.x * (kBlock * U) >= n_vec) return;
  const u32x4* __restrict__ x = m.x[blockIdx.y];
  u32x4* __restrict__ out = m.out[blockIdx.y];
  u32x4 raw[U];
  bool live[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t v = v0 + u * kBlock;
    live[u] = v < n_vec;
    raw[u] = live[u] ? __builtin_nontemporal_load(x + v) : u32x4{0, 0, 0, 0};
  }
  lut16_stage(lut, tab, a.shift);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t mx = row_max_dpp<LPR>(vec_absmax16(raw[u]));
    const RowScale16 s = row_scale16(mx, a.fpos.gmax, a.inv_gpos);
    const u32x4 o = quant_vec16<false>(raw[u], lut, a.shift, s.inv, s.inv_lo, s.s16x2, 0.f, 0.f, 0u);
    if (live[u]) __builtin_nontemporal_store(o, out + v0 + u * kBlock);
  }
}

// ---------------------------------------------------------------------------------
// KV-cache step (the reference's tr/basic_var.py:186-209): ONE launch
//   (a) quantizes, in place, the cache entries the previous step appended (their first - and, the quantizer being
//       idempotent on its own output, only - quantization), rows of 8 * LPR halves, and
//   (b) copies the new k / v rows (any batch / token pitch, e.g. views of the fused qkv output) behind them.
// The cache is fp16 [2 (k, v), batch, max_len, row_elems]; blockIdx.z = k / v, blockIdx.y = batch entry,
// blockIdx.x < q_tiles: job (a), else job (b).  Every branch is uniform over the workgroup.
// ---------------------------------------------------------------------------------
struct KvStepArgs {
  u32x4* cache;
  int64_t slab_vec;        // 16-byte vectors per (k|v, batch entry) slab = max_len * row_vec
  int row_vec;             // vectors per token row
  int batch;
  int64_t q_first_vec;     // first vector of the rows to quantize (inside a slab)
  int64_t q_vecs;
  int q_tiles;
  const uint16_t* src[2];  // new k, new v: [batch, n_new, row_elems], rows contiguous
  int64_t src_batch_pitch, src_token_pitch;   // in elements
  int64_t new_first_vec;
  int64_t new_vecs;
};

// job (a) of kv16_step_qkn_kernel (kv16_step_kernel's own, spelled out there): this workgroup's share of the previous step's rows
// of one slab, quantized in place
template <int LPR, int U>
__device__ __forceinline__ void kv16_quant_job(u32x4* slab, const KvStepArgs& k, const Lut16Args& a, const Lut16Tab& tab, uint16_t* lut) {
  u32x4* p = slab + k.q_first_vec;
  const int64_t v0 = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
  u32x4 raw[U];
  bool live[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t v = v0 + u * kBlock;
    live[u] = v < k.q_vecs;     // q_vecs is a multiple of LPR: a row is live or dead as a whole
    raw[u] = live[u] ? p[v] : u32x4{0, 0, 0, 0};
  }
  {
    lut16_stage(lut, tab, a.shift);
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t m = row_max_dpp<LPR>(vec_absmax16(raw[u]));
    const RowScale16 s = row_scale16(m, a.fpos.gmax, a.inv_gpos);
    const u32x4 o = quant_vec16<false>(raw[u], lut, a.shift, s.inv, s.inv_lo, s.s16x2, 0.f, 0.f, 0u);
    if (live[u]) p[v0 + u * kBlock] = o;
  }
}

template <int LPR, int U>
__global__ __launch_bounds__(kBlock) void kv16_step_kernel(KvStepArgs k, Lut16Args a, Lut16Tab tab) {
  __shared__ __attribute__((aligned(16))) uint16_t lut[kLutLdsEntries];   // static: a compile-time LDS address (a dynamic base is not folded into the ds_read offsets)
  const int kv = blockIdx.z, b = blockIdx.y;
  u32x4* slab = k.cache + ((int64_t)kv * k.batch + b) * k.slab_vec;
  if ((int)blockIdx.x < k.q_tiles) {
    u32x4* p = slab + k.q_first_vec;
    const int64_t v0 = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
    u32x4 raw[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = v0 + u * kBlock;
      live[u] = v < k.q_vecs;     // q_vecs is a multiple of LPR: a row is live or dead as a whole
      raw[u] = live[u] ? p[v] : u32x4{0, 0, 0, 0};
    }
    {
      lut16_stage(lut, tab, a.shift);
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t m = row_max_dpp<LPR>(vec_absmax16(raw[u]));
      const RowScale16 s = row_scale16(m, a.fpos.gmax, a.inv_gpos);
      const u32x4 o = quant_vec16<false>(raw[u], lut, a.shift, s.inv, s.inv_lo, s.s16x2, 0.f, 0.f, 0u);
      if (live[u]) p[v0 + u * kBlock] = o;
    }
  } else {
    const uint16_t* s = k.src[kv] + (int64_t)b * k.src_batch_pitch;
    u32x4* d = slab + k.new_first_vec;
    const int64_t v0 = (int64_t)((int)blockIdx.x - k.q_tiles) * (kBlock * U) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = v0 + u * kBlock;
      if (v < k.new_vecs) {
        const int64_t l = v / k.row_vec;
        const int c = (int)(v - l * k.row_vec);
        d[v] = *(const u32x4*)(s + l * k.src_token_pitch + c * 8);
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// KV-cache step of an attention block with attn_l2_norm (tr/basic_var.py:173-183; include/fpq.h fpq_kv_cache_step_qknorm):
// kv16_step_kernel's two jobs, the copy-in now
//     y = float(x16) + b32                        (the fp32 bias cat(q_bias, 0, v_bias) promotes the fp16 Linear output)
//     k = half(y / max(||y||_2, 1e-12))           per (token, head) over the head's 64 channels: F.normalize(k, dim=-1)
//     v = half(y)
// and a third job (blockIdx.z == 2) that writes q_out = half(y / max(||y||_2, 1e-12) * s_h), contiguous [batch, n, row_elems]:
// the whole qkv-to-cache work of a block-step in one launch.  Lanes: consecutive threads own consecutive 16-byte vectors of a
// token row, so the 64 channels of a head are the 8 vectors of 8 adjacent, 8-aligned lanes (kBlock and row_vec are multiples
// of 8) - the sum of squares is three DPP steps, every lane of the head ends with the same bits.  A lane past the end reads
// zeros: a head is live or dead as a whole (new_vecs is a multiple of row_vec).  The norm: a real square root, one real
// division per head (1 / n), and per element q = y * (1/n) with one residual step, q + (y - q n) (1/n) - the correctly
// rounded quotient but for rare ties, at three instructions instead of a division each.
// ---------------------------------------------------------------------------------
struct KvStepQkn {
  const uint16_t* q;       // new q: the pitches of new k
  u32x4* q_out;            // [batch, n_new, row_vec] vectors
  const float* q_scale;    // [row_elems / 64]: exp(min(scale_mul_1H11, log 100))
  const float* bias;       // [3 * row_elems] (q, k, v) or nullptr
  int row_elems;
};

// sum over the 8 lanes of an 8-aligned lane group (the same bits in every lane: each step adds a value and its mirror image)
__device__ __forceinline__ float head_sum8(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
  return v;
}

template <int LPR, int U>
__global__ __launch_bounds__(kBlock) void kv16_step_qkn_kernel(KvStepArgs k, KvStepQkn qn, Lut16Args a, Lut16Tab tab) {
  __shared__ __attribute__((aligned(16))) uint16_t lut[kLutLdsEntries];
  const int z = blockIdx.z, b = blockIdx.y;   // z: 0 k, 1 v (cache slabs), 2 q
  if ((int)blockIdx.x < k.q_tiles) {
    if (z == 2) return;
    kv16_quant_job<LPR, U>(k.cache + ((int64_t)z * k.batch + b) * k.slab_vec, k, a, tab, lut);
    return;
  }
  const uint16_t* s = (z == 2 ? qn.q : k.src[z]) + (int64_t)b * k.src_batch_pitch;
  u32x4* d = z == 2 ? qn.q_out + (int64_t)b * k.new_vecs : k.cache + ((int64_t)z * k.batch + b) * k.slab_vec + k.new_first_vec;
  const float* bias = qn.bias ? qn.bias + (int64_t)(z == 2 ? 0 : z + 1) * qn.row_elems : nullptr;   // bias order: q, k, v
  const int64_t v0 = (int64_t)((int)blockIdx.x - k.q_tiles) * (kBlock * U) + threadIdx.x;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t v = v0 + u * kBlock;
    const bool live = v < k.new_vecs;
    const int64_t l = live ? v / k.row_vec : 0;
    const int c = live ? (int)(v - l * k.row_vec) : 0;
    const u32x4 raw = live ? *(const u32x4*)(s + l * k.src_token_pitch + c * 8) : u32x4{0, 0, 0, 0};
    float y[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      y[2 * j] = h2f(raw[j] & 0xFFFFu);
      y[2 * j + 1] = h2f(raw[j] >> 16);
    }
    if (bias) {
      typedef float f4_t __attribute__((ext_vector_type(4)));
      const f4_t b0 = *(const f4_t*)(bias + c * 8), b1 = *(const f4_t*)(bias + c * 8 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        y[j] += b0[j];
        y[4 + j] += b1[j];
      }
    }
    if (z != 1) {   // uniform
      float ss = y[0] * y[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) ss = __builtin_fmaf(y[j], y[j], ss);
      ss = head_sum8(ss);
      float nrm = __builtin_sqrtf(ss);
      nrm = nrm < 1e-12f ? 1e-12f : nrm;   // clamp_min(eps) (a NaN stays a NaN)
      const float inv = 1.0f / nrm;
      const float nrm_r = nrm < __builtin_inff() ? nrm : 0.0f;   // inf / NaN norm: the residual step adds y * 0
      const float hs = z == 2 ? qn.q_scale[c >> 3] : 1.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float q = y[j] * inv;
        q = __builtin_fmaf(__builtin_fmaf(-q, nrm_r, y[j]), inv, q);
        y[j] = z == 2 ? q * hs : q;
      }
    }
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = f2h2(y[2 * j], y[2 * j + 1]);
    if (live) d[v] = o;
  }
}

// Same rows, but LPR lanes own a row of 2*LPR vectors (two 16-byte vectors per lane, LPR*16 bytes
// apart): the per-row work - cross-lane max, scale, reciprocal - is paid once per 16 elements of a
// lane instead of once per 8.  Every load / store instruction still touches whole 128-byte lines
// (LPR = 8: eight lanes x 16 B).  Used for the 128-element groups.
template <int LPR, bool DUAL, bool TAB_ARG>
__global__ __launch_bounds__(kBlock) void rows16_lut_pair_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ out,
                                                                int64_t n_vec, Lut16Args a, Lut16Tab tab) {
  __shared__ __attribute__((aligned(16))) uint16_t lut[kLutLdsEntries];   // static: a compile-time LDS address (a dynamic base is not folded into the ds_read offsets)
  constexpr int64_t kTile = (int64_t)kBlock * 2;
  const int64_t tiles = (n_vec + kTile - 1) / kTile;
  const int in_row = threadIdx.x % LPR, row_in_tile = threadIdx.x / LPR;
  bool first = true;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t va = tile * kTile + (int64_t)row_in_tile * (2 * LPR) + in_row;
    const int64_t vb = va + LPR;
    const bool live = va < n_vec;   // n_vec is a multiple of 2*LPR: both vectors live or both dead
    u32x4 ra = live ? __builtin_nontemporal_load(x + va) : u32x4{0, 0, 0, 0};
    u32x4 rb = live ? __builtin_nontemporal_load(x + vb) : u32x4{0, 0, 0, 0};
    if (first) {
      if (TAB_ARG) {
        lut16_stage(lut, tab, a.shift);
      } else {
        lut16_fill(lut, a);
      }
      __syncthreads();
      first = false;
    }
    u32x4 oa, ob;
    if (DUAL) {
      uint32_t un = 0, sg = 0, mn, mp;
      dual_max_acc(ra, un, sg);
      dual_max_acc(rb, un, sg);
      dual_max_finish(un, sg, mn, mp);
      mn = row_max_dpp<LPR>(mn);
      mp = row_max_dpp<LPR>(mp);
      if (__builtin_expect(dual_max_has_nan(mn, mp), 0)) {   // the exact rule (NaN belongs to neither side)
        uint32_t mn2, mp2;
        const uint32_t nan_any = vec_absmax16_dual(ra, mn, mp) | vec_absmax16_dual(rb, mn2, mp2);
        if (nan_any && a.nan_flag) atomicOr(a.nan_flag, 1u);
        mn = row_max_dpp<LPR>(mn > mn2 ? mn : mn2);
        mp = row_max_dpp<LPR>(mp > mp2 ? mp : mp2);
      }
      RowScale16 sn = row_scale16(mn, a.fneg.gmax, a.inv_gneg), sp = row_scale16(mp, a.fpos.gmax, a.inv_gpos);
      dual_poison(sn, sp);
      oa = quant_vec16<true>(ra, lut, a.shift, sn.inv, sn.inv_lo, sn.s16x2, sp.inv, sp.inv_lo, sp.s16x2);
      ob = quant_vec16<true>(rb, lut, a.shift, sn.inv, sn.inv_lo, sn.s16x2, sp.inv, sp.inv_lo, sp.s16x2);
    } else {
      const uint32_t m1 = vec_absmax16(ra), m2 = vec_absmax16(rb);
      const uint32_t m = row_max_dpp<LPR>(m1 > m2 ? m1 : m2);
      RowScale16 s = row_scale16(m, a.fpos.gmax, a.inv_gpos);
      oa = quant_vec16<false>(ra, lut, a.shift, s.inv, s.inv_lo, s.s16x2, 0.f, 0.f, 0u);
      ob = quant_vec16<false>(rb, lut, a.shift, s.inv, s.inv_lo, s.s16x2, 0.f, 0.f, 0u);
    }
    if (live) {
      __builtin_nontemporal_store(oa, out + va);
      __builtin_nontemporal_store(ob, out + vb);
    }
  }
}

// ---------------------------------------------------------------------------------
// long fp16 rows (per-token 1920 / 7680 / 2304 / 9216, per-channel weights in fp16):
// one workgroup walks a contiguous run of rows; a row's vectors stay in registers
// (<= MAXC per lane) between the max reduction (DPP + LDS) and the rounding.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_max16(uint32_t v, uint32_t* sh) {
  v = row_max_dpp<64>(v);
  __syncthreads();   // sh may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t r = sh[0];
#pragma unroll
  for (int i = 1; i < kBlock / 64; ++i) r = r > sh[i] ? r : sh[i];
  return r;
}

// GELU: as in rows16_lut_subwave_kernel - x is the fc1 output, every element goes through GELU(tanh) first (the W6A6 run's
// `fc2.act_quant(act(y))` with the per-token INT-/E2M3+ quantizer, tr/quant_utils.py:614-646 bound at :930-931).
template <bool DUAL, int MAXC, bool TAB_ARG, bool GELU = false>
__global__ __launch_bounds__(kBlock) void rows16_lut_block_kernel(const uint16_t* __restrict__ x,
                                                                 uint16_t* __restrict__ out, int64_t rows,
                                                                 int64_t cols, int64_t rows_per_block, Lut16Args a,
                                                                 Lut16Tab tab) {
  __shared__ __attribute__((aligned(16))) uint16_t lut[kLutLdsEntries];   // static: a compile-time LDS address (a dynamic base is not folded into the ds_read offsets)
  __shared__ uint32_t sh[kBlock / 64];
  const int64_t vec_per_row = cols >> 3;
  // rows blockIdx.x, blockIdx.x + gridDim.x, ...: the workgroups in flight sweep the tensor front to back together
  // (consecutive rows per workgroup measured 0.68 of 8 TB/s on [65536 x 7680], this order 0.79-0.81)
  (void)rows_per_block;
  bool first = true;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const u32x4* xr = (const u32x4*)(x + row * cols);
    u32x4* orow = (u32x4*)(out + row * cols);
    u32x4 raw[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      int64_t v = (int64_t)c * kBlock + threadIdx.x;
      raw[c] = (v < vec_per_row) ? __builtin_nontemporal_load(xr + v) : u32x4{0, 0, 0, 0};
    }
    if constexpr (GELU) {
      static_assert(DUAL, "the fused activation belongs to fc2's dual-format input quantizer");
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        const int64_t v = (int64_t)c * kBlock + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) raw[c][k] = f2h2(gelu_tanh_fast(h2f(raw[c][k] & 0xFFFFu)), gelu_tanh_fast(h2f(raw[c][k] >> 16)));
        if (a.gelu_out && v < vec_per_row) __builtin_nontemporal_store(raw[c], (u32x4*)((uint16_t*)a.gelu_out + row * cols) + v);
      }
    }
    if (first) {
      if (TAB_ARG) {
        lut16_stage(lut, tab, a.shift);
      } else {
        lut16_fill(lut, a);
      }
      first = false;   // the barriers inside block_max16 order the table before its first use
    }
    RowScale16 sn, sp;
    if (DUAL) {
      uint32_t mn = 0, mp = 0;
      auto block_reduce = [&]() {   // both maxima through one LDS exchange (one barrier pair instead of two)
        mn = row_max_dpp<64>(mn);
        mp = row_max_dpp<64>(mp);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (mn << 16) | mp;
        __syncthreads();
        mn = 0;
        mp = 0;
#pragma unroll
        for (int i = 0; i < kBlock / 64; ++i) {
          const uint32_t w = sh[i];
          mn = mn > (w >> 16) ? mn : (w >> 16);
          mp = mp > (w & 0xFFFFu) ? mp : (w & 0xFFFFu);
        }
      };
      {
        uint32_t un = 0, sg = 0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) dual_max_acc(raw[c], un, sg);
        dual_max_finish(un, sg, mn, mp);
      }
      block_reduce();
      if (__builtin_expect(mn > 0x7C00u || mp > 0x7C00u, 0)) {   // a NaN in the row (the same for every thread): the exact rule
        mn = 0;
        mp = 0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          uint32_t a1, b1;
          if (vec_absmax16_dual(raw[c], a1, b1) && a.nan_flag) atomicOr(a.nan_flag, 1u);
          mn = mn > a1 ? mn : a1;
          mp = mp > b1 ? mp : b1;
        }
        block_reduce();
      }
      sn = row_scale16(mn, a.fneg.gmax, a.inv_gneg);
      sp = row_scale16(mp, a.fpos.gmax, a.inv_gpos);
      dual_poison(sn, sp);
    } else {
      uint32_t m = 0;
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        uint32_t t = vec_absmax16(raw[c]);
        m = m > t ? m : t;
      }
      m = block_max16(m, sh);
      sn = row_scale16(m, a.fpos.gmax, a.inv_gpos);
      sp = sn;
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      int64_t v = (int64_t)c * kBlock + threadIdx.x;
      if (v < vec_per_row) {
        u32x4 o = quant_vec16<DUAL>(raw[c], lut, a.shift, sn.inv, sn.inv_lo, sn.s16x2, sp.inv, sp.inv_lo, sp.s16x2);
        __builtin_nontemporal_store(o, orow + v);
      }
    }
  }
}

// Medium rows (<= 64*MAXC vectors, e.g. per-token 1920 = 240 vectors): one WAVEFRONT per row, the
// row max by DPP/shuffles only - no LDS, no barrier in the row loop.
// HW6 (1: E2M3, 2: E3M2; rows of 193 .. 256 vectors = exactly 4 per lane, symmetric table): the levels from the FP6
// conversion hardware (fp6_levels_hw32) - no table, no LDS, no barrier.
template <bool DUAL, int MAXC, bool TAB_ARG, int HW6 = 0>
__global__ __launch_bounds__(kBlock) void rows16_lut_wave_kernel(const uint16_t* __restrict__ x,
                                                                uint16_t* __restrict__ out, int64_t rows, int64_t cols,
                                                                Lut16Args a, Lut16Tab tab) {
  static_assert(HW6 == 0 || (!DUAL && (MAXC == 4 || MAXC == 5)), "hardware FP6 levels: symmetric tables, 32 (+ 8) elements per lane");
  uint16_t* lut = nullptr;
  if constexpr (HW6 == 0) {
    __shared__ __attribute__((aligned(16))) uint16_t lut_s[kLutLdsEntries];   // static: a compile-time LDS address (a dynamic base is not folded into the ds_read offsets)
    lut = lut_s;
    if (TAB_ARG) {
      lut16_stage(lut, tab, a.shift);
    } else {
      lut16_fill(lut, a);
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t vpr = cols >> 3;
  constexpr int R = kBlock / 64;
  for (int64_t base = (int64_t)blockIdx.x * R; base < rows; base += (int64_t)gridDim.x * R) {
    const int64_t row = base + (threadIdx.x >> 6);
    if (row >= rows) continue;   // whole wavefront skips
    const u32x4* xr = (const u32x4*)(x + row * cols);
    u32x4* orow = (u32x4*)(out + row * cols);
    u32x4 raw[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int64_t v = (int64_t)c * 64 + lane;
      raw[c] = (v < vpr) ? __builtin_nontemporal_load(xr + v) : u32x4{0, 0, 0, 0};
    }
    RowScale16 sn, sp;
    if (DUAL) {
      uint32_t mn, mp;
      {
        uint32_t un = 0, sg = 0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) dual_max_acc(raw[c], un, sg);
        dual_max_finish(un, sg, mn, mp);
      }
      mn = row_max_dpp<64>(mn);
      mp = row_max_dpp<64>(mp);
      if (__builtin_expect(mn > 0x7C00u || mp > 0x7C00u, 0)) {   // a NaN in the row (wavefront-uniform): the exact rule
        uint32_t nan_any = 0;
        mn = 0;
        mp = 0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          uint32_t a1, b1;
          nan_any |= vec_absmax16_dual(raw[c], a1, b1);
          mn = mn > a1 ? mn : a1;
          mp = mp > b1 ? mp : b1;
        }
        if (nan_any && a.nan_flag) atomicOr(a.nan_flag, 1u);
        mn = row_max_dpp<64>(mn);
        mp = row_max_dpp<64>(mp);
      }
      sn = row_scale16(mn, a.fneg.gmax, a.inv_gneg);
      sp = row_scale16(mp, a.fpos.gmax, a.inv_gpos);
      dual_poison(sn, sp);
    } else {
      uint32_t m = 0;
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        uint32_t t = vec_absmax16(raw[c]);
        m = m > t ? m : t;
      }
      m = row_max_dpp<64>(m);
      sn = row_scale16(m, a.fpos.gmax, a.inv_gpos);
      sp = sn;
    }
    if constexpr (HW6 != 0) {
      scale_nan_if_not_finite(sn);
      uint32_t q[16], lv[16];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) q[4 * c + k] = div_pair16(raw[c][k], sn.inv, sn.inv_lo, sn.inv, sn.inv_lo);
      fp6_levels_hw32<HW6 == 2>(q, lv);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t v = (int64_t)c * 64 + lane;
        if (v < vpr)
          __builtin_nontemporal_store(u32x4{pk_fma0_f16(lv[4 * c], sn.s16x2), pk_fma0_f16(lv[4 * c + 1], sn.s16x2),
                                            pk_fma0_f16(lv[4 * c + 2], sn.s16x2), pk_fma0_f16(lv[4 * c + 3], sn.s16x2)}, orow + v);
      }
      if constexpr (MAXC == 5) {   // the fifth vector of lanes 0 .. (vpr - 256): a second conversion with 8 live values
        uint32_t q5[4], l5[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q5[k] = div_pair16(raw[4][k], sn.inv, sn.inv_lo, sn.inv, sn.inv_lo);
        fp6_levels_hw32<HW6 == 2, 4>(q5, l5);
        const int64_t v = 256 + lane;
        if (v < vpr)
          __builtin_nontemporal_store(u32x4{pk_fma0_f16(l5[0], sn.s16x2), pk_fma0_f16(l5[1], sn.s16x2), pk_fma0_f16(l5[2], sn.s16x2),
                                            pk_fma0_f16(l5[3], sn.s16x2)}, orow + v);
      }
      continue;
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int64_t v = (int64_t)c * 64 + lane;
      if (v < vpr) {
        u32x4 o = quant_vec16<DUAL>(raw[c], lut, a.shift, sn.inv, sn.inv_lo, sn.s16x2, sp.inv, sp.inv_lo, sp.s16x2);
        __builtin_nontemporal_store(o, orow + v);
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// F1: the online rotate fused in front of the per-group quant.
//
// Reference (tr/basic_var.py:263,266 under the driver's fp16 autocast):
//     x1 = matmul(half(producer * s), half(Q))            fp16 GEMM, fp32 accumulation
//     q  = fp_quant_*_per_group_cuda(x1, 4, 128)
// with Q block-diagonal, every 128x128 block = diag(D) . H128 / sqrt(128)
// (rotate_utils/rotation_utils.py:69-104, hadamard_utils.py:63-99), so per 128-chunk
//     x1 = half( c_h * FWHT128(h * D) ),   c_h = half(float32(1/sqrt(128))) = 0.08837890625   (one rounding:
//          v_fma_mixlo/hi_f16; the butterfly of fp16 inputs is nearly always exact in fp32)
// The transform runs on the matrix cores (fpq_rotate_mfma.h); the butterfly below (fwht128_h_n) serves what of the adaLN
// producers' rows does not: the first generation (C > 2560) and the groups beyond a tile in the third (fpq_adaln.h).  A dense fp16 GEMM of 2*rows*C^2 FLOPs and a 2 B/elem round trip
// disappear.
//
// Parity contract: the quant stage is bit-exact for the rotated values the kernels
// produce (it can emit them); the rotated values are within 1 fp16 ulp of the
// fp64-accumulated product (the reference GEMM's own summation order is unspecified).
// ---------------------------------------------------------------------------------
struct RotArgs {
  const float* smooth;   // [cols] per-channel factor (GALT s) or nullptr
  uint32_t sign[4];      // bit j set <=> D[j] = -1, j = 0..127
  float c_h;             // (float)half(float32(1/sqrt(128)))
  int64_t vec_per_row;   // cols / 8
  uint16_t* code_scales; // nullptr: `out` receives fake-quantized fp16 values.  Otherwise `out` receives packed
                         // hardware E2M1 codes (4 bytes per 8 elements), this array one fp16 scale per 128-group,
                         // and the staged table is the code table (fpq_gemm_fp4.h)
  int code_bits;         // per-token code emission: 8 = E4M3 bytes (fpq_gemm_fp8.h), 6 = dense 6-bit E2M3 (fpq_gemm_fp6.h)
  uint32_t km_rows;      // != 0: FP4 / FP6 codes go to a k-major image of this many rows (include/fpq.h) instead of row-major
  FastDiv km_gpr;        // ... groups (K steps) per row, for the kernels that walk the tensor as a flat run of groups
};

__device__ __forceinline__ float xlane_xor4(float v) {
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x101F));
}
__device__ __forceinline__ float xlane_xor8(float v) {
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x201F));
}
__device__ __forceinline__ float xlane_xor1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float xlane_xor2(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
}

// The butterfly's values travel as 4 float pairs (t[j], t[j+4]) so that the butterflies map onto the
// packed fp32 ALU (v_pk_add_f32 / v_pk_fma_f32: two results per issue slot).
typedef float f2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f2_t xlane2(f2_t v, int which) {
  f2_t r;
  if (which == 1) { r.x = xlane_xor1(v.x); r.y = xlane_xor1(v.y); }
  else if (which == 2) { r.x = xlane_xor2(v.x); r.y = xlane_xor2(v.y); }
  else if (which == 4) { r.x = xlane_xor4(v.x); r.y = xlane_xor4(v.y); }
  else { r.x = xlane_xor8(v.x); r.y = xlane_xor8(v.y); }
  return r;
}

// half(a * b) packed from two fp32 values: the rotated value half(c_h * FWHT(...)).  Two v_mul_f32 and one
// v_cvt_pk_f16_f32 (2 x 2.5 + 4.6 cycles of the vector pipe) instead of v_fma_mixlo/hi_f16 (2 x 8.2,
// profiles/r03_valu_issue_cost.txt).  The product is rounded to fp32 before it is rounded to fp16: the two roundings
// differ from one in ~2^-13 of the values, by one fp16 ulp; no torch op sequence is mirrored here (the reference's GEMM
// rounds its own fp32 accumulator) and the contract - within half an ulp (1.001) + the accumulation bound of the exact
// product, quantization exact on the values produced - holds as before.
__device__ __forceinline__ uint32_t mul2_to_h2(float lo, float hi, float b) { return f2h2(lo * b, hi * b); }

// D = s * (float)half(w) + (float)half(pw), lo / hi halves: both fp16 operands are widened by the instruction itself
__device__ __forceinline__ float fmix_hsh_lo(uint32_t w, float s, uint32_t pw) {
  float d;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(d) : "v"(w), "v"(s), "v"(pw));
  return d;
}
__device__ __forceinline__ float fmix_hsh_hi(uint32_t w, float s, uint32_t pw) {
  float d;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(w), "v"(s), "v"(pw));
  return d;
}

// FWHT over the 128 fp16 values held by 16 lanes x 4 packed registers (signs already applied), natural (Sylvester)
// order, fp32 results (not yet scaled by c_h).  N independent groups are transformed stage by stage (stage-major
// source order: N dependency chains for the in-order issue to interleave).  The butterfly stages commute, so the
// first one is the lane-bit-0 stage, taken straight from the PACKED halves: one DPP move fetches two partner
// values, and v_fma_mix_f32 widens mine and the partner's while it adds (exact) - no separate fp16 -> fp32
// conversion exists.  Then the three in-register stages on float pairs, then lane bits 1, 2, 3: partner + sign * mine
// (lower lane a + b, upper lane a - b; DPP quad_perm for lane ^ 2, ds_swizzle for lane ^ 4, lane ^ 8 - no LDS memory is
// touched).
template <int N>
__device__ __forceinline__ void fwht128_h_n(const u32x4 (&w)[N], float (&t)[N][8], int n, int lane_in_group) {
  const float s1 = (lane_in_group & 1) ? -1.0f : 1.0f, s2 = (lane_in_group & 2) ? -1.0f : 1.0f;
  const float s4 = (lane_in_group & 4) ? -1.0f : 1.0f, s8 = (lane_in_group & 8) ? -1.0f : 1.0f;
  f2_t p[N][4];
#pragma unroll
  for (int q = 0; q < N; ++q) {
    if (q >= n) continue;
    uint32_t pw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      pw[k] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[q][k], 0xB1, 0xF, 0xF, true);
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // element 2k, 2k+1 -> pair register (k & 1 ? .. ): t index j pairs with j + 4
      const float lo = fmix_hsh_lo(w[q][k], s1, pw[k]), hi = fmix_hsh_hi(w[q][k], s1, pw[k]);
      // elements 2k and 2k+1: p[j] = {t[j], t[j + 4]}
      if (k < 2) {
        p[q][2 * k].x = lo;
        p[q][2 * k + 1].x = hi;
      } else {
        p[q][2 * k - 4].y = lo;
        p[q][2 * k - 3].y = hi;
      }
    }
  }
  // index bit 0 and bit 1: whole pairs against whole pairs; index bit 2: inside each pair
#pragma unroll
  for (int q = 0; q < N; ++q) {
    if (q >= n) continue;
    f2_t a = p[q][0], b = p[q][1];
    p[q][0] = a + b;
    p[q][1] = a - b;
    a = p[q][2];
    b = p[q][3];
    p[q][2] = a + b;
    p[q][3] = a - b;
  }
#pragma unroll
  for (int q = 0; q < N; ++q) {
    if (q >= n) continue;
    f2_t a = p[q][0], b = p[q][2];
    p[q][0] = a + b;
    p[q][2] = a - b;
    a = p[q][1];
    b = p[q][3];
    p[q][1] = a + b;
    p[q][3] = a - b;
  }
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q < n) p[q][j] = f2_t{p[q][j].x + p[q][j].y, p[q][j].x - p[q][j].y};
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q < n) p[q][j] = __builtin_elementwise_fma(p[q][j], f2_t{s2, s2}, xlane2(p[q][j], 2));
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q < n) p[q][j] = __builtin_elementwise_fma(p[q][j], f2_t{s4, s4}, xlane2(p[q][j], 4));
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q < n) p[q][j] = __builtin_elementwise_fma(p[q][j], f2_t{s8, s8}, xlane2(p[q][j], 8));
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[q][j] = p[q][j].x;
      t[q][j + 4] = p[q][j].y;
    }
}

// group-of-16-lanes maxima of N values, the DPP steps interleaved
template <int N>
__device__ __forceinline__ void row_max_dpp16_n(uint32_t (&v)[N], int n) {
  auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
#pragma unroll
  for (int step = 0; step < 4; ++step)
#pragma unroll
    for (int q = 0; q < N; ++q) {
      if (q >= n) continue;
      uint32_t o;
      if (step == 0) o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[q], 0xB1, 0xF, 0xF, true);
      else if (step == 1) o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[q], 0x4E, 0xF, 0xF, true);
      else if (step == 2) o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[q], 0x141, 0xF, 0xF, true);
      else o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[q], 0x140, 0xF, 0xF, true);
      v[q] = mx(v[q], o);
    }
}

// ---------------------------------------------------------------------------------
// Host caches of the bucket tables, shared by every translation unit that launches a table kernel.  Each unit builds its
// own copy on first use (inline functions in an anonymous namespace: one static per unit).  That is safe: every cache is a
// deterministic function of the table ids, immutable once built, and lives on the host only - the tables reach the
// kernels as arguments (no device global is written from the host).
// ---------------------------------------------------------------------------------
inline int table_shift16(int id) {   // rounding thresholds are multiples of 2^shift in fp16 patterns
  return id == FPQ_INT_NEG ? 5 : 9 - kTables[id].mbits;
}

// host cache of prebuilt tables: built once per (neg, pos) pair, immutable afterwards
struct Lut16Host {
  Lut16Args args;
  Lut16Tab tab;                    // the compressed image that travels in the kernel arguments
  bool tab_valid;                  // false: kernels evaluate the closed form themselves (lut16_fill)
  uint16_t full[kLutLdsEntries];   // the full image (host side: derived code tables are built from it)
};

inline const Lut16Host& lut16_host(int neg_id, int pos_id) {
  static const auto* cache = [] {
    auto* c = new Lut16Host[FPQ_NUM_TABLES * FPQ_NUM_TABLES];
    for (int n = 0; n < FPQ_NUM_TABLES; ++n)
      for (int p = 0; p < FPQ_NUM_TABLES; ++p) {
        Lut16Host& h = c[n * FPQ_NUM_TABLES + p];
        h.args.fneg = make_fmt(n);
        h.args.fpos = make_fmt(p);
        h.args.inv_gneg = 1.0f / h.args.fneg.gmax;
        h.args.inv_gpos = 1.0f / h.args.fpos.gmax;
        h.args.shift = table_shift16(n) < table_shift16(p) ? table_shift16(n) : table_shift16(p);
        h.args.nan_flag = nullptr;
        h.args.clip_absmax = nullptr;
        h.args.clip_strength = 1.0f;
        h.args.gelu_out = nullptr;
        for (int i = 0; i < kLutLdsEntries; ++i) h.full[i] = 0;
        lut16_build_host(h.full, h.args);
        h.tab_valid = lut16_compress(h.full, h.args.shift, &h.tab);
      }
    return c;
  }();
  return cache[neg_id * FPQ_NUM_TABLES + pos_id];
}

// hardware-nibble codes of E2M1 (the FP4 GEMM's operands, fpq_codes_mx.h, and the packed KV cache)
inline const Lut16Tab& lut16_mx_codes_e2m1() {
  static const Lut16Tab* tab = [] {
    auto* t = new Lut16Tab;
    const Lut16Host& h = lut16_host(FPQ_E2M1, FPQ_E2M1);
    const int n = 1 << (16 - h.args.shift);
    uint16_t full[kLutLdsEntries] = {0};
    for (int i = 0; i < n; ++i) {
      uint32_t u = (uint32_t)i << h.args.shift;
      bool neg = (u >> 15) != 0;
      float qm = quant_mag(h2f(u & 0x7FFFu), 0u, h.args.fpos);
      // level -> magnitude index 0..7 (host twin of level_index)
      int li = (qm >= h.args.fpos.kmin) ? (int)((fbits(qm) >> h.args.fpos.mshift) - h.args.fpos.kmin_code_base)
                                        : (int)(qm * h.args.fpos.inv_step0);
      full[i] = (uint16_t)(li | ((neg && li != 0) ? 8 : 0));
    }
    if (!lut16_compress(full, h.args.shift, t)) abort();   // E2M1: 2 x 128 buckets, always fits
    return t;
  }();
  return *tab;
}

// level (exactly an E2M3 number, sign included) -> 6-bit code
__host__ __device__ __forceinline__ uint32_t e2m3_of_level(float q) {
  const uint32_t sgn = (q < 0.0f) ? 32u : 0u;
  const float a = q < 0.0f ? -q : q;
  uint32_t mag;
  if (a < 1.0f) mag = (uint32_t)(a * 8.0f);                                        // subnormal: m / 8
  else if (a < 2.0f) mag = (1u << 3) | (uint32_t)((a - 1.0f) * 8.0f);
  else if (a < 4.0f) mag = (2u << 3) | (uint32_t)((a * 0.5f - 1.0f) * 8.0f);
  else mag = (3u << 3) | (uint32_t)((a * 0.25f - 1.0f) * 8.0f);
  return sgn | mag;
}

// host: OCP E4M3 byte of a value that is exactly representable (every level of the symmetric tables is)
inline uint8_t e4m3_of(float v) {
  if (v == 0.0f) return 0;
  const uint8_t sgn = v < 0.0f ? 0x80 : 0;
  int e;
  const float m = frexpf(fabsf(v), &e);        // |v| = m * 2^e, m in [0.5, 1)
  const int ex = e - 1;                         // |v| = (2m) * 2^(e-1), 2m in [1, 2)
  const int man = (int)((2.0f * m - 1.0f) * 8.0f);
  return (uint8_t)(sgn | ((ex + 7) << 3) | man);
}

// bucket -> E4M3 code tables for the fast fp16 path, one per symmetric table, built once (immutable afterwards)
inline const Lut16Tab& lut16_codes8(int table_id) {
  static const Lut16Tab* tabs = [] {
    auto* t = new Lut16Tab[FPQ_NUM_TABLES]();
    for (int id = 0; id < FPQ_NUM_TABLES; ++id) {
      if (!kTables[id].symmetric) continue;
      const Lut16Host& h = lut16_host(id, id);
      if (!h.tab_valid) continue;
      const int n = 1 << (16 - h.args.shift);
      uint16_t full[kLutLdsEntries] = {0};
      for (int i = 0; i < n; ++i) full[i] = e4m3_of(h2f(h.full[i]));
      if (!lut16_compress(full, h.args.shift, &t[id])) abort();   // same structure as the level table it is derived from
    }
    return t;
  }();
  return tabs[table_id];
}

// level (exactly an E3M2 number, sign included) -> 6-bit BF6 code: sign, 3 exponent bits (bias 3), 2 mantissa bits; a zero of
// either sign is code 0
__host__ __device__ __forceinline__ uint32_t e3m2_of_level(float q) {
  const uint32_t sgn = (q < 0.0f) ? 32u : 0u;
  const float a = q < 0.0f ? -q : q;
  if (a < 0.25f) return sgn | (uint32_t)(a * 16.0f);                               // subnormal: m / 16
  const uint32_t u = __builtin_bit_cast(uint32_t, a);                              // normal: 2^(e - 3) (1 + m / 4), e = 1 .. 7
  return sgn | ((((((u >> 23) & 0xFFu) - 124u) << 2) | ((u >> 21) & 3u)) & 31u);   // (& 31: a code never reaches its neighbours' bits)
}

// bucket -> 6-bit code table of FPQ_E2M3 or FPQ_E3M2 (the FP6 / BF6 operand producers and the packed KV cache), each built once
// on first use (immutable afterwards)
inline const Lut16Tab& lut16_codes6(int table_id) {
  const auto build = [](int id) {
    auto* t = new Lut16Tab();
    const Lut16Host& h = lut16_host(id, id);
    const int n = 1 << (16 - h.args.shift);
    uint16_t full[kLutLdsEntries] = {0};
    for (int i = 0; i < n; ++i) full[i] = (uint16_t)(id == FPQ_E3M2 ? e3m2_of_level(h2f(h.full[i])) : e2m3_of_level(h2f(h.full[i])));
    if (!lut16_compress(full, h.args.shift, t)) abort();   // same structure as the level table it is derived from
    return t;
  };
  if (table_id == FPQ_E3M2) {
    static const Lut16Tab* bf6 = build(FPQ_E3M2);
    return *bf6;
  }
  static const Lut16Tab* fp6 = build(FPQ_E2M3);
  return *fp6;
}
inline const Lut16Tab& lut16_codes6_e2m3() { return lut16_codes6(FPQ_E2M3); }

// bucket -> 6-bit code table of the per-group A6W4 emitter (fpq_codes_g6.h): the bucket structure of FPQ_E1M2 with the FP6 E2M3
// codes of its levels (0, 0.25 .. 1.75 are E2M3 numbers) or of FPQ_E3M0 with the BF6 E3M2 codes of its levels (0, 0.25, 0.5, 1 ..
// 16 are E3M2 numbers); each built once on first use (immutable afterwards)
inline const Lut16Tab& lut16_codes_g6(int table_id) {
  const auto build = [](int id) {
    auto* t = new Lut16Tab();
    const Lut16Host& h = lut16_host(id, id);
    const int n = 1 << (16 - h.args.shift);
    uint16_t full[kLutLdsEntries] = {0};
    for (int i = 0; i < n; ++i) full[i] = (uint16_t)(id == FPQ_E3M0 ? e3m2_of_level(h2f(h.full[i])) : e2m3_of_level(h2f(h.full[i])));
    if (!lut16_compress(full, h.args.shift, t)) abort();   // same structure as the level table it is derived from
    return t;
  };
  if (table_id == FPQ_E3M0) {
    static const Lut16Tab* e3 = build(FPQ_E3M0);
    return *e3;
  }
  static const Lut16Tab* e1 = build(FPQ_E1M2);
  return *e1;
}

// k-major images are addressed with 32-bit byte offsets (and int buffer ranges) by their producers: the whole image must stay below 2 GiB
inline bool km_image_fits(int64_t rows, int64_t row_bytes) { return rows < (1ll << 31) && rows * row_bytes < (1ll << 31); }
