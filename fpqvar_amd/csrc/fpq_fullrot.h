// fpq_fullrot.h - the FULL-WIDTH online rotation in front of the per-group quantizer: y = half(c_h * h . diag(D) . H_C^T) with
// H_C = hadK (x) Sylvester(m) (rotation.hadamard_matrix: (K, m) = (60, 32) for C = 1920, (36, 64) for C = 2304), both factors on
// the matrix cores, then the per-group(128) quantizer on the rotated row - one launch.  Included by fpq_fullrot.hip after fpq_fast16.h.
//
// View the sign-applied row as X[K][m] (element j = kj * m + lj) and the output as Y[K][m] (o = ko * m + lo):
//     Y = c_h . hadK . X . Sylvester(m)        2 C (K + m) FLOP per row instead of the dense product's 2 C^2 (21 x / 23 x fewer).
// One wavefront owns a row at a time (persistent, rows blockIdx.x * 4 + wave, ...):
//   1. P = X . Sylvester(m) on v_mfma_f32_16x16x32_f16.  A = 16 row segments X[16 T + i][.]: lane (i = lane % 16, kq = lane / 16)
//      holds the 8 consecutive lj = 32 s + 8 kq .. - ONE 16-byte load per lane and (T, s), straight from the row in HBM (m = 32: the 64
//      lanes of a load cover 1 KiB in a row).  Loads go through a buffer resource of one row: the segments kj >= K of the last
//      M-tile (K = 60 -> 64, 36 -> 48) read zeros.  Signs D by xor (masks per operand and lane in LDS).  B = (-1)^popcount(lj & lo), a lane constant.
//      The accumulators leave lane (n, q) holding P[16 T + 4 q + r][16 N + n], r = 0 .. 3.
//   2. Y = hadK . P on v_mfma_f32_16x16x32_bf16, chained on those accumulators with no LDS traffic: the reduction index of an MFMA may
//      be permuted when the constant A operand is permuted alike, so k-slot (kq, e) of step tp is kj = 16 (2 tp + e / 4) + 4 kq + e % 4
//      - two M-tiles of stage 1 side by side.  The fp32 intermediate enters as THREE bf16 pieces by truncation, b1 = top 16 bits of
//      P, b2 = top 16 bits of P - b1, b3 = P - b1 - b2: 8 + 8 + 8 significant bits, so b1 + b2 + b3 == P EXACTLY (no range issue: bf16
//      has fp32's exponent; P is a multiple of 2^-24).  A row with a non-finite input runs a second copy of the body in which a
//      non-finite P keeps b1 (a NaN quieted) and zeroes b2, b3 (inf - inf); every other row spends four instructions per value.
//      hadK's padding is zero: zeros face the zero segments kj >= K only (0 . 0, never 0 . inf), the padded ROWS ko >= K produce outputs
//      that are dropped.  A = hadK[ko][kj] as +-1.0 bf16 from a table in the code object (fr_make_had_table; Paley I over GF(59) - NOT
//      symmetric - and Paley II over GF(17), as rotation.py builds them).
//   3. y = half(c_h * Y) goes as 2-byte pieces into the wavefront's fp16 row image in LDS (one ko per image row of 2 m + 16 bytes: the
//      four q of a write hit different banks), and the stand-alone quantizer's lane code (fpq_fast16.h: 16 lanes x one 16-byte
//      vector per group, row_max_dpp<16>, row_scale16, quant_vec16 / codes_vec16) runs on 16-byte vectors read back in row order:
//      out == fpq_quant_rows(y) / fpq_quant_rows_codes_mx[_km](y) by construction.
// Numerics: +-1 operands; every rounding is an fp32 rounding of a partial sum inside an MFMA (at most m - 1 in stage 1, 3 K - 1 in
// stage 2: K segments x three pieces), one of the product with c_h, one to fp16: tests/fullrot_model.py carries the bound.
// Built widths: kFullRotWidths.  The row loop is written ONCE, fullrot_rows_kernel<Front, Tail> at the end of this file: every
// full-width producer is an instantiation of it.  A FRONT makes a row's operands (FrPlainFront here: fr_load_row; FrAdalnFront in
// fpq_fulladaln.h: LayerNorm + modulate), a TAIL (FrTail) names what runs on the rotated row's LDS image: fr_quant_image here, one
// scale per 128 elements, or fr_token_image (fpq_fulltoken.h), one per row.  The host side of all of them: fpq_fullrot_launch.h.
#pragma once

typedef __bf16 fr_bf8_t __attribute__((ext_vector_type(8)));

constexpr int kFullRotWidths[] = {1920, 2304};   // 60 x 32, 36 x 64
constexpr int kFrMaxSignWords = 2304 / 32;
constexpr int kFrWaves = 4;                      // workgroups per CU the launch bounds ask for (= wavefronts per SIMD)
constexpr int kFrCUs = 256;

struct FullRotArgs {
  const float* smooth;      // device float[C] or nullptr
  uint16_t* code_scales;    // per group, codes: the group scales (fp16 [rows][G], k-major: fp32 [G][rows rounded up to 4]); per token: fp16 [rows]
  uint32_t km_rows;         // codes into a k-major image of this many rows; 0: row-major
  float c_h;                // float(half(float32(1 / sqrt(C))))
  uint32_t sign[kFrMaxSignWords];   // bit j set <=> D[j] == -1
};

struct FullAdalnArgs {      // what FrAdalnFront (fpq_fulladaln.h) takes beside them; here because the one host path fills it
  const void* scale;          // [rows / rows_per_batch][C] in the modulation dtype
  const void* shift;
  uint16_t* h_out;            // FrTail::EMIT: fp16 [rows][C] receiving h, or nullptr
  uint32_t rows_per_batch;
  float eps;
};

// What a tail writes.  kValues: fp16 values (the per-token tail: the rotated rows too where `rot_out` is given); kEmit, the per-group
// tail only: values + the rotated rows; kCodes: operand codes + scales (`outv`: the codes, `lut` staged from the code table)
enum class FrMode { kValues, kEmit, kCodes };

// The tail of a kernel.  TOKEN: fr_token_image, else fr_quant_image; ROT_MAYBE (kEmit): `rot_out` may be null.  EMIT: the form whose
// intermediates - the rotated rows, a front's h - go out where their pointers are given
template <bool TOKEN_, FrMode MODE_, bool ROT_MAYBE_>
struct FrTail {
  static constexpr bool TOKEN = TOKEN_, ROT_MAYBE = ROT_MAYBE_, EMIT = MODE_ == (TOKEN_ ? FrMode::kValues : FrMode::kEmit);
  static constexpr FrMode MODE = MODE_;
};

// hadK as stage 2's A operands: w[mo][tp][lane][.] = the 8 bf16 values hadK[16 mo + lane % 16][16 (2 tp + e / 4) + 4 (lane / 16) + e % 4],
// e = 0 .. 7 (two per word, even e in the low half); 0 beyond K
template <int K>
struct FrHadTable {
  uint32_t w[(K + 15) / 16][2][64][4];
};
template <int K>
constexpr FrHadTable<K> fr_make_had_table() {
  static_assert(K == 60 || K == 36, "Paley I over GF(59), Paley II over GF(17)");
  constexpr int q = K == 60 ? 59 : 17;
  int chi[64] = {};   // the quadratic-residue character of GF(q)
  for (int x = 1; x < q; ++x) chi[x] = -1;
  for (int y = 1; y < q; ++y) chi[(y * y) % q] = 1;
  auto entry = [&](int r, int c) -> int {
    if (K == 60) {   // first column +1, first row (+1, -1, ..., -1), core I - S, S[i][j] = chi(j - i)
      if (c == 0) return 1;
      if (r == 0) return -1;
      const int i = r - 1, j = c - 1;
      return (i == j ? 1 : 0) - chi[(j - i + q) % q];
    }
    // [[C + I, C - I], [C - I, -C - I]], C the conference matrix [[0, 1], [1, chi(j - i)]]
    const int n = q + 1, rb = r / n, cb = c / n, i = r % n, j = c % n;
    const int cij = (i == 0 && j == 0) ? 0 : (i == 0 || j == 0) ? 1 : chi[(j - i + q) % q];
    const int e = i == j ? 1 : 0;
    return rb == 0 ? (cb == 0 ? cij + e : cij - e) : (cb == 0 ? cij - e : -cij - e);
  };
  FrHadTable<K> t = {};
  for (int mo = 0; mo < (K + 15) / 16; ++mo)
    for (int tp = 0; tp < 2; ++tp)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int ko = 16 * mo + (lane & 15), kj = 16 * (2 * tp + (e >> 2)) + 4 * (lane >> 4) + (e & 3);
          const int v = (ko < K && kj < K) ? entry(ko, kj) : 0;
          const uint32_t bits = v > 0 ? 0x3F80u : v < 0 ? 0xBF80u : 0u;
          t.w[mo][tp][lane][e >> 1] |= bits << (16 * (e & 1));
        }
  return t;
}
__device__ const FrHadTable<60> kFrHad60 = fr_make_had_table<60>();
__device__ const FrHadTable<36> kFrHad36 = fr_make_had_table<36>();
template <int K>
__device__ __forceinline__ const FrHadTable<K>& fr_had_table() {
  if constexpr (K == 60) return kFrHad60;
  else return kFrHad36;
}

// The geometry of one width, shared by the kernel and its launcher
template <int K, int M>
struct FrGeom {
  static constexpr int C = K * M;
  static constexpr int KT = (K + 15) / 16;        // M-tiles of stage 1 = row tiles of hadK
  static constexpr int NT = M / 16;               // N-tiles: 16 lo each
  static constexpr int KS = M / 32;               // k-steps of stage 1
  static constexpr int VPR = C / 8;               // 16-byte vectors of a row
  static constexpr int STRIDE = 2 * M + 16;       // bytes of an image row (one ko)
  static constexpr int IMG = K * STRIDE;          // the wavefront's row image
  static constexpr int NPASS = (VPR + 63) / 64;
  static constexpr int SIGNW = KT * 16 * M / 32;  // sign words, the zero segments included
};

// fp32 -> three bf16 pieces by truncation: the TOP halves of h1 = p, h2 = p - top(p), h3 = h2 - top(h2) (fr_top2 packs them; h3
// has at most 8 significant bits left: its low half is zero).  FINITE: the row has no non-finite input, so p is finite (|p| < 2^22)
// and three instructions less per value are spent; else an infinite p keeps h1 and a NaN its quiet bit, h2 = h3 = 0 (no inf - inf).
template <bool FINITE>
__device__ __forceinline__ void fr_split3(float p, uint32_t& h1, uint32_t& h2, uint32_t& h3) {
  const uint32_t bits = fbits(p);
  const float r1 = p - u2f(bits & 0xFFFF0000u);
  const float r2 = r1 - u2f(fbits(r1) & 0xFFFF0000u);
  h1 = bits;
  h2 = fbits(r1);
  h3 = fbits(r2);
  if constexpr (!FINITE) {
    const bool fin = (bits & 0x7F800000u) != 0x7F800000u;
    h1 = (fin || !(bits & 0x007FFFFFu)) ? bits : bits | 0x00400000u;
    h2 = fin ? h2 : 0u;
    h3 = fin ? h3 : 0u;
  }
}
// the top halves of two fp32 patterns as a bf16 pair, `even` in the low half
__device__ __forceinline__ uint32_t fr_top2(uint32_t even, uint32_t odd) { return __builtin_amdgcn_perm(odd, even, 0x07060302u); }

struct FrLane {
  uint32_t syl[4];   // +-1.0 fp16 pairs: (-1)^popcount(e & lane % 8), e = 2 k, 2 k + 1
};
__device__ __forceinline__ FrLane fr_lane_consts(int lane) {
  FrLane c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t b0 = (uint32_t)__builtin_popcount((2 * k) & lane & 7) & 1u, b1 = (uint32_t)__builtin_popcount((2 * k + 1) & lane & 7) & 1u;
    c.syl[k] = 0x3C003C00u ^ (b0 << 15) ^ (b1 << 31);
  }
  return c;
}

// A row as stage 1's A operands, signs not yet applied: w[T][s] = h[(16 T + i) m + 32 s + 8 q ..], lane (i = lane % 16, q = lane / 16)
template <int K, int M>
struct FrRow {
  u32x4 w[FrGeom<K, M>::KT][FrGeom<K, M>::KS];
};
// first element of lane (i, q)'s vector of operand (T, s); beyond C in the zero segments
template <int M>
__device__ __forceinline__ int fr_col0(int T, int s, int lane) { return (16 * T + (lane & 15)) * M + 32 * s + 8 * (lane >> 4); }

// h = half(x * smooth) of one row from `src` (a buffer resource of the row: C * sizeof(Tin) bytes; `smooth`: of the C floats): one
// 16-byte load per lane and operand (fp32 rows: two); the zero segments read zeros
template <int K, int M, typename Tin, bool SMOOTH>
__device__ __forceinline__ void fr_load_row(__amdgpu_buffer_rsrc_t src, __amdgpu_buffer_rsrc_t smooth, int lane, FrRow<K, M>& h) {
  using G = FrGeom<K, M>;
#pragma unroll
  for (int T = 0; T < G::KT; ++T)
#pragma unroll
    for (int s = 0; s < G::KS; ++s) {
      const int col0 = fr_col0<M>(T, s, lane);
      u32x4 w;
      if constexpr (sizeof(Tin) == 2) {
        w = __builtin_amdgcn_raw_buffer_load_b128(src, col0 * 2, 0, kRqNt);
        if constexpr (SMOOTH) {   // h = half(float(x) * s): the widening rides on the multiply (x * s - 0 == x * s, signed zeros included)
          const u32x4 sa = __builtin_amdgcn_raw_buffer_load_b128(smooth, col0 * 4, 0, 0), sb = __builtin_amdgcn_raw_buffer_load_b128(smooth, col0 * 4 + 16, 0, 0);
          w[0] = f2h2(fmaf_h_lo(w[0], u2f(sa[0]), -0.0f), fmaf_h_hi(w[0], u2f(sa[1]), -0.0f));
          w[1] = f2h2(fmaf_h_lo(w[1], u2f(sa[2]), -0.0f), fmaf_h_hi(w[1], u2f(sa[3]), -0.0f));
          w[2] = f2h2(fmaf_h_lo(w[2], u2f(sb[0]), -0.0f), fmaf_h_hi(w[2], u2f(sb[1]), -0.0f));
          w[3] = f2h2(fmaf_h_lo(w[3], u2f(sb[2]), -0.0f), fmaf_h_hi(w[3], u2f(sb[3]), -0.0f));
        }
      } else {
        const u32x4 fa = __builtin_amdgcn_raw_buffer_load_b128(src, col0 * 4, 0, kRqNt), fb = __builtin_amdgcn_raw_buffer_load_b128(src, col0 * 4 + 16, 0, kRqNt);
        float f[8] = {u2f(fa[0]), u2f(fa[1]), u2f(fa[2]), u2f(fa[3]), u2f(fb[0]), u2f(fb[1]), u2f(fb[2]), u2f(fb[3])};
        if constexpr (SMOOTH) {   // h = half(x * s): the fp32 product, then the rounding to fp16 (f2h2 keeps them apart)
          const u32x4 sa = __builtin_amdgcn_raw_buffer_load_b128(smooth, col0 * 4, 0, 0), sb = __builtin_amdgcn_raw_buffer_load_b128(smooth, col0 * 4 + 16, 0, 0);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            f[k] *= u2f(sa[k]);
            f[4 + k] *= u2f(sb[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = f2h2(f[2 * k], f[2 * k + 1]);
      }
      h.w[T][s] = w;
    }
}

// One row transformed: the signs from `sgn_s` (LDS: the xor masks of operand (T, s) and lane at (T KS + s) 64 + lane), hadK's operands from
// `had_s` (FrHadTable<K>::w staged in LDS: 32 registers per lane otherwise); y = half(c_h * Y) goes into the row image `img` (element
// ko * m + lo at ko * STRIDE + 2 lo).
template <int K, int M>
__device__ __forceinline__ void fullrot_transform_row(const FrRow<K, M>& h, const u32x4* sgn_s, const u32x4* had_s, const FrLane& lc,
                                                      float c_h, char* img, int lane) {
  using G = FrGeom<K, M>;
  const int i = lane & 15, q = lane >> 4;
  // 1. the A operands, signs by xor; the largest |pattern| tells whether every input is finite
  rq_h8_t xa[G::KT][G::KS];
  uint32_t amax = 0u;
#pragma unroll
  for (int T = 0; T < G::KT; ++T)
#pragma unroll
    for (int s = 0; s < G::KS; ++s) {
      const u32x4 w = h.w[T][s] ^ sgn_s[(T * G::KS + s) * 64 + lane];
#pragma unroll
      for (int k = 0; k < 4; ++k) amax = pk_max_u16(amax, w[k] & 0x7FFF7FFFu);
      xa[T][s] = __builtin_bit_cast(rq_h8_t, w);
    }
  const bool all_finite = __builtin_amdgcn_ballot_w64((amax & 0xFFFFu) >= 0x7C00u || (amax >> 16) >= 0x7C00u) == 0;
  const rq_f4_t zero = {0.0f, 0.0f, 0.0f, 0.0f};
  auto body = [&](auto finite) {
    constexpr bool FINITE = finite.value;
#pragma unroll
    for (int nt = 0; nt < G::NT; ++nt) {
      // P[T] = X . S[.][16 nt ..]: B element (lj = 32 s + 8 q + e, lo = 16 nt + i) = (-1)^(popcount(e & i & 7) + popcount((4 s + q) & (2 nt + i / 8)))
      rq_f4_t P[G::KT];
#pragma unroll
      for (int T = 0; T < G::KT; ++T) P[T] = zero;
#pragma unroll
      for (int s = 0; s < G::KS; ++s) {
        const uint32_t flip = ((uint32_t)__builtin_popcount((4 * s + q) & (2 * nt + (i >> 3))) & 1u) ? 0x80008000u : 0u;
        const u32x4 bw = {lc.syl[0] ^ flip, lc.syl[1] ^ flip, lc.syl[2] ^ flip, lc.syl[3] ^ flip};
        const rq_h8_t b = __builtin_bit_cast(rq_h8_t, bw);
#pragma unroll
        for (int T = 0; T < G::KT; ++T) P[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xa[T][s], b, P[T], 0, 0, 0);
      }
      // 2. Y[mo] = hadK[16 mo ..][.] . P over kj = 16 (2 tp + e / 4) + 4 q + e % 4, three bf16 pieces
      rq_f4_t Y[G::KT];
#pragma unroll
      for (int mo = 0; mo < G::KT; ++mo) Y[mo] = zero;
#pragma unroll
      for (int tp = 0; tp < 2; ++tp) {
        uint32_t hp[3][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int T = 2 * tp + (e >> 2);
          if (T < G::KT) fr_split3<FINITE>(P[T][e & 3], hp[0][e], hp[1][e], hp[2][e]);
          else hp[0][e] = hp[1][e] = hp[2][e] = 0u;   // no such M-tile: zeros opposite hadK's zero columns
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const u32x4 bw = {fr_top2(hp[p][0], hp[p][1]), fr_top2(hp[p][2], hp[p][3]), fr_top2(hp[p][4], hp[p][5]), fr_top2(hp[p][6], hp[p][7])};
          const fr_bf8_t b = __builtin_bit_cast(fr_bf8_t, bw);
#pragma unroll
          for (int mo = 0; mo < G::KT; ++mo)
            Y[mo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(fr_bf8_t, had_s[(mo * 2 + tp) * 64 + lane]), b, Y[mo], 0, 0, 0);
        }
      }
      // 3. lane (i, q) holds Y[16 mo + 4 q + r][16 nt + i]
#pragma unroll
      for (int mo = 0; mo < G::KT; ++mo)
        if (mo < G::KT - 1 || q < (K - 16 * (G::KT - 1)) / 4) {   // ko < K: the last tile's live rows are whole quarters (K % 4 == 0)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            *(uint16_t*)(img + (16 * mo + 4 * q + rr) * G::STRIDE + (16 * nt + i) * 2) = (uint16_t)f2h(Y[mo][rr] * c_h);
        }
    }
  };
  if (all_finite) body(Bool<true>{});
  else body(Bool<false>{});
}

// The tables every wavefront of a workgroup reads, staged once (two barriers): hadK's operands, the quantizer's bucket table, and
// the xor masks of the signs per operand and lane (`sign_s`: the sign words on their way there).
template <int K, int M>
__device__ __forceinline__ void fr_stage_tables(const FullRotArgs& r, const Lut16Args& a, const Lut16Tab& tab, uint16_t* lut, uint32_t* sign_s,
                                                u32x4* had_s, u32x4* sgn_s) {
  using G = FrGeom<K, M>;
  for (int n = threadIdx.x; n < G::KT * 2 * 64; n += kBlock) had_s[n] = ((const u32x4*)fr_had_table<K>().w)[n];
  // the sign words travel by value in the kernel arguments: a lane-indexed read is a load from the argument segment, as lut16_stage's
  if ((int)threadIdx.x < G::SIGNW) sign_s[threadIdx.x] = (int)threadIdx.x < G::C / 32 ? r.sign[threadIdx.x] : 0u;   // zero for the zero segments
  lut16_stage(lut, tab, a.shift);
  __syncthreads();
  for (int n = threadIdx.x; n < G::KT * G::KS * 64; n += kBlock) {   // the xor masks of operand n / 64 and lane n % 64
    const uint32_t sbyte = ((const uint8_t*)sign_s)[fr_col0<M>(n / 64 / G::KS, n / 64 % G::KS, n % 64) >> 3];
    u32x4 m;
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = (((sbyte >> (2 * k)) & 1u) << 15) | (((sbyte >> (2 * k + 1)) & 1u) << 31);
    sgn_s[n] = m;
  }
  __syncthreads();   // the tables and the signs (workgroup-wide, once); everything behind it is private to the wavefront
}

// The per-group tail: the stand-alone quantizer's lane code on the wavefront's row image: vector v of the row = ko v / (m / 8), chunk
// v % (m / 8).  MODE: FrMode's; ROT_MAYBE: FrTail's; code_scales, km_rows: FullRotArgs', by value (fullrot_rows_kernel's note)
template <int K, int M, FrMode MODE, bool ROT_MAYBE>
__device__ __forceinline__ void fr_quant_image(const char* img, const uint16_t* lut, int lane, int64_t row, void* __restrict__ outv,
                                               u32x4* __restrict__ rot_out, uint16_t* code_scales, uint32_t km_rows, const Lut16Args& a) {
  using G = FrGeom<K, M>;
#pragma unroll 1   // (unrolled, the passes' quantizer chains interleave and the C = 2304 code form runs out of registers)
  for (int pv = 0; pv < G::NPASS; ++pv) {
    const int v = pv * 64 + lane;
    const bool live = v < G::VPR;   // a group (16 vectors, 16 lanes) is live or dead as a whole
    const int at = live ? (v / (M / 8)) * G::STRIDE + (v % (M / 8)) * 16 : 0;
    u32x4 w = *(const u32x4*)(img + at);
    if (!live) w = u32x4{0, 0, 0, 0};
    const uint32_t m = row_max_dpp<16>(vec_absmax16(w));
    const RowScale16 s = row_scale16(m, a.fpos.gmax, a.inv_gpos);
    if constexpr (MODE == FrMode::kCodes) {
      const uint32_t codes = codes_vec16(w, lut, a.shift, s.inv, s.inv_lo);
      const uint32_t g = (uint32_t)v >> 4, l16 = (uint32_t)v & 15u, t = (uint32_t)row;
      if (live) {
        if (km_rows) {   // the k-major images (include/fpq.h), as rows16_codes_mx_kernel writes them
          if (l16 == 0) ((float*)code_scales)[(int64_t)g * ((km_rows + 3u) & ~3u) + t] = (float)__builtin_bit_cast(_Float16, (uint16_t)(s.s16x2 & 0xFFFFu));
          ((uint32_t*)outv)[(km4_off(t, g, l16 >> 2, km_rows) >> 2) + (l16 & 3u)] = codes;
        } else {
          if (l16 == 0) code_scales[row * (G::C / 128) + g] = (uint16_t)(s.s16x2 & 0xFFFFu);
          __builtin_nontemporal_store(codes, (uint32_t*)outv + row * G::VPR + v);
        }
      }
    } else {
      const u32x4 o = quant_vec16<false>(w, lut, a.shift, s.inv, s.inv_lo, s.s16x2, 0.f, 0.f, 0u);
      if (live) {
        __builtin_nontemporal_store(o, (u32x4*)outv + row * G::VPR + v);
        if constexpr (MODE == FrMode::kEmit)
          if (!ROT_MAYBE || rot_out) __builtin_nontemporal_store(w, rot_out + row * G::VPR + v);
      }
    }
  }
}
// the per-token tail (fpq_fulltoken.h)
template <int K, int M, FrMode MODE>
__device__ __forceinline__ void fr_token_image(const char* img, const uint16_t* lut, int lane, int64_t row, void* __restrict__ outv,
                                               u32x4* __restrict__ rot_out, uint16_t* code_scales, uint32_t km_rows, const Lut16Args& a);

// The plain front: the row is loaded as the operands themselves, h = half(x * smooth) (fr_load_row).  What a front owns: Raw, the
// row as load() leaves it in registers; row(), Raw -> the FrRow of h; PREFETCH, whether the next row's load() is issued under the
// tail - where Raw fits beside the quantizer's registers - or behind it; WAVES, the wavefronts per SIMD of the launch bounds.
template <int K_, int M_, typename Tin_, bool SMOOTH>
struct FrPlainFront {
  static constexpr int K = K_, M = M_, WAVES = kFrWaves;
  using Tin = Tin_;
  using Raw = FrRow<K, M>;
  // 16 registers at C = 1920; the 24 of C = 2304 spill at four wavefronts per SIMD
  static constexpr bool PREFETCH = FrGeom<K, M>::KT * FrGeom<K, M>::KS * 4 <= 16;
  __amdgpu_buffer_rsrc_t smooth;
  __device__ __forceinline__ FrPlainFront(const FullRotArgs& r) : smooth(rq_rsrc(r.smooth, SMOOTH ? K * M * 4 : 0)) {}
  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t src, int lane, Raw& x) const { fr_load_row<K, M, Tin, SMOOTH>(src, smooth, lane, x); }
  __device__ __forceinline__ const FrRow<K, M>& row(const Raw& x, int64_t, int) const { return x; }
};

// THE row loop of every full-width producer.  FrontArgs: the kernel arguments of the front beside FullRotArgs (none, or
// FullAdalnArgs), given explicitly at the instantiation.  Four things keep the machine code what separate kernels had (DESIGN.md
// 4g): the loop is the __global__ function itself, not a device function under per-family wrappers; a front without arguments
// has NO parameter, not an empty one; the tail is called here, not through a member of the tag; and it takes the two fields of
// FullRotArgs it reads by value, not the block by reference.
template <typename Front, typename Tail, typename... FrontArgs>
__global__ __launch_bounds__(kBlock, Front::WAVES) void fullrot_rows_kernel(const void* __restrict__ xv, void* __restrict__ outv,
                                                                        u32x4* __restrict__ rot_out, int64_t rows, FullRotArgs r,
                                                                        FrontArgs... fa, Lut16Args a, Lut16Tab tab) {
  constexpr int K = Front::K, M = Front::M;
  using G = FrGeom<K, M>;
  using Tin = typename Front::Tin;
  __shared__ __attribute__((aligned(16))) uint16_t lut[kLutLdsEntries];
  __shared__ __attribute__((aligned(16))) char img_s[kBlock / 64][G::IMG];
  __shared__ uint32_t sign_s[G::SIGNW];
  __shared__ u32x4 had_s[G::KT * 2 * 64];
  __shared__ u32x4 sgn_s[G::KT * G::KS * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t step = (int64_t)gridDim.x * (kBlock / 64);
  int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + wave;
  const Front front(r, fa...);
  auto row_rsrc = [&](int64_t t) { return rq_rsrc((const char*)xv + t * (G::C * (int64_t)sizeof(Tin)), G::C * (int)sizeof(Tin)); };
  constexpr bool PREFETCH = Front::PREFETCH;
  typename Front::Raw x;
  if (row < rows) front.load(row_rsrc(row), lane, x);   // in flight while the tables are staged
  fr_stage_tables<K, M>(r, a, tab, lut, sign_s, had_s, sgn_s);
  char* img = img_s[wave];
  const FrLane lc = fr_lane_consts(lane);
  while (row < rows) {
    fullrot_transform_row<K, M>(front.row(x, row, lane), sgn_s, had_s, lc, r.c_h, img, lane);
    __builtin_amdgcn_wave_barrier();
    const int64_t next = row + step;
    if (PREFETCH && next < rows) front.load(row_rsrc(next), lane, x);   // in flight under the quantizer
    if constexpr (Tail::TOKEN) fr_token_image<K, M, Tail::MODE>(img, lut, lane, row, outv, rot_out, r.code_scales, r.km_rows, a);
    else fr_quant_image<K, M, Tail::MODE, Tail::ROT_MAYBE>(img, lut, lane, row, outv, rot_out, r.code_scales, r.km_rows, a);
    __builtin_amdgcn_wave_barrier();   // the image is rewritten by the next row
    row = next;
    if (!PREFETCH && row < rows) front.load(row_rsrc(row), lane, x);
  }
}

// ---- the host side (fpq_fullrot_launch.h) ----
// Persistent wavefronts, one row each at a time: the grid is what the chip holds resident - kFrCUs x kFrWaves workgroups of 4
// wavefronts (the launch bounds' occupancy; LDS: 4 row images + the table, ~25 KiB per workgroup) - or one wavefront per row.
inline int fullrot_grid(int64_t rows) { return grid_for((rows + kBlock / 64 - 1) / (kBlock / 64), (int64_t)kFrCUs * kFrWaves); }

inline bool fullrot_width_built(int64_t cols) {
  for (int c : kFullRotWidths)
    if (cols == c) return true;
  return false;
}

inline FullRotArgs fullrot_args(int cols, int64_t rows, const float* smooth, const uint32_t* sign_words, uint16_t* code_scales, bool km) {
  FullRotArgs r;
  r.smooth = smooth;
  r.code_scales = code_scales;
  r.km_rows = km ? (uint32_t)rows : 0u;
  r.c_h = h2f(f2h(1.0f / __builtin_sqrtf((float)cols)));   // torch.tensor(C).sqrt() is float32; autocast makes Q fp16
  for (int i = 0; i < kFrMaxSignWords; ++i) r.sign[i] = i < cols / 32 ? sign_words[i] : 0u;
  return r;
}
