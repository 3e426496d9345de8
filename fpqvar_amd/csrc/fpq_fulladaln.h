// fpq_fulladaln.h - the adaLN FRONT of the full-width producers: LayerNorm + modulate in front of fpq_fullrot.h's rotation, one launch:
//     h = half( ((LayerNorm(x) * half(scale + 1)) + shift) * smooth ),  y = half(c_h * h . diag(D) . H_C^T),  out = per-group quant(y)
// (tr/basic_var.py:263,266 in the reference's `--rotate` without `--block_rotate`).  Included by fpq_fulladaln.hip and fpq_fulltoken.hip
// after fpq_adaln.h (wave_sum_dpp) and fpq_fullrot.h.
//
// FrAdalnFront is what fullrot_rows_kernel (fpq_fullrot.h) runs in front of fullrot_transform_row in place of FrPlainFront:
//   1. The RAW row is loaded in the FrRow operand layout (fr_col0: 8 consecutive channels per lane and operand (T, s), a buffer
//      resource of one row: the segments kj >= K read zeros) - 16 registers per lane for fp16 rows of 1920, 48 for fp32 rows of 2304.
//   2. The statistics of the raw x in fp32, ALWAYS centred (the row is in registers: the second pass costs no memory traffic, so
//      there is no one-pass branch and no switch point): one accumulator per operand, 8 sequential additions each (fp16 rows: 4
//      v_dot2_f32_f16), the KT KS accumulators joined in turn, wave_sum_dpp's 6 levels; mean = sum * fl(1 / C); then the same
//      for (x - mean)^2 with one fma per element.  The zero segments add exact zeros to the sum; their (0 - mean)^2 is thrown away
//      per accumulator (an operand of the last M-tile is live or padding as a whole per lane) and the divisor is C, not the
//      padded length.  rstd = v_rsq_f32 + one Newton step, as adaln_mfma_kernel's.
//   3. The modulate with adaln_mfma_kernel's arithmetic: A = fl(half_or_float(scale + 1) s), B = fl(shift s) (fp16 modulation adds
//      the 1 in fp16), nm = -mean rstd, h = half(fma(fma(x, rstd, nm), A, B)).  scale / shift are read PER ROW at the lane's own
//      columns of the row's batch entry (a wavefront's consecutive rows are gridDim x 4 apart, so the batch entry changes from row
//      to row; [batches, C] stays in L2).  `smooth` is a run-time select: s = 1 is exact in both products, and a template
//      parameter would double the 24 kernels for the sake of 8 multiplies per operand.  Each operand's 8 (fp32 rows: 16) raw
//      registers die as its 4 registers of h are made; the padding segments are set to zero, so fullrot_transform_row sees
//      exactly what fr_load_row would have loaded from h: rotated and out are rotate_quant_full(h)'s bit for bit.
//   4. The rest of the row loop - fullrot_transform_row, then the tail - is the one text every front shares.
// tests/fulladaln_model.py carries the bound on h (depth 8 + KT KS - 1 + 6 additions) and a model of this arithmetic in source order.
#pragma once

// a raw row of at most this many registers per lane is prefetched under the quantizer: fp16 rows of 1920, as FrPlainFront's
// (at 32 - fp32 rows of 1920, fp16 rows of 2304 - each of the 12 forms it adds spills 1 - 22 registers at four wavefronts per SIMD)
constexpr int kFaPrefetchRegs = 16;

// A raw row as it is loaded: the 8 channels of lane (i, q) and operand (T, s) in one (fp16 rows) or two (fp32) 16-byte vectors
template <int K, int M, typename Tin>
struct FaRaw {
  static constexpr int W = sizeof(Tin) / 2;
  u32x4 w[FrGeom<K, M>::KT][FrGeom<K, M>::KS][W];
};

template <int K, int M, typename Tin>
__device__ __forceinline__ void fa_load_raw(__amdgpu_buffer_rsrc_t src, int lane, FaRaw<K, M, Tin>& x) {
  using G = FrGeom<K, M>;
#pragma unroll
  for (int T = 0; T < G::KT; ++T)
#pragma unroll
    for (int s = 0; s < G::KS; ++s)
#pragma unroll
      for (int v = 0; v < FaRaw<K, M, Tin>::W; ++v)
        x.w[T][s][v] = __builtin_amdgcn_raw_buffer_load_b128(src, fr_col0<M>(T, s, lane) * (int)sizeof(Tin) + 16 * v, 0, kRqNt);
}

// element k (0 .. 7) of an operand as fp32 (fp16 rows: the widening is exact)
template <typename Tin>
__device__ __forceinline__ float fa_elem(const u32x4* w, int k) {
  if constexpr (sizeof(Tin) == 2) return h2f((k & 1) ? (w[0][k >> 1] >> 16) : (w[0][k >> 1] & 0xFFFFu));
  else return u2f(w[k >> 2][k & 3]);
}

// mean and the biased variance of the C live channels -> rstd = 1 / sqrt(var + eps), nm = -mean rstd
template <int K, int M, typename Tin>
__device__ __forceinline__ void fa_stats(const FaRaw<K, M, Tin>& x, int lane, float eps, float& rstd, float& nm) {
  using G = FrGeom<K, M>;
  constexpr float inv_c = 1.0f / (float)G::C;
  const bool last_live = (lane & 15) < K - 16 * (G::KT - 1);   // this lane's segment of the last M-tile is part of the row
  float sum = 0.0f;
#pragma unroll
  for (int T = 0; T < G::KT; ++T)
#pragma unroll
    for (int s = 0; s < G::KS; ++s) {
      float a1 = 0.0f;
      if constexpr (sizeof(Tin) == 2) {
        const h2v_t ones = {(_Float16)1.0f, (_Float16)1.0f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t xw = x.w[T][s][0][k];   // (a copy: __builtin_bit_cast of the vector element itself reads element 0 for every k)
          a1 = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2v_t, xw), ones, a1, false);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) a1 += fa_elem<Tin>(x.w[T][s], k);
      }
      sum = (T == 0 && s == 0) ? a1 : sum + a1;
    }
  const float mean = wave_sum_dpp(sum) * inv_c;
  float s2 = 0.0f;
#pragma unroll
  for (int T = 0; T < G::KT; ++T)
#pragma unroll
    for (int s = 0; s < G::KS; ++s) {
      float a2 = 0.0f;
      if constexpr (sizeof(Tin) == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float d0 = fmaf_h_lo(x.w[T][s][0][k], 1.0f, -mean), d1 = fmaf_h_hi(x.w[T][s][0][k], 1.0f, -mean);
          a2 = __builtin_fmaf(d1, d1, __builtin_fmaf(d0, d0, a2));
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d0 = fa_elem<Tin>(x.w[T][s], k) - mean;
          a2 = __builtin_fmaf(d0, d0, a2);
        }
      }
      if (T == G::KT - 1 && !last_live) a2 = 0.0f;   // the zero padding is not part of the row
      s2 = (T == 0 && s == 0) ? a2 : s2 + a2;
    }
  const float var = wave_sum_dpp(s2) * inv_c;
  const float ve = var + eps;
  rstd = __builtin_amdgcn_rsqf(ve);
  rstd = __builtin_fmaf(rstd * __builtin_fmaf(-ve * rstd, rstd, 1.0f), 0.5f, rstd);
  nm = -mean * rstd;
}

// h of one row from its raw registers; `sc`, `sh`: buffer resources of the batch entry's C modulation values, `smooth` of the C
// floats (has_smooth) ; `h_dst`: of the row of h_out (EMIT; no bytes when h is not asked for: the stores are dropped)
template <int K, int M, typename Tin, typename Tmod, bool EMIT>
__device__ __forceinline__ void fa_modulate(const FaRaw<K, M, Tin>& x, float rstd, float nm, __amdgpu_buffer_rsrc_t sc, __amdgpu_buffer_rsrc_t sh,
                                            __amdgpu_buffer_rsrc_t smooth, bool has_smooth, __amdgpu_buffer_rsrc_t h_dst, int lane,
                                            FrRow<K, M>& h) {
  using G = FrGeom<K, M>;
  const bool last_live = (lane & 15) < K - 16 * (G::KT - 1);
#pragma unroll
  for (int T = 0; T < G::KT; ++T)
#pragma unroll
    for (int s = 0; s < G::KS; ++s) {
      const int col0 = fr_col0<M>(T, s, lane);
      float sm[8], A[8], B[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) sm[k] = 1.0f;
      if (has_smooth) {
        const u32x4 sa = __builtin_amdgcn_raw_buffer_load_b128(smooth, col0 * 4, 0, 0), sb = __builtin_amdgcn_raw_buffer_load_b128(smooth, col0 * 4 + 16, 0, 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          sm[k] = u2f(sa[k]);
          sm[4 + k] = u2f(sb[k]);
        }
      }
      if constexpr (sizeof(Tmod) == 2) {   // scale.add(1) is an fp16 op in the reference; the widening rides on the product with s
        const u32x4 ws = __builtin_amdgcn_raw_buffer_load_b128(sc, col0 * 2, 0, 0), wh = __builtin_amdgcn_raw_buffer_load_b128(sh, col0 * 2, 0, 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t s1p = pk_add_f16(ws[k], 0x3C003C00u);
          A[2 * k] = fmaf_h_lo(s1p, sm[2 * k], -0.0f);
          A[2 * k + 1] = fmaf_h_hi(s1p, sm[2 * k + 1], -0.0f);
          B[2 * k] = fmaf_h_lo(wh[k], sm[2 * k], -0.0f);
          B[2 * k + 1] = fmaf_h_hi(wh[k], sm[2 * k + 1], -0.0f);
        }
      } else {
        const u32x4 a0 = __builtin_amdgcn_raw_buffer_load_b128(sc, col0 * 4, 0, 0), a1 = __builtin_amdgcn_raw_buffer_load_b128(sc, col0 * 4 + 16, 0, 0);
        const u32x4 b0 = __builtin_amdgcn_raw_buffer_load_b128(sh, col0 * 4, 0, 0), b1 = __builtin_amdgcn_raw_buffer_load_b128(sh, col0 * 4 + 16, 0, 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          A[k] = (u2f(a0[k]) + 1.0f) * sm[k];
          A[4 + k] = (u2f(a1[k]) + 1.0f) * sm[4 + k];
          B[k] = u2f(b0[k]) * sm[k];
          B[4 + k] = u2f(b1[k]) * sm[4 + k];
        }
      }
      u32x4 hw;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float t0, t1;
        if constexpr (sizeof(Tin) == 2) {
          t0 = fmaf_h_lo(x.w[T][s][0][k], rstd, nm);
          t1 = fmaf_h_hi(x.w[T][s][0][k], rstd, nm);
        } else {
          t0 = __builtin_fmaf(fa_elem<Tin>(x.w[T][s], 2 * k), rstd, nm);
          t1 = __builtin_fmaf(fa_elem<Tin>(x.w[T][s], 2 * k + 1), rstd, nm);
        }
        hw[k] = f2h2(__builtin_fmaf(t0, A[2 * k], B[2 * k]), __builtin_fmaf(t1, A[2 * k + 1], B[2 * k + 1]));
      }
      if (T == G::KT - 1 && !last_live) hw = u32x4{0, 0, 0, 0};   // the zero segments kj >= K, as fr_load_row reads them
      if constexpr (EMIT) __builtin_amdgcn_raw_buffer_store_b128(hw, h_dst, col0 * 2, 0, kRqNt);   // beyond the row: dropped
      h.w[T][s] = hw;
    }
}

// Wavefronts per SIMD the launch bounds ask for: the plain front's four, but three where 48 raw registers (fp32 rows of 2304) meet
// 32 of modulation loads per operand (fp32 scale, shift and smooth): that one form spills 4 - 6 registers at four.
template <int K, int M, typename Tin, typename Tmod>
constexpr int kFaWaves = (FrGeom<K, M>::KT * FrGeom<K, M>::KS * 4 * (int)sizeof(Tin) / 2 > 32 && sizeof(Tmod) == 4) ? 3 : kFrWaves;

// The adaLN front of fullrot_rows_kernel (FrPlainFront's members).  EMIT: the tail's (FrTail::EMIT) - h goes out where ad.h_out is
// given; no bytes behind a null pointer: the stores are dropped
template <int K_, int M_, typename Tin_, typename Tmod, bool EMIT>
struct FrAdalnFront {
  static constexpr int K = K_, M = M_, WAVES = kFaWaves<K, M, Tin_, Tmod>;
  using G = FrGeom<K, M>;
  using Tin = Tin_;
  using Raw = FaRaw<K, M, Tin>;
  static constexpr bool PREFETCH = G::KT * G::KS * 4 * Raw::W <= kFaPrefetchRegs;   // the census: profiles/adaln_full_ab.txt
  const FullAdalnArgs& ad;
  bool has_smooth;
  __amdgpu_buffer_rsrc_t smooth;
  __device__ __forceinline__ FrAdalnFront(const FullRotArgs& r, const FullAdalnArgs& ad_)
      : ad(ad_), has_smooth(r.smooth != nullptr), smooth(rq_rsrc(r.smooth, r.smooth != nullptr ? G::C * 4 : 0)) {}
  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t src, int lane, Raw& x) const { fa_load_raw<K, M, Tin>(src, lane, x); }
  __device__ __forceinline__ FrRow<K, M> row(const Raw& x, int64_t row, int lane) const {
    const uint32_t b = (uint32_t)row / ad.rows_per_batch;   // rows < 2^31
    const int64_t mod_at = (int64_t)b * (G::C * (int64_t)sizeof(Tmod));
    const bool emit_h = EMIT && ad.h_out != nullptr;
    FrRow<K, M> h;
    float rstd, nm;
    fa_stats<K, M, Tin>(x, lane, ad.eps, rstd, nm);
    fa_modulate<K, M, Tin, Tmod, EMIT>(x, rstd, nm, rq_rsrc((const char*)ad.scale + mod_at, G::C * (int)sizeof(Tmod)),
                                       rq_rsrc((const char*)ad.shift + mod_at, G::C * (int)sizeof(Tmod)), smooth, has_smooth,
                                       rq_rsrc(emit_h ? ad.h_out + row * G::C : nullptr, emit_h ? G::C * 2 : 0), lane, h);
    return h;
  }
};

