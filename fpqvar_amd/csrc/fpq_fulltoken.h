// fpq_fulltoken.h - the PER-TOKEN quantizer tail of the full-width rotation (W6A6: per-token E2M3 / E3M2 activations): the second
// tail beside fr_quant_image on the wavefront's row image, run by fullrot_rows_kernel (fpq_fullrot.h) under FrTail<true, ..> behind
// either front.  Included by fpq_fulltoken.hip after fpq_fullrot.h and fpq_fulladaln.h.
//
// When the transform returns, the rotated fp16 row y sits complete in the wavefront's LDS image, so ONE scale per row costs no
// second pass over memory:
//   1. The row maximum: every lane reads its vector v = 64 pass + lane of every pass (NPASS = 4 at C = 1920, 5 at 2304) and keeps
//      the largest |pattern| (vec_absmax16); the dead vectors v >= VPR of the last pass (16 lanes at 1920, 32 at 2304) read
//      nothing and contribute zero; row_max_dpp<64> joins the lanes.  row_scale16 makes the scale and its reciprocal exactly as
//      rows16_lut_wave_kernel / rows16_codes6_wave_kernel do: an all-zero row, a row with an inf and a row with a NaN come out as
//      the stand-alone per-token quantizer's on the same y.
//   2. The second walk over the image, one 16-byte vector per lane and pass in row order, runs that quantizer's lane code with the
//      row's scale.  kValues: quant_vec16 on the level table -> fp16 values (and y itself where `rot_out` is given).  kCodes:
//      the 8 codes of the vector from the 6-bit code table (lut16_codes6: E2M3 or E3M2) as 48 bits; the four lanes of a quad
//      own one 32-element block = 24 contiguous bytes of the row, and lane q of the quad takes the (3 - q) upper 16-bit words of
//      its own string and the q + 1 lower words of its right neighbour's (one quad_perm DPP move each half), so lanes 0 .. 2 store 8
//      aligned bytes each - the byte string rows16_codes6_wave_kernel packs per block, at the same place: row-major behind the
//      row's start, or (k-major, include/fpq.h) bytes 24 (b % 4) + 8 q of K step b / 4 at km6_off.  VPR % 4 == 0: a quad is
//      live or dead as a whole.
// The image walk (vector -> image address, live / dead) is fr_quant_image's; what differs is one maximum for the row instead
// of one per 16 lanes, and the 6-bit store.
#pragma once

// the image address of vector v of the row (fr_quant_image's): image row v / (m / 8), chunk v % (m / 8)
template <int K, int M>
__device__ __forceinline__ int fr_image_at(int v) { return (v / (M / 8)) * FrGeom<K, M>::STRIDE + (v % (M / 8)) * 16; }

// kValues: values out (`rot_out`: the rotated rows too, or null); kCodes: dense 6-bit operand codes (`outv`: row-major [rows][C * 3 / 4]
// or the k-major image of km_rows rows; `lut` staged from the code table).  code_scales: the row scales (fp16 [rows]; kValues: or null)
template <int K, int M, FrMode MODE>
__device__ __forceinline__ void fr_token_image(const char* img, const uint16_t* lut, int lane, int64_t row, void* __restrict__ outv,
                                               u32x4* __restrict__ rot_out, uint16_t* code_scales, uint32_t km_rows, const Lut16Args& a) {
  using G = FrGeom<K, M>;
  static_assert(G::VPR % 4 == 0, "a quad of lanes is live or dead as a whole");
  uint32_t m = 0;
#pragma unroll 1   // (unrolled, the passes' lane-constant image addresses are hoisted out of the row loop: two forms spill 1 - 4 registers)
  for (int pv = 0; pv < G::NPASS; ++pv) {
    const int v = pv * 64 + lane;
    const bool live = v < G::VPR;
    u32x4 w = *(const u32x4*)(img + (live ? fr_image_at<K, M>(v) : 0));
    if (!live) w = u32x4{0, 0, 0, 0};
    const uint32_t t = vec_absmax16(w);
    m = m > t ? m : t;
  }
  m = row_max_dpp<64>(m);
  const RowScale16 s = row_scale16(m, a.fpos.gmax, a.inv_gpos);
  if ((MODE == FrMode::kCodes || code_scales) && lane == 0) code_scales[row] = (uint16_t)(s.s16x2 & 0xFFFFu);
#pragma unroll 1   // (as fr_quant_image's: unrolled, the passes' quantizer chains interleave and cost registers)
  for (int pv = 0; pv < G::NPASS; ++pv) {
    const int v = pv * 64 + lane;
    const bool live = v < G::VPR;
    u32x4 w = *(const u32x4*)(img + (live ? fr_image_at<K, M>(v) : 0));
    if (!live) w = u32x4{0, 0, 0, 0};
    if constexpr (MODE == FrMode::kCodes) {
      uint32_t lo4, hi4;   // eight 6-bit codes, one per byte
      codes8_vec16(w, lut, a.shift, s.inv, s.inv_lo, lo4, hi4);
      const uint64_t own = (uint64_t)((lo4 & 0x3Fu) | ((lo4 >> 2) & 0xFC0u) | ((lo4 >> 4) & 0x3F000u) | ((lo4 >> 6) & 0xFC0000u)) |
                           ((uint64_t)((hi4 & 0x3Fu) | ((hi4 >> 2) & 0xFC0u) | ((hi4 >> 4) & 0x3F000u) | ((hi4 >> 6) & 0xFC0000u)) << 24);
      const uint32_t nlo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)own, 0xF9, 0xF, 0xF, false);   // quad_perm [1,2,3,3]
      const uint32_t nhi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(own >> 32), 0xF9, 0xF, 0xF, false);
      const uint64_t nb = ((uint64_t)nhi << 32) | nlo;
      const uint32_t qp = (uint32_t)v & 3u, b = (uint32_t)v >> 2, sr = 16u * qp;
      const uint64_t w6 = (own >> sr) | (nb << (48u - sr));
      if (live && qp < 3u) {
        const u32x2 o2 = {(uint32_t)w6, (uint32_t)(w6 >> 32)};
        if (km_rows) {   // plain stores: the rows of a workgroup fill whole lines of a plane between them (fpq_codes_fp6.h)
          const uint32_t wb = 24u * (b & 3u) + 8u * qp;
          *(u32x2*)((uint8_t*)outv + km6_off((uint32_t)row, b >> 2, wb >> 4, km_rows) + (wb & 15u)) = o2;
        } else {
          __builtin_nontemporal_store(o2, (u32x2*)((uint8_t*)outv + row * (G::C / 4 * 3) + 24u * b + 8u * qp));
        }
      }
    } else {
      const u32x4 o = quant_vec16<false>(w, lut, a.shift, s.inv, s.inv_lo, s.s16x2, 0.f, 0.f, 0u);
      if (live) {
        __builtin_nontemporal_store(o, (u32x4*)outv + row * G::VPR + v);
        if (rot_out) __builtin_nontemporal_store(w, rot_out + row * G::VPR + v);
      }
    }
  }
}
