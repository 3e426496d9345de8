// fpq_codes_g6.h - the operand-emitting quantizer of the A6W4 GEMM (fpq_gemm_g6.h): per-group(128) quantization on the E1M2 or
// E3M0 table straight to dense 6-bit hardware codes (E1M2 levels as FP6 E2M3 codes, E3M0 levels as BF6 E3M2 codes) + one scale per
// group.  Included by fpq_kernels.hip only, behind fpq_codes_fp8.h (codes8_vec16); the code tables: lut16_codes_g6, fpq_fast16.h.
#pragma once

// Fast form for fp16 rows: rows16_codes_mx_kernel's shape - 16 lanes own a group, a lane 8 elements - with 6-bit codes as the
// bucket table's entries.  A lane's 8 codes are 48 bits and a group leaves 96 bytes: the four lanes of a quad hold one 24-byte
// k-block between them, lane q takes what its right-hand neighbour holds (one quad_perm DPP move per half) and lanes 0 .. 2 of
// the quad store bytes 8q .. 8q + 7 of the block: twelve 8-byte stores per group, 96 contiguous bytes per 16 lanes.
__global__ __launch_bounds__(kBlock) void group6_emit16_kernel(const u32x4* __restrict__ x, uint8_t* __restrict__ codes,
                                                              uint16_t* __restrict__ scales, int64_t n_vec, Lut16Args a, Lut16Tab tab) {
  __shared__ __attribute__((aligned(16))) uint16_t lut[kLutLdsEntries];   // static: a compile-time LDS address
  {
    lut16_stage(lut, tab, a.shift);
    __syncthreads();
  }
  const uint32_t q = threadIdx.x & 3u;
  // (n_vec % 16 == 0 and the grid stride is a multiple of 16: whole 16-lane clusters enter or leave the loop together)
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n_vec; v += (int64_t)gridDim.x * kBlock) {
    const u32x4 w = __builtin_nontemporal_load(x + v);
    const uint32_t m = row_max_dpp<16>(vec_absmax16(w));
    const RowScale16 s = row_scale16(m, a.fpos.gmax, a.inv_gpos);
    if ((threadIdx.x & 15) == 0) scales[v >> 4] = (uint16_t)(s.s16x2 & 0xFFFFu);
    uint32_t lo4, hi4;                         // eight 6-bit codes, one per byte
    codes8_vec16(w, lut, a.shift, s.inv, s.inv_lo, lo4, hi4);
    const uint32_t p_lo = (lo4 & 0x3Fu) | ((lo4 >> 2) & 0xFC0u) | ((lo4 >> 4) & 0x3F000u) | ((lo4 >> 6) & 0xFC0000u);   // codes 0 .. 3: 24 bits
    const uint32_t p_hi = (hi4 & 0x3Fu) | ((hi4 >> 2) & 0xFC0u) | ((hi4 >> 4) & 0x3F000u) | ((hi4 >> 6) & 0xFC0000u);   // codes 4 .. 7
    const uint32_t n_lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p_lo, 0x39, 0xF, 0xF, true);   // quad_perm [1,2,3,0]: the next lane's
    const uint32_t n_hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p_hi, 0x39, 0xF, 0xF, true);
    const uint64_t p48 = (uint64_t)p_lo | ((uint64_t)p_hi << 24), n48 = (uint64_t)n_lo | ((uint64_t)n_hi << 24);
    // the block's 192-bit string = p48 of lanes 0 .. 3 at bits 48q: word q (64 bits) = this lane's bits from 16q up, then the next lane's
    const uint64_t word = (p48 >> (16u * q)) | (n48 << (48u - 16u * q));
    if (q < 3u) __builtin_nontemporal_store(u32x2{(uint32_t)word, (uint32_t)(word >> 32)}, (u32x2*)(codes + (v >> 2) * 24 + q * 8u));
  }
}

// The same emitter writing the A6W4 GEMM's K-MAJOR IMAGES (include/fpq.h; a kernel of its own, so that the row-major one keeps its
// code): the activation side's 6-bit image [G][rows][96] - km6_off places a group's 16-byte chunks in the rotated order of the
// GEMM's LDS image - and the fp32 scale image [G][rows rounded up to 4] (padding rows are not written).  Same arithmetic, the same
// twelve 8-byte stores per group.  A workgroup's 256 vectors are ONE group of 16 consecutive rows, as in rows16_codes_mx_kernel's
// k-major form: what it writes is 1.5 KiB in a row (12 whole lines) inside the group's plane; unit u = row block u / G, group u % G.
__global__ __launch_bounds__(kBlock) void group6_km_emit16_kernel(const u32x4* __restrict__ x, uint8_t* __restrict__ image,
                                                                 float* __restrict__ scale_image, Lut16Args a, Lut16Tab tab,
                                                                 uint32_t km_rows, FastDiv km_gpr) {
  __shared__ __attribute__((aligned(16))) uint16_t lut[kLutLdsEntries];   // static: a compile-time LDS address
  {
    lut16_stage(lut, tab, a.shift);
    __syncthreads();
  }
  const uint32_t G = km_gpr.d, lane16 = threadIdx.x & 15u, row_in = threadIdx.x >> 4, q = threadIdx.x & 3u;
  const uint32_t rows4 = (km_rows + 3u) & ~3u, units = ((km_rows + 15u) >> 4) * G;
  for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
    const uint32_t rb = fast_div_q(u, km_gpr), g = u - rb * G, t = rb * 16u + row_in;
    if (t >= km_rows) continue;   // whole 16-lane clusters drop out
    const u32x4 w = __builtin_nontemporal_load(x + ((int64_t)t * G + g) * 16 + lane16);
    const uint32_t m = row_max_dpp<16>(vec_absmax16(w));
    const RowScale16 s = row_scale16(m, a.fpos.gmax, a.inv_gpos);
    if (lane16 == 0) scale_image[(int64_t)g * rows4 + t] = (float)__builtin_bit_cast(_Float16, (uint16_t)(s.s16x2 & 0xFFFFu));
    uint32_t lo4, hi4;                         // eight 6-bit codes, one per byte
    codes8_vec16(w, lut, a.shift, s.inv, s.inv_lo, lo4, hi4);
    const uint32_t p_lo = (lo4 & 0x3Fu) | ((lo4 >> 2) & 0xFC0u) | ((lo4 >> 4) & 0x3F000u) | ((lo4 >> 6) & 0xFC0000u);   // codes 0 .. 3: 24 bits
    const uint32_t p_hi = (hi4 & 0x3Fu) | ((hi4 >> 2) & 0xFC0u) | ((hi4 >> 4) & 0x3F000u) | ((hi4 >> 6) & 0xFC0000u);   // codes 4 .. 7
    const uint32_t n_lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p_lo, 0x39, 0xF, 0xF, true);   // quad_perm [1,2,3,0]: the next lane's
    const uint32_t n_hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p_hi, 0x39, 0xF, 0xF, true);
    const uint64_t p48 = (uint64_t)p_lo | ((uint64_t)p_hi << 24), n48 = (uint64_t)n_lo | ((uint64_t)n_hi << 24);
    const uint64_t word = (p48 >> (16u * q)) | (n48 << (48u - 16u * q));   // (group6_emit16_kernel)
    // the quad's k-block lane16 >> 2 = bytes 24 (lane16 >> 2) .. + 23 of the group's 96; this lane's 8 of them never straddle a chunk
    // (plain stores: the workgroup's sixteen rows fill whole lines between them - L2 has to be allowed to merge them)
    const uint32_t wb = 24u * (lane16 >> 2) + 8u * q;
    if (q < 3u) *(u32x2*)(image + km6_off(t, g, wb >> 4, km_rows) + (wb & 15u)) = u32x2{(uint32_t)word, (uint32_t)(word >> 32)};
  }
}

// Generic form (fp32 rows: weights, the residual stream): four lanes own a group, a lane one 32-element k-block (24 bytes
// out); the arithmetic of codes128_kernel.  BF6: the codes of E3M0 levels in E3M2, else of E1M2 levels in E2M3.
template <typename Tin, bool BF6>
__global__ __launch_bounds__(kBlock) void group6_emit_kernel(const u32x4* __restrict__ x, uint8_t* __restrict__ codes,
                                                            Tin* __restrict__ scales, int64_t n_blk, Fmt fs) {
  constexpr int V = DT<Tin>::kVec, NV = 32 / V;
  // (n_blk % 4 == 0: the four lanes of a group enter or leave the loop together)
  for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < n_blk; b += (int64_t)gridDim.x * kBlock) {
    float xf[32];
    uint32_t m = 0;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const u32x4 raw = __builtin_nontemporal_load(x + b * NV + v);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        xf[v * V + i] = DT<Tin>::get(raw, i);
        const uint32_t ab = DT<Tin>::absbits(xf[v * V + i]);
        m = m > ab ? m : ab;
      }
    }
    m = lanes_max<4>(m);
    const float s = scale_of<Tin>(m, fs.gmax);
    if ((threadIdx.x & 3) == 0) store_scalar<Tin>(scales + (b >> 2), s);
    uint32_t o[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const float xn = DT<Tin>::round(xf[j] / s);
      const uint32_t neg = (xn < 0.0f) ? 1u : 0u;
      const float qm = quant_mag(fabsf(xn), neg, fs);
      const float lv = (neg && qm != 0.0f) ? -qm : qm;
      const uint32_t code = BF6 ? e3m2_of_level(lv) : e2m3_of_level(lv);
      const int bit = 6 * j;
      o[bit >> 5] |= code << (bit & 31);
      if ((bit & 31) > 26) o[(bit >> 5) + 1] |= code >> (32 - (bit & 31));
    }
    u32x2* dst = (u32x2*)(codes + b * 24);
    dst[0] = u32x2{o[0], o[1]};
    dst[1] = u32x2{o[2], o[3]};
    dst[2] = u32x2{o[4], o[5]};
  }
}
