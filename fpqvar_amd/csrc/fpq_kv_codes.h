// fpq_kv_codes.h - the producer of the packed KV cache (include/fpq.h, fpq_kv_pack): fresh fp16 k / v rows quantized straight
// into code slots - E2M3 rows of 64 (one head) or E2M1 groups of 128 (two heads).  The decisions are fpq_kv_cache_step's: the
// same lanes-per-row form (kv16_step_kernel: 8 or 16 lanes, one 16-byte vector each), the same row maximum and scale
// (row_scale16) and the same bucket table index per element, with the code tables the GEMM operand producers use
// (rows16_codes6_wave_kernel, rows16_codes_mx_kernel) in place of the level table.  Included by fpq_kernels.hip only.
#pragma once

struct KvPackArgs {
  const uint16_t* src[2];             // new k, new v: [batch, n_new, row_elems], rows contiguous
  int64_t src_batch_pitch, src_token_pitch;   // in elements
  uint8_t* codes;                     // [2, batch, max_len, heads, row_bytes]
  uint16_t* scales;                   // [2, batch, max_len, heads] (E2M3) or [2, batch, max_len, heads / 2] (E2M1)
  int64_t codes_slab, scales_slab;    // bytes / scales of one (K or V) slab
  int64_t max_len, pos;
  int64_t new_vecs;                   // 16-byte vectors of one batch entry's new rows = n_new * row_vec
  int row_vec;                        // vectors per token row = heads * 8
};

// grid: x = tiles of kBlock * U vectors, y = batch entry, z = k / v
template <int BITS, int U>
__global__ __launch_bounds__(kBlock) void kv_pack_kernel(KvPackArgs k, Lut16Args a, Lut16Tab tab) {
  __shared__ __attribute__((aligned(16))) uint16_t lut[kLutLdsEntries];   // static: a compile-time LDS address
  constexpr int LPR = BITS == 6 ? 8 : 16;                               // lanes per scale group (64 or 128 halves)
  const int z = blockIdx.z, b = blockIdx.y;
  const uint16_t* s = k.src[z] + (int64_t)b * k.src_batch_pitch;
  const int64_t v0 = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
  u32x4 raw[U];
  bool live[U];
  int64_t tok[U];                     // row of the [batch, max_len] slab this vector lands in
  int c[U];                           // vector in the token row
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t v = v0 + u * kBlock;
    live[u] = v < k.new_vecs;         // new_vecs is a multiple of LPR: a group is live or dead as a whole
    const int64_t l = live[u] ? v / k.row_vec : 0;
    c[u] = live[u] ? (int)(v - l * k.row_vec) : 0;
    tok[u] = (int64_t)b * k.max_len + k.pos + l;
    raw[u] = live[u] ? *(const u32x4*)(s + l * k.src_token_pitch + c[u] * 8) : u32x4{0, 0, 0, 0};
  }
  {
    lut16_stage(lut, tab, a.shift);
    __syncthreads();
  }
  uint8_t* codes = k.codes + z * k.codes_slab;
  uint16_t* scales = k.scales + z * k.scales_slab;
  const int heads = k.row_vec >> 3;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t m = row_max_dpp<LPR>(vec_absmax16(raw[u]));
    const RowScale16 sc = row_scale16(m, a.fpos.gmax, a.inv_gpos);
    if constexpr (BITS == 6) {
      uint32_t lo4, hi4;              // eight 6-bit codes, one per byte
      codes8_vec16(raw[u], lut, a.shift, sc.inv, sc.inv_lo, lo4, hi4);
      const uint32_t c24lo = (lo4 & 0x3Fu) | ((lo4 >> 2) & 0xFC0u) | ((lo4 >> 4) & 0x3F000u) | ((lo4 >> 6) & 0xFC0000u);
      const uint32_t c24hi = (hi4 & 0x3Fu) | ((hi4 >> 2) & 0xFC0u) | ((hi4 >> 4) & 0x3F000u) | ((hi4 >> 6) & 0xFC0000u);
      // 48 bits per lane, dense in channel order; the even lane of a pair writes both lanes' 12 bytes (4-byte aligned)
      const uint32_t w0 = c24lo | (c24hi << 24), w1 = c24hi >> 8;          // this lane: w0 + the low 16 bits of w1
      const uint32_t p0 = __shfl_xor(w0, 1), p1 = __shfl_xor(w1, 1);       // the odd neighbour's
      if (live[u] && (c[u] & 1) == 0) {
        uint32_t* d = (uint32_t*)(codes + tok[u] * heads * 48 + c[u] * 6);
        d[0] = w0;
        d[1] = w1 | (p0 << 16);
        d[2] = (p0 >> 16) | (p1 << 16);
      }
      if (live[u] && (c[u] & 7) == 0) scales[tok[u] * heads + (c[u] >> 3)] = (uint16_t)(sc.s16x2 & 0xFFFFu);
    } else {
      const uint32_t w = codes_vec16(raw[u], lut, a.shift, sc.inv, sc.inv_lo);
      if (live[u]) *(uint32_t*)(codes + tok[u] * heads * 32 + c[u] * 4) = w;
      if (live[u] && (c[u] & 15) == 0) scales[tok[u] * (heads >> 1) + (c[u] >> 4)] = (uint16_t)(sc.s16x2 & 0xFFFFu);
    }
  }
}
