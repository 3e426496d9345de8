// fpq_packed_operands.h - the packed weight file's codewords <-> the matrix-core GEMMs' weight operands (include/fpq.h:
// fpq_packed_to_operands, fpq_operands_to_packed).  The file holds an INDEX into the sorted, de-duplicated value table, the GEMMs
// take the hardware CODE of the same level: a fixed map per field and a layout, no arithmetic on values and no second quantization
// decision.  Included by fpq_kernels.hip only.
//
// The maps, per field (Z = the table's zero index: 7 of 15 levels, 31 of 63; T = 2 Z + 2 the field's range):
//   index i -> magnitude |i - Z|, negative below Z; the one index no table has (T - 1) -> code 0
//   E2M1: nibble  sign << 3 | magnitude          E2M3 / E3M2: field sign << 5 | magnitude        (the tables' levels ascend as their codes do)
//   E1M2 -> E2M3: sign << 5 | magnitude << 1 (m / 4 = 2 m / 8: the subnormals, then 1 + (2 m - 8) / 8)
//   E3M0 -> E3M2: sign << 5 | magnitude << 2 (level m = exponent field m, mantissa 0)
// and back: magnitude = (code >> shift) & Z, index = Z -/+ magnitude (either zero -> Z; a code that is no level of the table still
// gives an index in range).  Done on four fields at a time, one per byte of a 32-bit word: no byte's sum leaves its byte.
#pragma once

constexpr uint32_t po_bytes(uint32_t b) { return b * 0x01010101u; }

// four indices (one per byte, each < T = 1 << BITS) -> four codes: magnitude << sh, `sign` or'ed in below the zero index
template <int BITS>
__host__ __device__ __forceinline__ uint32_t po_codes_of_indices(uint32_t v, uint32_t sh, uint32_t sign) {
  constexpr uint32_t T = 1u << BITS, Z = T / 2 - 1;
  const uint32_t t = v + po_bytes(T - Z);                                   // bit BITS: index >= Z; below it: index - Z
  const uint32_t ge = ((t >> BITS) & po_bytes(1)) * 0xFFu;
  const uint32_t neg = ((v ^ po_bytes(T - 1)) + po_bytes(Z + 1)) & po_bytes(T - 1);   // (T - 1 - v) + Z + 1 = T + (Z - v)
  const uint32_t mag = (t & po_bytes(T - 1) & ge) | (neg & ~ge);
  const uint32_t none = (((v + po_bytes(1)) >> BITS) & po_bytes(1)) * 0xFFu;          // index T - 1: no level
  return ((mag << sh) | (po_bytes(sign) & ~ge)) & ~none;
}
// four codes (one per byte; sign at bit `sbit`, magnitude << sh below it) -> four indices in 0 .. 2 Z
template <int BITS>
__host__ __device__ __forceinline__ uint32_t po_indices_of_codes(uint32_t c, uint32_t sh, uint32_t sbit) {
  constexpr uint32_t Z = (1u << BITS) / 2 - 1;
  const uint32_t mag = (c >> sh) & po_bytes(Z);
  const uint32_t sm = ((c >> sbit) & po_bytes(1)) * 0xFFu;
  return ((po_bytes(Z) + mag) & ~sm) | ((po_bytes(Z) - mag) & sm);
}

// four 6-bit fields of a 24-bit string <-> one per byte
__host__ __device__ __forceinline__ uint32_t po_spread6(uint32_t t) {
  return (t & 0x3Fu) | ((t << 2) & 0x3F00u) | ((t << 4) & 0x3F0000u) | ((t << 6) & 0x3F000000u);
}
__host__ __device__ __forceinline__ uint32_t po_pack6(uint32_t b) {
  return (b & 0x3Fu) | ((b >> 2) & 0xFC0u) | ((b >> 4) & 0x3F000u) | ((b >> 6) & 0xFC0000u);
}
// four bytes -> four 6-bit fields twelve bits apart (the even or the odd elements of eight), and back
__host__ __device__ __forceinline__ uint64_t po_spread12(uint32_t b) {
  return (uint64_t)(b & 0xFFu) | (uint64_t)((b & 0xFF00u) << 4) | ((uint64_t)(b & 0xFF0000u) << 8) | ((uint64_t)(b & 0xFF000000u) << 12);
}
__host__ __device__ __forceinline__ uint32_t po_gather12(uint64_t p) {
  return (uint32_t)(p & 0x3Fu) | (uint32_t)((p >> 4) & 0x3F00u) | (uint32_t)((p >> 8) & 0x3F0000u) | (uint32_t)((p >> 12) & 0x3F000000u);
}

// what a lane converts (a UNIT) and the bytes a 128-group has on either side
enum PoMode { kPo44 = 0,    // E2M1: 32 index nibbles (16 bytes) -> 32 code nibbles (one 16-byte chunk)
              kPo46 = 1,    // E1M2 / E3M0: 32 index nibbles (16 bytes) -> 32 six-bit codes (24 bytes: three 8-byte pieces)
              kPo66 = 2 };  // E2M3 / E3M2: 64 six-bit indices (three 16-byte chunks) -> 64 six-bit codes (three chunks)
template <int MODE> struct PoGeom {
  static constexpr int kUnits = MODE == kPo66 ? 2 : 4;        // per group
  static constexpr int kPacked = MODE == kPo66 ? 96 : 64;     // bytes of a group in the file
  static constexpr int kOperand = MODE == kPo44 ? 64 : 96;    // ... and in the operand
};

// --- a unit's arithmetic, registers only ---------------------------------------------------------------------------------
__device__ __forceinline__ u32x4 po_fwd44(u32x4 w) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = po_codes_of_indices<4>(w[i] & 0x0F0F0F0Fu, 0, 8) | (po_codes_of_indices<4>((w[i] >> 4) & 0x0F0F0F0Fu, 0, 8) << 4);
  return o;
}
__device__ __forceinline__ u32x4 po_inv44(u32x4 w) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = po_indices_of_codes<4>(w[i] & 0x0F0F0F0Fu, 0, 3) | (po_indices_of_codes<4>((w[i] >> 4) & 0x0F0F0F0Fu, 0, 3) << 4);
  return o;
}
// 32 nibbles -> 192 bits: word i's eight codes are 48 bits, even elements from the low nibbles
__device__ __forceinline__ void po_fwd46(u32x4 w, uint32_t sh, uint64_t (&o)[3]) {
  uint64_t p[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    p[i] = po_spread12(po_codes_of_indices<4>(w[i] & 0x0F0F0F0Fu, sh, 32)) |
           (po_spread12(po_codes_of_indices<4>((w[i] >> 4) & 0x0F0F0F0Fu, sh, 32)) << 6);
  o[0] = p[0] | (p[1] << 48);
  o[1] = (p[1] >> 16) | (p[2] << 32);
  o[2] = (p[2] >> 32) | (p[3] << 16);
}
__device__ __forceinline__ u32x4 po_inv64(const uint64_t (&o)[3], uint32_t sh) {
  constexpr uint64_t M = (1ull << 48) - 1;
  const uint64_t p[4] = {o[0] & M, ((o[0] >> 48) | (o[1] << 16)) & M, ((o[1] >> 32) | (o[2] << 32)) & M, o[2] >> 16};
  u32x4 w;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    w[i] = po_indices_of_codes<4>(po_gather12(p[i]), sh, 5) | (po_indices_of_codes<4>(po_gather12(p[i] >> 6), sh, 5) << 4);
  return w;
}
// twelve words = four strings of 96 bits = sixteen of 24: FWD index -> code, else code -> index
template <bool FWD>
__device__ __forceinline__ void po_map66(uint32_t (&w)[12]) {
#pragma unroll
  for (int i = 0; i < 12; i += 3) {
    uint32_t t[4] = {w[i] & 0xFFFFFFu, (w[i] >> 24) | ((w[i + 1] & 0xFFFFu) << 8), (w[i + 1] >> 16) | ((w[i + 2] & 0xFFu) << 16), w[i + 2] >> 8};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      t[j] = po_pack6(FWD ? po_codes_of_indices<6>(po_spread6(t[j]), 0, 32) : po_indices_of_codes<6>(po_spread6(t[j]), 0, 5));
    w[i] = t[0] | (t[1] << 24);
    w[i + 1] = (t[1] >> 8) | (t[2] << 16);
    w[i + 2] = (t[2] >> 16) | (t[3] << 8);
  }
}

// --- the two kernels -----------------------------------------------------------------------------------------------------
// Where unit u of group s of operand row j lives.  Row-major: in the row's own bytes.  K-major (image_rows > 0): at km4_off /
// km6_off of each 16-byte chunk (fpq_common.h); `piece` = byte offset inside the group's 64 / 96.
template <int MODE>
__device__ __forceinline__ int64_t po_operand_off(int64_t j, int64_t s, int64_t steps, uint32_t piece, uint32_t image_rows) {
  if (image_rows == 0) return (j * steps + s) * PoGeom<MODE>::kOperand + piece;
  if (MODE == kPo44) return (int64_t)km4_off((uint32_t)j, (uint32_t)s, piece >> 4, image_rows) + (piece & 15u);
  return (int64_t)km6_off((uint32_t)j, (uint32_t)s, piece >> 4, image_rows) + (piece & 15u);
}

// One lane per unit of the OPERAND, padding rows of a k-major image included (zero codes, zero scales): a wavefront writes 1 KiB
// (1.5 KiB) in a row.  Row-major: units in the tensor's order.  K-major: in the image's order - slot j of a plane holds tensor row
// km_dealt_row(j), whose group is one contiguous 64- / 96-byte read.  The unit-0 lane of a group also converts its scale
// (scale image: natural row order, fpq_scales_to_kmajor).  scales == nullptr: per-channel, the scale vector is not an operand.
template <int MODE, typename Ts>
__global__ __launch_bounds__(kBlock) void packed_to_operands_kernel(const uint8_t* __restrict__ codes, const Ts* __restrict__ scales,
                                                                   uint8_t* __restrict__ w_codes, float* __restrict__ w_scales,
                                                                   int64_t outs, int64_t steps, uint32_t image_rows, uint32_t sh) {
  using G = PoGeom<MODE>;
  const int64_t op_rows = image_rows ? (int64_t)image_rows : outs, n = op_rows * steps * G::kUnits;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const uint32_t u = (uint32_t)i & (G::kUnits - 1);
    const int64_t rest = i / G::kUnits;
    int64_t j, s, row;
    if (image_rows) {
      s = rest / op_rows, j = rest - s * op_rows, row = km_dealt_row(j);
    } else {
      j = rest / steps, s = rest - j * steps, row = j;
    }
    const bool live = row < outs;
    const uint8_t* src = codes + (row * steps + s) * G::kPacked;
    if (u == 0 && scales) {
      const float sc = live ? (float)scales[row * steps + s] : 0.0f;
      w_scales[image_rows ? s * op_rows + row : row * steps + s] = sc;
    }
    if (MODE == kPo44) {
      u32x4 o = u32x4{0, 0, 0, 0};
      if (live) o = po_fwd44(__builtin_nontemporal_load((const u32x4*)src + u));
      *(u32x4*)(w_codes + po_operand_off<MODE>(j, s, steps, 16u * u, image_rows)) = o;
    } else if (MODE == kPo46) {
      uint64_t o[3] = {0, 0, 0};
      if (live) po_fwd46(__builtin_nontemporal_load((const u32x4*)src + u), sh, o);
#pragma unroll
      for (int p = 0; p < 3; ++p)   // 8-byte pieces at 24 u + 8 p: none straddles a chunk
        *(u32x2*)(w_codes + po_operand_off<MODE>(j, s, steps, 24u * u + 8u * p, image_rows)) = u32x2{(uint32_t)o[p], (uint32_t)(o[p] >> 32)};
    } else {
      uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      if (live) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const u32x4 v = __builtin_nontemporal_load((const u32x4*)src + 3 * u + p);
          w[4 * p] = v[0], w[4 * p + 1] = v[1], w[4 * p + 2] = v[2], w[4 * p + 3] = v[3];
        }
        po_map66<true>(w);
      }
#pragma unroll
      for (int p = 0; p < 3; ++p)
        *(u32x4*)(w_codes + po_operand_off<MODE>(j, s, steps, 16u * (3 * u + p), image_rows)) = u32x4{w[4 * p], w[4 * p + 1], w[4 * p + 2], w[4 * p + 3]};
    }
  }
}

// The inverse: one lane per unit of the FILE's codes (rows of the tensor only), reading the operand where the kernel above wrote it.
template <int MODE>
__global__ __launch_bounds__(kBlock) void operands_to_packed_kernel(const uint8_t* __restrict__ w_codes, const float* __restrict__ w_scales,
                                                                   uint8_t* __restrict__ codes, float* __restrict__ scales,
                                                                   int64_t outs, int64_t steps, uint32_t image_rows, uint32_t sh) {
  using G = PoGeom<MODE>;
  const int64_t n = outs * steps * G::kUnits;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const uint32_t u = (uint32_t)i & (G::kUnits - 1);
    const int64_t rest = i / G::kUnits, row = rest / steps, s = rest - row * steps;
    const int64_t j = image_rows ? km_dealt_slot(row) : row;
    uint8_t* dst = codes + (row * steps + s) * G::kPacked;
    if (u == 0 && scales) scales[row * steps + s] = w_scales[image_rows ? s * (int64_t)image_rows + row : row * steps + s];
    if (MODE == kPo44) {
      ((u32x4*)dst)[u] = po_inv44(*(const u32x4*)(w_codes + po_operand_off<MODE>(j, s, steps, 16u * u, image_rows)));
    } else if (MODE == kPo46) {
      uint64_t o[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const u32x2 v = *(const u32x2*)(w_codes + po_operand_off<MODE>(j, s, steps, 24u * u + 8u * p, image_rows));
        o[p] = (uint64_t)v[0] | ((uint64_t)v[1] << 32);
      }
      ((u32x4*)dst)[u] = po_inv64(o, sh);
    } else {
      uint32_t w[12];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const u32x4 v = *(const u32x4*)(w_codes + po_operand_off<MODE>(j, s, steps, 16u * (3 * u + p), image_rows));
        w[4 * p] = v[0], w[4 * p + 1] = v[1], w[4 * p + 2] = v[2], w[4 * p + 3] = v[3];
      }
      po_map66<false>(w);
#pragma unroll
      for (int p = 0; p < 3; ++p) ((u32x4*)dst)[3 * u + p] = u32x4{w[4 * p], w[4 * p + 1], w[4 * p + 2], w[4 * p + 3]};
    }
  }
}

// --- the entry points' shared checks (include/fpq.h lists them in this order) ---------------------------------------------
struct PoCall {
  int mode;
  uint32_t sh, image_rows;
  int64_t steps, units;   // units: lanes of work on the operand side (forward) - the inverse has outs * steps * kUnits
};
inline int po_check(int64_t outs, int64_t k, int64_t cols, int table_id, int kmajor, int scale_dtype, PoCall* c) {
  if (table_id < FPQ_E2M1 || table_id > FPQ_E3M2) return FPQ_ERR_TABLE;
  if (outs < 0 || k < 0 || cols < 0) return FPQ_ERR_ARG;
  if (!is_f16_or_f32(scale_dtype)) return FPQ_ERR_DTYPE;
  const bool four = table_id <= FPQ_E3M0;
  if (k % 128 != 0 || (cols != 128 && cols != k) || (cols == k && k != 128 && four)) return FPQ_ERR_SHAPE;
  const int64_t rows64 = (outs + 63) / 64 * 64;
  c->mode = table_id == FPQ_E2M1 ? kPo44 : four ? kPo46 : kPo66;
  if (!km_image_fits(rows64, k / 128 * (c->mode == kPo44 ? 64 : 96))) return FPQ_ERR_SHAPE;   // the operand, padded: < 2 GiB in either layout
  c->sh = table_id == FPQ_E1M2 ? 1u : table_id == FPQ_E3M0 ? 2u : 0u;
  c->image_rows = kmajor ? (uint32_t)rows64 : 0u;
  c->steps = k / 128;
  c->units = (kmajor ? rows64 : outs) * c->steps * (c->mode == kPo66 ? 2 : 4);
  return FPQ_OK;
}
inline bool po_aligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0);
}
